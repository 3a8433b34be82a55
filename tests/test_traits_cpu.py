"""CPU: what the fp64 fits do to Y and Z on the host before a kernel runs (bwgr_amd/csrc/traits.h).

tests/traits_check.cpp compares the reader of Y under both refusal rules, the missingness patterns, the mask packers, Z without its padding
and the cumulative marker order with plain loops of its own and with values worked out by hand, as a program of its own under
AddressSanitizer and UBSan -- built and run as tests/test_devbufs_cpu.py does its program."""
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_devbufs_cpu import CSRC, FLAGS, ROOT, _sanitizing_compiler  # noqa: E402


def test_traits_under_sanitizers(tmp_path):
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible: no sanitizer build runs on a GPU machine")
    cxx = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no C++ compiler with the AddressSanitizer and UBSan runtimes")
    exe = str(tmp_path / "traits_check")
    built = subprocess.run([cxx] + FLAGS + ["-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "traits_check.cpp")],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "" and run.stdout.strip() == "traits_check ok", (run.returncode, run.stdout, run.stderr)


def test_traits_header_is_plain_cxx():
    txt = open(os.path.join(CSRC, "traits.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", txt)
