"""CPU: the holder that owns every handle's and every call's device arrays, streams and events (bwgr_amd/csrc/devbufs.h).

tests/devbufs_check.cpp runs it on a counting fake backend that fails the N-th allocation, stream or event creation, as a program of its own
under AddressSanitizer and UBSan: the all-or-nothing take at every failing position, get / drop, and the order of destruction.  The library
has no allocation-failure injection and a sanitizer build never runs beside a GPU, so this is where the failure paths are exercised."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bwgr_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _sanitizing_compiler(workdir):
    """The first C++ compiler that builds and runs a program with the two sanitizers' runtimes, or None."""
    probe = os.path.join(workdir, "probe.cpp")
    with open(probe, "w") as f:
        f.write("#include <vector>\nint main() { std::vector<int> v(3, 1); return v[2] - 1; }\n")
    for cxx in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if not path:
            continue
        exe = os.path.join(workdir, "probe")
        built = subprocess.run([path] + FLAGS + ["-o", exe, probe], capture_output=True)
        if built.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0:
            return path
    return None


def test_holder_under_sanitizers(tmp_path):
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible: no sanitizer build runs on a GPU machine")
    cxx = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no C++ compiler with the AddressSanitizer and UBSan runtimes")
    exe = str(tmp_path / "devbufs_check")
    built = subprocess.run([cxx] + FLAGS + ["-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "devbufs_check.cpp")],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "" and run.stdout.strip() == "devbufs_check ok", (run.returncode, run.stdout, run.stderr)


def test_one_place_allocates():
    """hipMalloc( and hipFree( occur once each under bwgr_amd/csrc/, inside the HIP backend of the holder; and whatever creates or destroys a
    stream or an event (every hipEventCreate*, hipEventDestroy*, hipStreamCreate*, hipStreamDestroy*) occurs there and nowhere else, in code,
    comments or messages."""
    found = {"hipMalloc(": [], "hipFree(": []}
    inside_only = {"hipEventCreate": [], "hipEventDestroy": [], "hipStreamCreate": [], "hipStreamDestroy": []}
    for name in sorted(os.listdir(CSRC)):
        txt = open(os.path.join(CSRC, name)).read()
        for table in (found, inside_only):
            for call in table:
                table[call] += [(name, m.start()) for m in re.finditer(re.escape(call), txt)]
    src = open(os.path.join(CSRC, "bwgr_hip.hip")).read()
    begin = src.index("struct HipBackend {")
    end = src.index("\n};", begin)
    for call, where in found.items():
        assert len(where) == 1, (call, where)
        name, at = where[0]
        assert name == "bwgr_hip.hip" and begin < at < end, (call, where)
    for call, where in inside_only.items():
        assert where, call   # (the backend does create and destroy them)
        assert all(name == "bwgr_hip.hip" and begin < at < end for name, at in where), (call, where)


def test_holder_header_is_plain_cxx():
    txt = open(os.path.join(CSRC, "devbufs.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", txt)
