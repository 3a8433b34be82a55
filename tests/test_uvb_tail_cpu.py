"""CPU: the host algebra of the per-trait fits (bwgr_amd/csrc/uvb_tail.h) without a GPU.

tests/uvb_tail_check.cpp replays uvb_start and uvb_update on the per-sweep records of the line-cited restatements (tests/uvb_restatement.py::
solver, tests/sem2_restatement.py::solver2x) as a program of its own under AddressSanitizer and UBSan -- built and run as
tests/test_devbufs_cpu.py does its program -- and checks uvb_result and uvb_slots against values written out by hand.  Agreement is to 1e-9
of the restatement's value, the bound tests/test_uvb_cpu.py uses between two evaluations of these formulas; the sweep counts and the stop
decisions agree exactly."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sem2_restatement as S2  # noqa: E402
import uvb_restatement as UR  # noqa: E402
from test_devbufs_cpu import CSRC, FLAGS, ROOT, _sanitizing_compiler  # noqa: E402

VARIANTS = {"D": 0, "F": 1, "X": 2, "Z": 3}


def _data(seed, n=12, p=7, q=3):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 3, size=(n, p)).astype(np.float64)
    Z = rng.normal(size=(n, q)) * (4.0 / (1.0 + np.arange(q))) + rng.normal(size=q)
    y = (X - X.mean(0)) @ rng.normal(size=p) * 0.4 + rng.normal(size=n) + 3.0
    return y, X, Z


def _fits():
    """[(name, variant, two designs, maxit, record)]: every variant for five sweeps, solver2x with and without a constant design, a trait
    that stops by the default tolerance, and one whose cnv goes NaN (one design, every marker constant: TrXSX = 0, lambda = 0, b = 0 / 0)."""
    out = []

    def one(name, variant, seed=5, maxit=5, tol=0, X=None):
        y, X0, _ = _data(seed)
        rec = {}
        r = UR.solver(y, X0 if X is None else X, variant, maxit=maxit, tol=tol, record=rec)
        out.append((name, variant, False, maxit, rec))
        return r

    def two(name, seed=7, maxit=5, tol=0, X=None, Z=None):
        y, X0, Z0 = _data(seed)
        rec = {}
        r = S2.solver2x(y, Z0 if Z is None else Z, X0 if X is None else X, maxit=maxit, tol=tol, record=rec)
        out.append((name, "D", True, maxit, rec))
        return r

    for v in "DFXZ":
        assert one("five sweeps " + v, v)["its"] == 5
    assert two("solver2x")["its"] == 5
    r = two("solver2x TrXSX1 = 0", Z=np.tile([0.5, -1.25, 2.0], (12, 1)))
    assert r["its"] == 5 and np.isnan(r["vb1"]) and not r["b1"].any() and r["b2"].any()
    r = two("solver2x TrXSX = 0", X=np.ones((12, 7)))
    assert r["its"] == 5 and np.isnan(r["vb2"]) and not r["b2"].any() and r["b1"].any()
    r = one("default tolerance", "D", maxit=100, tol=10e-7)
    assert 1 < r["its"] < 100 and r["cnv"] < np.log10(10e-7)
    r = one("NaN cnv", "D", X=np.ones((12, 7)))
    assert r["its"] == 1 and np.isnan(r["cnv"])
    return out


def _num(v):
    return "%.17g" % v


def _cases_text():
    fits = _fits()
    lines = [str(len(fits))]
    for _, variant, two, maxit, rec in fits:
        g = lambda d, key: d.get(key, np.nan if key == "vb1" else 0.0)      # noqa: E731  (the one-design solver has no leg: zeros, unread; its vb1 stays NaN)
        lines.append(" ".join([str(VARIANTS[variant]), str(int(two)), str(maxit), _num(rec["logtol"]), _num(rec["df0"]), str(rec["p"]),
                               str(rec.get("q1", 0)), str(len(rec["sweeps"]))]))
        lines.append(" ".join(_num(rec[key]) for key in ("nt", "mu", "sumy", "vy", "TrXSX")) + " " + _num(g(rec, "TrXSX1")))
        lines.append(" ".join(_num(g(rec, key)) for key in ("ve", "vb", "lam", "vb1", "lam1"))
                     + " %d %d" % (int(two and rec["TrXSX1"] == 0), int(two and rec["TrXSX"] == 0)))
        for s in rec["sweeps"]:
            lines.append(" ".join(_num(g(s, key)) for key in ("se", "ey", "ee", "bb", "tb", "db2", "d1", "bb1", "tb1")))
            lines.append(" ".join(_num(g(s, key)) for key in ("mu", "ve", "vb", "vb1", "lam", "lam1", "cnv")) + " %d %d" % (s["its"], int(s["on"])))
    return "\n".join(lines) + "\n"


def test_the_records_leave_the_restatements_outputs_alone():
    y, X, Z = _data(5)
    for v in "DFXZ":
        a, b = UR.solver(y, X, v, maxit=4, tol=0), UR.solver(y, X, v, maxit=4, tol=0, record={})
        assert all(np.array_equal(a[key], b[key], equal_nan=True) for key in a)
    a, b = S2.solver2x(y, Z, X, maxit=4, tol=0), S2.solver2x(y, Z, X, maxit=4, tol=0, record={})
    assert all(np.array_equal(a[key], b[key], equal_nan=True) for key in a)


def test_uvb_tail_under_sanitizers(tmp_path):
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible: no sanitizer build runs on a GPU machine")
    cxx = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no C++ compiler with the AddressSanitizer and UBSan runtimes")
    exe, cases = str(tmp_path / "uvb_tail_check"), str(tmp_path / "cases.txt")
    built = subprocess.run([cxx] + FLAGS + ["-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "uvb_tail_check.cpp")], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    with open(cases, "w") as f:
        f.write(_cases_text())
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "" and run.stdout.strip() == "uvb_tail_check ok", (run.returncode, run.stdout, run.stderr[-2000:])


def test_uvb_tail_header_is_plain_cxx():
    txt = open(os.path.join(CSRC, "uvb_tail.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", txt) and "__global__" not in txt and "__device__" not in txt
    for name in ("uvb.hip.h", "uvb2.hip.h"):      # the kernels' headers take the two PODs from it
        assert '#include "uvb_tail.h"' in open(os.path.join(CSRC, name)).read()
