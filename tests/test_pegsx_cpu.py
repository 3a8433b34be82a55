"""CPU: PEGSX without a GPU -- the branch guards of every case in tests/pegsx_cases.py on the restatement alone, the host work (the trait set-up
of bwgr_amd/csrc/pegsx_setup.h and the new functions of bwgr_amd/csrc/pegs_tail.h) as a program of its own under AddressSanitizer and UBSan
against tests/pegsx_restatement.py, and the surface (C ABI, the Python signature, the plan hook, BWGR_ENODEV)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pegsx_cases as XC  # noqa: E402
import pegsx_restatement as XR  # noqa: E402
from test_devbufs_cpu import CSRC, FLAGS, ROOT, _sanitizing_compiler  # noqa: E402

FLOOR_BITS = {"denom": 1, "ve": 2, "tr": 4, "sd": 8, "cnv": 16}   # PEGSX_FL_* of pegs_tail.h


# ---- the branch guards: every case of the table, none left out ----

@pytest.mark.parametrize("case", XC.CASES, ids=[c["id"] for c in XC.CASES])
def test_case_is_away_from_the_discontinuous_branches(case):
    """In every sweep and effect |MinDVb - covMinEv| >= 1e-3 covMinEv (the GPU's values differ from the restatement's by rounding, orders of
    magnitude less) and an eigen-gap of at least 1e-3 where XFA truncates; every kept eigenvalue of every M'M is at least 1e-3 of the largest
    and every dropped one at most 1e-10 of it; no floor is active, except in a case that names it."""
    _, _, _, fit = XC.restate(case)
    kw = case["kw"]
    cm = float(np.float32(kw.get("covMinEv", 10e-4)))
    k = len(fit["ve"])
    trunc = bool(kw.get("XFA", False)) and 0 < kw.get("NumXFA", 3) < k
    assert fit["trace"]
    floors = set(fit["floors0"])
    for s, recs in enumerate(fit["trace"]):
        for e, r in enumerate(recs):
            assert abs(r["MinDVb"] - cm) >= 1e-3 * cm, (s, e, r["MinDVb"])
            if trunc:
                assert r["gap"] is not None and r["gap"] >= 1e-3, (s, e, r["gap"])
            else:
                assert r["gap"] is None
            floors |= r["floors"]
    assert floors == set(XC.NAMED_FLOORS.get(case["id"], ())), floors
    for t, m in enumerate(fit["mm"]):
        assert m["kept"].size and m["kept"].min() >= 1e-3, (t, m["kept"].min())
        assert m["dropped"].size == 0 or m["dropped"].max() <= 1e-10, (t, m["dropped"])
        assert (m["dropped"].size > 0) == (case["id"] in XC.RANK_DEFICIENT), (t, m["dropped"])
    if case["id"] in XC.BENDS:
        assert all(r["inflated"] and r["MinDVb"] < cm for recs in fit["trace"] for r in recs) and fit["bend"][0] > 0
    if kw["logtol"] == XC.NOSTOP:
        assert fit["its"] == kw["maxit"]


@pytest.mark.parametrize("case", XC.CODE_CASES, ids=[c["id"] for c in XC.CODE_CASES])
def test_code_case_is_well_conditioned(case):
    """The restatement on the rows in reverse order (hat put back) is the same mathematics summed in another order.  The two agree to 1e-9
    on every output, TrZSZ included: a condition on the case's data -- with an intercept in X and codes of a large mean TrZSZ is a difference
    of two large numbers -- that entitles the GPU's parity to 1e-6 on it.  Measured: 1.2e-11 at worst (vb_list, and 9.5e-12 on TrZSZ, on
    tpod + 100), below 1e-14 on every other panel."""
    Y, X, effects, fit = XC.restate(case)
    rev = XR.pegsx(Y[::-1], X[::-1], [D[::-1] for D in XC.designs(effects)], dense=[e[0] == "dense" for e in effects], **case["kw"])
    rev["hat"] = rev["hat"][::-1]
    assert rev["its"] == fit["its"]
    for key in ("TrZSZ", "b", "u", "vb_list", "GC_list", "ve", "hat", "bend", "cnv"):
        pairs = zip(fit[key], rev[key]) if isinstance(fit[key], list) else [(fit[key], rev[key])]
        for a, b in pairs:
            assert np.all(np.isfinite(a)) and XR.scaled_err(b, a) <= 1e-9, (key, XR.scaled_err(b, a))


def test_gram_bound_fit_is_away_from_the_branches_and_well_conditioned():
    """the shape of test_gpu_pegsx.py::test_int32_gram_bound under the same guards"""
    Z, Y, _ = XC.PC.gram_bound()
    Z = Z[:XC.PC.GRAM_BOUND_N].astype(np.float64)
    X = np.ones((len(Z), 1))
    kw = dict(maxit=2, logtol=XC.NOSTOP)
    fit, rev = XR.pegsx(Y, X, [Z], trace=True, **kw), XR.pegsx(Y[::-1], X, [Z[::-1]], **kw)
    rev["hat"] = rev["hat"][::-1]
    assert all(r["MinDVb"] < 0.5e-3 and r["inflated"] and not r["floors"] for recs in fit["trace"] for r in recs) and not fit["floors0"]
    for key in ("TrZSZ", "b", "u", "vb_list", "GC_list", "ve", "hat", "bend", "cnv"):
        for a, b in zip(fit[key], rev[key]) if isinstance(fit[key], list) else [(fit[key], rev[key])]:
            assert np.all(np.isfinite(a)) and XR.scaled_err(b, a) <= 1e-9, key


def test_code_cases_cover_what_the_gpu_tests_promise():
    shapes = {}
    for c in XC.CODE_CASES:
        Y, X, effs = c["data"]()
        shapes[c["id"]] = (Y.shape[0], Y.shape[1], X.shape[1], effs[0][2])
        assert np.all(X[:, 0] == 1.0) and effs[0][1].dtype == np.int8      # an intercept beside an int8 panel
    assert shapes["codes_full_slabs_f70_k5"] == (700, 5, 70, dict(nwg=3)) and shapes["codes_const_cols_f1"][2] == 1
    assert all(shapes["codes_" + name][1:3] == (3, 3) for name in ("signed", "full", "offset", "pm127", "offset_xfa2"))
    # the cancellation case: on tpod + 100 the two sums of TrZSZ are some 1e4 times their difference
    Y, X, effs, fit = XC.restate(XC.by_id("codes_offset"))
    Z = XC.designs(effs)[0]
    for t in range(3):
        w = ~np.isnan(Y[:, t])
        assert 5e3 < (Z[w] ** 2).sum() / fit["TrZSZ"][0][t] < 5e4


def test_stop_rule_case_stops_at_the_fifth_sweep():
    """cnv is below logtol = 0 by sweep 3 at the latest, so the `its >= 5` half of the rule is what ends the fit"""
    case = XC.by_id("stop_rule")
    fit = XC.restate(case)[3]
    assert np.all(fit["cnv_trace"][2:] < -0.5) and fit["its"] == 5 and case["kw"]["maxit"] == 50


def test_case_table_covers_what_the_gpu_tests_promise():
    ids = [c["id"] for c in XC.CASES]
    assert len(set(ids)) == len(ids) and set(XC.BENDS) <= set(ids) and set(XC.RANK_DEFICIENT) <= set(ids)
    shapes = {}
    for c in XC.CASES:
        Y, X, effs = c["data"]()
        shapes[c["id"]] = (Y.shape[0], Y.reshape(len(Y), -1).shape[1], X.shape[1], [e[0] for e in effs])
    assert {s[1] for s in shapes.values()} >= {1, 3, 5, 16}
    assert {s[2] for s in shapes.values()} >= {1, 2, 3, 4, 70}
    assert shapes["f70_slabs_k5"][:3] == (700, 5, 70) and shapes["dense_only_n1500"] == (1500, 3, 3, ["dense"])
    assert shapes["panel_dense70"][3] == ["panel", "dense"] and shapes["dense70_panel"][3] == ["dense", "panel"]
    assert shapes["two_panels"][3] == ["panel", "panel"] and shapes["k16_shared_patterns"][1] == 16
    import bwgr_amd
    assert bwgr_amd.pegsx_plan(1500, 3, 3)["threads"] == 1024 < 1500     # rows past one trip of the fixed step


def test_xfa_with_numxfa_zero_is_xfa_off():
    a, b = XC.restate(XC.by_id("tpod_k3_xfa_num0"))[3], XC.restate(XC.by_id("tpod_k3_defaults"))[3]
    for key in ("b", "ve", "hat", "cnv"):
        assert np.array_equal(a[key], b[key]), key


def test_rank_deficient_x_projects_as_the_reduced_coding_does():
    """dropping one of the two complementary dummies spans the same space: the same projected traits and the same projected traces (the
    fits themselves differ, because f enters the degrees of freedom as the number of columns, not as the rank)"""
    case = XC.by_id("rank_deficient_x")
    Y, X, effs, fit = XC.restate(case)
    red = XR.pegsx(Y, X[:, [0, 1, 3]], XC.designs(effs), trace=True, **dict(case["kw"], maxit=0))
    assert XR.scaled_err(fit["setup"]["y"], red["setup"]["y"]) <= 1e-10
    assert XR.scaled_err(fit["TrZSZ"][0], red["TrZSZ"][0]) <= 1e-10
    assert XR.scaled_err(X @ fit["setup"]["b0"], X[:, [0, 1, 3]] @ red["setup"]["b0"]) <= 1e-10


# ---- the host work under the sanitizers ----

def _fmt(v):
    return " ".join("%.17g" % x for x in np.asarray(v, np.float64).ravel())


def _bits(names):
    return sum(FLOOR_BITS[n] for n in names)


def _tail_case(fit, kw, setup):
    tr, st, su = fit["trace"], fit["start"], fit["setup"]
    ne, k = st["Tr"].shape
    n, f = su["X"].shape
    logtol = float(np.float32(kw.get("logtol", -8.0)))
    out = ["%d %d %d %d %d %d %s %.17g %.17g %.17g %d %d %d" % (k, ne, len(tr), f, n, int(setup), repr(logtol), np.float32(kw.get("covbend", 1.1)),
                                                              np.float32(kw.get("covMinEv", 10e-4)), np.float32(kw.get("df0", 1.1)), int(kw.get("NNC", False)),
                                                              int(kw.get("XFA", False)), int(kw.get("NumXFA", 3))),
           _fmt(st["nt"]), _fmt(st["ssy"])]
    if setup:
        cond = [1.0 / m["kept"].min() for m in fit["mm"]]
        out += [_fmt(su["Y"].T), _fmt(su["X"].T), _fmt(np.concatenate([a.ravel() for a in su["iXX"]])), _fmt(cond), _fmt(su["b0"].T), _fmt(su["y"].T)]
    out += [_fmt(st["Tr"]), _fmt(st["ve"]), _fmt(np.concatenate([v.ravel() for v in st["vb"]])), "%d" % _bits(fit["floors0"])]
    for sw, recs in enumerate(tr):
        r0 = recs[0]
        out += [_fmt(r0["ey"]), _fmt(np.concatenate([r["TH"].ravel() for r in recs])), _fmt(r0["db2"]), _fmt(r0["ve"]),
                "%s %d" % (repr(float(r0["cnv"])), int(sw + 1 >= 5 and r0["cnv"] < logtol))]
        for r in recs:
            out += [_fmt(r["vb"]), _fmt(r["iG"]), "%.17g %.17g %.17g %d %.17g %d" % (r["inflate"], r["MinDVb"], r["maxEv"], int(r["inflated"]),
                                                                                      -1.0 if r["gap"] is None else r["gap"], _bits(r["floors"]))]
    out += [_fmt(np.concatenate([g.ravel() for g in fit["GC_list"]]))]
    return "\n".join(out)


TAIL_CASES = ["tpod_k3_defaults", "tpod_k3_nnc", "tpod_k3_xfa1", "tpod_k3_xfa2", "tpod_k3_xfa3", "tpod_k3_xfa_num0", "tpod_k3_df0_20", "tpod_k3_covbend2",
              "f1_intercept", "f70_slabs_k5", "k1", "k16_shared_patterns", "rank_deficient_x", "bending_nnc_on", "bending_nnc_off", "two_panels", "panel_dense70",
              "stop_rule"]
SETUP_CASES = ("tpod_k3_defaults", "f1_intercept", "f70_slabs_k5", "k1", "k16_shared_patterns", "rank_deficient_x")


def _tail_input():
    texts, seen = [], dict(k=set(), f=set(), xfa=set(), nnc=set(), bent=False, stopped=False, dropped=False)
    fits = [(XC.restate(XC.by_id(i))[3], XC.by_id(i)["kw"], i in SETUP_CASES) for i in TAIL_CASES]
    for fit, kw, setup in fits:
        k = len(fit["ve"])
        seen["k"].add(k); seen["f"].add(fit["start"]["f"])
        seen["xfa"].add("off" if not (kw.get("XFA") and kw.get("NumXFA", 3) > 0) else "k" if kw["NumXFA"] >= k else "trunc")
        seen["nnc"].add(bool(kw.get("NNC", False)))
        seen["bent"] |= any(r["inflated"] and r["MinDVb"] < 1e-6 for recs in fit["trace"] for r in recs)
        seen["stopped"] |= fit["its"] < kw["maxit"]
        seen["dropped"] |= setup and any(m["dropped"].size for m in fit["mm"])
        texts.append(_tail_case(fit, kw, setup))
    assert seen["k"] >= {1, 3, 5, 16} and seen["f"] >= {1, 3, 4, 70} and seen["xfa"] == {"off", "k", "trunc"} and seen["nnc"] == {True, False}
    assert seen["bent"] and seen["stopped"] and seen["dropped"]
    return "%d\n" % len(texts) + "\n".join(texts) + "\n"


def test_host_work_under_sanitizers(tmp_path):
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible: no sanitizer build runs on a GPU machine")
    cxx = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no C++ compiler with the AddressSanitizer and UBSan runtimes")
    exe, cases = str(tmp_path / "pegsx_tail_check"), str(tmp_path / "cases.txt")
    built = subprocess.run([cxx] + FLAGS + ["-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "pegsx_tail_check.cpp")], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    with open(cases, "w") as f:
        f.write(_tail_input())
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "" and run.stdout.strip() == "pegsx_tail_check ok", (run.returncode, run.stdout, run.stderr[-2000:])


def test_headers_are_plain_cxx():
    for name in ("pegs_tail.h", "pegsx_setup.h"):
        txt = open(os.path.join(CSRC, name)).read()
        assert not re.search(r"#\s*include\s*[<\"]hip", txt) and "__global__" not in txt and "__device__" not in txt, name
    host = open(os.path.join(CSRC, "pegsx_host.hip.h")).read()
    assert "__global__" not in host and "k_mrr_mu_shift" not in host
    main = open(os.path.join(CSRC, "bwgr_hip.hip")).read()
    assert main.index('#include "pegs_host.hip.h"') < main.index('#include "pegsx_host.hip.h"')


# ---- the surface ----

def test_entries_are_declared_exported_and_bound():
    from bwgr_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bwgr.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, nargs in (("bwgr_pegsx", 29), ("bwgr_debug_pegsx_plan", 4), ("bwgr_debug_pegsx_timing", 2), ("bwgr_debug_pegs_launch_plan", 3)):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == nargs, name
    assert int(re.search(r"#define\s+BWGR_PEGSX_MAXF\s+(\d+)", hdr).group(1)) == 256
    assert "InnerGS" in hdr and "NoInv" in hdr


def test_signature_equals_the_reference():
    """R/RcppExports.R:284"""
    import bwgr_amd as B
    E = inspect.Parameter.empty
    pos = [(p.name, p.default) for p in inspect.signature(B.PEGSX).parameters.values() if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert pos == [("Y", E), ("X", E), ("Z_list", E), ("maxit", 500), ("logtol", -8.0), ("covbend", 1.1), ("covMinEv", 10e-4), ("cores", 1), ("verbose", False),
                   ("df0", 1.1), ("NNC", False), ("InnerGS", False), ("NoInv", False), ("XFA", False), ("NumXFA", 3)]
    assert B.api.PEGSX_KEYS == ("TrZSZ", "b", "u", "vb_list", "GC_list", "ve", "hat", "its", "cnv", "bend")


def test_no_gpu_means_enodev_and_refusals_need_none():
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    Y = np.random.default_rng(1).normal(size=(8, 2))
    X = XC.fixed(8, 1, 2)
    Z = bwgr_amd.dense(np.random.default_rng(2).normal(size=(8, 3)))
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.PEGSX(Y, X, [Z])
    assert ei.value.code == 5   # BWGR_ENODEV
    for word, kw in (("InnerGS", dict(InnerGS=True)), ("NoInv", dict(NoInv=True))):
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            bwgr_amd.PEGSX(Y, X, [Z], **kw)
        assert ei.value.code == 1 and word in str(ei.value)
    for word, call in (("effects", lambda: bwgr_amd.PEGSX(Y, X, [])), ("f = 0", lambda: bwgr_amd.PEGSX(Y, np.zeros((8, 0)), [Z])),
                       ("f = 257", lambda: bwgr_amd.PEGSX(Y, np.ones((8, 257)), [Z])), ("rows", lambda: bwgr_amd.PEGSX(Y, X[:7], [Z]))):
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            call()
        assert ei.value.code == 1 and word in str(ei.value), (word, str(ei.value))


def test_plan_hook_is_host_arithmetic():
    import bwgr_amd
    from bwgr_amd import _lib
    src = open(os.path.join(ROOT, "include", "bwgr.h")).read()
    assert int(re.search(r"#define\s+BWGR_PEGSX_PLAN_NOUT\s+(\d+)", src).group(1)) == 6
    pl = bwgr_amd.pegsx_plan(196, 3, 3)
    assert pl["threads"] == 256 and pl["lds_bytes"] == 8 * 2 * 3 and pl["ws_bytes"] == 8 * (196 * 3 + 3 * 9 + 9)
    assert pl["jc"] == 4 and pl["fc"] == 4 and pl["trace_lds_bytes"] == 8 * (4 * 4 * 3 + 4 * 16)
    assert bwgr_amd.pegsx_plan(5000, 64, 16)["threads"] == 1024 and bwgr_amd.pegsx_plan(1, 1, 1)["threads"] == 64
    for f in range(1, 257):   # within the 64 KiB a workgroup gets without asking for more, for every f up to the cap
        p = bwgr_amd.pegsx_plan(5000, f, 16)
        assert p["lds_bytes"] <= 64 * 1024 and p["trace_lds_bytes"] <= 64 * 1024
    L = _lib.lib()
    out = (C.c_int64 * 7)(*[-1] * 7)
    assert L.bwgr_debug_pegsx_plan(196, 3, 3, out) == 0 and out[6] == -1
    for bad in ((0, 3, 3), (196, 0, 3), (196, 257, 3), (196, 3, 0), (196, 3, 17)):
        assert L.bwgr_debug_pegsx_plan(*bad, out) == 1 and b"pegsx plan" in L.bwgr_last_error()
    assert L.bwgr_debug_pegsx_plan(196, 3, 3, None) == 1
