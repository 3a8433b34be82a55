"""CPU: PEGS / PEGSZ without a GPU -- the host tail (bwgr_amd/csrc/pegs_tail.h) as a program of its own under AddressSanitizer and UBSan
against tests/pegs_restatement.py, properties of the restatement itself, the branch guards of every case in tests/pegs_cases.py, and the
surface (C ABI, Python signatures, the plan hook, BWGR_ENODEV)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pegs_cases as PC  # noqa: E402
import pegs_restatement as PR  # noqa: E402
from test_devbufs_cpu import CSRC, FLAGS, ROOT, _sanitizing_compiler  # noqa: E402


# ---- the tail header ----

def _fmt(v):
    return " ".join("%.17g" % x for x in np.asarray(v, np.float64).ravel())


def _tail_case(fit, kw, own_text):
    """one fit of the restatement as text: start values, then per sweep the sums the sweep left and what the tail made of them"""
    tr, st = fit["trace"], fit["start"]
    ne, k = st["MSx"].shape
    XFA = kw.get("XFA", -1)
    out = ["%d %d %d %s %.17g %.17g %d %d %d" % (k, ne, len(tr), repr(float(np.float32(kw.get("logtol", -4.0)))), np.float32(kw.get("covbend", 1.1)),
                                                np.float32(kw.get("covMinEv", 10e-4)), XFA, int(kw.get("NNC", True)), int(own_text)),
           _fmt(st["nt"]), _fmt(st["vy"]), _fmt(st["mu0"]), _fmt(st["MSx"])]
    logtol = float(np.float32(kw.get("logtol", -4.0)))
    for recs in tr:
        r0 = recs[0]
        out += [_fmt(np.concatenate([r0["ey"], r0["se"]])), _fmt(np.concatenate([r["TH"].ravel() for r in recs])), _fmt(r0["db2"]),
                _fmt(r0["ve"]), _fmt(r0["d"]), _fmt(r0["mu"]), "%s %d" % (repr(float(r0["cnv"])), int(r0["cnv"] < logtol))]
        for r in recs:
            out += [_fmt(r["vb"]), _fmt(r["iG"]), "%.17g %.17g %.17g %d %.17g" % (r["inflate"], r["MinDVb"], r["maxEv"], int(r["inflated"]), -1.0 if r["gap"] is None else r["gap"])]
    out += [_fmt(fit["h2"]), _fmt(np.concatenate([g.ravel() for g in fit["GC"]]))]
    return "\n".join(out)


TAIL_CASES = ["k1", "tpod_k3_defaults", "tpod_k3_xfa0", "tpod_k3_xfa1", "tpod_k3_xfa2", "tpod_k3_nnc_off", "tpod_k3_covbend2", "slabs_k5_patterns",
              "k16_shared_patterns", "bending_nnc_on", "bending_nnc_off", "pegsz_two_panels", "pegsz_panel_dense1", "default_logtol"]


def _tail_input():
    texts, seen = [], dict(k=set(), xfa=set(), nnc=set(), bent=False, stopped=False)
    fits = [(PC.restate(PC.by_id(i))[2], PC.by_id(i)["kw"], PC.by_id(i)["entry"] == "PEGS") for i in TAIL_CASES]
    Y, effs = PC.by_id("tpod_k3_defaults")["data"]()
    for own in (True, False):   # XFA = k: PEGS's text takes the XFA branch, PEGSZ's does not
        kw = dict(maxit=4, logtol=PC.NOSTOP, XFA=3)
        fits.append((PR.pegsz(Y, PC.designs(effs), own_text=own, trace=True, **kw), kw, own))
    for fit, kw, own in fits:
        k = len(fit["mu"])
        XFA = kw.get("XFA", -1)
        seen["k"].add(k)
        seen["xfa"].add("k" if XFA < 0 else "0" if XFA == 0 else ("own_k" if own else "z_k") if XFA == k else "trunc")
        seen["nnc"].add(bool(kw.get("NNC", True)))
        seen["bent"] |= any(r["inflated"] and r["MinDVb"] < 1e-6 for recs in fit["trace"] for r in recs)
        seen["stopped"] |= fit["numit"] < kw["maxit"] if "maxit" in kw else fit["numit"] < 100
        texts.append(_tail_case(fit, kw, own))
    assert seen["k"] >= {1, 3, 5, 16} and seen["xfa"] == {"k", "0", "trunc", "own_k", "z_k"} and seen["nnc"] == {True, False}
    assert seen["bent"] and seen["stopped"]
    return "%d\n" % len(texts) + "\n".join(texts) + "\n"


def test_tail_under_sanitizers(tmp_path):
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible: no sanitizer build runs on a GPU machine")
    cxx = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no C++ compiler with the AddressSanitizer and UBSan runtimes")
    exe, cases = str(tmp_path / "pegs_tail_check"), str(tmp_path / "cases.txt")
    built = subprocess.run([cxx] + FLAGS + ["-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "pegs_tail_check.cpp")], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    with open(cases, "w") as f:
        f.write(_tail_input())
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "" and run.stdout.strip() == "pegs_tail_check ok", (run.returncode, run.stdout, run.stderr[-2000:])


def test_tail_header_is_plain_cxx():
    txt = open(os.path.join(CSRC, "pegs_tail.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", txt) and "__global__" not in txt and "__device__" not in txt
    assert '#include "pegs_tail.h"' in open(os.path.join(CSRC, "mrr.hip.h")).read()   # mrr's tail shares its eigh / pinv


# ---- properties of the restatement ----

def test_pegs_and_pegsz_with_one_effect_agree():
    Y, effs = PC.by_id("tpod_k3_defaults")["data"]()
    X = PC.designs(effs)
    for kw in (dict(), dict(XFA=0), dict(XFA=2), dict(NNC=False)):
        a = PR.pegs(Y, X[0], maxit=6, logtol=PC.NOSTOP, **kw)
        z = PR.pegsz(Y, X, maxit=6, logtol=PC.NOSTOP, **kw)
        assert a["numit"] == z["numit"] == 6
        for key in ("mu", "b", "hat", "h2", "GC", "bend", "cnv"):
            zz = z[key][0] if key in ("b", "GC", "bend") else z[key]
            assert PR.scaled_err(a[key], zz) <= 1e-9, (kw, key)


def test_k1_sweep_is_the_scalar_ridge_step():
    """k = 1: b1 = (x'e + xx b0) / (xx + ve / vb), the step of the per-trait solvers"""
    Y, effs = PC.by_id("k1")["data"]()
    X = PC.designs(effs)[0]
    import bwgr_amd
    r = PR.pegs(Y, X, maxit=1, logtol=PC.NOSTOP)
    y = np.asarray(Y, np.float32).astype(np.float64)[:, 0]
    z = ~np.isnan(y)
    n = z.sum()
    yc = np.where(z, y - y[z].mean(), 0.0)
    xx = (X ** 2 * z[:, None]).sum(0)
    MSx = (xx / n - ((X * z[:, None]).sum(0) / n) ** 2).sum()
    ve = yc @ yc / (n - 1) * 0.5
    lam = ve / (ve / MSx)
    b, e = np.zeros(X.shape[1]), yc.copy()
    for J in bwgr_amd.em_order(X.shape[1], 0):
        b1 = (X[:, J] @ e + xx[J] * b[J]) / (xx[J] + lam)
        e -= X[:, J] * z * (b1 - b[J])
        b[J] = b1
    assert PR.scaled_err(r["b"][:, 0], b) <= 1e-12


def test_xfa0_decouples_the_traits():
    """XFA = 0 with the bending threshold out of reach (below it the joint fit adds one inflate to every trait's variance)"""
    Y, effs = PC.by_id("pegsz_panel_dense70")["data"]()
    X = PC.designs(effs)
    kw = dict(maxit=5, logtol=PC.NOSTOP, XFA=0, covMinEv=1e-7)
    j = PR.pegsz(Y, X, **kw)
    for t in range(Y.shape[1]):
        s = PR.pegsz(Y[:, t], X, **kw)
        # (cnv sums over the traits, so the joint fit's is not a single fit's; everything else is)
        for key in ("mu", "hat", "h2"):
            assert PR.scaled_err(j[key][..., t], s[key][..., 0]) <= 1e-9, (t, key)
        for f in range(len(X)):
            assert PR.scaled_err(j["b"][f][:, t], s["b"][f][:, 0]) <= 1e-9, (t, f)


# ---- the branch guards: every case of the table, none left out ----

@pytest.mark.parametrize("case", PC.CASES, ids=[c["id"] for c in PC.CASES])
def test_case_is_away_from_the_discontinuous_branches(case):
    """|MinDVb - covMinEv| >= 1e-3 covMinEv in every sweep and effect (the `< covMinEv` test is the fit's only discontinuous branch: max(., 0)
    and the running maximum are continuous), and an eigen-gap of at least 1e-3 where XFA truncates."""
    _, _, fit = PC.restate(case)
    cm = float(np.float32(case["kw"].get("covMinEv", 10e-4)))
    k = len(fit["mu"])
    XFA = case["kw"].get("XFA", -1)
    assert fit["trace"]
    for s, recs in enumerate(fit["trace"]):
        for f, r in enumerate(recs):
            assert abs(r["MinDVb"] - cm) >= 1e-3 * cm, (s, f, r["MinDVb"])
            if 0 < XFA < k:
                assert r["gap"] is not None and r["gap"] >= 1e-3, (s, f, r["gap"])
            else:
                assert r["gap"] is None
    if case["id"] in PC.BENDS:
        assert all(r["inflated"] and r["MinDVb"] < cm for recs in fit["trace"] for r in recs) and fit["bend"][0] > 0
    if case["kw"]["logtol"] == PC.NOSTOP:
        assert fit["numit"] == case["kw"]["maxit"]
    else:
        assert 1 < fit["numit"] < case["kw"].get("maxit", 100)


@pytest.mark.parametrize("case", PC.CODE_CASES, ids=[c["id"] for c in PC.CODE_CASES])
def test_code_case_is_well_conditioned(case):
    """The restatement on the rows in reverse order (hat put back) is the same mathematics summed in another order.  The two agree to 1e-9
    on every output: a condition on the case's data -- on codes with a large mean XSX = XX / n - (S / n)^2 loses digits -- that entitles the
    GPU's parity to 1e-6 on it.  Measured: 2.6e-13 at worst (h2 on tpod + 100), at most 1.1e-14 elsewhere."""
    Y, effects, fit = PC.restate(case)
    rev = PR.pegsz(Y[::-1], [D[::-1] for D in PC.designs(effects)], own_text=case["entry"] == "PEGS", **case["kw"])
    rev["hat"] = rev["hat"][::-1]
    assert rev["numit"] == fit["numit"]
    for key in ("mu", "b", "hat", "h2", "GC", "bend", "cnv"):
        pairs = zip(fit[key], rev[key]) if isinstance(fit[key], list) else [(fit[key], rev[key])]
        for a, b in pairs:
            assert np.all(np.isfinite(a)) and PR.scaled_err(b, a) <= 1e-9, (key, PR.scaled_err(b, a))


def test_gram_bound_fit_is_away_from_the_branch_and_well_conditioned():
    """the shape of test_gpu_pegs.py::test_int32_gram_bound under the same two guards"""
    X, Y, _ = PC.gram_bound()
    X = X[:PC.GRAM_BOUND_N].astype(np.float64)
    kw = dict(maxit=2, logtol=PC.NOSTOP)
    fit, rev = PR.pegs(Y, X, trace=True, **kw), PR.pegs(Y[::-1], X[::-1], **kw)
    rev["hat"] = rev["hat"][::-1]
    assert all(r["MinDVb"] < 0.5e-3 and r["inflated"] for recs in fit["trace"] for r in recs)
    for key in ("mu", "b", "hat", "h2", "GC", "bend", "cnv"):
        assert np.all(np.isfinite(fit[key])) and PR.scaled_err(rev[key], fit[key]) <= 1e-9, key


def test_code_panels_are_what_they_say():
    P = {name: PC._panel(name) for name in PC.CODE_PANELS}
    assert all(X.dtype == np.int8 and X.flags.f_contiguous for X in P.values())
    assert sorted(np.unique(P["signed"])) == [-1, 0, 1] and np.array_equal(P["signed"].astype(int) + 1, PC.tpod())
    assert sorted(np.unique(P["offset"])) == [100, 101, 102] and sorted(np.unique(P["pm127"])) == [-127, 127] and P["pm127"].shape == (500, 70)
    for name, shape in (("full", (300, 200)), ("full_slabs", (700, 900))):
        X = P[name]
        assert X.shape == shape and X[:, 0].min() == -128 and X[:, 0].max() == 127 and len(np.unique(X)) == 256
    C = P["const_cols"]
    zero, two = np.flatnonzero(np.all(C == 0, 0)), np.flatnonzero(np.all(C == 2, 0))
    assert len(zero) == 1 and len(two) == 1      # XX = 0; XSX = 0 with XX > 0
    assert PC.slabs900().shape == P["full_slabs"].shape and PC.by_id("codes_full_slabs_k5")["data"]()[1][0][2] == dict(nwg=3)
    ids = {c["id"] for c in PC.CODE_CASES}
    unbent = {i for i in ids if i.endswith("_unbent")}
    assert len(unbent) == 3 and not unbent & set(PC.BENDS)
    for i in unbent:     # the other side of the branch on the same panels: no sweep inflates
        assert not any(r["inflated"] for recs in PC.restate(PC.by_id(i))[2]["trace"] for r in recs)


def test_case_table_covers_what_the_gpu_tests_promise():
    ids = {c["id"] for c in PC.CASES}
    assert len(ids) == len(PC.CASES) and set(PC.BENDS) <= ids
    ks = {len(PC.restate(c)[2]["mu"]) for c in PC.CASES}
    assert {1, 3, 5, 16} <= ks
    from mrr_cases import plan, regime
    _, linv, ngl, _, _ = plan(16, len(set(PC.K16_IDS)))
    assert regime(linv, ngl, len(set(PC.K16_IDS))) == 4   # the inverses do not fit in LDS


# ---- the surface ----

def test_entries_are_declared_exported_and_bound():
    from bwgr_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bwgr.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, nargs in (("bwgr_pegs", 21), ("bwgr_debug_pegs_plan", 4), ("bwgr_debug_pegs_launch_plan", 3)):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs
    assert "bwgr_pegs_effect" in hdr
    L.bwgr_abi_version.restype = int
    assert L.bwgr_abi_version() == 1


def test_signatures_equal_the_reference():
    """R/RcppExports.R:280, 288"""
    import bwgr_amd as B
    E = inspect.Parameter.empty

    def pos(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
    opts = [("maxit", 100), ("logtol", -4.0), ("covbend", 1.1), ("covMinEv", 10e-4), ("XFA", -1), ("NNC", True)]
    assert pos(B.PEGS) == [("Y", E), ("X", E)] + opts
    assert pos(B.PEGSZ) == [("Y", E), ("X_list", E)] + opts
    assert B.api.PEGS_KEYS == ("mu", "b", "hat", "h2", "GC", "bend", "numit", "cnv")


def test_no_gpu_means_enodev():
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    Y = np.random.default_rng(1).normal(size=(8, 2))
    Z = np.random.default_rng(2).normal(size=(8, 3))
    for call in (lambda: bwgr_amd.PEGS(Y, np.ones((8, 4), np.int8)), lambda: bwgr_amd.PEGS(Y, Z), lambda: bwgr_amd.PEGSZ(Y, [Z, bwgr_amd.dense(np.ones((8, 2)))])):
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            call()
        assert ei.value.code == 5   # BWGR_ENODEV


def test_shared_effect_check_runs_without_a_device_and_names_its_caller():
    """a NaN in a dense effect is refused by the check PEGSZ and PEGSX share (mt_check_effects, mtfit_host.hip.h): before a device is asked
    for, in the caller's name, with the effect's index"""
    import bwgr_amd
    from bwgr_amd import dense
    Y = np.random.default_rng(1).normal(size=(8, 2))
    Z = np.random.default_rng(2).normal(size=(8, 3))
    Zbad = Z.copy()
    Zbad[5, 1] = np.nan
    for call, who, e in ((lambda: bwgr_amd.PEGSZ(Y, [dense(Zbad)]), "pegs:", 0), (lambda: bwgr_amd.PEGSX(Y, np.ones((8, 1)), [dense(Z), dense(Zbad)]), "pegsx:", 1)):
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            call()
        msg = str(ei.value)
        assert ei.value.code == 1 and "not finite" in msg and "effect %d" % e in msg, msg
        assert msg.startswith("bwgr status 1: " + who), msg   # (BwgrError puts the status in front of the library's message)


def test_repeated_steps_are_launched_in_one_file_only():
    """what the multi-trait entries do alike is MtFit's: these kernels are launched, and these calls made, in mtfit_host.hip.h and in none of
    the entries' files (the per-trait fits' own pack_row_bits call, with other arguments, is not meant)"""
    src = {name: open(os.path.join(CSRC, name)).read() for name in ("mrr_host.hip.h", "uvb_host.hip.h", "kernels_host.hip.h", "pegs_host.hip.h", "pegsx_host.hip.h", "mtfit_host.hip.h")}
    pats = [r"hipLaunchKernelGGL\(\s*%s\s*," % kn for kn in ("k_mrr_tilde", "k_mrr_ey", "k_mrr_hat_part", "k_pegs_dense_leg", "k_pegs_dense_setup", "k_mrr_setup_cols")]
    pats += [re.escape("pack_row_bits(S, (int64_t)0"), r"hipFuncSetAttribute\([^;]*\bk_mrr_solve\b"]
    for pat in pats:
        where = sorted(name for name, txt in src.items() if re.search(pat, txt))
        assert where == ["mtfit_host.hip.h"], (pat, where)
    main = open(os.path.join(CSRC, "bwgr_hip.hip")).read()
    at = [main.index('#include "%s_host.hip.h"' % name) for name in ("mtfit", "mrr", "uvb", "kernels", "pegs")]
    assert at == sorted(at), at


def test_effect_kinds():
    """the documented rule: integer-valued -> panel, a non-integer value -> dense, dense(Z) -> dense whatever it holds"""
    import bwgr_amd
    from bwgr_amd.api import _pegs_effect, dense
    E, own = _pegs_effect(np.array([[0.5, 1.0], [2.0, 3.0]]), {})
    assert isinstance(E, dense) and not own and E.Z.flags.f_contiguous and E.Z.dtype == np.float64
    E, _ = _pegs_effect(dense(np.array([[0, 1], [2, 1]], np.int8)), {})
    assert isinstance(E, dense)
    with pytest.raises(bwgr_amd.BwgrError):
        dense(np.zeros((2, 2, 2)))
    if bwgr_amd.device_count() == 0:   # an integer-valued float matrix goes to a panel: staging it needs the device
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            _pegs_effect(np.array([[0.0, 1.0], [2.0, 1.0]]), {})
        assert ei.value.code == 5


def test_plan_hook_is_host_arithmetic():
    import bwgr_amd
    from bwgr_amd import _lib
    src = open(os.path.join(ROOT, "include", "bwgr.h")).read()
    assert int(re.search(r"#define\s+BWGR_PEGS_PLAN_NOUT\s+(\d+)", src).group(1)) == 3
    pl = bwgr_amd.pegs_plan(196, 70, 3)
    assert pl["threads"] == 256 and pl["lds_bytes"] == 8 * (4 * 16 + 32)
    assert pl["ws_bytes"] == 8 * (196 * 70 + 4 * 70 * 3 + 70 * 9 + 16) + 4 * 70
    assert bwgr_amd.pegs_plan(5000, 64, 16)["threads"] == 1024 and bwgr_amd.pegs_plan(1, 1, 1)["threads"] == 64
    assert bwgr_amd.pegs_plan(5000, 10 ** 6, 16)["lds_bytes"] == bwgr_amd.pegs_plan(5000, 1, 16)["lds_bytes"]   # q is not capped by LDS
    L = _lib.lib()
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    assert L.bwgr_debug_pegs_plan(196, 70, 3, out) == 0 and out[3] == -1
    for bad in ((0, 70, 3), (196, 0, 3), (196, 70, 0), (196, 70, 17)):
        assert L.bwgr_debug_pegs_plan(*bad, out) == 1 and b"pegs plan" in L.bwgr_last_error()
    assert L.bwgr_debug_pegs_plan(196, 70, 3, None) == 1
