"""CPU: the sparse effects of PEGS / PEGSZ / PEGSX without a GPU -- the host-side CSC work (bwgr_amd/csrc/csc.h) as a program of its own
under AddressSanitizer and UBSan, the premise of the disjoint leg on the restatement (a row-disjoint effect does not depend on the order of
its columns, an overlapping one does), the branch guards of every case in tests/pegs_sparse_cases.py, the plan hook, the surface (C ABI,
Python signatures, the `sparse` class) and the refusals, which need no device."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pegs_restatement as PR  # noqa: E402
import pegs_sparse_cases as SC  # noqa: E402
import pegs_sparse_restatement as SR  # noqa: E402
from test_devbufs_cpu import CSRC, FLAGS, ROOT, _sanitizing_compiler  # noqa: E402


# ---- the CSC header ----

def test_csc_under_sanitizers(tmp_path):
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible: no sanitizer build runs on a GPU machine")
    cxx = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no C++ compiler with the AddressSanitizer and UBSan runtimes")
    exe = str(tmp_path / "csc_check")
    built = subprocess.run([cxx] + FLAGS + ["-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "csc_check.cpp")], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "" and run.stdout.strip() == "csc_check ok", (run.returncode, run.stdout, run.stderr[-2000:])


def test_csc_header_is_plain_cxx_and_the_kernels_are_included():
    txt = open(os.path.join(CSRC, "csc.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", txt) and "__global__" not in txt and "__device__" not in txt
    main = open(os.path.join(CSRC, "bwgr_hip.hip")).read()
    assert main.index('#include "traits.h"') < main.index('#include "csc.h"') < main.index('#include "mtfit_host.hip.h"')
    assert main.index('#include "pegs.hip.h"') < main.index('#include "pegs_sparse.hip.h"') < main.index('#include "mtfit_host.hip.h"')
    kern = open(os.path.join(CSRC, "pegs_sparse.hip.h")).read()
    for name in ("k_pegs_sparse_setup", "k_pegs_sparse_leg", "k_pegs_sparse_leg_disjoint", "k_pegs_sparse_hat", "k_pegsx_trace_sparse"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % name, kern), name
    assert "atomic" not in kern.lower().replace("no atomic", "")
    # both legs run the one per-column routine
    assert len(re.findall(r"\bpegs_sparse_column\s*\(A, c,", kern)) == 2
    hdrs = [open(os.path.join(p, f)).read() for p, f in ((CSRC, "mtfit_host.hip.h"), (CSRC, "pegsx_host.hip.h"), (os.path.join(ROOT, "include"), "bwgr.h"))]
    assert not any("no sparse storage" in h for h in hdrs)


# ---- the premise of the disjoint leg, on the existing restatement ----

def _orders(qs, maxit, kind, seed=0):
    rng = np.random.default_rng(seed)
    one = {"natural": lambda q: np.arange(q), "reversed": lambda q: np.arange(q)[::-1], "shuffled": lambda q: rng.permutation(q)}[kind]
    return [[one(q) for q in qs] for _ in range(maxit)]


def test_row_disjoint_effect_does_not_depend_on_the_column_order():
    """exactly: a column's step reads and writes its own rows alone.  An overlapping effect does depend on it (measured 5.3e-4 on b between the natural
    and the reversed order; the bar is 1e-4)."""
    Y, effects = SC.by_id("ps_inc12_k3")["data"]()
    A = SC.design(effects[0])
    assert SR.row_disjoint(A)
    fits = [PR.pegsz(Y, [A], maxit=6, logtol=SC.NOSTOP, orders=_orders([12], 6, kind)) for kind in ("natural", "reversed", "shuffled")]
    for f in fits[1:]:
        for key in ("b", "hat", "mu", "cnv_trace"):
            for a, b in SC.pairs(fits[0][key], f[key]):
                d = float(np.max(np.abs(np.asarray(a) - np.asarray(b))))
                print("disjoint", key, d)
                assert d == 0.0, (key, d)
    Y, effects = SC.by_id("ps_overlap_k3")["data"]()
    B = SC.design(effects[0])
    assert not SR.row_disjoint(B)
    nat, rev = (PR.pegsz(Y, [B], maxit=6, logtol=SC.NOSTOP, orders=_orders([25], 6, kind)) for kind in ("natural", "reversed"))
    err = PR.scaled_err(rev["b"][0], nat["b"][0])
    print("overlapping, natural vs reversed order: scaled err of b %.3e" % err)
    assert err > 1e-4


def test_text2_is_pegsz_but_for_the_intercept_divisor():
    """one sweep: b is the same (the intercept step comes after it), mu's step differs by the factor (n_t - 1) / n_t"""
    Y, effects = SC.by_id("pzs_two_inc_k3")["data"]()
    D = [SC.design(e) for e in effects]
    z, s = PR.pegsz(Y, D, maxit=1, logtol=SC.NOSTOP), SR.pegsz_sparse(Y, D, maxit=1, logtol=SC.NOSTOP)
    for a, b in zip(z["b"], s["b"]):
        assert np.array_equal(a, b)
    nt = (~np.isnan(Y)).sum(0)
    mu0 = np.nanmean(np.asarray(Y, np.float32).astype(np.float64), 0)
    assert PR.scaled_err((s["mu"] - mu0) * nt, (z["mu"] - mu0) * (nt - 1)) <= 1e-9
    z8, s8 = PR.pegsz(Y, D, maxit=8, logtol=SC.NOSTOP), SR.pegsz_sparse(Y, D, maxit=8, logtol=SC.NOSTOP)
    assert np.max(np.abs(z8["mu"] - s8["mu"])) > 1e-6


# ---- the branch guards: every case of the table ----

@pytest.mark.parametrize("case", SC.CASES, ids=[c["id"] for c in SC.CASES])
def test_case_is_away_from_the_discontinuous_branches(case):
    """|MinDVb - covMinEv| >= 1e-3 covMinEv in every sweep and effect, an eigen-gap of at least 1e-3 where XFA truncates, and every output
    finite (tests/test_pegs_cpu.py states why)."""
    data, fit = SC.restate(case)
    cm = float(np.float32(case["kw"].get("covMinEv", 10e-4)))
    assert fit["trace"] and fit["numit" if "numit" in fit else "its"] == case["kw"]["maxit"]
    for s, recs in enumerate(fit["trace"]):
        for f, r in enumerate(recs):
            assert abs(r["MinDVb"] - cm) >= 1e-3 * cm, (s, f, r["MinDVb"])
            if r["gap"] is not None:
                assert r["gap"] >= 1e-3, (s, f, r["gap"])
    for key in SC.outputs(case):
        for a, _ in SC.pairs(fit[key], fit[key]):
            assert np.all(np.isfinite(a)), key


SECOND_ROUND = ("ps_setup_trip_k3", "px_trace_cap_k3", "px_f70_k16", "px_f256_k3", "ps_overlap_long_k16", "pzs_inc_overlap_long_k3", "ps_weighted_k3",
                "ps_unobserved_level_k3")


def test_case_table_covers_what_the_gpu_tests_promise():
    import bwgr_amd
    ids = [c["id"] for c in SC.CASES]
    assert len(set(ids)) == len(ids) and set(SC.DISJOINT) <= set(ids) and set(SECOND_ROUND) <= set(ids) and set(SC.TRZSZ_ALONE) <= set(ids)
    ks, xfas, entries, qs, colmax = set(), set(), set(), set(), 0
    for c in SC.CASES:
        data = c["data"]()
        Y, effects = data[0], data[1]
        n, k = Y.shape
        ks.add(k); xfas.add(c["kw"].get("XFA", -1)); entries.add(c["entry"])
        # (the cases of the second round run fewer sweeps: their restatements are the wide and the long ones)
        assert (2 if c["id"] in SECOND_ROUND else 6) <= c["kw"]["maxit"] <= 8 and c["kw"]["logtol"] == SC.NOSTOP
        assert n % 64 != 0 and 0.15 < np.isnan(Y).mean() < 0.3 and np.isnan(Y).all(1).sum() >= 3
        sp = [e for e in effects if e[0] == "sparse"]
        assert sp and all(np.array_equal(SR.f32(e[1]), e[1]) for e in sp)
        assert (c["id"] in SC.DISJOINT) == all(SR.row_disjoint(e[1]) for e in sp)
        for e in sp:
            qs.add(e[1].shape[1]); colmax = max(colmax, int((e[1] != 0).sum(0).max()))
        first = sp[0][1]
        if first.shape[1] in (12, 70):              # a trait with no record on a whole (non-empty) level
            seen = (first != 0).T.astype(float) @ (~np.isnan(Y)).astype(float)
            assert ((seen == 0) & ((first != 0).sum(0) > 0)[:, None]).any(), c["id"]
    assert ks == {1, 3, 5, 16} and {-1, 0, 2} <= xfas and entries == {"PEGS_sparse", "PEGSZ_sparse", "PEGSZ", "PEGSX"}
    assert {1, 12, 70} <= qs and colmax > 1024
    trip = bwgr_amd.pegs_sparse_plan(SC.N, SC.TRIP_COLS + 37, SC.N, 2, 3, True)["trip_cols"]
    assert trip == SC.TRIP_COLS and max(qs) > trip                           # a q that takes two trips of the disjoint grid
    long_ = SC.design(SC.by_id("ps_long_cols_k3")["data"]()[1][0])
    assert long_.shape[0] == 2100 and sorted((long_ != 0).sum(0))[-2:] == [700, 1100] and ((long_ != 0).sum(0) > 64).sum() >= 3
    empty = SC.design(SC.by_id("ps_empty_col_k3")["data"]()[1][0])
    assert ((empty != 0).sum(0) == 0).sum() == 1
    A, stored = SC.by_id("ps_overlap_k3")["data"]()[1][0][1:]
    assert 0.06 < stored.mean() < 0.1 and (stored & (A == 0)).sum() > 0 and (A < 0).any()
    kinds = [[e[0] for e in c["data"]()[1]] for c in SC.CASES]
    assert ["panel", "sparse"] in kinds and ["panel", "sparse", "sparse", "dense"] in kinds and ["sparse", "sparse"] in kinds


def _ceil(a, b):
    return -(-a // b)


def _sparse_effect(cid, i=0):
    """(case, data, A, stored mask, the sparse plan) of effect i of a case"""
    import bwgr_amd
    case = SC.by_id(cid)
    data = case["data"]()
    e = data[1][i]
    A = e[1]
    stored = e[2] if len(e) > 2 else A != 0
    pl = bwgr_amd.pegs_sparse_plan(A.shape[0], A.shape[1], int(stored.sum()), int(stored.sum(0).max()), data[0].shape[1], SR.row_disjoint(A))
    return case, data, A, stored, pl


def test_second_round_cases_reach_what_they_are_listed_for():
    """Each case of the second round against the library's own host arithmetic (bwgr_debug_pegs_sparse_plan, bwgr_debug_pegs_launch_plan,
    bwgr_debug_pegsx_plan, bwgr_debug_launch_plan): a case that stops reaching its edge after a later plan change fails here.  The sparse trace
    kernel runs on the trace grid of the launch plan with ONE column per wave, four per workgroup and trip (csrc/pegs_sparse.hip.h)."""
    import bwgr_amd
    import tall_cases as tc
    # ps_setup_trip_k3: two trips of the set-up kernel, every column of the second occupied; three of k_mrr_tilde over d2; nine of the disjoint leg
    case, data, A, stored, pl = _sparse_effect("ps_setup_trip_k3")
    n, q = A.shape
    per_trip = pl["setup_wg"] * (pl["setup_threads"] // 64)
    assert (n, q) == (SC.N, SC.SETUP_TRIP_COLS + 37) and pl["setup_wg"] == 8192 and per_trip == SC.SETUP_TRIP_COLS and _ceil(q, per_trip) == 2
    assert (stored.sum(0)[per_trip:] == 1).all() and stored[:, q - 1].sum() == 1 and SR.row_disjoint(A) and stored.sum() == n
    rc, lp = tc.launch_plan(n, _ceil(n, 128) * 128, q, 3)
    assert rc == 0 and _ceil(q, lp["mrr_np"] * 256) == 3 and (stored.sum(0)[2 * lp["mrr_np"] * 256:] == 1).all()
    assert pl["leg"] == "disjoint" and pl["disjoint_wg"] == 1024 and _ceil(q, pl["trip_cols"]) == 9
    assert not set(np.flatnonzero(stored[:, q - 40:].any(1))) & {7, n // 2, n - 1}     # (the placed rows are none of those without any record)
    assert A.nbytes <= 100e6                                                           # (the dense copy of the legs test)
    # px_trace_cap_k3: the trace grid at its cap, five trips of 4 096 columns, the last workgroup of the last trip with one column
    case, data, A, stored, pl = _sparse_effect("px_trace_cap_k3")
    n, q = A.shape
    gp = bwgr_amd.pegs_launch_plan(n, q)
    assert q == 16501 and gp["trace_wg"] == 1024 and _ceil(q, gp["trace_wg"] * 4) == 5 and q % (gp["trace_wg"] * 4) == 117 and q % 4 == 1
    assert stored[:, q - 1].sum() == 1 and (stored.sum(0)[4 * 4096:] > 0).sum() >= 40 and data[2].shape[1] == 3 and case["id"] in SC.TRZSZ_ALONE
    assert pl["leg"] == "disjoint" and _ceil(q, pl["trip_cols"]) == 5 and pl["setup_wg"] == _ceil(q, 4)
    # px_f70_k16: a second step of the trace's lane loops, sixteen patterns, k = 16 on both legs
    case, data, A, stored, pl = _sparse_effect("px_f70_k16")
    Y, X = data[0], data[2]
    f, k = X.shape[1], Y.shape[1]
    xp = bwgr_amd.pegsx_plan(SC.N, f, k)
    assert (f, k) == (70, 16) and _ceil(f, 64) == 2 and len({np.isnan(Y[:, t]).tobytes() for t in range(k)}) == 16
    assert xp["trace_lds_bytes"] == 8 * (4 * xp["jc"] * f + 4 * 16) and np.array_equal(X, SR.f32(X)) and (X[:, 0] == 1).all()
    assert A.shape == (SC.N, 70) and pl["leg"] == "disjoint" and _sparse_effect("px_f70_k16", 1)[4]["leg"] == "serial"
    assert ((~np.isnan(Y)).sum(0) > f).all()
    # px_f256_k3: f at the cap, four steps, the whole of a wave's region of LDS; more records per trait than columns in X
    case, data, A, stored, pl = _sparse_effect("px_f256_k3")
    Y, X = data[0], data[2]
    xp = bwgr_amd.pegsx_plan(SC.N2, 256, 3)
    assert X.shape == (SC.N2, 256) == (700, 256) and _ceil(256, 64) == 4 and xp["trace_lds_bytes"] == 33280 <= 64 * 1024
    assert ((~np.isnan(Y)).sum(0) >= 256 + 200).all() and np.linalg.matrix_rank(X[~np.isnan(Y).any(1)]) == 256
    assert np.array_equal(X, tc.XC.fixed(SC.N2, 255, 501))                             # (as tall_cases' f256 job builds it)
    assert A.shape == (700, 12) and pl["leg"] == "disjoint" and _sparse_effect("px_f256_k3", 1)[4]["leg"] == "serial"
    assert _ceil(SC.N2, 256) == 3                                                      # (workgroups of k_pegs_sparse_hat)
    # ps_overlap_long_k16: every column three lane strides long, more columns than a wave has lanes, rows shared, k = 16
    case, data, A, stored, pl = _sparse_effect("ps_overlap_long_k16")
    assert A.shape == (700, 130) and stored.sum(0).min() > 128 and stored.sum(0).max() <= 256 and A.shape[1] > 64 and data[0].shape[1] == 16
    assert pl["leg"] == "serial" and (pl["serial_threads"], pl["serial_wg"]) == (64, 1) and case["kw"]["XFA"] == 2
    assert 0.2 < stored.mean() < 0.3 and (stored & (A == 0)).sum() == 7 and (A < 0).any()
    # consecutive columns share rows whose entries lie in different lane strides of the two columns
    r0, r1 = np.flatnonzero(stored[:, 0]), np.flatnonzero(stored[:, 1])
    both = np.intersect1d(r0, r1)
    assert any(np.searchsorted(r0, r) // 64 >= 1 and np.searchsorted(r0, r) % 64 != np.searchsorted(r1, r) % 64 for r in both)
    case2, data2, A2, stored2, pl2 = _sparse_effect("pzs_inc_overlap_long_k3", 1)
    assert np.array_equal(A2, A) and np.array_equal(stored2, stored) and data2[0].shape[1] == 3 and pl2["leg"] == "serial"
    assert data2[1][0][1].shape == (700, 12) and case2["entry"] == "PEGSZ_sparse"
    # ps_weighted_k3: row-disjoint, and no incidence
    case, data, A, stored, pl = _sparse_effect("ps_weighted_k3")
    v = A[stored]
    assert pl["leg"] == "disjoint" and SR.row_disjoint(A) and stored.sum(1).max() == 1 and A.shape == (SC.N, 12)
    assert (v < 0).sum() > 50 and (v == 0).sum() == 5 and (v != np.round(v)).sum() > 250 and np.array_equal(A, SR.f32(A))
    # ps_unobserved_level_k3: stored entries, and no record under them in any trait
    case, data, A, stored, pl = _sparse_effect("ps_unobserved_level_k3")
    j = SC.unobserved_column(A, data[0])
    assert list(np.flatnonzero(A[:, j])) == [7, SC.N // 2, SC.N - 1] and np.isnan(data[0][A[:, j] != 0]).all() and pl["leg"] == "disjoint"
    assert ((A != 0).sum(0) > 0).all() and len(data[1]) == 1


# ---- the plan hook ----

def test_plan_hook_is_host_arithmetic():
    import bwgr_amd
    from bwgr_amd import _lib
    src = open(os.path.join(ROOT, "include", "bwgr.h")).read()
    assert int(re.search(r"#define\s+BWGR_PEGS_SPARSE_PLAN_NOUT\s+(\d+)", src).group(1)) == 9
    # the trial of the issue: 20 000 levels on 100 000 plots
    big = bwgr_amd.pegs_sparse_plan(100000, 20000, 100000, 12, 4, True)
    assert big["ws_bytes"] < 100e6 and bwgr_amd.pegs_plan(100000, 20000, 4)["ws_bytes"] > 10e9
    assert big["leg"] == "disjoint" and big["disjoint_wg"] == 1024 and big["trip_cols"] == 4096 and big["setup_wg"] == 5000
    # proportional to nnz + q k^2, never to n q: doubling n adds the row pointers alone
    n2 = bwgr_amd.pegs_sparse_plan(200000, 20000, 100000, 12, 4, True)
    assert n2["ws_bytes"] - big["ws_bytes"] == 8 * 100000
    nz, q, k = 100000, 20000, 4
    assert big["ws_bytes"] == 2 * nz * 12 + 8 * (q + 1 + 100000 + 1) + 8 * (5 * q * k + q * k * k + 16) + 4 * q
    # the table's shapes
    for q, wg in ((1, 1), (12, 3), (70, 18), (SC.TRIP_COLS + 37, 1024)):
        for disjoint in (True, False):
            pl = bwgr_amd.pegs_sparse_plan(SC.N, q, min(SC.N, 2 ** 20), min(SC.N, 300), 3, disjoint)
            assert (pl["setup_threads"], pl["setup_wg"]) == (256, min((q + 3) // 4, 8192))
            assert (pl["serial_threads"], pl["serial_wg"]) == (64, 1)
            assert (pl["disjoint_threads"], pl["disjoint_wg"], pl["trip_cols"]) == (256, wg, 4 * wg)
            assert pl["leg"] == ("disjoint" if disjoint else "serial")
    L = _lib.lib()
    out = (C.c_int64 * 10)(*([-1] * 10))
    assert L.bwgr_debug_pegs_sparse_plan(300, 12, 300, 40, 3, 1, out) == 0 and out[9] == -1 and out[8] > 0
    for bad in ((0, 12, 300, 40, 3), (300, 0, 300, 40, 3), (300, 12, -1, 0, 3), (300, 12, 2 ** 31, 40, 3), (300, 12, 300, 301, 3), (300, 12, 10, 11, 3),
                (300, 12, 300, 40, 0), (300, 12, 300, 40, 17)):
        assert L.bwgr_debug_pegs_sparse_plan(*bad, 1, out) == 1 and b"pegs sparse plan" in L.bwgr_last_error()
    assert L.bwgr_debug_pegs_sparse_plan(300, 12, 300, 40, 3, 1, None) == 1


# ---- the surface ----

def test_entries_are_declared_exported_and_bound():
    from bwgr_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bwgr.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, nargs in (("bwgr_pegs_ex", 21), ("bwgr_pegsx_ex", 29), ("bwgr_debug_pegs_sparse_plan", 7)):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs
    m = re.search(r"typedef struct bwgr_pegs_effect_ex \{(.*?)\} bwgr_pegs_effect_ex;", hdr, re.S)
    fields = re.findall(r"\*?(\w+)\s*[,;]", m.group(1))
    assert fields == ["panel", "Z", "q", "ldz", "colptr", "rowidx", "val", "flags"]
    # the narrow struct and entries keep their layout
    assert re.search(r"typedef struct bwgr_pegs_effect \{ bwgr_panel \*panel; const double \*Z; int64_t q, ldz; \} bwgr_pegs_effect;", hdr)
    from bwgr_amd.api import _Eff
    assert [f[0] for f in _Eff._fields_] == fields and C.sizeof(_Eff) == 64
    L.bwgr_abi_version.restype = int
    assert L.bwgr_abi_version() == 1


def test_signatures_equal_the_reference():
    """R/RcppExports.R:292, 296"""
    import bwgr_amd as B
    E = inspect.Parameter.empty

    def pos(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]

    def kwonly(fn):
        return {p.name for p in inspect.signature(fn).parameters.values() if p.kind == inspect.Parameter.KEYWORD_ONLY}
    opts = [("maxit", 100), ("logtol", -4.0), ("covbend", 1.1), ("covMinEv", 10e-4), ("XFA", -1), ("NNC", True)]
    assert pos(B.PEGS_sparse) == [("Y", E), ("S", E)] + opts
    assert pos(B.PEGSZ_sparse) == [("Y", E), ("X_list", E)] + opts
    assert kwonly(B.PEGS_sparse) == kwonly(B.PEGSZ_sparse) == kwonly(B.PEGSZ) == {"device", "cnv_trace"}
    for name in ("PEGS_sparse", "PEGSZ_sparse", "sparse", "pegs_sparse_plan"):
        assert name in B.__all__ and hasattr(B, name)


def test_sparse_class():
    import bwgr_amd
    from bwgr_amd import sparse
    from bwgr_amd.api import _pegs_effect
    rng = np.random.default_rng(5)
    A = np.where(rng.random((9, 4)) < 0.4, rng.normal(size=(9, 4)), 0.0)
    A[:, 2] = 0.0                                            # an empty column
    a = sparse(A)
    b = sparse(SR.csc(A), shape=A.shape)
    for s in (a, b):
        assert s.shape == (9, 4) and s.data.dtype == np.float64 and s.indices.dtype == np.int32 and s.indptr.dtype == np.int64 and not s.serial
        assert s.indptr[0] == 0 and s.indptr[-1] == len(s.data) == np.count_nonzero(A) and s.indptr[2] == s.indptr[3]
        assert np.array_equal(s.data, SR.f32(s.data)) and np.array_equal(s.toarray(), SR.f32(A))     # rounded to float, once
    assert not np.array_equal(a.data, SR.csc(A)[0])
    for key in ("data", "indices", "indptr"):
        assert np.array_equal(getattr(a, key), getattr(b, key))
    assert sparse(a, serial=True).serial and np.array_equal(sparse(a).data, a.data)
    assert sparse(np.arange(3.0)).shape == (3, 1)
    E, own = _pegs_effect(a, {})
    assert E is a and not own
    with pytest.raises(bwgr_amd.BwgrError):
        sparse(SR.csc(A))                                    # no shape
    with pytest.raises(bwgr_amd.BwgrError):
        sparse(np.zeros((2, 2, 2)))
    with pytest.raises(bwgr_amd.BwgrError):
        sparse((np.ones(3), np.arange(3), np.array([0, 3])), shape=(4, 2))


def test_sparse_class_takes_scipy_matrices():
    sp = pytest.importorskip("scipy.sparse")
    from bwgr_amd import sparse
    from bwgr_amd.api import _pegs_effect
    rng = np.random.default_rng(6)
    A = np.where(rng.random((11, 5)) < 0.3, rng.normal(size=(11, 5)), 0.0)
    want = sparse(A)
    r, c = np.nonzero(A)
    dup = sp.coo_matrix((np.concatenate([A[r, c] * 0.25, A[r, c] * 0.75]), (np.concatenate([r, r]), np.concatenate([c, c]))), shape=A.shape)   # duplicates, unsorted
    for M in (sp.csc_matrix(A), sp.csr_matrix(A), sp.coo_matrix(A), dup):
        s = sparse(M)
        assert np.array_equal(s.indices, want.indices) and np.array_equal(s.indptr, want.indptr) and np.allclose(s.data, want.data, rtol=1e-6, atol=0)
        E, own = _pegs_effect(M, {})
        assert isinstance(E, sparse) and not own and E.shape == A.shape


# ---- refusals: none needs a device ----

def _csc_call(n, q, ptr, idx, val, Z=None, flags=0, k=2, text=1, entry="pegs"):
    """the C entry on one hand-made sparse effect -> (status, message)"""
    from bwgr_amd import _lib
    from bwgr_amd.api import _Eff
    L = _lib.lib()
    ptr, idx, val = np.asarray(ptr, np.int64), np.asarray(idx, np.int32), np.asarray(val, np.float64)
    ce = (_Eff * 1)()
    ce[0].colptr = ptr.ctypes.data; ce[0].rowidx = idx.ctypes.data if idx.size else 0; ce[0].val = val.ctypes.data if val.size else 0
    ce[0].q = q; ce[0].flags = flags
    if Z is not None:
        ce[0].Z = Z.ctypes.data; ce[0].ldz = n
    Y = np.asfortranarray(np.random.default_rng(3).normal(size=(n, k)))
    b = np.zeros((max(q, 1), k), order="F")
    bp = (C.c_void_p * 1)(b.ctypes.data)
    its = C.c_int()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    if entry == "pegs":
        rc = L.bwgr_pegs_ex(0, C.cast(ce, C.c_void_p), 1, dp(Y), n, k, 3, -4.0, 1.1, 1e-3, -1, 1, text, None, C.cast(bp, C.c_void_p), None, None, None, None, C.byref(its), None)
    else:
        X = np.asfortranarray(np.ones((n, 1)))
        rc = L.bwgr_pegsx_ex(0, C.cast(ce, C.c_void_p), 1, dp(X), n, 1, dp(Y), n, k, 3, -8.0, 1.1, 1e-3, 1.1, 0, 0, 3, 0, 0, None, None, C.cast(bp, C.c_void_p), None, None,
                             None, None, C.byref(its), None, None)
    return rc, L.bwgr_last_error().decode()


GOOD = dict(n=6, q=3, ptr=[0, 2, 3, 5], idx=[0, 3, 1, 2, 4], val=[1.0, 1.0, 1.0, 1.0, 1.0])
BAD = [
    ("q0", dict(q=0, ptr=[0]), "q = 0", None),
    ("ptr0", dict(ptr=[1, 2, 3, 5]), "colptr[0] is not 0", "column 0"),
    ("ptr_decreases", dict(ptr=[0, 2, 1, 5]), "colptr decreases", "column 1"),
    ("nnz", dict(q=1, ptr=[0, 2 ** 31]), "2^31 - 1", "column 1"),
    ("row_n", dict(idx=[0, 3, 1, 2, 6]), "outside [0, n)", "column 2, entry 4"),
    ("row_negative", dict(idx=[0, 3, -1, 2, 4]), "outside [0, n)", "column 1, entry 2"),
    ("duplicate", dict(idx=[3, 3, 1, 2, 4]), "strictly increase", "column 0, entry 1"),
    ("unsorted", dict(idx=[0, 3, 1, 4, 2]), "strictly increase", "column 2, entry 4"),
    ("nan", dict(val=[1.0, 1.0, np.nan, 1.0, 1.0]), "not finite", "column 1, entry 2"),
    ("inf", dict(val=[1.0, 1.0, 1.0, 1.0, np.inf]), "not finite", "column 2, entry 4"),
]


@pytest.mark.parametrize("entry", ["pegs", "pegsx"])
@pytest.mark.parametrize("name,change,why,where", BAD, ids=[b[0] for b in BAD])
def test_refusals_name_the_effect_the_column_and_the_entry(entry, name, change, why, where):
    rc, msg = _csc_call(entry=entry, **dict(GOOD, **change))
    assert rc == 1 and msg.startswith(entry + ":") and "effect 0" in msg and why in msg, msg
    if where:
        assert where in msg, msg


def test_other_refusals_and_what_is_not_refused():
    import bwgr_amd
    rc, msg = _csc_call(Z=np.zeros((6, 3), order="F"), **GOOD)
    assert rc == 1 and "both Z and colptr" in msg and "effect 0" in msg
    rc, msg = _csc_call(text=3, **GOOD)
    assert rc == 1 and "text = 3" in msg
    rc, msg = _csc_call(**dict(GOOD, idx=[], val=[]))
    assert rc == 1 and "null pointer" in msg
    if bwgr_amd.device_count() == 0:
        # a valid matrix, an empty column, a stored zero, the serial flag: past every check, to the device
        for change in (dict(), dict(ptr=[0, 2, 2, 4], idx=[0, 3, 2, 4], val=[1.0, 1.0, 1.0, 1.0]), dict(val=[1.0, 0.0, 1.0, 1.0, -2.5]), dict(flags=1)):
            for entry in ("pegs", "pegsx"):
                rc, msg = _csc_call(entry=entry, **dict(GOOD, **change))
                assert rc == 5, (change, msg)       # BWGR_ENODEV
        A = np.zeros((8, 3))
        A[np.arange(8), np.arange(8) % 3] = 1.0
        Y = np.random.default_rng(1).normal(size=(8, 2))
        for call in (lambda: bwgr_amd.PEGS_sparse(Y, A), lambda: bwgr_amd.PEGSZ_sparse(Y, [A, bwgr_amd.sparse(A)]),
                     lambda: bwgr_amd.PEGSZ(Y, [bwgr_amd.sparse(A), bwgr_amd.dense(np.random.default_rng(2).normal(size=(8, 2)))]),
                     lambda: bwgr_amd.PEGSX(Y, np.ones((8, 1)), [bwgr_amd.sparse(A)])):
            with pytest.raises(bwgr_amd.BwgrError) as ei:
                call()
            assert ei.value.code == 5
    # the Python face passes the engine's refusal on
    bad = bwgr_amd.sparse((np.ones(3), np.array([0, 2, 1]), np.array([0, 3])), shape=(4, 1))
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.PEGS_sparse(np.random.default_rng(1).normal(size=(4, 2)), bad)
    assert ei.value.code == 1 and "strictly increase" in str(ei.value) and "column 0, entry 2" in str(ei.value)
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.PEGSZ(np.zeros((5, 2)), [bwgr_amd.sparse(np.eye(4))])
    assert ei.value.code == 1 and "nrow" in str(ei.value)
