"""CPU: tests/ld_linalg.py against numpy and against its own residuals in long double; then the yardstick of tests/test_gpu_mt_tight.py
(tests/mt_tight.py) on every case of tests/mt_tight_cases.py: it is finite, it puts the bound on the coefficients at least five orders below the
suite's 1e-6, and it bites: the restatement with one float temporary in the step's dependent dot x_J'e -- what a float partial sum in a
kernel's dot does -- lands at least a hundred bounds away, on every effect's coefficients.  The decisions of a fit (mrr's bending; PEGS's
inflation, truncation and clamp) are the same in the long double run and the nine float64 runs and none is near its threshold, and the cases
reach the regimes, trips, patterns, code ranges and kappa they are there for.  Every yardstick and ratio is printed.

PEGSX has two more mutants: a float in the fixed step's M_t'e_t, which must move b or the first effect's u (whichever it moves by more
bounds) a hundred bounds away, and a float in the trace's M_g'z_j, which must do so to every effect's TrZSZ wherever X has a non-integer
column (beside an intercept alone the sums are integers below 2^24 and the float is exact).  Its other decisions -- the rank of every M'M,
the floors -- are held as the tail's are.  Last, the float64 restatements of PEGS, PEGSZ, PEGSZ_sparse and PEGSX return the bits they
returned before they learnt long double, and the 49 cases that were here before keep their bounds bit for bit."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ld_linalg as LL  # noqa: E402
import mrr_cases  # noqa: E402
import mt_tight as T  # noqa: E402
import mt_tight_cases as TC  # noqa: E402
import restatement_fields as RF  # noqa: E402

LD = T.LD
B_BOUND = 1e-11     # the bound on b must not exceed this: a condition on the inputs
# ... but for the cases whose k x k tail is ill-conditioned by design, held to 1e-9 (at most three)
B_BOUND_LOOSE = {"mrr/bending": 1e-9}
BITE = 100          # the mutant moves b by at least this many bounds


# ---- tests/ld_linalg.py ----
def _sym(kind, k, seed, dtype):
    """Q diag(w) Q' with Q orthogonal to float64 rounding: spd (w in 0.5 .. 2), deficient (the same with the smaller half of w zero; k = 1:
    the zero matrix) and indefinite (w in +-(0.5 .. 2), both signs where k > 1)"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.normal(size=(k, k)))[0]
    w = rng.uniform(0.5, 2.0, k)
    if kind == "deficient":
        w[:(k + 1) // 2] = 0
    elif kind == "indefinite":
        w[::2] *= -1
    A = (np.asarray(Q, dtype) * np.asarray(w, dtype)) @ np.asarray(Q, dtype).T
    return (A + A.T) / 2


KS = (1, 2, 5, 16)
KINDS = ("spd", "deficient", "indefinite")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", KINDS)
def test_ld_linalg_agrees_with_numpy_at_float64(kind, k):
    A = _sym(kind, k, 10 * k + len(kind), np.float64)
    eps, norm = 2.0 ** -52, max(np.abs(np.linalg.eigvalsh(A)).max(), 1e-300)
    w, V = LL.eigh(A)
    assert w.dtype == np.float64 and np.all(np.diff(w) >= 0)
    assert np.abs(w - np.linalg.eigvalsh(A)).max() <= 8 * k * eps * norm          # eigenvalues of a symmetric matrix: condition 1
    assert np.array_equal(LL.eigvalsh(A), w)
    assert np.abs(V.T @ V - np.eye(k)).max() <= 8 * k * eps
    P, Pn = LL.pinv(A), np.linalg.pinv(A, hermitian=True)
    assert np.linalg.matrix_rank(A, hermitian=True) == (k // 2 if kind == "deficient" else k) == np.sum(np.abs(w) > LL.RCOND * np.abs(w).max())
    cond = 4.0                                                                    # w in 0.5 .. 2 on the range
    assert np.abs(P - Pn).max() <= 8 * k * eps * cond * max(np.abs(Pn).max(), 1e-300)
    if kind == "spd":
        B = np.random.default_rng(k).normal(size=(k, 3))
        for got, want in ((LL.solve(A, B), np.linalg.solve(A, B)), (LL.solve(A, B[:, 0]), np.linalg.solve(A, B[:, 0])), (LL.inv(A), np.linalg.inv(A))):
            assert got.dtype == np.float64 and got.shape == want.shape
            assert np.abs(got - want).max() <= 8 * k * eps * cond * np.abs(want).max()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", KINDS)
def test_ld_linalg_residuals_at_long_double(kind, k):
    """|A x - b|, |V'AV - diag(w)| and |A A+ A - A| (largest entry) below k 2^-63 |A| (spectral norm), the residuals formed in long double; the
    solve's right-hand side is A x0 with max |x0| = 1, so that the bound needs no factor |x|"""
    A = _sym(kind, k, 10 * k + len(kind), LD)
    assert A.dtype == LD
    w, V = LL.eigh(A)
    assert w.dtype == LD and V.dtype == LD and np.all(np.diff(w) >= 0)
    norm = np.abs(w).max()
    tol = k * LD(2) ** -63 * norm
    print(kind, k, "eigh %.1e" % float(np.abs(V.T @ A @ V - np.diag(w)).max() / max(tol, np.finfo(LD).tiny)), end=" ")
    assert np.abs(V.T @ A @ V - np.diag(w)).max() <= tol
    assert np.abs(V.T @ V - np.eye(k)).max() <= k * LD(2) ** -63
    P = LL.pinv(A)
    assert P.dtype == LD
    print("pinv %.1e" % float(np.abs(A @ P @ A - A).max() / max(tol, np.finfo(LD).tiny)), end=" ")
    assert np.abs(A @ P @ A - A).max() <= tol
    if kind == "spd":
        x0 = np.asarray(np.random.default_rng(k).uniform(-1, 1, size=(k, 2)), LD)
        x0[0] = 1
        b = A @ x0
        x = LL.solve(A, b)
        assert x.dtype == LD
        print("solve %.1e" % float(np.abs(A @ x - b).max() / tol), end=" ")
        assert np.abs(A @ x - b).max() <= tol
        assert np.abs(A @ LL.inv(A) - np.eye(k)).max() <= tol * 4 / norm           # |A^-1| <= 2: the same bound with |x| = 2, and |A| >= 1/2
    print()


def test_ld_linalg_solves_a_batch_as_it_solves_each():
    rng = np.random.default_rng(3)
    A = np.stack([_sym("spd", 5, s, LD) for s in range(7)])
    B = np.asarray(rng.normal(size=(7, 5)), LD)
    X, I = LL.solve(A, B), LL.inv(A)
    assert X.shape == (7, 5) and I.shape == (7, 5, 5) and X.dtype == LD and I.dtype == LD
    for m in range(7):
        assert np.array_equal(X[m], LL.solve(A[m], B[m])) and np.array_equal(I[m], LL.inv(A[m]))
    assert np.isnan(LL.cholesky(_sym("indefinite", 5, 1, LD))).any()     # not positive definite: NaN, never a silent answer


# ---- the yardstick on every case ----
def _mutant(c, i):
    return T.float_dot if "effects" not in c else [T.float_dot if f == i else None for f in range(len(c["effects"]))]


def _bites(name, what, key, moved, bound):
    print(name, key, "%s %.2e, bound %.2e, ratio %.0f" % (what, moved, bound[key], moved / bound[key]))
    assert moved >= BITE * bound[key], (what, key, moved, bound[key])


@pytest.mark.parametrize("name", TC.NAMES)
def test_yardstick_is_finite_tight_and_bites(name):
    c = TC.case(name)
    o, yard, bound = T.ref(name), T.yard(name), T.bound(name)
    print(name, "kappa %.2f" % T.kappa(c), {key: "%.1e" % v for key, v in yard.items()})
    for key in T.keys(c):
        assert np.isfinite(yard[key]) and np.isfinite(bound[key]) and bound[key] >= T.FLOOR, (key, yard[key])
    for key in T.b_keys(c):
        assert bound[key] <= B_BOUND_LOOSE.get(name, B_BOUND), (key, bound[key])
    for i, key in enumerate(k for k in T.b_keys(c) if c["family"] != "pegsx" or k != "b"):      # the step's dot, once per effect
        _bites(name, "mutant", key, T.errs(name, T.run(name, dot=_mutant(c, i)), o)[key], bound)
    if c["family"] == "pegsx":
        e = T.errs(name, T.run(name, fixed_dot=T.float_tdot), o)
        print(name, "fixed_dot moves b by %.0f bounds and u0 by %.0f" % (e["b"] / bound["b"], e["u0"] / bound["u0"]))
        key = max(("b", "u0"), key=lambda key: e[key] / bound[key])
        _bites(name, "fixed_dot", key, e[key], bound)
        e = T.errs(name, T.run(name, trace_dot=T.float_tdot), o)
        X32 = T.f32(c["X"])
        for r in range(len(c["effects"])):
            if np.any(X32 != np.rint(X32)):
                _bites(name, "trace_dot", "TrZSZ%d" % r, e["TrZSZ%d" % r], bound)
            else:
                print(name, "TrZSZ%d" % r, "trace_dot %.2e beside integer columns alone" % e["TrZSZ%d" % r])


def test_no_more_than_three_cases_have_the_looser_bound_on_b():
    assert len(B_BOUND_LOOSE) <= 3 and set(B_BOUND_LOOSE) <= set(TC.NAMES) and all(v <= 1e-9 for v in B_BOUND_LOOSE.values())


def test_a_long_double_run_leaves_nothing_in_float64():
    for name in ("mrr/k7_npat7", "mrr/tpod_k3_float", "mrr/opt_ACS", "mrr/opt_TH", "mrr/opt_updateMu", "mrr/bending", "dense/r65", "pegs/k5_inflated",
                 "pegsz/panel_dense5", "pegs/xfa2", "pegsx/f17", "pegsx/mixed4", "pegsx/nnc", "pegsx/xfa1", "pegsx/rank_deficient", "sparse/ps_q12",
                 "sparse/pzs_two_inc", "sparse/pz_panel_inc"):
        c, o = TC.case(name), T.ref(name)
        for key in T.keys(c):
            if key != "hat_own":
                assert np.asarray(o[key]).dtype == LD, (name, key)
        for sweep in o["dec"]:                      # ... nor on the way: every sweep's eigenvalues, gaps and margins as the tail made them
            for v in (sweep if "effects" not in c else [v for rec in sweep for v in rec]):
                assert isinstance(v, (LD, bool, np.bool_, type(None))), (name, type(v))
        for _, kept, dropped in o.get("mm", ()):
            assert isinstance(kept, LD) and isinstance(dropped, (LD, int)), (name, type(kept), type(dropped))
    # the start values and the sweep's own arrays, as the restatements' traces hold them
    c = TC.case("mrr/k7_npat7")
    r = T.MR.mrr(c["Y"], c["X"], trace=True, dtype=LD, orders=T.orders("mrr/k7_npat7"), **c["kw"])
    for t in r["trace"]:
        for key in ("e", "y", "Z", "Xc", "b", "ve_sweep", "iG_sweep", "mu"):
            assert t[key].dtype == LD, key
    c = TC.case("pegsz/panel_dense5")
    r = T.PR.pegsz(c["Y"], T.designs(c), trace=True, dtype=LD, orders=T.orders("pegsz/panel_dense5"), **c["kw"])
    for key, v in r["start"].items():
        assert np.asarray(v).dtype == LD, key
    for recs in r["trace"]:
        for rec in recs:
            for key in ("TH", "vb", "iG", "inflate"):
                assert np.asarray(rec[key]).dtype == LD, key
        for key in ("ey", "se", "d", "ve", "cnv", "mu"):
            assert np.asarray(recs[0][key]).dtype == LD, key
        assert all(isinstance(v, LD) for v in recs[0]["db2"])
    c = TC.case("pegsx/mixed4")
    r = T.XR.pegsx(c["Y"], c["X"], T.designs(c), trace=True, dtype=LD, orders=T.orders("pegsx/mixed4"), **c["kw"])
    for key in ("nt", "ssy", "Tr", "ve"):
        assert np.asarray(r["start"][key]).dtype == LD, key
    for key in ("iXX", "b0", "y", "Y", "X"):
        assert np.asarray(r["setup"][key]).dtype == LD, key
    assert all(m[key].dtype == LD for m in r["mm"] for key in ("kept", "dropped")) and all(v.dtype == LD for v in r["start"]["vb"])
    for recs in r["trace"]:
        for rec in recs:
            for key in ("TH", "vb", "iG", "inflate", "MinDVb", "maxEv"):
                assert np.asarray(rec[key]).dtype == LD, key
        for key in ("ey", "ve", "cnv"):
            assert np.asarray(recs[0][key]).dtype == LD, key
        assert all(isinstance(v, LD) for v in recs[0]["db2"])
    for key in ("TrZSZ", "u", "vb_list", "GC_list"):
        assert all(v.dtype == LD for v in r[key]), key
    assert all(np.asarray(r[key]).dtype == LD for key in ("b", "ve", "hat", "cnv", "bend", "cnv_trace"))


@pytest.mark.parametrize("name", TC.NAMES)
def test_decisions_are_the_same_in_all_ten_runs_and_away_from_their_thresholds(name):
    c, o = TC.case(name), T.ref(name)
    decs = [o["dec"]] + [r[1] for r in T.runs(name)]
    assert len(decs) == 1 + T.NRUNS and all(len(d) == o["its"] for d in decs)
    if "effects" not in c:
        print(name, [(bool(b), "%.2e" % float(lam)) for b, lam in o["dec"]])
        for d in decs:
            assert [b for b, _ in d] == [b for b, _ in o["dec"]]
            assert all(abs(lam) >= 1e-6 for _, lam in d), [float(lam) for _, lam in d]
        return
    k, kw = c["Y"].shape[1], c["kw"]
    XFA, covMinEv = kw.get("XFA", -1), float(np.float32(kw.get("covMinEv", 10e-4)))
    NNC = kw.get("NNC", True)
    if c["family"] == "pegsx":       # XFA is a switch there and NumXFA the count of factors; NNC is off unless asked for
        XFA, NNC = (min(kw.get("NumXFA", 3), k) if kw.get("XFA", False) and kw.get("NumXFA", 3) > 0 else k), kw.get("NNC", False)
        mms = [o["mm"]] + [r[2]["mm"] for r in T.runs(name)]
        print(name, "M'M: kept %s, smallest kept ratio %.1e, largest dropped %.1e" % ([m[0] for m in o["mm"]], min(m[1] for mm in mms for m in mm),
                                                                                      max(m[2] for mm in mms for m in mm)))
        for mm in mms:
            assert [m[0] for m in mm] == [m[0] for m in o["mm"]]
            assert all(m[0] >= 1 and m[1] >= 1e-3 and m[2] <= 1e-10 for m in mm), mm
        assert not o["floors"] and not any(r[2]["floors"] for r in T.runs(name))
    print(name, [["%d MinDVb %.2e maxEv %.2e gap %s near0 %s" % ((r[0], r[1], r[2]) + tuple(v if v is None else "%.1e" % v for v in r[3:])) for r in recs]
                 for recs in o["dec"]])
    for d in decs:
        assert [[r[0] for r in recs] for recs in d] == [[r[0] for r in recs] for recs in o["dec"]]
        for recs in d:
            for inflated, MinDVb, maxEv, gap, near0 in recs:
                assert abs(MinDVb - covMinEv) >= 1e-6 * maxEv, (MinDVb, covMinEv, maxEv)
                if 0 < XFA < k:
                    assert gap >= 1e-6, gap
                else:
                    assert gap is None or XFA == k, gap
                if NNC:
                    assert near0 >= 1e-9, near0
                else:
                    assert near0 is None


def _npat(Y):
    return len({np.isnan(Y[:, t]).tobytes() for t in range(Y.shape[1])})


def test_case_preconditions():
    import bwgr_amd
    import tall_cases
    # the panels: code ranges and kappa
    for pname, X in (("panel132", TC.panel132()), ("tpod", TC.tpod()), ("rows2200", TC.rows2200())) + tuple(("tpod_p%d" % p, TC.tpod()[:, :p]) for p in (1, 63, 64, 65)):
        assert pname in TC.ORDINARY_012 and X.min() == 0 and X.max() == 2 and TC.kappa(X) < 4, (pname, TC.kappa(X))
    for name in TC.NAMES:
        c = TC.case(name)
        if c["family"] == "mrr" and c["panel"] not in TC.ORDINARY_012:
            assert c["panel"] in ("wide_freq", "signed132", "full_range"), c["panel"]
        print(name, "kappa %.2f" % T.kappa(c))
    assert TC.panel132().shape == (700, 132) and tall_cases._panel_plan(700, 132, 0, 3)["ld"] // 64 == 12
    assert 20 < TC.kappa(TC.wide_freq()) < 40 and TC.wide_freq().min() == 0 and TC.wide_freq().max() == 2
    assert TC.signed132().min() == -1 and TC.signed132().max() == 1
    assert TC.full_range().min() == -128 and TC.full_range().max() == 127 and TC.full_range().shape == (300, 200)
    assert T.kappa(TC.case("dense/r65")) == 1 and T.kappa(TC.case("pegs/k3")) == 1
    # k_mrr_solve's regimes
    for (k, npat), regime in TC.REGIMES.items():
        c = TC.case("mrr/k%d_npat%d" % (k, npat))
        rc, linv, ngl, _, _ = mrr_cases.plan(k, npat)
        assert rc == 0 and mrr_cases.regime(linv, ngl, npat) == regime and c["Y"].shape == (700, k) and _npat(c["Y"]) == npat, (k, npat)
        assert c["kw"]["maxit"] == 3 and c["panel_kw"] == dict(nwg=3)
    assert sorted(TC.REGIMES.values()) == [1, 2, 2, 3, 4, 5]
    for i, (k, npat) in enumerate(((8, 3), (16, 10))):
        Y = TC.case("mrr/shared_k%d" % k)["Y"]
        assert Y.shape[1] == k and _npat(Y) == npat == len(set(mrr_cases.SHARED[i]))
    # the tile loop's second trip: 32 pass workgroups
    ld = tall_cases._panel_plan(2200, 68, 0, 0)["ld"]
    assert ld // 64 > 32, ld
    c = TC.case("mrr/awkward_rows")
    assert np.isnan(c["Y"][list(TC.ALL_MISSING)]).all() and np.sum(~np.isnan(c["Y"][:, 5])) == 5 and _npat(c["Y"]) == 4
    assert len({r // 256 for r in TC.FIVE_ROWS}) == 3
    assert any(b for b, _ in T.ref("mrr/bending")["dec"])
    # the stopping case: it stops by its tolerance, and no sweep's cnvB lies within 0.02 of log10(tol) in any of the ten runs -- all of which
    # ran the same number of sweeps (mt_tight.errs), so the last entry is the one below log10(tol)
    o = T.ref("mrr/stopping")
    assert 3 < o["its"] < 500 and len(T.runs("mrr/stopping")) == T.NRUNS
    c = TC.case("mrr/stopping")
    logtol = np.log10(TC.STOP_TOL)
    for pm in T.perms(c["Y"].shape[0]):
        r = T.run("mrr/stopping", perm=pm)
        near = min(abs(float(v) - logtol) for v in r["cnvB"])
        assert near >= 0.02 and r["its"] == o["its"] and r["cnvB"][-1] < logtol, near
    assert min(abs(float(v) - logtol) for v in o["cnvB"]) >= 0.02
    # the dense train: blocks, trips, patterns
    for r, (nblk, edge) in {1: (1, 1), 63: (1, 63), 64: (1, 64), 65: (2, 1), 132: (3, 4)}.items():
        c = TC.case("dense/r%d" % r)
        pl = bwgr_amd.mrr_dense_plan(200, r, 4, _npat(c["Y"]))
        assert (pl["nblk"], pl["edge"], pl["trips"]) == (nblk, edge, 1) and c["X"].shape == (200, r), (r, pl)
    c = TC.case("dense/k16")
    assert c["Y"].shape[1] == 16 and _npat(c["Y"]) == 16
    c = TC.case("dense/rows2200")
    pl = bwgr_amd.mrr_dense_plan(2200, 65, 4, _npat(c["Y"]))
    assert pl["tiles"] == 36 > pl["pass_wg"] == 32 and pl["trips"] == 2, pl
    c = TC.case("dense/mkr_grm150")
    assert c["X"].shape == (150, 149) and c["K"].shape == (150, 150) and np.array_equal(c["X"], c["X"].astype(np.float32).astype(np.float64))
    assert TC.case("dense/device").get("device") is True
    # PEGS: k = 5 inflates in every sweep; the dense effects' widths
    assert all(r[0] for recs in T.ref("pegs/k5_inflated")["dec"] for r in recs)
    for q in (1, 5, 70):
        assert [D.shape for D in T.designs(TC.case("pegsz/panel_dense%d" % q))] == [(700, 132), (700, q)]
    assert TC.case("pegs/k16")["Y"].shape[1] == 16 and _npat(TC.case("pegs/k16")["Y"]) == 5


# ---- PEGSX and the sparse legs: what each case is there for, from the library's host-only plan hooks ----
def _ceil(a, b):
    return -(-a // b)


def _sparse_plan(c, e):
    import bwgr_amd
    A = e[1]
    stored = (A != 0) if len(e) < 3 else np.asarray(e[2])
    return bwgr_amd.pegs_sparse_plan(A.shape[0], A.shape[1], int(stored.sum()), int(stored.sum(0).max()), c["Y"].shape[1], T.SR.row_disjoint(A)), stored


def test_pegsx_and_sparse_case_preconditions():
    import bwgr_amd
    px = {name: TC.case(name) for name in TC.NAMES if name.startswith("pegsx/")}
    sp = {name: TC.case(name) for name in TC.NAMES if name.startswith("sparse/")}
    assert len(px) == 17 and len(sp) == 14 and len(TC.OLD_NAMES) == 49 and TC.NAMES[:49] == TC.OLD_NAMES
    for name, c in list(px.items()) + list(sp.items()):
        assert c["kw"]["logtol"] == TC.PC.NOSTOP and 2 <= c["kw"]["maxit"] <= 6 and T.kappa(c) == 1, name
        assert T.ref(name)["its"] == c["kw"]["maxit"], name
    # f: the tiles of PEGSX_FC columns, the waves of the fixed step's column loop, the lanes of the quadratic form
    shape = lambda c: (c["Y"].shape[0], c["X"].shape[1], c["Y"].shape[1])
    assert [shape(px["pegsx/f%s" % f])[1] for f in (1, 3, 17, "70_k5_inflated")] == [1, 3, 17, 70]
    for name, c in px.items():
        n, f, k = shape(c)
        assert f <= 70 and c["X"].shape[0] == n and np.all(c["X"][:, 0] == 1.0), name
        pl = bwgr_amd.pegsx_plan(n, f, k)
        assert pl["threads"] == min(_ceil(n, 64) * 64, 1024) and pl["jc"] == 4 and pl["fc"] == 4, (name, pl)
        assert f % pl["fc"] != 0, (name, f)                     # every f here ends on a partial tile of X's columns
    pl = bwgr_amd.pegsx_plan(*shape(px["pegsx/f17"]))
    assert 17 > pl["threads"] // 64 == 11                       # more columns than the fixed step has waves: its column loop wraps
    assert 70 > 64 > 17                                         # ... and the 64-lane loops of the quadratic form wrap at f = 70 alone
    assert shape(px["pegsx/k1"])[2] == 1 and shape(px["pegsx/k16_shared"])[2] == 16 and _npat(px["pegsx/k16_shared"]["Y"]) == 5
    assert shape(px["pegsx/f70_k5_inflated"])[2] == 5 and _npat(px["pegsx/f70_k5_inflated"]["Y"]) == 5
    assert all(r[0] for recs in T.ref("pegsx/f70_k5_inflated")["dec"] for r in recs)
    # the panel in three slabs; signed codes
    for name in ("pegsx/f1", "pegsx/f3", "pegsx/f17", "pegsx/f70_k5_inflated", "pegsx/k16_shared", "pegsx/quad_missing"):
        e = px[name]["effects"][0]
        assert e[0] == "panel" and e[1].shape == (700, 132) and e[2] == dict(nwg=3) and 132 % 4 == 0, name
    Z = px["pegsx/signed"]["effects"][0][1]
    assert Z.dtype == np.int8 and Z.min() == -1 and Z.max() == 1
    # the kinds of effect, each first in a list once, and the partial PEGSX_JC groups of the dense ones
    kinds = {name: [e[0] for e in c["effects"]] for name, c in px.items()}
    assert kinds["pegsx/panel_dense1"] == ["panel", "dense"] and kinds["pegsx/dense5_panel"] == ["dense", "panel"] and kinds["pegsx/dense70_n1501"] == ["dense"]
    assert kinds["pegsx/inc12"] == ["sparse"] and kinds["pegsx/mixed4"] == ["panel", "sparse", "sparse", "dense"]
    qs = {name: [e[1].shape[1] for e in c["effects"] if e[0] == "dense"] for name, c in px.items()}
    assert (qs["pegsx/panel_dense1"], qs["pegsx/dense5_panel"], qs["pegsx/dense70_n1501"], qs["pegsx/mixed4"]) == ([1], [5], [70], [9])
    assert all(q % 4 != 0 for q in (1, 5, 70, 9)) and 376 % 4 == 0
    inc, ovl = px["pegsx/mixed4"]["effects"][1:3]
    assert _sparse_plan(px["pegsx/mixed4"], inc)[0]["leg"] == "disjoint" and _sparse_plan(px["pegsx/mixed4"], ovl)[0]["leg"] == "serial"
    assert px["pegsx/inc12"]["effects"][0][1].shape == (300, 12) and _sparse_plan(px["pegsx/inc12"], px["pegsx/inc12"]["effects"][0])[0]["leg"] == "disjoint"
    # n no multiple of 4, and a second row trip of the fixed step
    c = px["pegsx/dense70_n1501"]
    n, f, k = shape(c)
    assert (n, f) == (TC.N1501, 3) and n % 4 == 1 and _ceil(n, bwgr_amd.pegsx_plan(n, f, k)["threads"]) == 2
    assert bwgr_amd.pegs_launch_plan(n, 70)["fixed_threads"] == 1024
    # whole aligned quads of rows without a record: in one pattern (the others have records there), and in every pattern
    Y = px["pegsx/quad_missing"]["Y"]
    a, b = TC.QUAD_ONE
    assert a % 4 == 0 and b - a == 4 and np.isnan(Y[a:b, 1]).all() and (~np.isnan(Y[a:b, [0, 2]])).any(0).all() and _npat(Y) == 3
    a, b = TC.QUAD_ALL
    assert a % 4 == 0 and (b - a) % 4 == 0 and np.isnan(Y[a:b]).all()
    # the options
    assert px["pegsx/nnc"]["kw"]["NNC"] is True and all(r[4] is not None for recs in T.ref("pegsx/nnc")["dec"] for r in recs)
    assert px["pegsx/xfa1"]["kw"]["NumXFA"] == 1 < shape(px["pegsx/xfa1"])[2] and all(r[3] is not None for recs in T.ref("pegsx/xfa1")["dec"] for r in recs)
    assert px["pegsx/df0_20"]["kw"]["df0"] == 20.0
    X = px["pegsx/rank_deficient"]["X"]
    assert np.array_equal(X[:, 1] + X[:, 2], X[:, 0]) and [m[0] for m in T.ref("pegsx/rank_deficient")["mm"]] == [X.shape[1] - 1] * 3
    assert all(m[0] == shape(c)[1] for name, c in px.items() if name != "pegsx/rank_deficient" for m in T.ref(name)["mm"])
    # the sparse legs
    legs = {}
    for name, c in sp.items():
        for e in c["effects"]:
            if e[0] == "sparse":
                legs.setdefault(name, []).append(_sparse_plan(c, e)[0]["leg"])
    assert legs.pop("sparse/ps_overlap_serial_leg") == ["serial"] and all(v == ["disjoint"] * len(v) for v in legs.values()), legs
    assert sp["sparse/ps_q12_forced_serial"]["serial"] is True and not any(c["serial"] for name, c in sp.items() if name != "sparse/ps_q12_forced_serial")
    assert np.array_equal(sp["sparse/ps_q12_forced_serial"]["effects"][0][1], sp["sparse/ps_q12"]["effects"][0][1])
    assert [sp["sparse/ps_q%d" % q]["effects"][0][1].shape for q in (1, 12, 70)] == [(300, 1), (300, 12), (300, 70)]
    assert [sp["sparse/ps_q12_k%d" % k]["Y"].shape[1] for k in (1, 5, 16)] == [1, 5, 16]
    assert ((sp["sparse/ps_empty_col"]["effects"][0][1] != 0).sum(0) == 0).sum() == 1
    A = sp["sparse/ps_long_cols"]["effects"][0][1]
    assert A.shape == (2100, 4) and sorted((A != 0).sum(0)) == [50, 250, 700, 1100] and _ceil(1100, 64) == 18
    A, stored = sp["sparse/ps_overlap_serial_leg"]["effects"][0][1:3]
    assert (A < 0).any() and (stored & (A == 0)).sum() == 7
    A, stored = sp["sparse/ps_weighted"]["effects"][0][1:3]
    assert T.SR.row_disjoint(A) and (A < 0).any() and np.any(A != np.rint(A)) and np.array_equal(A, T.f32(A))
    assert [sp["sparse/pzs_two_inc"]["entry"]] + [e[0] for e in sp["sparse/pzs_two_inc"]["effects"]] == ["PEGSZ_sparse", "sparse", "sparse"]
    assert [sp["sparse/pz_panel_inc"]["entry"]] + [e[0] for e in sp["sparse/pz_panel_inc"]["effects"]] == ["PEGSZ", "panel", "sparse"]
    c = sp["sparse/ps_q4133"]
    pl = _sparse_plan(c, c["effects"][0])[0]
    assert c["effects"][0][1].shape[1] == 4133 and pl["trip_cols"] == 4096 and _ceil(4133, pl["trip_cols"]) == 2 and c["kw"]["maxit"] == 2


# ---- the float64 restatements return the bits of the commit before this yardstick reached them ----
# what PEGSZ_sparse's fit has gained by becoming a call of pegsz with its trace (and "start"); a PEGSX record has gained near0
ADDED_TEXT2 = ("TH", "vb", "iG", "inflate", "ey", "se", "db2", "d", "ve", "cnv", "mu")


def _is_new(path, text2_ids, pegsx_ids):
    """whether the field <cases module>/<case id>/<key>/... (a trace's: .../trace/<sweep>/<effect>/<key>) is one the parent's fit lacks"""
    part = path.split("/")
    if tuple(part[:2]) in text2_ids:
        return part[2] == "start" or (part[2] == "trace" and part[5] in ADDED_TEXT2)
    return tuple(part[:2]) in pegsx_ids and part[2] == "trace" and part[5] == "near0"


def _new_fields():
    import pegs_sparse_cases as SC
    import pegsx_cases as XC
    text2 = {("pegs_sparse_cases", c["id"]) for c in SC.CASES if c["entry"] == "PEGSZ_sparse"}
    pegsx = {("pegs_sparse_cases", c["id"]) for c in SC.CASES if c["entry"] == "PEGSX"} | {("pegsx_cases", c["id"]) for c in XC.CASES}
    return lambda path: _is_new(path, text2, pegsx)


@pytest.fixture(scope="module")
def parent(tmp_path_factory):
    """dict(fields, bounds) of the commit RF.PARENT, computed by its own files in a process of its own; None where git cannot give them"""
    import tarfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("parent")
    tar = os.path.join(tmp, "tests.tar")
    try:
        got = subprocess.run(["git", "-C", root, "archive", "-o", tar, RF.PARENT, "tests"], capture_output=True, timeout=120)
    except (OSError, subprocess.TimeoutExpired):
        return None
    if got.returncode != 0:
        return None
    with tarfile.open(tar) as fh:
        fh.extractall(tmp, **({"filter": "data"} if hasattr(tarfile, "data_filter") else {}))
    prog = os.path.join(tmp, "tests", "restatement_fields.py")
    with open(RF.__file__) as src, open(prog, "w") as dst:
        dst.write(src.read())
    out = os.path.join(tmp, "parent.pkl")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    subprocess.run([sys.executable, "-s", prog, out], check=True, cwd=os.path.join(tmp, "tests"), env=env, timeout=900)
    with open(out, "rb") as fh:
        return pickle.load(fh)


def _recorded():
    import json
    with open(RF.RECORDED) as fh:
        rec = json.load(fh)
    assert rec["commit"] == RF.PARENT
    if rec["probe"] != RF.probe():
        pytest.skip("no git checkout that has %s, and numpy's BLAS sums in another order here than where the digests were recorded" % RF.PARENT[:7])
    return rec


def test_float64_restatements_return_the_parents_bits(parent):
    """pegsx, pegsz and pegsz_sparse at float64 on every case of pegsx_cases.py, pegs_cases.py and pegs_sparse_cases.py: every field the
    parent's fit has, the new fit has with the same dtype, shape and bits (13 815 fields)"""
    now, is_new = RF.all_fields(), _new_fields()
    if parent is not None:
        then = parent["fields"]
        for path, a in then.items():
            assert path in now and now[path].dtype == a.dtype and np.array_equal(now[path], a, equal_nan=a.dtype.kind == "f"), path
        assert all(is_new(path) for path in now if path not in then), [path for path in now if path not in then and not is_new(path)][:5]
    else:
        rec = _recorded()
        then = {case: tuple(v) for case, v in rec["fields"].items()}
        got = {case: tuple(v) for case, v in RF.digests({path: a for path, a in now.items() if not is_new(path)}).items()}
        assert got == then, sorted(case for case in then if got.get(case) != then[case])
    print(len(then), "cases' fields" if parent is None else "fields", "compared")
    assert parent is None or len(then) == 13815


def test_the_49_earlier_cases_keep_their_bounds_bit_for_bit(parent):
    then = parent["bounds"] if parent is not None else _recorded()["bounds"]
    now = RF.old_bounds()
    assert sorted(then) == sorted(TC.OLD_NAMES) == sorted(now) and len(then) == 49
    for name in TC.OLD_NAMES:
        assert now[name] == then[name], (name, {key: (now[name].get(key), v) for key, v in then[name].items() if now[name].get(key) != v})
    print(sum(len(v) for v in then.values()), "bounds compared")
