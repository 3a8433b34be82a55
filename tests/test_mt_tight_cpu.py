"""CPU: tests/ld_linalg.py against numpy and against its own residuals in long double; then the yardstick of tests/test_gpu_mt_tight.py
(tests/mt_tight.py) on every case of tests/mt_tight_cases.py: it is finite, it puts the bound on the coefficients at least five orders below the
suite's 1e-6, and it bites: the restatement with one float temporary in the step's dependent dot x_J'e -- what a float partial sum in a
kernel's dot does -- lands at least a hundred bounds away, on every effect's coefficients.  The decisions of a fit (mrr's bending; PEGS's
inflation, truncation and clamp) are the same in the long double run and the nine float64 runs and none is near its threshold, and the cases
reach the regimes, trips, patterns, code ranges and kappa they are there for.  Every yardstick and ratio is printed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ld_linalg as LL  # noqa: E402
import mrr_cases  # noqa: E402
import mt_tight as T  # noqa: E402
import mt_tight_cases as TC  # noqa: E402

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
    return T.float_dot if c["family"] != "pegs" else [T.float_dot if f == i else None for f in range(len(c["effects"]))]


@pytest.mark.parametrize("name", TC.NAMES)
def test_yardstick_is_finite_tight_and_bites(name):
    c = TC.case(name)
    o, yard, bound = T.ref(name), T.yard(name), T.bound(name)
    print(name, "kappa %.2f" % T.kappa(c), {key: "%.1e" % v for key, v in yard.items()})
    for key in T.keys(c):
        assert np.isfinite(yard[key]) and np.isfinite(bound[key]) and bound[key] >= T.FLOOR, (key, yard[key])
    for i, key in enumerate(T.b_keys(c)):
        assert bound[key] <= B_BOUND_LOOSE.get(name, B_BOUND), (key, bound[key])
        moved = T.errs(name, T.run(name, dot=_mutant(c, i)), o)[key]
        print(name, key, "mutant %.2e, bound %.2e, ratio %.0f" % (moved, bound[key], moved / bound[key]))
        assert moved >= BITE * bound[key], (key, moved, bound[key])


def test_no_more_than_three_cases_have_the_looser_bound_on_b():
    assert len(B_BOUND_LOOSE) <= 3 and set(B_BOUND_LOOSE) <= set(TC.NAMES) and all(v <= 1e-9 for v in B_BOUND_LOOSE.values())


def test_a_long_double_run_leaves_nothing_in_float64():
    for name in ("mrr/k7_npat7", "mrr/tpod_k3_float", "mrr/opt_ACS", "mrr/opt_TH", "mrr/opt_updateMu", "mrr/bending", "dense/r65", "pegs/k5_inflated",
                 "pegsz/panel_dense5", "pegs/xfa2"):
        c, o = TC.case(name), T.ref(name)
        for key in T.keys(c):
            if key != "hat_own":
                assert np.asarray(o[key]).dtype == LD, (name, key)
        for sweep in o["dec"]:                      # ... nor on the way: every sweep's eigenvalues, gaps and margins as the tail made them
            for v in (sweep if c["family"] != "pegs" else [v for rec in sweep for v in rec]):
                assert isinstance(v, (LD, bool, np.bool_, type(None))), (name, type(v))
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


@pytest.mark.parametrize("name", TC.NAMES)
def test_decisions_are_the_same_in_all_ten_runs_and_away_from_their_thresholds(name):
    c, o = TC.case(name), T.ref(name)
    decs = [o["dec"]] + [d for _, d in T.runs(name)]
    assert len(decs) == 1 + T.NRUNS and all(len(d) == o["its"] for d in decs)
    if c["family"] != "pegs":
        print(name, [(bool(b), "%.2e" % float(lam)) for b, lam in o["dec"]])
        for d in decs:
            assert [b for b, _ in d] == [b for b, _ in o["dec"]]
            assert all(abs(lam) >= 1e-6 for _, lam in d), [float(lam) for _, lam in d]
        return
    k, kw = c["Y"].shape[1], c["kw"]
    XFA, covMinEv = kw.get("XFA", -1), float(np.float32(kw.get("covMinEv", 10e-4)))
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
                if kw.get("NNC", True):
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
