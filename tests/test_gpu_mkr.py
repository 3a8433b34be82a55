"""GPU: mkr / K2X and mrr(Y, dense(X)) -- the dense fp64 train of bwgr_mrr_dense -- against the float64 restatement
in tests/mrr_restatement.py on the cases of tests/mkr_cases.py: every fit is compared on mu, b, hat, h2, GC, vb, ve, MSx, the three convergence
traces and Its, at 1e-6 scaled.  The library and the restatement get the same float-rounded design, so b is compared as it is.

The second round of cases (MC.SOLVE .. MC.OPTION) goes through the same _check: k_mrrd_solve's five LDS regimes, traits that share patterns
across the ngl line, the row counts beside a tile, a trip and the eight-at-a-time sum of the partials, the column kernels' second trip,
degenerate columns and rows, a fit to the default tolerance, and the options where ngl < npat; then the device layouts, the live counts and
a fit of another shape in between."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mkr_cases as MC  # noqa: E402
import mrr_restatement as MR  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("mu", "b", "hat", "h2", "GC", "vb", "ve", "MSx", "cnvB", "cnvH2", "cnvV")
MRR_LIST = ("mu", "b", "hat", "h2", "GC", "vb", "ve", "MSx", "cnvB", "cnvH2", "cnvV", "b_Weights", "Its")
TOL = 1e-6


def _check(g, o, tol=TOL):
    assert tuple(g) == MRR_LIST
    assert g["Its"] == o["Its"] >= 3
    errs = {k: MR.scaled_err(np.asarray(g[k]).reshape(np.asarray(o[k]).shape), o[k]) for k in KEYS}
    print("scaled errors:", {k: "%.2e" % v for k, v in errs.items()})
    assert all(np.all(np.isfinite(g[k])) for k in KEYS)
    assert all(v <= tol for v in errs.values()), errs
    return errs


def _same_bits(a, b):
    assert a["Its"] == b["Its"]
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(Y, X, opts, the restatement's fit) of a case, made once and shared; nobody writes into it"""
    Y, X, opts = MC.case(name)
    return Y, X, opts, MR.mrr(Y, X, **opts)


def _fit(name):
    import bwgr_amd
    Y, X, opts, o = _ref(name)
    return bwgr_amd.mrr(Y, bwgr_amd.dense(X), **opts), o


def test_mkr_on_the_grm_at_the_defaults():
    """mkr(Y, K) = MRR3(Y, K2X(K)): r = 149 columns (blocks of 64, 64, 21), 150 rows, k = 3 with three missingness patterns"""
    import bwgr_amd
    K = MC.grm150()
    Y, X, opts = MC.case("grm150")
    assert opts == {} and X.shape == (150, 149) and MC.npat(Y) == 3
    g = bwgr_amd.mkr(Y, K)
    o = MR.mrr(Y, X)
    _check(g, o)
    assert g["b"].shape == (149, 3) and g["hat"].shape == (150, 3) and g["b_Weights"].shape == (149, 3)
    # the same fit through its parts, and MRR3 by name
    _same_bits(g, bwgr_amd.MRR3(Y, bwgr_amd.dense(bwgr_amd.K2X(K))))


@pytest.mark.parametrize("name", ["r1", "r64", "r65", "r130", "tall", "k1", "k16", "k4full", "TH", "updateMu", "XFA"])
def test_dense_design_parity(name):
    """random real designs: one column, exactly one block, a last block of one and of two columns; a second trip of the pass's workgroups;
    k = 1, k = 16 with sixteen patterns (ngl < npat), one pattern; the options that reach device kernels"""
    import bwgr_amd
    Y, X, opts = MC.case(name)
    g = bwgr_amd.mrr(Y, bwgr_amd.dense(X), **opts)
    o = MR.mrr(Y, X, **opts)
    _check(g, o)


@pytest.mark.parametrize("name", list(MC.SOLVE))
def test_solve_regimes(name):
    """k = 4 .. 16 at r = 70: Linv in LDS with 3, 2 and 1 of the Gram matrices beside it (regime 2), with none (regime 3, ngl = 0), and Linv global
    with every Gram in LDS (regime 4); the plan facts are asserted in tests/test_mkr_cpu.py"""
    _check(*_fit(name))


@pytest.mark.parametrize("name", list(MC.SHARED))
def test_shared_patterns_across_the_ngl_line(name):
    """neighbouring traits whose Gram rows come one from LDS and one from global memory"""
    _check(*_fit(name))


@pytest.mark.parametrize("name", list(MC.ROWS) + list(MC.SMALLEST))
def test_row_counts(name):
    """n beside one tile and beside ld = 128; 8 and 8 + 2 partials in the solve's sum; 32 tiles (the last single trip), 34 (a second trip of two
    workgroups), 66 (a third); n = 2 and n = 3, the smallest the entry takes"""
    g, o = _fit(name)
    _check(g, o)
    Y, X, _, _ = _ref(name)
    assert g["hat"].shape == Y.shape and g["b"].shape == (X.shape[1], Y.shape[1])


def test_wide_design_takes_the_column_kernels_second_trip():
    """r = 32 800: k_mrrd_centre and k_mrrd_setup stride past their 8 192 workgroups of four waves for the last 32 columns, which are also the
    last block.  A column left uncentred or without its XX shows in b, hat and MSx."""
    g, o = _fit("wide")
    _check(g, o)
    assert MR.scaled_err(g["b"][32768:], o["b"][32768:]) <= TOL and np.any(g["b"][32768:] != 0)


@pytest.mark.parametrize("name", MC.DEGENERATE)
def test_degenerate_inputs(name):
    g, o = _fit(name)
    _check(g, o)
    if name == "deg_const_cols":          # XX = XSX = 0, LHS = iG, RHS = 0: exactly zero, as the restatement's
        assert np.all(o["b"][[5, 66]] == 0.0) and np.all(g["b"][[5, 66]] == 0.0)
    if name == "deg_default_tol":         # stopped by the tolerance on both sides
        assert _ref(name)[2] == {} and g["Its"] == o["Its"] < 500


@pytest.mark.parametrize("name", list(MC.OPTION))
def test_options_where_ngl_is_below_npat(name):
    """HCS, ACS, OneVarB, OneVarE and TH with updateMu on six traits of four patterns, three of them in LDS"""
    _check(*_fit(name))


def test_float_flavour_rounds_its_inputs():
    import bwgr_amd
    Y, X, opts = MC.case("r65")
    g = bwgr_amd.mrr_float(Y, bwgr_amd.dense(X), **opts)
    f = lambda A: np.asarray(A, np.float32).astype(np.float64)  # noqa: E731
    o = MR.mrr(f(Y), f(X), **opts)
    _check(g, o)


def test_device_resident_design():
    """K2X of a GRM(..., device_out=True) tensor stays on the device and is fitted there: bit for bit the fit of the same values from the host"""
    import torch
    import bwgr_amd
    Z = MC.genotypes(150, 400, 7).astype(np.int8)
    Kd = bwgr_amd.GRM(Z, device_out=True)
    assert Kd.is_cuda
    Xd = bwgr_amd.K2X(Kd)
    assert Xd.is_cuda and Xd.dtype == torch.float64 and Xd.shape == (150, 149)
    Xh = np.asfortranarray(Xd.cpu().numpy())
    assert np.array_equal(Xh, Xh.astype(np.float32).astype(np.float64))
    Y = MC.traits(Xh, 3, 21, frac=0.15)
    gd = bwgr_amd.mrr(Y, bwgr_amd.dense(Xd), maxit=30)
    gh = bwgr_amd.mrr(Y, bwgr_amd.dense(Xh), maxit=30)
    _same_bits(gd, gh)
    assert np.array_equal(Xd.cpu().numpy(), Xh)                                # the caller's tensor is not centred in place
    _check(gd, MR.mrr(Y, Xh, maxit=30))
    # a strided view of a wider device matrix (ldx > n) gives the same bits
    W = torch.zeros((149, 170), dtype=torch.float64, device=Xd.device)
    W[:, :150] = Xd.t()
    _same_bits(bwgr_amd.mrr(Y, bwgr_amd.dense(W.t()[:150]), maxit=30), gh)
    # mkr on the device tensor: the whole chain without leaving the device
    gm = bwgr_amd.mkr(Y, Kd, maxit=30)
    assert gm["Its"] == gh["Its"]
    for k in ("mu", "hat", "h2", "GC", "vb", "ve", "MSx"):                     # (b carries the eigensolver's signs)
        assert MR.scaled_err(gm[k], gh[k]) <= TOL, k


def test_two_calls_give_the_same_bits():
    import bwgr_amd
    Y, X, opts = MC.case("k16")
    _same_bits(bwgr_amd.mrr(Y, bwgr_amd.dense(X), **opts), bwgr_amd.mrr(Y, bwgr_amd.dense(X), **opts))
    Y, X, opts = MC.case("tall")
    _same_bits(bwgr_amd.mrr(Y, bwgr_amd.dense(X), **opts), bwgr_amd.mrr(Y, bwgr_amd.dense(X), **opts))


def test_two_calls_give_the_same_bits_in_regimes_2_and_3():
    import bwgr_amd
    for name in ("solve_k8p8", "solve_k14p14"):
        Y, X, opts, _ = _ref(name)
        _same_bits(bwgr_amd.mrr(Y, bwgr_amd.dense(X), **opts), bwgr_amd.mrr(Y, bwgr_amd.dense(X), **opts))


def test_device_layouts():
    """what _mrr_dense takes of a device tensor, on a fit with ngl < npat (k = 8, eight patterns, two Grams in LDS): each gives the bits of the
    host fit of the same values and leaves the caller's tensor as it was"""
    import torch
    import bwgr_amd
    Y, X, opts, _ = _ref("solve_k8p8")
    Xr = np.ascontiguousarray(X)              # (torch.tensor keeps a numpy array's order: the cases' designs are column-major)
    dev = torch.device("cuda")

    def fitted(T, fn=bwgr_amd.mrr):
        keep = T.clone()
        g = fn(Y, bwgr_amd.dense(T), **opts)
        assert T.dtype == keep.dtype and T.stride() == keep.stride() and torch.equal(T, keep)
        return g

    # torch's default row-major order
    gh = bwgr_amd.mrr(Y, bwgr_amd.dense(X), **opts)
    T = torch.tensor(Xr, device=dev)
    assert T.is_cuda and T.dtype == torch.float64 and T.stride() == (X.shape[1], 1)
    _same_bits(fitted(T), gh)
    T = torch.tensor(X, device=dev)           # and column-major, read where it is
    assert T.stride() == (1, X.shape[0])
    _same_bits(fitted(T), gh)
    # a float32 tensor of float-representable values, row-major and column-major
    X32 = Xr.astype(np.float32)
    g32 = bwgr_amd.mrr(Y, bwgr_amd.dense(X32.astype(np.float64)), **opts)
    T = torch.tensor(X32, device=dev)
    assert T.dtype == torch.float32 and T.stride() == (X.shape[1], 1)
    _same_bits(fitted(T), g32)
    _same_bits(fitted(torch.tensor(X32, device=dev).t().contiguous().t()), g32)
    # r = 1: an n x 1 and a 1-D tensor
    x1 = np.ascontiguousarray(X[:, 3])
    g1 = bwgr_amd.mrr(Y, bwgr_amd.dense(x1[:, None]), **opts)
    assert g1["b"].shape == (1, 8)
    T = torch.tensor(x1[:, None], device=dev)
    assert tuple(T.shape) == (200, 1)
    _same_bits(fitted(T), g1)
    T = torch.tensor(x1, device=dev)
    assert T.dim() == 1
    _same_bits(fitted(T), g1)
    # the float flavour rounds a device tensor as it rounds a host array
    gf = bwgr_amd.mrr_float(Y, bwgr_amd.dense(X), **opts)
    _same_bits(fitted(torch.tensor(Xr, device=dev), bwgr_amd.mrr_float), gf)
    _same_bits(fitted(torch.tensor(X, device=dev), bwgr_amd.mrr_float), gf)
    f = lambda A: np.asarray(A, np.float32).astype(np.float64)  # noqa: E731
    _check(gf, MR.mrr(f(Y), f(X), **opts))


def test_a_fit_of_another_shape_in_between_changes_nothing():
    """n = 513 (ld = 640), then n = 65 (ld = 128) and the wide case, then n = 513 again: no stale padding row, Gram or partial is picked up"""
    import bwgr_amd
    Y, X, opts, o = _ref("n513")
    first = bwgr_amd.mrr(Y, bwgr_amd.dense(X), **opts)
    _check(first, o)
    for other in ("n65", "wide"):
        _check(*_fit(other))
        _same_bits(bwgr_amd.mrr(Y, bwgr_amd.dense(X), **opts), first)


def test_two_engines_on_one_design():
    """the int8 panel train and the dense fp64 train on the same 300 x 500 0/1/2 matrix"""
    import bwgr_amd
    Y, X, opts = MC.case("int012")
    gd = bwgr_amd.mrr(Y, bwgr_amd.dense(X), **opts)
    P = bwgr_amd.Panel(np.asfortranarray(X.astype(np.int8)))
    try:
        gp = bwgr_amd.mrr(Y, P, **opts)
    finally:
        P.close()
    assert gd["Its"] == gp["Its"]
    errs = {k: MR.scaled_err(gd[k], gp[k]) for k in KEYS}
    print("dense against panel:", {k: "%.2e" % v for k, v in errs.items()})
    assert all(v <= TOL for v in errs.values()), errs
    _check(gd, MR.mrr(Y, X, **opts))


def test_refusals():
    import bwgr_amd as B
    rng = np.random.default_rng(9)
    X = rng.normal(size=(60, 10))
    Y = rng.normal(size=(60, 3))
    # a dense fit and every refusal leave the library's live device arrays, streams and events as they were
    live = B.debug_live()
    good = B.mrr(Y, B.dense(X), maxit=5)
    assert B.debug_live() == live
    with pytest.raises(B.BwgrError, match="k = 17"):
        B.mrr(rng.normal(size=(60, 17)), B.dense(X))
    assert B.debug_live() == live
    with pytest.raises(B.BwgrError, match="nrow"):
        B.mrr(Y[:50], B.dense(X))
    assert B.debug_live() == live
    Xn = X.copy()
    Xn[7, 2] = np.nan
    with pytest.raises(B.BwgrError, match=r"X\[7, 2\]"):
        B.mrr(Y, B.dense(Xn))
    assert B.debug_live() == live
    with pytest.raises(B.BwgrError, match="r = 0"):
        B.mrr(Y, B.dense(np.zeros((60, 0))))
    assert B.debug_live() == live
    Y1 = Y.copy()
    Y1[1:, 2] = np.nan
    with pytest.raises(B.BwgrError, match="trait 2 of Y"):
        B.mrr(Y1, B.dense(X))
    assert B.debug_live() == live
    with pytest.raises(B.BwgrError, match="NoInv"):
        B.mrr(Y, B.dense(X), NoInv=True)
    assert B.debug_live() == live
    with pytest.raises(B.BwgrError, match="square"):
        B.mkr(Y, X)
    assert B.debug_live() == live
    # the library is usable after every refusal
    g = B.mrr(Y, B.dense(X), maxit=5)
    assert g["Its"] >= 1 and np.all(np.isfinite(g["hat"]))
    _same_bits(g, good)
    assert B.debug_live() == live
