"""GPU: mkr / K2X and mrr(Y, dense(X)) -- the dense fp64 train of bwgr_mrr_dense -- against the float64 restatement
in tests/mrr_restatement.py on the cases of tests/mkr_cases.py: every fit is compared on mu, b, hat, h2, GC, vb, ve, MSx, the three convergence
traces and Its, at 1e-6 scaled.  The library and the restatement get the same float-rounded design, so b is compared as it is."""
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
    with pytest.raises(B.BwgrError, match="k = 17"):
        B.mrr(rng.normal(size=(60, 17)), B.dense(X))
    with pytest.raises(B.BwgrError, match="nrow"):
        B.mrr(Y[:50], B.dense(X))
    Xn = X.copy()
    Xn[7, 2] = np.nan
    with pytest.raises(B.BwgrError, match=r"X\[7, 2\]"):
        B.mrr(Y, B.dense(Xn))
    with pytest.raises(B.BwgrError, match="r = 0"):
        B.mrr(Y, B.dense(np.zeros((60, 0))))
    Y1 = Y.copy()
    Y1[1:, 2] = np.nan
    with pytest.raises(B.BwgrError, match="trait 2 of Y"):
        B.mrr(Y1, B.dense(X))
    with pytest.raises(B.BwgrError, match="NoInv"):
        B.mrr(Y, B.dense(X), NoInv=True)
    with pytest.raises(B.BwgrError, match="square"):
        B.mkr(Y, X)
    # the library is usable after every refusal
    g = B.mrr(Y, B.dense(X), maxit=5)
    assert g["Its"] >= 1 and np.all(np.isfinite(g["hat"]))
