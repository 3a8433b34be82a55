"""GPU: mrr_svd on the resident panel (bwgr_amd.svd) against the float64 restatement in tests/mrr_svd_restatement.py on
the cases of tests/mrr_svd_cases.py, at 1e-6 scaled, the project's parity tolerance.
  engine:     bwgr_mrr_svd_fit on the restatement's own design -- mu, b, hat, h2, GC, vb, ve, the three traces, and Its equal
  driver:     mrr_svd(Y, W) against the restatement on numpy's SVD of the centred matrix, all eleven keys (none depends on a sign)
  identities: FittedValues - Intercepts = W_c MarkerEffects through panel_xb; the torch and the numpy route; p < n
  refusals:   through the C entry"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrr_svd_cases as MC  # noqa: E402
import mrr_svd_restatement as SR  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("mu", "b", "hat", "h2", "GC", "vb", "ve", "cnvB", "cnvH2", "cnvV")
FIT_LIST = KEYS + ("Its",)
TOL = 1e-6


def _check(g, o, keys=KEYS, its="Its"):
    assert g[its] == o[its] >= 3
    errs = {k: SR.scaled_err(np.asarray(g[k]).reshape(np.asarray(o[k]).shape), o[k]) for k in keys}
    print("scaled errors:", {k: "%.2e" % v for k, v in errs.items()})
    assert all(np.all(np.isfinite(np.asarray(g[k]))) for k in keys)
    assert all(v <= TOL for v in errs.values()), errs


@pytest.mark.parametrize("name", list(MC.FIT))
def test_engine(name):
    """r = 64, 65, 128, 129, 149, 299, 300 columns; k = 1 .. 16; a pattern per trait and one shared by all; fits that bend; fits that converge"""
    from bwgr_amd import svd
    Y, X, o = MC.engine_ref(name)
    g = svd.mrr_svd_fit(Y, X, maxit=MC.FIT[name]["maxit"])
    assert tuple(g) == FIT_LIST and g["b"].shape == o["b"].shape and g["hat"].shape == Y.shape
    _check(g, o)
    if name == "k16_r149":
        assert any(t["bent"] for t in o["trace"])


def test_device_design_and_two_calls_give_the_same_bits():
    import torch
    from bwgr_amd import svd
    Y, X, o = MC.engine_ref("k6_r129")
    a = svd.mrr_svd_fit(Y, X, maxit=30)
    b = svd.mrr_svd_fit(Y, X, maxit=30)
    Xd = torch.from_numpy(X.T.copy()).cuda().t()                 # column-major on the device
    d = svd.mrr_svd_fit(Y, Xd, maxit=30)
    Xp = torch.zeros((X.shape[1], X.shape[0] + 7), dtype=torch.float64, device="cuda")
    Xp[:, :X.shape[0]] = torch.from_numpy(X.T.copy()).cuda()
    e = svd.mrr_svd_fit(Y, Xp.t()[:X.shape[0]], maxit=30)        # a column stride beyond n
    for other in (b, d, e):
        assert other["Its"] == a["Its"]
        for k in KEYS:
            assert np.array_equal(other[k], a[k]), k


@pytest.mark.parametrize("name", MC.DRIVER)
def test_driver(name):
    from bwgr_amd import svd
    W, Y, o = MC.driver_ref(name)
    g = svd.mrr_svd(Y, W, maxit=MC.FIT[name]["maxit"])
    assert tuple(g) == svd.WMODEL_KEYS == tuple(o)
    assert g["MarkerEffects"].shape == (W.shape[1], Y.shape[1]) and g["FittedValues"].shape == Y.shape
    _check(g, o, keys=svd.WMODEL_KEYS[:-1], its="NumOfIterations")


def test_fitted_values_are_the_centred_panel_times_the_marker_effects():
    from bwgr_amd import svd
    from bwgr_amd.panel import as_panel
    for name in ("k3_r65", "k16_p_lt_n"):
        W, Y, _ = MC.driver_ref(name)
        with as_panel(W) as P:
            g = svd.mrr_svd(Y, P, maxit=MC.FIT[name]["maxit"])
            beta = g["MarkerEffects"]
            xbar = W.sum(0, dtype=np.int64) / float(W.shape[0])
            Wc_beta = P.xb(beta) - xbar @ beta
        assert SR.scaled_err(Wc_beta, g["FittedValues"] - g["Intercepts"]) <= TOL


def test_p_below_n_keeps_p_directions():
    from bwgr_amd import svd
    W, Y = MC.data("k16_p_lt_n")
    n, p = W.shape
    D = svd.svd_design(W)
    assert p < n and tuple(D["X"].shape) == (n, p) and len(D["d"]) == p and D["xbar_free"] is True


def test_torch_route_and_numpy_route_agree(monkeypatch):
    import torch  # noqa: F401
    from bwgr_amd import svd
    W, Y, _ = MC.driver_ref("k3_r65")
    Dt = svd.svd_design(W)
    assert Dt["X"].is_cuda and Dt["X"].stride(0) == 1
    gt = svd.mrr_svd(Y, W, maxit=30)
    gd = svd.mrr_svd(Y, W, maxit=30, device_out=True)
    assert gd["MarkerEffects"].is_cuda and np.array_equal(gd["MarkerEffects"].cpu().numpy(), gt["MarkerEffects"])
    monkeypatch.delitem(sys.modules, "torch")
    Dn = svd.svd_design(W)
    assert isinstance(Dn["X"], np.ndarray) and Dn["X"].flags.f_contiguous and Dn["X"].shape == tuple(Dt["X"].shape)
    assert SR.scaled_err(Dn["d"], Dt["d"].cpu().numpy()) <= 1e-10
    gn = svd.mrr_svd(Y, W, maxit=30)
    _check(gt, gn, keys=svd.WMODEL_KEYS[:-1], its="NumOfIterations")


def test_refusals():
    from bwgr_amd import _lib
    L = _lib.lib()
    n, r = 40, 5
    rng = np.random.default_rng(2)
    X = np.asfortranarray(rng.normal(size=(n, r)))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731

    def call(X_=X, Y_=None, k=2, maxit=3, n_=n, r_=r, ldx=n, memloc=0, b=True, its=True):
        Y_ = np.asfortranarray(rng.normal(size=(n, max(k, 1)))) if Y_ is None else Y_
        outs = [np.zeros(max(k, 1)), np.zeros((r, max(k, 1)), order="F"), np.zeros((n, max(k, 1)), order="F"), np.zeros(max(k, 1)),
                np.zeros((max(k, 1),) * 2), np.zeros((max(k, 1),) * 2), np.zeros(max(k, 1)), np.zeros(max(maxit, 1)), np.zeros(max(maxit, 1)), np.zeros(max(maxit, 1))]
        ptrs = [dp(a) for a in outs]
        if not b:
            ptrs[1] = None
        it = C.c_int()
        return L.bwgr_mrr_svd_fit(0, None if X_ is None else X_.ctypes.data_as(C.c_void_p), memloc, n_, r_, ldx, None if Y_ is False else dp(Y_), k, maxit, 1e-8, 0,
                                  *ptrs, C.byref(it) if its else None)
    assert call() == 0
    assert call(k=17, Y_=np.asfortranarray(rng.normal(size=(n, 17)))) == 1 and b"k = 17" in L.bwgr_last_error()
    assert call(k=0) == 1
    assert call(maxit=-1) == 1 and b"maxit" in L.bwgr_last_error()
    Y1 = np.asfortranarray(rng.normal(size=(n, 2)))
    Y1[1:, 1] = np.nan                                           # a trait with one record
    assert call(Y_=Y1) == 1 and b"observed rows" in L.bwgr_last_error()
    assert call(X_=None) == 1 and call(Y_=False) == 1 and call(b=False) == 1 and call(its=False) == 1
    assert b"null pointer" in L.bwgr_last_error()
    assert call(ldx=n - 1) == 1 and call(r_=0) == 1 and call(n_=1) == 1 and call(memloc=3) == 1
    Xn = X.copy(order="F")
    Xn[3, 2] = np.inf
    assert call(X_=Xn) == 1 and b"not finite" in L.bwgr_last_error()
