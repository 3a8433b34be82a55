"""GPU: the relationship kernels on the resident panel -- the exact X X' (k_xxt_*) against numpy's int64 product, bit for bit, and the five
finishes (k_kfin_*) against the float64 restatement of the reference's formulas (tests/kernels_restatement.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernels_restatement as KR   # noqa: E402
from conftest import scaled_err, synth_small   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6      # the project's parity bound for fp64 engines against fp64 restatements (tests/test_gpu_mrr.py)
EINVAL = 1


def _tpod_x(tpod):
    return np.ascontiguousarray(tpod["gen"]).astype(np.int8)


def _synth_x():
    return np.ascontiguousarray(synth_small(700, 900, seed=3)[0])


def _check_product(X, **panel_kw):
    import bwgr_amd
    P = bwgr_amd.Panel(X, **panel_kw)
    try:
        G = P.crossprod()
    finally:
        P.close()
    ref = KR.crossprod(X)
    assert G.dtype == np.int64 and G.shape == ref.shape
    assert np.array_equal(G, ref), "max |diff| = %d at %s" % (np.abs(G - ref).max(), np.unravel_index(np.argmax(np.abs(G - ref)), G.shape))
    return G


def test_crossprod_tpod(tpod):
    _check_product(_tpod_x(tpod))


def test_crossprod_three_slabs_partial_last_block():
    _check_product(_synth_x(), nwg=3)


@pytest.mark.parametrize("n", [130, 257])
@pytest.mark.parametrize("p", [1, 63, 64, 65, 129])
def test_crossprod_edge_shapes(n, p):
    rng = np.random.default_rng(1000 * n + p)
    _check_product(rng.integers(0, 3, size=(n, p)).astype(np.int8))


def test_crossprod_signed_panel():
    rng = np.random.default_rng(11)
    _check_product(rng.integers(-2, 3, size=(300, 500)).astype(np.int8))


def test_crossprod_full_range_two_natural_chunks():
    """Values in -128..127, p = 140 000 > 131 071: two chunks by the rule, and entries beyond 2^31 (the diagonal is about p * 128^2 / 3)."""
    rng = np.random.default_rng(12)
    X = rng.integers(-128, 128, size=(96, 140000)).astype(np.int8)
    X[0, :] = -128      # the largest entry there can be: p * 2^14 = 2.3e9
    G = _check_product(X)
    assert G.max() > 2 ** 31


@pytest.mark.parametrize("kchunk", ["64", "100"])
def test_crossprod_forced_chunks_give_the_same_bits(kchunk, monkeypatch):
    import bwgr_amd
    X = _synth_x()
    G0 = _check_product(X, nwg=3)
    monkeypatch.setenv("BWGR_KCHUNK", kchunk)     # read when the root panel is made
    G1 = _check_product(X, nwg=3)
    assert np.array_equal(G0, G1)


def test_crossprod_clone_and_centred_panel_give_the_roots_bits(tpod):
    import bwgr_amd
    X = _tpod_x(tpod)
    P = bwgr_amd.Panel(X)
    try:
        G = P.crossprod()
        Q = P.clone()
        assert np.array_equal(Q.crossprod(), G)
        K0 = P.kernel("GRM")
        Q.close()
        P.set_centred(True)
        assert np.array_equal(P.crossprod(), G)
        assert np.array_equal(P.kernel("GRM"), K0)
        P.set_centred(False)
    finally:
        P.close()
    assert np.array_equal(G, KR.crossprod(X))


def test_crossprod_follows_a_row_permutation():
    """An asymmetric check: rows in a random order must permute G accordingly."""
    import bwgr_amd
    X = _synth_x()
    perm = np.random.default_rng(5).permutation(X.shape[0])
    G = bwgr_amd.crossprod(X)
    Gp = bwgr_amd.crossprod(np.ascontiguousarray(X[perm]))
    assert np.array_equal(Gp, G[np.ix_(perm, perm)])
    assert np.array_equal(G, KR.crossprod(X))


@pytest.mark.parametrize("which", ["tpod", "synth"])
@pytest.mark.parametrize("kind,kw", KR.KINDS, ids=["%s-%s" % (k, "-".join("%s" % v for v in kw.values())) for k, kw in KR.KINDS])
def test_kernel_matches_the_restatement(tpod, which, kind, kw):
    import bwgr_amd
    X = _tpod_x(tpod) if which == "tpod" else _synth_x()
    f = getattr(bwgr_amd, kind)
    P = bwgr_amd.Panel(X)
    try:
        K = f(P, **kw)
        K2 = f(P, **kw)
    finally:
        P.close()
    ref = KR.restate(kind, X, **kw)
    err = scaled_err(K, ref)
    print("%s %s %s: scaled_err = %.3e" % (which, kind, kw, err))
    assert K.dtype == np.float64 and K.shape == ref.shape and np.all(np.isfinite(K))
    assert err <= TOL, err
    assert np.array_equal(K, K.T)
    assert np.array_equal(K, K2)      # two calls: identical bits


def test_device_out_equals_the_host_result(tpod):
    import torch
    import bwgr_amd
    X = _tpod_x(tpod)
    P = bwgr_amd.Panel(X)
    try:
        for kind in ("GRM", "EigenGAU", "EigenARC"):
            Kh = P.kernel(kind)
            Kd = P.kernel(kind, device_out=True)
            assert isinstance(Kd, torch.Tensor) and Kd.is_cuda and Kd.device.index == P.device and Kd.dtype == torch.float64
            assert np.array_equal(Kd.cpu().numpy(), Kh)
        Gd = P.crossprod(device_out=True)
        assert Gd.dtype == torch.int64 and np.array_equal(Gd.cpu().numpy(), P.crossprod())
        w = torch.linalg.eigvalsh(P.kernel("GRM", device_out=True))      # what device_out is for
        assert torch.isfinite(w).all()
    finally:
        P.close()


def test_ldk_beyond_n_leaves_the_padding_untouched(tpod):
    import bwgr_amd
    from bwgr_amd import _lib
    L = _lib.lib()
    X = _tpod_x(tpod)
    n = X.shape[0]
    P = bwgr_amd.Panel(X)
    try:
        ld = n + 5
        K = np.full((n, ld), -7.25)
        assert L.bwgr_panel_kernel(P._h, 0, 1.0, 0, K.ctypes.data_as(C.c_void_p), ld, 0) == 0
        assert np.array_equal(K[:, n:], np.full((n, 5), -7.25))
        assert np.array_equal(K[:, :n], P.kernel("GRM"))
        G = np.full((n, ld), -9, np.int64)
        assert L.bwgr_panel_crossprod(P._h, G.ctypes.data_as(C.c_void_p), ld, 0) == 0
        assert np.array_equal(G[:, n:], np.full((n, 5), -9)) and np.array_equal(G[:, :n], KR.crossprod(X))
    finally:
        P.close()


def test_refusals_leave_the_panel_usable(tpod):
    import bwgr_amd
    from bwgr_amd import _lib
    L = _lib.lib()
    X = _tpod_x(tpod)
    n = X.shape[0]
    y = tpod["y"]
    P = bwgr_amd.Panel(X)
    Pf = bwgr_amd.Panel(X.astype(np.float32) + 0.25, as_int8=False)
    try:
        before = bwgr_amd.BayesRR(y, P, it=5, bi=1, seed=3)
        K = np.empty((n, n))
        ptr = K.ctypes.data_as(C.c_void_p)
        assert L.bwgr_panel_kernel(Pf._h, 0, 1.0, 0, ptr, n, 0) == EINVAL and b"fp32" in L.bwgr_last_error()
        assert L.bwgr_panel_crossprod(Pf._h, ptr, n, 0) == EINVAL
        assert L.bwgr_panel_kernel(P._h, 5, 1.0, 0, ptr, n, 0) == EINVAL and b"kind" in L.bwgr_last_error()
        assert L.bwgr_panel_kernel(P._h, -1, 1.0, 0, ptr, n, 0) == EINVAL
        assert L.bwgr_panel_kernel(P._h, 0, 1.0, 0, ptr, n - 1, 0) == EINVAL and b"leading dimension" in L.bwgr_last_error()
        assert L.bwgr_panel_crossprod(P._h, ptr, n - 1, 0) == EINVAL
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            P.kernel(17)
        assert ei.value.code == EINVAL
        after = bwgr_amd.BayesRR(y, P, it=5, bi=1, seed=3)
        assert np.array_equal(before["b"], after["b"]) and np.array_equal(before["hat"], after["hat"])
        assert np.array_equal(P.crossprod(), KR.crossprod(X))
    finally:
        P.close(); Pf.close()


def test_grm_feeds_wgr(tpod):
    """End to end: K = GRM(P), eigen(K) on the host, wgr with the kernel term."""
    import bwgr_amd
    X = _tpod_x(tpod)
    y = tpod["y"]
    P = bwgr_amd.Panel(X)
    try:
        K = bwgr_amd.GRM(P)
        w, v = np.linalg.eigh(K)
        w, v = w[::-1], v[:, ::-1]
        wr = np.linalg.eigvalsh(KR.GRM(X))[::-1]
        assert scaled_err(w, wr) <= TOL
        out = bwgr_amd.wgr(y, P, it=30, bi=10, eigK={"values": w, "vectors": v}, seed=7)
    finally:
        P.close()
    assert np.all(np.isfinite(out["hat"])) and np.all(np.isfinite(out["u"])) and np.isfinite(out["Vk"])
