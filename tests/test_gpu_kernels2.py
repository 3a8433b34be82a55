"""GPU: the founder-by-sample kernels on two resident panels -- the exact X_f X_s' (k_xyt_mfma_i8) against numpy's int64 product, bit for
bit, the two finishes (k_kfin2_*) and the drivers EigenArcZ / EigenGauZ against the float64 restatement of the reference's formulas
(tests/kernels2_restatement.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernels2_restatement as K2   # noqa: E402
from conftest import scaled_err, synth_small   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6      # the project's parity bound for fp64 engines against fp64 restatements (tests/test_gpu_mrr.py)
EINVAL = 1
KINDS = [("ARC", 1.0), ("ARC", 0.5), ("GAU", 1.0), ("GAU", 0.5)]     # (phi is ignored under ARC)


def _tpod_split(tpod):
    X = np.ascontiguousarray(tpod["gen"]).astype(np.int8)
    return np.ascontiguousarray(X[:130]), np.ascontiguousarray(X[130:])


def _synth_split():
    X = np.ascontiguousarray(synth_small(500, 900, seed=3)[0])
    return np.ascontiguousarray(X[:300]), np.ascontiguousarray(X[300:])


def _split(tpod, which):
    return _tpod_split(tpod) if which == "tpod" else _synth_split()


_REF = {}


def _restated(tpod, which, kind, phi):
    """(Kff, Kfs) of the restatement, computed once per case and shared (read-only)"""
    key = (which, kind, phi if kind == "GAU" else 1.0)
    if key not in _REF:
        F, S = _split(tpod, which)
        _REF[key] = tuple(K2.kernels(kind, F, S, phi))
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


def _same(G, ref):
    assert G.dtype == np.int64 and G.shape == ref.shape
    assert np.array_equal(G, ref), "max |diff| = %d at %s" % (np.abs(G - ref).max(), np.unravel_index(np.argmax(np.abs(G - ref)), G.shape))


def _check_product(Xf, Xs, kwf=None, kws=None, slabs_differ=None):
    import bwgr_amd
    Pf = bwgr_amd.Panel(Xf, **(kwf or {}))
    Ps = bwgr_amd.Panel(Xs, **(kws or {}))
    try:
        print("founders %d x %d slab rows %d, samples %d x %d slab rows %d" % (Pf.n, Pf.p, Pf.slab_rows, Ps.n, Ps.p, Ps.slab_rows))
        if slabs_differ is not None:
            assert (Pf.slab_rows != Ps.slab_rows) == slabs_differ
        G = Pf.crossprod2(Ps)
    finally:
        Pf.close(); Ps.close()
    _same(G, K2.crossprod2(Xf, Xs))
    return G


# ---- the product ----
@pytest.mark.parametrize("nf,ns", [(130, 257), (257, 130), (128, 2)])
@pytest.mark.parametrize("p", [1, 63, 64, 65, 129])
def test_crossprod2_edge_shapes(nf, ns, p):
    rng = np.random.default_rng(100000 * nf + 100 * ns + p)
    _check_product(rng.integers(0, 3, size=(nf, p)).astype(np.int8), rng.integers(0, 3, size=(ns, p)).astype(np.int8))


def test_crossprod2_three_slab_founders_default_samples():
    X = np.ascontiguousarray(synth_small(1000, 900, seed=4)[0])
    _check_product(np.ascontiguousarray(X[:700]), np.ascontiguousarray(X[700:]), kwf={"nwg": 3})


def test_crossprod2_different_slab_heights():
    """Founders in three slabs of 256 rows, samples in three slabs of 128: each operand's addresses come from its own slab height.  (The
    tpod split, one slab of 256 against one of 128, is the second such case: every tpod test below.)"""
    X = np.ascontiguousarray(synth_small(1000, 900, seed=4)[0])
    _check_product(np.ascontiguousarray(X[:700]), np.ascontiguousarray(X[700:]), kwf={"nwg": 3}, kws={"nwg": 3}, slabs_differ=True)
    _check_product(np.ascontiguousarray(X[700:]), np.ascontiguousarray(X[:700]), kwf={"nwg": 3}, kws={"nwg": 3}, slabs_differ=True)


def test_crossprod2_tpod_split(tpod):
    F, S = _tpod_split(tpod)
    _check_product(F, S, slabs_differ=True)


def test_crossprod2_signed_panels():
    rng = np.random.default_rng(11)
    _check_product(rng.integers(-2, 3, size=(300, 500)).astype(np.int8), rng.integers(-3, 4, size=(170, 500)).astype(np.int8))


def test_crossprod2_full_range_two_natural_chunks():
    """Values in -128..127, p = 140 000 > 131 071: two chunks by the rule; one founder row and one sample row are -128 throughout, so their
    entry is p * 2^14 = 2.3e9 > 2^31."""
    rng = np.random.default_rng(12)
    F = rng.integers(-128, 128, size=(96, 140000)).astype(np.int8)
    S = rng.integers(-128, 128, size=(40, 140000)).astype(np.int8)
    F[5, :] = -128
    S[7, :] = -128
    G = _check_product(F, S)
    assert G[5, 7] == 140000 * 2 ** 14 and G.max() > 2 ** 31


@pytest.mark.parametrize("kchunk", ["64", "100"])
def test_crossprod2_forced_chunks_give_the_same_bits(kchunk, monkeypatch):
    F, S = _synth_split()
    G0 = _check_product(F, S, kwf={"nwg": 3})
    monkeypatch.setenv("BWGR_KCHUNK", kchunk)     # read when the founders' root panel is made
    G1 = _check_product(F, S, kwf={"nwg": 3})
    assert np.array_equal(G0, G1)


def test_crossprod2_swapped_is_the_transpose_and_same_panel_is_crossprod():
    import bwgr_amd
    F, S = _synth_split()
    Pf, Ps = bwgr_amd.Panel(F), bwgr_amd.Panel(S)
    try:
        Gfs, Gsf = Pf.crossprod2(Ps), Ps.crossprod2(Pf)
        assert np.array_equal(Gfs, Gsf.T)
        _same(Gfs, K2.crossprod2(F, S))
        Gff = Pf.crossprod2(Pf)
        assert np.array_equal(Gff, Pf.crossprod())
        _same(Gff, K2.crossprod2(F, F))
        assert np.array_equal(bwgr_amd.crossprod2(F, F), Gff) and np.array_equal(bwgr_amd.crossprod2(F, S.astype(np.float64)), Gfs)
    finally:
        Pf.close(); Ps.close()


def test_crossprod2_clones_and_centred_panels_give_the_roots_bits(tpod):
    import bwgr_amd
    F, S = _tpod_split(tpod)
    Pf, Ps = bwgr_amd.Panel(F), bwgr_amd.Panel(S)
    try:
        G = Pf.crossprod2(Ps)
        K = Pf.kernel2(Ps, "ARC")
        Qf, Qs = Pf.clone(), Ps.clone()
        assert np.array_equal(Qf.crossprod2(Ps), G) and np.array_equal(Pf.crossprod2(Qs), G) and np.array_equal(Qf.crossprod2(Qs), G)
        Qf.close(); Qs.close()
        for P in (Pf, Ps):
            P.set_centred(True)
            assert np.array_equal(Pf.crossprod2(Ps), G)
            K1 = Pf.kernel2(Ps, "ARC")
            assert np.array_equal(K1[0], K[0]) and np.array_equal(K1[1], K[1])
            P.set_centred(False)
    finally:
        Pf.close(); Ps.close()
    _same(G, K2.crossprod2(F, S))


def test_ld_beyond_the_row_length_leaves_the_padding_untouched(tpod):
    import bwgr_amd
    from bwgr_amd import _lib
    L = _lib.lib()
    F, S = _tpod_split(tpod)
    nf, ns = F.shape[0], S.shape[0]
    Pf, Ps = bwgr_amd.Panel(F), bwgr_amd.Panel(S)
    try:
        ld = ns + 5
        G = np.full((nf, ld), -9, np.int64)
        assert L.bwgr_panel_crossprod2(Pf._h, Ps._h, G.ctypes.data_as(C.c_void_p), ld, 0) == 0
        assert np.array_equal(G[:, ns:], np.full((nf, 5), -9)) and np.array_equal(G[:, :ns], K2.crossprod2(F, S))
        for kind in (0, 1):
            Kff, Kfs = np.full((nf, nf + 3), -7.25), np.full((nf, ld), -7.25)
            assert L.bwgr_panel_kernel2(Pf._h, Ps._h, kind, 1.0, Kff.ctypes.data_as(C.c_void_p), nf + 3, Kfs.ctypes.data_as(C.c_void_p), ld, 0) == 0
            assert np.array_equal(Kff[:, nf:], np.full((nf, 3), -7.25)) and np.array_equal(Kfs[:, ns:], np.full((nf, 5), -7.25))
            K = Pf.kernel2(Ps, kind)
            assert np.array_equal(Kff[:, :nf], K[0]) and np.array_equal(Kfs[:, :ns], K[1])
    finally:
        Pf.close(); Ps.close()


def test_device_out_equals_the_host_result(tpod):
    import torch
    import bwgr_amd
    F, S = _tpod_split(tpod)
    Pf, Ps = bwgr_amd.Panel(F), bwgr_amd.Panel(S)
    try:
        Gd = Pf.crossprod2(Ps, device_out=True)
        assert isinstance(Gd, torch.Tensor) and Gd.is_cuda and Gd.dtype == torch.int64 and tuple(Gd.shape) == (130, 66)
        assert np.array_equal(Gd.cpu().numpy(), Pf.crossprod2(Ps))
        for kind in ("ARC", "GAU"):
            Kh = Pf.kernel2(Ps, kind)
            Kd = Pf.kernel2(Ps, kind, device_out=True)
            for h, d in zip(Kh, Kd):
                assert d.is_cuda and d.device.index == Pf.device and d.dtype == torch.float64
                assert np.array_equal(d.cpu().numpy(), h)
    finally:
        Pf.close(); Ps.close()


# ---- the finishes ----
@pytest.mark.parametrize("which", ["tpod", "synth"])
@pytest.mark.parametrize("kind,phi", KINDS, ids=["%s-%s" % k for k in KINDS])
def test_kernel2_matches_the_restatement(tpod, which, kind, phi):
    import bwgr_amd
    F, S = _split(tpod, which)
    Pf, Ps = bwgr_amd.Panel(F), bwgr_amd.Panel(S)
    try:
        Kff, Kfs = Pf.kernel2(Ps, kind, phi)
        Kff2, Kfs2 = Pf.kernel2(Ps, kind, phi)
    finally:
        Pf.close(); Ps.close()
    rff, rfs = _restated(tpod, which, kind, phi)
    eff, efs = scaled_err(Kff, rff), scaled_err(Kfs, rfs)
    print("%s %s phi=%s: scaled_err Kff = %.3e, Kfs = %.3e" % (which, kind, phi, eff, efs))
    assert Kff.dtype == np.float64 and Kff.shape == rff.shape and Kfs.dtype == np.float64 and Kfs.shape == rfs.shape
    assert np.all(np.isfinite(Kff)) and np.all(np.isfinite(Kfs))
    assert eff <= TOL, eff
    assert efs <= TOL, efs
    assert np.array_equal(Kff, Kff.T)
    assert np.array_equal(Kff, Kff2) and np.array_equal(Kfs, Kfs2)      # two calls: identical bits


@pytest.mark.parametrize("kind", ["ARC", "GAU"])
def test_kernel2_multi_slab_panels_of_different_slab_heights(kind):
    """Founders in three slabs of 256 rows, samples in three slabs of 128 (test_crossprod2_different_slab_heights' panels): the row
    reductions X_f s, X_s s and q_s and both finishes address a second and a third slab on either side."""
    import bwgr_amd
    X = np.ascontiguousarray(synth_small(1000, 900, seed=4)[0])
    F, S = np.ascontiguousarray(X[:700]), np.ascontiguousarray(X[700:])
    Pf, Ps = bwgr_amd.Panel(F, nwg=3), bwgr_amd.Panel(S, nwg=3)
    try:
        print("founders %d x %d slab rows %d, samples %d x %d slab rows %d" % (Pf.n, Pf.p, Pf.slab_rows, Ps.n, Ps.p, Ps.slab_rows))
        assert Pf.slab_rows != Ps.slab_rows
        Kff, Kfs = Pf.kernel2(Ps, kind, 0.5)
        Kff2, Kfs2 = Pf.kernel2(Ps, kind, 0.5)
    finally:
        Pf.close(); Ps.close()
    rff, rfs = K2.kernels(kind, F, S, 0.5)
    eff, efs = scaled_err(Kff, rff), scaled_err(Kfs, rfs)
    print("%s: scaled_err Kff = %.3e, Kfs = %.3e" % (kind, eff, efs))
    assert Kff.shape == (700, 700) and Kfs.shape == (700, 300)
    assert eff <= TOL, eff
    assert efs <= TOL, efs
    assert np.array_equal(Kff, Kff.T)
    assert np.array_equal(Kff, Kff2) and np.array_equal(Kfs, Kfs2)      # two calls: identical bits


# ---- the drivers ----
def _driver(kind):
    import bwgr_amd
    return bwgr_amd.EigenArcZ if kind == "ARC" else (lambda F, S, phi=1.0, **kw: bwgr_amd.EigenGauZ(F, S, phi, **kw))


@pytest.mark.parametrize("which", ["tpod", "synth"])
@pytest.mark.parametrize("kind,phi", [("ARC", 1.0), ("GAU", 1.0), ("GAU", 0.5)], ids=["ARC", "GAU-1.0", "GAU-0.5"])
def test_driver_parts_and_projection(tpod, which, kind, phi):
    import bwgr_amd
    F, S = _split(tpod, which)
    r = bwgr_amd.EigenArcZ(F, S, parts=True) if kind == "ARC" else bwgr_amd.EigenGauZ(F, S, phi, parts=True)
    assert sorted(r) == ["Kff", "Kfs", "Z", "values", "vectors"]
    Z, w, V = r["Z"], r["values"], r["vectors"]
    assert Z.dtype == np.float64 and Z.shape == (S.shape[0], F.shape[0]) and np.all(np.diff(w) >= 0) and w[0] > 0
    e1 = scaled_err(Z @ (V * np.sqrt(w)).T, r["Kfs"].T)
    rff, rfs = _restated(tpod, which, kind, phi)
    cond = np.linalg.cond(rff)
    assert cond <= 1e5, cond           # a condition on the inputs: the restated Kff is well conditioned
    e2 = scaled_err(Z @ Z.T, rfs.T @ np.linalg.solve(rff, rfs))
    print("%s %s phi=%s: Z (V sqrt(L))' against Kfs' %.3e; Z Z' against Kfs' Kff^-1 Kfs %.3e (cond %.3g)" % (which, kind, phi, e1, e2, cond))
    assert e1 <= TOL, e1
    assert e2 <= TOL, e2
    Z2 = bwgr_amd.EigenArcZ(F, S) if kind == "ARC" else bwgr_amd.EigenGauZ(F, S, phi)
    assert np.array_equal(Z2, Z)


def test_eigenarcz_of_the_founders_reproduces_kff(tpod):
    import bwgr_amd
    for which in ("tpod", "synth"):
        F, _ = _split(tpod, which)
        P = bwgr_amd.Panel(F)
        try:
            r = bwgr_amd.EigenArcZ(P, P, parts=True)
        finally:
            P.close()
        err = scaled_err(r["Z"] @ r["Z"].T, r["Kff"])
        print(which, "EigenArcZ(F, F): Z Z' against Kff", err)
        assert err <= TOL, err
        assert scaled_err(r["Kfs"], r["Kff"]) <= 1e-12      # the two blocks coincide
        assert scaled_err(r["Kff"], K2.arc_kernels(F, F)[0]) <= TOL


def test_gauz_coordinates_feed_uvbeta_dense(tpod):
    """End to end: the founders' and the samples' coordinates in the same rotation; a ridge fit on the founders predicts the samples.
    (emRR takes genotypes, not float designs: the dense per-trait fit is the one that regresses on Z.)"""
    import bwgr_amd
    F, S = _tpod_split(tpod)
    yf = tpod["y"][:130]
    Pf, Ps = bwgr_amd.Panel(F), bwgr_amd.Panel(S)
    try:
        Zf = bwgr_amd.EigenGauZ(Pf, Pf)
        Zs = bwgr_amd.EigenGauZ(Pf, Ps)
    finally:
        Pf.close(); Ps.close()
    fit = bwgr_amd.uvbeta_dense(yf, Zf)
    b = np.asarray(fit["b"], np.float64).reshape(Zf.shape[1], -1)
    pred = Zs @ b
    assert pred.shape == (66, 1) and np.all(np.isfinite(pred)) and np.all(np.isfinite(b))


# ---- refusals and leaks ----
def test_refusals_leave_both_panels_usable(tpod):
    import bwgr_amd
    from bwgr_amd import _lib
    L = _lib.lib()
    F, S = _tpod_split(tpod)
    nf, ns = F.shape[0], S.shape[0]
    yf, ys = tpod["y"][:nf], tpod["y"][nf:]
    Pf, Ps = bwgr_amd.Panel(F), bwgr_amd.Panel(S)
    P32 = bwgr_amd.Panel(S.astype(np.float32) + 0.25, as_int8=False)
    Pq = bwgr_amd.Panel(np.ascontiguousarray(S[:, :300]))
    try:
        before = [bwgr_amd.BayesRR(y, P, it=5, bi=1, seed=3) for y, P in ((yf, Pf), (ys, Ps))]
        G0 = [Pf.crossprod(), Ps.crossprod()]
        live = bwgr_amd.debug_live()
        Kff, Kfs, G = np.empty((nf, nf)), np.empty((nf, ns)), np.empty((nf, ns), np.int64)
        pff, pfs, pg = (a.ctypes.data_as(C.c_void_p) for a in (Kff, Kfs, G))
        err = lambda: L.bwgr_last_error()     # noqa: E731
        # fp32 on either side; the message says which
        assert L.bwgr_panel_kernel2(P32._h, Ps._h, 0, 1.0, pff, ns, pfs, ns, 0) == EINVAL and b"fp32" in err() and b"founders" in err()
        assert L.bwgr_panel_kernel2(Pf._h, P32._h, 0, 1.0, pff, nf, pfs, ns, 0) == EINVAL and b"fp32" in err() and b"samples" in err()
        assert L.bwgr_panel_crossprod2(P32._h, Ps._h, pg, ns, 0) == EINVAL and b"founders" in err()
        assert L.bwgr_panel_crossprod2(Pf._h, P32._h, pg, ns, 0) == EINVAL and b"samples" in err()
        # different p
        assert L.bwgr_panel_kernel2(Pf._h, Pq._h, 0, 1.0, pff, nf, pfs, ns, 0) == EINVAL and b"markers" in err()
        assert L.bwgr_panel_crossprod2(Pf._h, Pq._h, pg, ns, 0) == EINVAL and b"markers" in err()
        with pytest.raises(ValueError):
            Pf.crossprod2(Pq)
        # an unknown kind
        for kind in (2, -1):
            assert L.bwgr_panel_kernel2(Pf._h, Ps._h, kind, 1.0, pff, nf, pfs, ns, 0) == EINVAL and b"kind" in err()
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            Pf.kernel2(Ps, 17)
        assert ei.value.code == EINVAL
        # short leading dimensions
        assert L.bwgr_panel_kernel2(Pf._h, Ps._h, 0, 1.0, pff, nf - 1, pfs, ns, 0) == EINVAL and b"leading dimension" in err()
        assert L.bwgr_panel_kernel2(Pf._h, Ps._h, 0, 1.0, pff, nf, pfs, ns - 1, 0) == EINVAL and b"leading dimension" in err()
        assert L.bwgr_panel_crossprod2(Pf._h, Ps._h, pg, ns - 1, 0) == EINVAL and b"leading dimension" in err()
        # null pointers, a bad memloc
        assert L.bwgr_panel_kernel2(Pf._h, Ps._h, 0, 1.0, None, nf, pfs, ns, 0) == EINVAL and b"null" in err()
        assert L.bwgr_panel_kernel2(Pf._h, Ps._h, 0, 1.0, pff, nf, None, ns, 0) == EINVAL and b"null" in err()
        assert L.bwgr_panel_kernel2(None, Ps._h, 0, 1.0, pff, nf, pfs, ns, 0) == EINVAL and b"null" in err()
        assert L.bwgr_panel_crossprod2(Pf._h, None, pg, ns, 0) == EINVAL and b"null" in err()
        assert L.bwgr_panel_crossprod2(Pf._h, Ps._h, None, ns, 0) == EINVAL and b"null" in err()
        assert L.bwgr_panel_crossprod2(Pf._h, Ps._h, pg, ns, 2) == EINVAL and b"memloc" in err()
        assert L.bwgr_panel_kernel2(Pf._h, Ps._h, 0, 1.0, pff, nf, pfs, ns, 7) == EINVAL and b"memloc" in err()
        assert bwgr_amd.debug_live() == live                  # a refusal leaves nothing behind
        after = [bwgr_amd.BayesRR(y, P, it=5, bi=1, seed=3) for y, P in ((yf, Pf), (ys, Ps))]
        for b0, b1 in zip(before, after):
            assert np.array_equal(b0["b"], b1["b"]) and np.array_equal(b0["hat"], b1["hat"])
        assert np.array_equal(Pf.crossprod(), G0[0]) and np.array_equal(Ps.crossprod(), G0[1])
        _same(Pf.crossprod2(Ps), K2.crossprod2(F, S))
    finally:
        Pf.close(); Ps.close(); P32.close(); Pq.close()


def test_every_entry_point_returns_what_it_took(tpod):
    """bwgr_debug_live (device arrays, streams, events owned by the library) is back at its starting counts after each call."""
    import torch   # noqa: F401  (device_out)
    import bwgr_amd
    F, S = _tpod_split(tpod)
    start = bwgr_amd.debug_live()
    Pf, Ps = bwgr_amd.Panel(F), bwgr_amd.Panel(S)
    Qs = Ps.clone()        # a clone runs on a stream of its own: the call orders the two streams with an event
    try:
        base = bwgr_amd.debug_live()
        for call in (lambda: Pf.crossprod2(Ps), lambda: Pf.crossprod2(Qs), lambda: Pf.crossprod2(Ps, device_out=True),
                     lambda: Pf.kernel2(Ps, "ARC"), lambda: Pf.kernel2(Qs, "GAU", 0.5), lambda: Pf.kernel2(Ps, "GAU", device_out=True),
                     lambda: Pf.kernel2(Ps, "ARC", device_out=True), lambda: bwgr_amd.EigenArcZ(Pf, Qs), lambda: bwgr_amd.EigenGauZ(Pf, Ps)):
            call()
            assert bwgr_amd.debug_live() == base
        with pytest.raises(bwgr_amd.BwgrError):
            Pf.kernel2(Ps, 9)
        assert bwgr_amd.debug_live() == base
    finally:
        Qs.close(); Pf.close(); Ps.close()
    # the drivers on matrices make and close their own panels
    bwgr_amd.EigenArcZ(F, S); bwgr_amd.EigenGauZ(F, S, 0.5); bwgr_amd.crossprod2(F, S)
    assert bwgr_amd.debug_live() == start
