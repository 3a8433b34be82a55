"""GPU: the transpose product X'A / X_c'A on the resident int8 panel (bwgr_panel_xta) on the shapes of
tests/mrr_svd_cases.py -- against a numpy.longdouble reference within (n + 8) 2^-53 (|X|'|A| + |xbar| sum|A|) elementwise; exact where the
arithmetic is (integer A, ones, one-hot columns, the implicit centring recomputed from the raw result); bit-equal between two calls, a host and
a device A, a panel and a wider panel of the same rows and slab height, a clone on a caller's stream, and a trait alone or in a second trait
group; with column strides beyond n and p; and the refusals of the C entry."""
import ctypes as C
import functools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrr_svd_cases as MC  # noqa: E402
import mrr_svd_restatement as SR  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _panel(name, cols=None):
    """(W, its panel) of a case, made once and shared; cols: the first columns only"""
    import bwgr_amd
    W = MC.xta_W(name)
    if cols is not None:
        W = np.ascontiguousarray(W[:, :cols])
    return W, bwgr_amd.Panel(W, block=MC.XTA[name]["block"])


def _xta(P, A, centre, **kw):
    from bwgr_amd import svd
    return svd.panel_xta(P, A, centre, **kw)


def _within_bound(out, W, A, centre):
    ref, bound = SR.xta_ld(W, A, centre)
    err = np.abs(out.astype(np.longdouble) - ref).astype(np.float64)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print("largest error / bound: %.3g" % worst)
    assert out.shape == ref.shape and np.all(np.isfinite(out))
    assert np.all(err <= bound), (worst, np.unravel_index(np.argmax(err - bound), err.shape))


@pytest.mark.parametrize("centre", [False, True])
@pytest.mark.parametrize("k", MC.XTA_K)
def test_two_slabs_every_k(k, centre):
    """300 x 700: n no multiple of 64, two slabs, p = 10 * 64 + 60; k = 1, 16, 17 (a second trait group of one), 33"""
    W, P = _panel("two_slabs")
    assert P.slab_rows == 256 and P.n == 300 and P.p % 64 != 0
    _within_bound(_xta(P, MC.xta_A("two_slabs", k), centre), W, MC.xta_A("two_slabs", k), centre)


@pytest.mark.parametrize("name", ["tall_slab", "padded_slab", "two_trips", "int8_codes"])
def test_shape_edges(name):
    """a second slab of 1 024 rows; one padded slab; a second trip of the grid; the whole int8 range with constant columns -- raw and centred"""
    from bwgr_amd import svd
    W, P = _panel(name)
    assert P.slab_rows == MC.slab_rows(P.n, P.p, MC.XTA[name]["block"])
    if name == "two_trips":
        assert svd.xta_plan(P.n, P.p, 17, P.slab_rows)["trips"] == 2
    A = MC.xta_A(name, 17)
    for centre in (False, True):
        _within_bound(_xta(P, A, centre), W, A, centre)


def test_integer_products_are_exact():
    """integer A with |a| <= 2^20: every partial sum is an integer below 2^53, so the raw product is numpy's int64 product bit for bit; ones give
    the column sums, a one-hot column a row of X"""
    for name in ("two_slabs", "int8_codes", "tall_slab"):
        W, P = _panel(name)
        rng = np.random.default_rng(5)
        A = rng.integers(-2 ** 20, 2 ** 20 + 1, (P.n, 18)).astype(np.float64)
        A[:, 0] = 1.0
        A[:, 1] = 0.0
        A[P.n - 1, 1] = 1.0
        out = _xta(P, A, False)
        want = W.astype(np.int64).T @ A.astype(np.int64)
        assert np.array_equal(out, want.astype(np.float64))
        assert np.array_equal(out[:, 0], W.sum(0, dtype=np.int64)) and np.array_equal(out[:, 1], W[P.n - 1].astype(np.float64))


def _fma(a, b, c):
    """fma(a, b, c) correctly rounded, by exact rational arithmetic"""
    v = Fraction(a) * Fraction(b) + Fraction(c)
    return v.numerator / v.denominator


@pytest.mark.parametrize("name", ["two_slabs", "int8_codes"])
def test_centring_is_the_fma_of_the_raw_result(name):
    """centre = 1 is fma(-xbar_j, s_t, raw_jt) with xbar_j the exact column sum over n and s_t the sum of A's column in the entry's stated order"""
    W, P = _panel(name)
    A = MC.xta_A(name, 3)
    raw, cen = _xta(P, A, False), _xta(P, A, True)
    xbar = W.sum(0, dtype=np.int64).astype(np.float64) / float(P.n)
    s = SR.asum(A)
    want = np.array([[_fma(-xbar[j], s[t], raw[j, t]) for t in range(3)] for j in range(P.p)])
    assert np.array_equal(cen, want)
    const = [j for j in range(P.p) if len(set(W[:, j])) == 1]
    if name == "int8_codes":
        assert len(const) >= 5 and np.all(np.abs(cen[const]) <= SR.xta_ld(W, A, True)[1][const])


def test_two_calls_and_the_device_route_give_the_same_bits():
    import torch
    W, P = _panel("two_slabs")
    A = MC.xta_A("two_slabs", 17)
    for centre in (False, True):
        a = _xta(P, A, centre)
        assert np.array_equal(a, _xta(P, A, centre))
        Ad = torch.from_numpy(A.T.copy()).cuda().t()             # n x k, column-major on the device
        d = _xta(P, Ad, centre)
        assert d.is_cuda and tuple(d.shape) == (P.p, 17) and np.array_equal(d.cpu().numpy(), a)
        assert np.array_equal(_xta(P, Ad.contiguous(), centre).cpu().numpy(), a)      # a row-major tensor is laid out anew
        t = _xta(P, A, centre, device_out=True)
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), a)


def test_a_column_does_not_depend_on_the_panels_width():
    """columns 0 .. 199 of the 700-column panel and the 200-column panel of the same rows, both with slabs of 256 rows"""
    W, P = _panel("two_slabs")
    W2, P2 = _panel("two_slabs", 200)
    assert P2.slab_rows == P.slab_rows and P2.p == 200 and np.array_equal(W2, W[:, :200])
    A = MC.xta_A("two_slabs", 16)
    for centre in (False, True):
        assert np.array_equal(_xta(P, A, centre)[:200], _xta(P2, A, centre))


def test_a_trait_does_not_depend_on_its_group():
    """trait t of a k = 17 call -- t = 16 alone in the second group -- and the same column alone"""
    W, P = _panel("two_slabs")
    A = MC.xta_A("two_slabs", 17)
    for centre in (False, True):
        full = _xta(P, A, centre)
        for t in (0, 5, 16):
            assert np.array_equal(_xta(P, A[:, t], centre)[:, 0], full[:, t])


def test_a_clone_on_a_callers_stream_gives_the_same_bits():
    import torch
    W, P = _panel("two_slabs")
    A = MC.xta_A("two_slabs", 17)
    want = _xta(P, A, True)
    Q = P.clone()
    s = torch.cuda.Stream()
    try:
        Q.set_stream(s.cuda_stream)
        assert np.array_equal(_xta(Q, A, True), want)
        Ad = torch.from_numpy(A.T.copy()).cuda().t()
        torch.cuda.synchronize()
        assert np.array_equal(_xta(Q, Ad, True).cpu().numpy(), want)
    finally:
        Q.close()
    assert np.array_equal(_xta(P, A, True), want)


def test_column_strides_beyond_n_and_p():
    """lda > n and ldo > p through the C entry, from the host and on the device: the same bits, and nothing written behind a column"""
    import torch
    from bwgr_amd import _lib
    W, P = _panel("two_slabs")
    n, p, k = P.n, P.p, 17
    A = MC.xta_A("two_slabs", k)
    want = _xta(P, A, True)
    lda, ldo = n + 5, p + 3
    Ap = np.full((lda, k), 7.0, order="F")
    Ap[:n] = A
    out = np.full((ldo, k), -3.0, order="F")
    L = _lib.lib()
    _lib.check(L.bwgr_panel_xta(P._h, Ap.ctypes.data_as(C.c_void_p), lda, k, 1, 0, out.ctypes.data_as(C.c_void_p), ldo))
    assert np.array_equal(out[:p], want) and np.all(out[p:] == -3.0)
    Ad = torch.from_numpy(Ap.T.copy()).cuda()                    # (k, lda): column t of A at row t
    od = torch.full((k, ldo), -3.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.bwgr_panel_xta(P._h, C.c_void_p(Ad.data_ptr()), lda, k, 1, 1, C.c_void_p(od.data_ptr()), ldo))
    torch.cuda.synchronize()
    oh = od.cpu().numpy().T
    assert np.array_equal(oh[:p], want) and np.all(oh[p:] == -3.0)


def test_refusals():
    import bwgr_amd
    from bwgr_amd import _lib
    W, P = _panel("int8_codes")
    n, p = P.n, P.p
    L = _lib.lib()
    A = np.zeros((n, 2), order="F")
    out = np.zeros((p, 2), order="F")
    pa, po = A.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert L.bwgr_panel_xta(P._h, pa, n, 2, 1, 0, po, p) == 0
    for args in ((None, pa, n, 2, 1, 0, po, p), (P._h, None, n, 2, 1, 0, po, p), (P._h, pa, n, 2, 1, 0, None, p),      # null pointers
                 (P._h, pa, n, 0, 1, 0, po, p), (P._h, pa, n, -1, 1, 0, po, p),                                        # k < 1
                 (P._h, pa, n, 2, 1, 2, po, p), (P._h, pa, n, 2, 1, -1, po, p),                                        # a bad memloc
                 (P._h, pa, n - 1, 2, 1, 0, po, p), (P._h, pa, n, 2, 1, 0, po, p - 1)):                                # lda < n, ldo < p
        assert L.bwgr_panel_xta(*args) == 1, args
        assert b"panel_xta" in L.bwgr_last_error()
    for bad in (np.nan, np.inf):
        A[n - 1, 1] = bad
        assert L.bwgr_panel_xta(P._h, pa, n, 2, 1, 0, po, p) == 1 and b"not finite" in L.bwgr_last_error()
    A[n - 1, 1] = 0.0
    F = bwgr_amd.Panel(W.astype(np.float32), as_int8=False)
    try:
        assert L.bwgr_panel_xta(F._h, pa, n, 2, 1, 0, po, p) == 1 and b"fp32" in L.bwgr_last_error()
        from bwgr_amd import svd
        with pytest.raises(bwgr_amd.BwgrError, match="fp32"):
            svd.panel_xta(F, np.zeros(n))
    finally:
        F.close()
