"""CPU: the relationship kernels' restatement against itself, the product's plan (bwgr_debug_xxt_plan: host arithmetic), the Python
signatures (R/RcppExports.R:100-150) and the refusals that need no GPU."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernels_restatement as KR   # noqa: E402
from conftest import scaled_err, synth_small   # noqa: E402

EINVAL = 1


def _panels(tpod):
    return [("tpod", np.ascontiguousarray(tpod["gen"]).astype(np.int8)), ("synth", np.ascontiguousarray(synth_small(700, 900, seed=3)[0]))]


def test_centring_identity_equals_the_direct_product(tpod):
    for name, X in _panels(tpod):
        err = scaled_err(KR.zz_identity(X), KR.zz_direct(X))
        print(name, "centring identity against (X - mean)(X - mean)':", err)
        assert err <= 1e-12, (name, err)


def test_restated_kernels_are_finite_symmetric_and_well_defined(tpod):
    for name, X in _panels(tpod):
        G = KR.crossprod(X)
        d = np.diag(G)
        d2 = d[:, None] + d[None, :] - 2 * G
        off = d2[~np.eye(G.shape[0], dtype=bool)]
        assert off.min() == (2 if name == "tpod" else 530), (name, off.min())    # no duplicate rows: md > 0, sqrt well away from 0
        for kind, kw in KR.KINDS:
            K = KR.restate(kind, X, **kw)
            assert K.shape == G.shape and np.all(np.isfinite(K)), (name, kind, kw)
            assert np.array_equal(K, K.T), (name, kind, kw)
            if kind in ("GAU", "EigenGAU"):
                assert np.array_equal(np.diag(K), np.ones(G.shape[0])), (name, kind)
        # EigenARC's acos argument: at most 1 / sqrt(1.001) by construction (Cauchy-Schwarz on the Gram matrix)
        for cen in (True, False):
            A = KR.zz_identity(X) if cen else G.astype(np.float64)
            dg = np.diag(A)
            arg = np.abs(A / np.sqrt(dg[:, None] * dg[None, :] * 1.001))
            assert arg.max() <= 1.0 / np.sqrt(1.001) + 1e-12


def _plan(n, p, xmax, kchunk=0):
    from bwgr_amd import _lib
    L = _lib.lib()
    out = (C.c_int64 * 8)()
    rc = L.bwgr_debug_xxt_plan(n, p, xmax, kchunk, out)
    return rc, [int(v) for v in out], L.bwgr_last_error().decode()


def test_xxt_plan_chunk_rule():
    for xmax, chunk in ((1, 2147483647), (2, 536870911), (3, 238609294), (127, 133144), (128, 131071)):
        rc, o, _ = _plan(96, 140000, xmax)
        assert rc == 0 and o[0] == chunk == (2 ** 31 - 1) // (xmax * xmax), (xmax, o)
        assert o[1] == -(-140000 // chunk)
    rc, o, _ = _plan(96, 140000, 128)
    assert o[1] == 2                                  # the full-range panel of the GPU tests: two natural chunks
    rc, o, _ = _plan(10000, 1000000, 2)               # C4: one chunk
    assert rc == 0 and o[1] == 1
    T = (10000 + 127) // 128
    assert o[5] == T and o[2] == T * (T + 1) // 2
    assert o[3] == o[2] * o[1] * o[6]                 # workgroups = tiles x chunks x pieces
    assert o[4] >= 10000 * 10000 * 8                  # a host-output call holds one n x n 8-byte array


def test_xxt_plan_forced_chunk_and_tiles():
    for n in (2, 128, 129, 130, 257, 700, 5000):
        for p, k in ((900, 64), (900, 100), (1, 0), (65, 0), (50000, 0), (50000, 1000)):
            rc, o, msg = _plan(n, p, 2, k)
            assert rc == 0, msg
            chunk = k if k else 536870911
            T = -(-n // 128)
            assert o[0] == chunk and o[1] == -(-p // chunk) and o[5] == T and o[2] == T * (T + 1) // 2
            # the pieces are whole 64-marker steps and cover a chunk
            assert o[7] % 64 == 0 and o[6] * o[7] >= min(chunk, p) and (o[6] - 1) * o[7] < min(chunk, p)
            assert o[3] == o[2] * o[1] * o[6]
    # a forced chunk beyond the exact range is cut to the rule
    rc, o, _ = _plan(96, 140000, 128, 10 ** 6)
    assert rc == 0 and o[0] == 131071
    # small n: chunks are split again so that the launch fills the chip; large n: they are not
    assert _plan(196, 1000000, 2)[1][6] > 1
    assert _plan(10000, 100000, 2)[1][6] == 1


def test_xxt_plan_refusals():
    for args in ((1, 10, 2, 0), (10, 0, 2, 0), (10, 10, 129, 0), (10, 10, -1, 0), (10, 10, 2, -5)):
        rc, _, msg = _plan(*args)
        assert rc == EINVAL and msg, (args, rc, msg)
    # xmax^2 * n * p >= 2^63: n = p = 2^31 - 512 (within the panel range), xmax = 128
    big = 2 ** 31 - 512
    rc, _, msg = _plan(big, big, 128)
    assert rc == EINVAL and "2^63" in msg, msg
    # a chunk so short that the chunks exceed the launch grid
    rc, _, msg = _plan(1000, 10 ** 7, 2, 64)
    assert rc == EINVAL and "BWGR_KCHUNK" in msg, msg


def test_python_signatures_match_the_reference():
    """R/RcppExports.R:100-106, 140-150: names, positional order, defaults."""
    import bwgr_amd as B

    def pos(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
    E = inspect.Parameter.empty
    assert pos(B.GRM) == [("X", E), ("Code012", False)]
    assert pos(B.GAU) == [("X", E)]
    assert pos(B.EigenGRM) == [("X", E), ("centralizeZ", True), ("cores", 1)]
    assert pos(B.EigenGAU) == [("X", E), ("phi", 1.0), ("cores", 1)]
    assert pos(B.EigenARC) == [("X", E), ("centralizeX", True), ("cores", 1)]
    assert pos(B.crossprod) == [("X", E)]
    for f in (B.GRM, B.GAU, B.EigenGRM, B.EigenGAU, B.EigenARC, B.crossprod):
        assert inspect.signature(f).parameters["device_out"].kind == inspect.Parameter.KEYWORD_ONLY
        assert inspect.signature(f).parameters["device_out"].default is False
    assert callable(B.Panel.kernel) and callable(B.Panel.crossprod)


def test_a_non_integer_float_matrix_is_refused_before_the_library():
    import bwgr_amd as B
    X = np.array([[0.0, 1.0, 2.0], [1.0, 0.5, 0.0], [2.0, 1.0, 1.0]])
    for f in (B.GRM, B.GAU, B.EigenGRM, B.EigenGAU, B.EigenARC, B.crossprod):
        with pytest.raises(ValueError):
            f(X)
    with pytest.raises(ValueError):
        B.GRM(np.array([[0.0, 200.0], [1.0, 2.0]]))
    with pytest.raises(ValueError):
        B.GRM(np.array([[0.0, np.nan], [1.0, 2.0]]))


def test_no_cpu_fallback_for_the_kernels():
    import bwgr_amd as B
    if B.device_count() > 0:
        X = np.array([[0, 1, 2, 1], [1, 1, 0, 2], [2, 0, 1, 1]], np.int8)    # (with a GPU: the functions run)
        assert B.crossprod(X).dtype == np.int64
        return
    X = np.zeros((8, 4), np.int8)
    for f in (B.GRM, B.GAU, B.EigenGRM, B.EigenGAU, B.EigenARC, B.crossprod):
        with pytest.raises(B.BwgrError) as ei:
            f(X)
        assert ei.value.code == 5   # BWGR_ENODEV
        with pytest.raises(B.BwgrError) as ei:
            f(X.astype(np.float64))     # an all-integer float matrix is an int8 panel
        assert ei.value.code == 5
