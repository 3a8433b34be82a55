"""CPU: the founder-by-sample kernels' restatement against itself, the rectangular product's plan (bwgr_debug_xyt_plan: host arithmetic), the
Python signatures (R/RcppExports.R:248-254) and the refusals that need no GPU."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernels2_restatement as K2   # noqa: E402
from conftest import scaled_err, synth_small   # noqa: E402

EINVAL = 1


def _splits(tpod):
    """(name, founders, samples): the tpod genotypes 130 / 66, a binomial panel 300 / 200, a signed panel 70 / 50"""
    T = np.ascontiguousarray(tpod["gen"]).astype(np.int8)
    S = np.ascontiguousarray(synth_small(500, 900, seed=3)[0])
    Z = np.random.default_rng(21).integers(-2, 3, size=(120, 400)).astype(np.int8)
    return [("tpod", T[:130], T[130:]), ("synth", S[:300], S[300:]), ("signed", Z[:70], Z[70:])]


def test_centring_identity_equals_the_direct_product(tpod):
    for name, F, S in _splits(tpod):
        for k, (a, b) in enumerate(zip(K2.arc_centred_identity(F, S), K2.arc_centred_direct(F, S))):
            err = scaled_err(a, b)
            print(name, ("A_ff", "A_fs", "d_s")[k], "identity against the direct form:", err)
            assert err <= 1e-12, (name, k, err)
        for a, b in zip(K2.arc_kernels(F, S), K2.arc_kernels(F, S, direct=True)):
            assert scaled_err(a, b) <= 1e-12


def test_restated_kernels_are_finite_and_symmetric(tpod):
    for name, F, S in _splits(tpod):
        for kind, phi in (("ARC", 1.0), ("GAU", 1.0), ("GAU", 0.5)):
            Kff, Kfs = K2.kernels(kind, F, S, phi)
            assert Kff.shape == (F.shape[0], F.shape[0]) and Kfs.shape == (F.shape[0], S.shape[0])
            assert np.all(np.isfinite(Kff)) and np.all(np.isfinite(Kfs)), (name, kind)
            assert np.array_equal(Kff, Kff.T), (name, kind)
            if kind == "GAU":
                assert np.array_equal(np.diag(Kff), np.ones(F.shape[0]))
            else:
                assert abs(np.mean(np.diag(Kff)) - 1.0) <= 1e-12
        # with the samples = the founders the two blocks coincide
        for kind in ("ARC", "GAU"):
            Kff, Kfs = K2.kernels(kind, F, F)
            assert scaled_err(Kfs, Kff) <= 1e-12


def test_restated_eigenarcz_of_the_founders_reproduces_kff(tpod):
    for name, F, _ in _splits(tpod):
        Z = K2.EigenArcZ(F, F)
        Kff = K2.arc_kernels(F, F)[0]
        err = scaled_err(Z @ Z.T, Kff)
        print(name, "Z Z' against K_ff:", err, "cond", np.linalg.cond(Kff))
        assert Z.shape == (F.shape[0], F.shape[0]) and err <= 1e-9, (name, err)


def _plan(nf, ns, p, xf, xs, kchunk=0):
    from bwgr_amd import _lib
    L = _lib.lib()
    out = (C.c_int64 * 10)(*([-1] * 10))
    rc = L.bwgr_debug_xyt_plan(nf, ns, p, xf, xs, kchunk, out)
    assert out[9] == -1      # BWGR_XYT_PLAN_NOUT = 9 values
    return rc, [int(v) for v in out[:9]], L.bwgr_last_error().decode()


CHUNK, NCHUNKS, TILES, WGS, WS, TF, TS, SUB, PIECE = range(9)


def test_xyt_plan_nout_is_nine():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert int(re.search(r"#define\s+BWGR_XYT_PLAN_NOUT\s+(\d+)", open(os.path.join(root, "include", "bwgr.h")).read()).group(1)) == 9


def test_xyt_plan_chunk_rule_with_mixed_maxima():
    rc, o, _ = _plan(96, 40, 140000, 2, 128)
    assert rc == 0 and o[CHUNK] == (2 ** 31 - 1) // 256 == 8388607
    for xf, xs in ((1, 1), (2, 2), (2, 3), (127, 128), (128, 128), (0, 0), (0, 5)):
        rc, o, msg = _plan(96, 40, 140000, xf, xs)
        chunk = (2 ** 31 - 1) // (max(xf, 1) * max(xs, 1))
        assert rc == 0 and o[CHUNK] == chunk and o[NCHUNKS] == -(-140000 // chunk), (xf, xs, o, msg)
    assert _plan(96, 40, 140000, 128, 128)[1][NCHUNKS] == 2       # the full-range panels of the GPU tests: two natural chunks
    # the rule is symmetric in the two maxima
    assert _plan(96, 40, 140000, 2, 128)[1][:4] == _plan(96, 40, 140000, 128, 2)[1][:4]


def test_xyt_plan_tiles_pieces_and_accumulate():
    for nf, ns in ((2, 2), (128, 2), (130, 257), (257, 130), (700, 300), (5000, 5000), (10000, 500)):
        for p, k in ((900, 64), (900, 100), (1, 0), (65, 0), (50000, 0), (50000, 1000)):
            rc, o, msg = _plan(nf, ns, p, 2, 2, k)
            assert rc == 0, msg
            chunk = k if k else 536870911
            Tf, Ts = -(-nf // 128), -(-ns // 128)
            assert o[CHUNK] == chunk and o[NCHUNKS] == -(-p // chunk)
            assert o[TF] == Tf and o[TS] == Ts and o[TILES] == Tf * Ts          # every tile: no triangle
            # the pieces are whole 64-marker steps and cover a chunk
            span = min(chunk, p)
            assert o[PIECE] % 64 == 0 and o[SUB] * o[PIECE] >= span and (o[SUB] - 1) * o[PIECE] < span
            assert o[WGS] == o[TILES] * o[NCHUNKS] * o[SUB]
            # the workgroups of a tile add into it exactly when there are several of them
            assert (o[WGS] > o[TILES]) == (o[NCHUNKS] * o[SUB] > 1)
    # a forced chunk beyond the exact range is cut to the rule
    rc, o, _ = _plan(96, 40, 140000, 128, 128, 10 ** 6)
    assert rc == 0 and o[CHUNK] == 131071
    rc, o, _ = _plan(96, 40, 140000, 2, 128, 10 ** 8)
    assert rc == 0 and o[CHUNK] == 8388607
    # small panels: chunks are split again so that the launch fills the chip; large ones: they are not
    assert _plan(130, 66, 1000000, 2, 2)[1][SUB] > 1
    assert _plan(10000, 10000, 100000, 2, 2)[1][SUB] == 1
    # with the same panel on both sides the chunks and pieces are those of the symmetric product's plan
    from bwgr_amd import _lib
    sym = (C.c_int64 * 8)()
    assert _lib.lib().bwgr_debug_xxt_plan(5000, 50000, 2, 0, sym) == 0
    o = _plan(5000, 5000, 50000, 2, 2)[1]
    assert (o[CHUNK], o[NCHUNKS]) == (sym[0], sym[1]) and o[TILES] == sym[5] * sym[5]


def test_xyt_plan_workspace_bytes():
    for nf, ns, p in ((130, 66, 376), (300, 200, 900), (10000, 500, 100000)):
        rc, o, _ = _plan(nf, ns, p, 2, 2)
        ldf, lds = -(-nf // 128) * 128, -(-ns // 128) * 128
        # the n_f x n_s and n_f x n_f 8-byte arrays; s (int32) and q; X_f s, X_s s, the samples' row sums of squares; the founders' diagonal; the
        # partial sums of the distance sum (1024 + 1); two doubles per founder and per sample
        want = nf * ns * 8 + nf * nf * 8 + p * 12 + (ldf + 2 * lds) * 8 + nf * 8 + 1025 * 8 + (nf + ns) * 16
        assert rc == 0 and o[WS] == want, (nf, ns, p, o[WS], want)


def test_xyt_plan_refusals():
    for args in ((1, 10, 10, 2, 2, 0), (10, 1, 10, 2, 2, 0), (10, 10, 0, 2, 2, 0), (10, 10, 10, 129, 2, 0), (10, 10, 10, 2, 129, 0),
                 (10, 10, 10, -1, 2, 0), (10, 10, 10, 2, -1, 0), (10, 10, 10, 2, 2, -5), (2 ** 31, 10, 10, 2, 2, 0), (10, 2 ** 31, 10, 2, 2, 0)):
        rc, _, msg = _plan(*args)
        assert rc == EINVAL and msg, (args, rc, msg)
    big = 2 ** 31 - 512              # within the panel range
    # X_f s_f: max|x_f|^2 * n_f * p >= 2^63
    rc, _, msg = _plan(big, 10, big, 128, 1)
    assert rc == EINVAL and "2^63" in msg and "X_f s" in msg, msg
    # X_s s_f: max|x_f| * max|x_s| * n_f * p >= 2^63 while the founders' own bound holds
    rc, _, msg = _plan(big, 10, big, 1, 128)
    assert rc == EINVAL and "2^63" in msg and "X_s s" in msg, msg
    assert _plan(10, big, big, 1, 128)[0] == 0       # the samples' row count does not enter
    # (max|x_f| max|x_s| p >= 2^53 cannot be reached by an int8 panel within the panel range: 2^14 * 2^31 = 2^45)
    # a chunk so short that the chunks exceed the launch grid
    rc, _, msg = _plan(1000, 1000, 10 ** 7, 2, 2, 64)
    assert rc == EINVAL and "BWGR_KCHUNK" in msg, msg
    # more tiles than the launch grid takes
    rc, _, msg = _plan(big, big, 1, 1, 1)
    assert rc == EINVAL and "tiles" in msg, msg
    from bwgr_amd import _lib
    assert _lib.lib().bwgr_debug_xyt_plan(10, 10, 10, 2, 2, 0, None) == EINVAL


def test_python_signatures_match_the_reference():
    """R/RcppExports.R:248-254: names, positional order, defaults."""
    import bwgr_amd as B

    def pos(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
    E = inspect.Parameter.empty
    assert pos(B.EigenArcZ) == [("Zfndr", E), ("Zsamp", E), ("cores", 1)]
    assert pos(B.EigenGauZ) == [("Zfndr", E), ("Zsamp", E), ("phi", 1.0), ("cores", 1)]
    assert pos(B.crossprod2) == [("Xf", E), ("Xs", E)]
    for f in (B.EigenArcZ, B.EigenGauZ):
        assert inspect.signature(f).parameters["parts"].kind == inspect.Parameter.KEYWORD_ONLY
        assert inspect.signature(f).parameters["parts"].default is False
        assert "up to sign" in f.__doc__ and "rotation" in f.__doc__
    for f in (B.crossprod2, B.Panel.crossprod2, B.Panel.kernel2):
        assert inspect.signature(f).parameters["device_out"].kind == inspect.Parameter.KEYWORD_ONLY
        assert inspect.signature(f).parameters["device_out"].default is False
    assert pos(B.Panel.crossprod2) == [("self", E), ("other", E)]
    assert pos(B.Panel.kernel2) == [("self", E), ("other", E), ("kind", E), ("par", 1.0)]
    assert B.KERNELS2 == {"ARC": 0, "GAU": 1}


def test_bad_inputs_are_refused_before_the_library(monkeypatch):
    import torch
    import bwgr_amd as B
    from bwgr_amd import _lib

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    I = np.array([[0, 1, 2], [1, 1, 0], [2, 0, 1]], np.int8)
    fns = (B.EigenArcZ, B.EigenGauZ, B.crossprod2)
    for f in fns:
        with pytest.raises(ValueError, match="columns"):          # different column counts
            f(I, I[:, :2])
        with pytest.raises(ValueError, match="columns"):
            f(I.astype(np.float64), np.zeros((5, 4)))
        for bad in (np.array([[0.0, 1.0, 2.0], [1.0, 0.5, 0.0]]), np.array([[0.0, 200.0, 1.0]]), np.array([[0.0, np.nan, 1.0]])):
            with pytest.raises(ValueError, match="integer genotypes"):   # non-integer floats, on either side
                f(bad, I)
            with pytest.raises(ValueError, match="integer genotypes"):
                f(I, bad)
        with pytest.raises(ValueError, match="int8"):              # an fp32 tensor (p, ldx), on either side
            f(torch.zeros((3, 8), dtype=torch.float32), I)
        with pytest.raises(ValueError, match="int8"):
            f(I, torch.zeros((3, 8), dtype=torch.float32))


def test_no_cpu_fallback_for_the_kernels2():
    import bwgr_amd as B
    X = np.array([[0, 1, 2, 1], [1, 1, 0, 2], [2, 0, 1, 1]], np.int8)
    if B.device_count() > 0:
        assert B.crossprod2(X, X[:2]).dtype == np.int64         # (with a GPU: the functions run)
        return
    for f in (B.EigenArcZ, B.EigenGauZ, B.crossprod2):
        with pytest.raises(B.BwgrError) as ei:
            f(X, X)
        assert ei.value.code == 5   # BWGR_ENODEV
