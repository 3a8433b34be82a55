"""GPU: k_sweep3f, the fixed-shape instantiation of the trajectory engine (128-marker blocks, 16-bit Gram entries, 128-row DMA streamers), against
k_sweep3 on the same panel and against the CPU oracle.

Each case builds its panel twice -- as shipped, and with BWGR_FIXED3=0 (the switch is read when a root panel is made) -- asserts through
bwgr_debug_sweep3_kernel() that the two runs were launched as k_sweep3f and as k_sweep3, and asks for the same bits in every returned array: the two
kernels are one source, the fixed one with the block geometry as constants.  The oracle comparison uses test_gpu_parity.py's tolerances.

Shapes, n = 600 rows (the suite's conftest forces k_sweep3 for every selection sweep, whatever the inclusion rate):
  nwg = 5: five slabs of 128 rows, a streamer each;  nwg = 3: three slabs of 256 rows, converted to two 128-row streamers a slab (sub = 2)
  p = 1536: twelve whole blocks, the far field at its full depth D = 12;  p = 1600: a last block of 64 markers (no second half);
  p = 1764: a last block of 100 markers;  p = 640: five blocks, D clamped to 5
  pi = 0.99: sparse lists;  pi = 0.7: about 38 included markers a block -- more than the eight row slots of a block (S3_NRX) and more far-field rows
  than a wave keeps in flight."""
import ctypes as C

import numpy as np
import pytest

from conftest import scaled_err, synth_small

pytestmark = pytest.mark.gpu
TOL = 1e-6   # (tests/test_gpu_parity.py)
N, IT, BI = 600, 5, 1
GENERIC, FIXED = 1, 2

CASES = [(1536, 5, 0.99), (1536, 5, 0.7), (1600, 5, 0.99), (1600, 5, 0.7), (1764, 5, 0.99), (1764, 5, 0.7), (640, 5, 0.99), (640, 5, 0.7),
         (1536, 3, 0.99), (1600, 3, 0.7)]


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def _which(P):
    from bwgr_amd import _lib
    w = C.c_int(-1)
    _lib.check(_lib.lib().bwgr_debug_sweep3_kernel(P._h, C.byref(w)))
    return w.value


_data = {}


def _inputs(p):
    if p not in _data:
        _data[p] = synth_small(N, p, seed=100 + p)
    return _data[p]


def _chain(monkeypatch, fixed, X, y, model, pi, nwg, block=0):
    import bwgr_amd
    if fixed:
        monkeypatch.delenv("BWGR_FIXED3", raising=False)
    else:
        monkeypatch.setenv("BWGR_FIXED3", "0")
    P = bwgr_amd.Panel(X, nwg=nwg, block=block)
    info = {"which": _which(P), "block": P.block, "nwg": P.nwg, "slab_rows": P.slab_rows, "generation": P.pipeline(True)["generation"]}
    ch = bwgr_amd.Chain(P, model, y, it=IT, bi=BI, pi=pi, df=5, R2=0.5, seed=23)
    ch.run(IT)
    res, st = ch.result(), ch.state()
    assert _which(P) == info["which"]   # (a live chain is no clone: the selection stands)
    ch.close(); P.close()
    return info, res, st


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


@pytest.mark.parametrize("model", ["BayesB", "BayesC"])
@pytest.mark.parametrize("p,nwg,pi", CASES)
def test_fixed_kernel_runs_the_same_chain(monkeypatch, model, p, nwg, pi):
    from oracle import oracle as O
    X, y = _inputs(p)
    f, rf, sf = _chain(monkeypatch, True, X, y, model, pi, nwg)
    assert f == {"which": FIXED, "block": 128, "nwg": nwg, "slab_rows": 128 if nwg == 5 else 256, "generation": 3}
    g, rg, sg = _chain(monkeypatch, False, X, y, model, pi, nwg)
    assert g == dict(f, which=GENERIC)
    _same(rf, rg, "result"); _same(sf, sg, "state")
    if pi == 0.7:   # the dense setting does fill more than a block's row slots (expected 38 a block)
        d = np.asarray(sf["d"])
        assert max(d[j:j + 128].sum() for j in range(0, p, 128)) > 8
    o = O.bayes(model, y, X, it=IT, bi=BI, pi=pi, df=5, R2=0.5, seed=23)
    assert scaled_err(rf["b"], o["b"]) < TOL
    assert scaled_err(rf["hat"], o["hat"]) < TOL
    assert _rel(rf["ve"], o["ve"]) < TOL and _rel(rf["mu"], o["mu"]) < TOL and _rel(rf["h2"], o["h2"]) < 5 * TOL
    assert scaled_err(np.atleast_1d(rf["vb"]), np.atleast_1d(o["vb"])) < 5 * TOL
    assert np.array_equal(rf["d"], o["d"])
    assert scaled_err(sf["e"], o["last"]["e"]) < TOL
    assert scaled_err(sf["b"], o["last"]["b"]) < TOL
    assert _rel(sf["ve"], o["last"]["ve"]) < TOL


def test_other_block_sizes_keep_the_generic_kernel(monkeypatch):
    """64-marker blocks do not match the fixed shape: k_sweep3 serves them, as shipped and with the switch off, and the chain is the oracle's."""
    from oracle import oracle as O
    X, y = _inputs(640)
    i1, r1, s1 = _chain(monkeypatch, True, X, y, "BayesB", 0.9, 5, block=64)
    assert i1 == {"which": GENERIC, "block": 64, "nwg": 5, "slab_rows": 128, "generation": 3}
    i0, r0, s0 = _chain(monkeypatch, False, X, y, "BayesB", 0.9, 5, block=64)
    assert i0 == i1
    _same(r1, r0, "result"); _same(s1, s0, "state")
    o = O.bayes("BayesB", y, X, it=IT, bi=BI, pi=0.9, df=5, R2=0.5, seed=23)
    assert scaled_err(r1["b"], o["b"]) < TOL and scaled_err(s1["e"], o["last"]["e"]) < TOL and np.array_equal(r1["d"], o["d"])
