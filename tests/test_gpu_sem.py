"""GPU: X B on the panel (bwgr_panel_xb) against numpy's float64 product, and the latent-space fits XSEMF / ZSEMF / YSEMF against the float64
restatement tests/sem_restatement.py, end to end and stage by stage.

Parity is mrr_restatement.scaled_err(got, restatement) <= 1e-6 with NaN in the same places (1e-12 for the product: exact integers times
doubles, fp64 sums).  Every end-to-end comparison first asserts, on the restatement, that neighbouring singular values of G differ by at least
5 % of the largest: a precondition, not a tolerance -- near-degenerate pairs make the singular vectors ill-defined for the reference too.  The
trait seeds were picked on the CPU so that it holds (tpod, k = 4, seed 227: gaps 0.136 for XSEMF's G and 0.143 for ZSEMF's; the 700 x 900
panel, seed 302: 0.278 and 0.243)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrr_restatement as MR  # noqa: E402
import sem_restatement as SR  # noqa: E402
from test_gpu_mrr import _traits  # noqa: E402
from test_gpu_uvb import _f32, _slabs900, _tpod  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6
OUT = {"XSEMF": ("b", "GC", "hat"), "ZSEMF": ("mu", "b", "hat", "h2", "GC"), "YSEMF": ("mu", "b", "hat", "h2", "GC")}
NPC = {"0": 0, "-1": -1, "2": 2}


def _err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return MR.scaled_err(np.nan_to_num(a), np.nan_to_num(b))


def _well_posed(o):
    s = o["s"]
    gap = float(np.min(-np.diff(s)) / s[0])
    assert gap >= 0.05, (gap, s)
    return gap


def _check(name, g, o):
    assert tuple(g) == OUT[name]
    errs = {key: _err(g[key], o[key]) for key in OUT[name]}
    print(name, errs)
    assert all(v <= TOL for v in errs.values()), errs


# ---- panel_xb ----
@pytest.mark.parametrize("k", [1, 3, 17])
def test_xb_tpod(k):
    """196 x 376: one row tile with most of its threads beyond the panel, three marker chunks with a short last one; 17 columns: two slices."""
    import bwgr_amd
    X = _tpod()
    B = np.random.default_rng(k).normal(size=(376, k))
    g = bwgr_amd.panel_xb(X, B)
    assert g.shape == (196, k) and MR.scaled_err(g, X.astype(np.float64) @ B) <= 1e-12
    if k == 1:
        assert np.array_equal(bwgr_amd.panel_xb(X, B[:, 0]), g)


def test_xb_on_slabs_a_centred_panel_and_twice():
    import bwgr_amd
    X = _slabs900()
    B = np.random.default_rng(5).normal(size=(900, 5))
    live = bwgr_amd.debug_live()
    P = bwgr_amd.Panel(X, nwg=3)
    try:
        assert P.nwg == 3 and P.n == 700
        inside = bwgr_amd.debug_live()
        a, b = P.xb(B), P.xb(B)
        assert bwgr_amd.debug_live() == inside
        P.set_centred(True)
        c = P.xb(B)
        P.set_centred(False)
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            P.xb(B[:-1])
        assert ei.value.code == 1
        d = P.xb(B)
    finally:
        P.close()
    assert bwgr_amd.debug_live() == live
    assert MR.scaled_err(a, X.astype(np.float64) @ B) <= 1e-12
    for other in (b, c, d):   # raw genotypes: implicit centring does not change a bit
        assert np.array_equal(a, other)


def test_xb_signed_codes_and_refusals():
    import bwgr_amd
    rng = np.random.default_rng(91)
    X = rng.integers(-128, 128, size=(300, 200)).astype(np.int8)
    X[0, 0], X[1, 0] = -128, 127
    X = np.asfortranarray(X)
    B = rng.normal(size=(200, 4))
    assert MR.scaled_err(bwgr_amd.panel_xb(X, B), X.astype(np.float64) @ B) <= 1e-12
    P = bwgr_amd.Panel(X.astype(np.float32) + 0.5)
    try:
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            P.xb(B)
    finally:
        P.close()
    assert ei.value.code == 1 and "fp32" in str(ei.value)
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.panel_xb(X, B[:, :0])
    assert ei.value.code == 1 and "k = 0" in str(ei.value)


# ---- the drivers on tpod ----
@functools.lru_cache(None)
def _tpod_traits():
    Y = _f32(_traits(_tpod(), 4, 0.1, seed=227))
    Y.setflags(write=False)
    return Y


@functools.lru_cache(None)
def _tpod_ref(name, npc):
    return getattr(SR, name)(_tpod_traits(), _tpod(), npc, maxit=6, tol=0)


@pytest.mark.parametrize("npc", list(NPC))
@pytest.mark.parametrize("name", ["XSEMF", "ZSEMF", "YSEMF"])
def test_drivers_end_to_end(name, npc):
    import bwgr_amd
    o = _tpod_ref(name, NPC[npc])
    _well_posed(o)
    assert o["npc"] == {"0": 4, "-1": 4, "2": 2}[npc]
    g = getattr(bwgr_amd, name)(_tpod_traits(), _tpod(), NPC[npc], maxit=6, tol=0)
    _check(name, g, o)
    if name == "XSEMF":
        assert g["b"].shape == (376, 4) and g["GC"].shape == (4, 4) and g["hat"].shape == (196, 4)


@pytest.mark.parametrize("name", ["XSEMF", "YSEMF"])
def test_drivers_stage_by_stage(name):
    """The stages the driver is composed of, called as the driver calls them: BETA, G, Z up to the sign of each column, the second stage's
    coefficients (signs matched), and YSEMF's third fit on Y - G."""
    import bwgr_amd
    from bwgr_amd import api
    X, Y = _tpod(), _tpod_traits()
    o = _tpod_ref(name, 0)
    _well_posed(o)
    v = "X" if name == "XSEMF" else "Z"
    P = bwgr_amd.Panel(X)
    try:
        s1 = bwgr_amd.uvbeta(Y, P, v, maxit=6, tol=0)
        G = P.xb(s1["b"])
        Z, V = api._sem_latent(G, 0, name)
        s2 = bwgr_amd.uvbeta_dense(Y, Z, v, maxit=6, tol=0)
        if name == "YSEMF":
            s3 = api._uvb_panel(P, Y - o["G_fa"], api.UVB_VARIANTS["Z"], 6, 0.0, float(np.float32(20.0)))
    finally:
        P.close()
    assert _err(s1["b"], o["BETA"]["b"]) <= TOL and _err(G, o["G"]) <= TOL
    sign = np.sign((Z * o["Z"]).sum(0))
    assert np.all(sign != 0)
    assert _err(Z * sign, o["Z"]) <= TOL and _err(V * sign, o["V"]) <= TOL
    assert _err(s2["b"] * sign[:, None], o["second"]["b"]) <= TOL
    for key in ("mu", "cnv") + (() if v == "X" else ("ve", "vb", "h2")):
        assert _err(s2[key], o["second"][key]) <= TOL, key
    assert np.array_equal(s2["its"], o["second"]["its"])
    if name == "YSEMF":
        for key in ("b", "mu", "h2"):
            assert _err(s3[key], o["third"][key]) <= TOL, key


# ---- the reference's defaults ----
def _strong(X, k, seed):
    """k traits with strong signal on scales 1, 2, 4 (so that G's singular values lie well apart), 10 % missing."""
    rng = np.random.default_rng(seed)
    Xf = X.astype(np.float64)
    n, p = X.shape
    G = (Xf - Xf.mean(0)) @ (rng.normal(size=(p, k)) / np.sqrt(p))
    Y = G / G.std(0) * np.array([1.0, 2.0, 4.0])[:k] + 0.5 * rng.normal(size=(n, k)) + 3.0
    Y[rng.random((n, k)) < 0.1] = np.nan
    return _f32(Y)


@functools.lru_cache(None)
def _slab_traits():
    return _strong(_slabs900(), 3, seed=302)


@pytest.mark.parametrize("name", ["XSEMF", "ZSEMF", "YSEMF"])
def test_drivers_with_the_references_defaults(name):
    """maxit = 100, tol = 10e-7 on the 700 x 900 three-slab panel: every stage stops by its own test, and no trait's cnv comes nearer than
    0.02 to log10(tol) at any sweep of any stage of the restatement (asserted; the nearest is 0.025), so the sweep counts agree."""
    import bwgr_amd
    X, Y = _slabs900(), _slab_traits()
    o = getattr(SR, name)(Y, X)
    _well_posed(o)
    stages = [o["BETA"], o["second"]] + ([o["third"]] if name == "YSEMF" else [])
    logtol = np.log10(float(np.float32(10e-7)))
    near = min(abs(c - logtol) for d in stages for tr in d["trace"] for c in tr)
    print(name, [list(d["its"]) for d in stages], near)
    assert near >= 0.02 and all(d["its"].max() < 100 for d in stages) and o["npc"] == 3
    P = bwgr_amd.Panel(X, nwg=3)
    try:
        g = getattr(bwgr_amd, name)(Y, P)
        again = P.xb(g["b"])      # the panel that was passed in stays usable
    finally:
        P.close()
    _check(name, g, o)
    assert MR.scaled_err(again, X.astype(np.float64) @ g["b"]) <= 1e-12


# ---- degenerate input, refusals, state ----
@pytest.mark.parametrize("name", ["XSEMF", "ZSEMF", "YSEMF"])
def test_an_all_nan_trait_among_others(name):
    """Trait 2 has no record: its columns of b and G are zero, G has rank 3 and the three latent columns carry everything (npc = 3: a fourth
    would be the null direction, which is not defined).  Its row and column of GC are 0 / 0 = NaN, exactly where the restatement's are."""
    import bwgr_amd
    X = _tpod()
    Y = np.array(_tpod_traits())
    Y[:, 2] = np.nan
    o = getattr(SR, name)(Y, X, 3, maxit=6, tol=0)
    gap = -np.diff(o["s"][:3]) / o["s"][0]
    assert gap.min() >= 0.05 and o["s"][3] <= 1e-12 * o["s"][0], o["s"]
    assert np.isnan(o["GC"][2]).all() and np.isnan(o["GC"][:, 2]).all() and np.isfinite(np.delete(np.delete(o["GC"], 2, 0), 2, 1)).all()
    g = getattr(bwgr_amd, name)(Y, X, 3, maxit=6, tol=0)
    _check(name, g, o)
    assert not g["b"][:, 2].any()
    if name != "XSEMF":
        assert not g["hat"][:, 2].any() and g["mu"][2] == 0 and g["h2"][2] == 0


def test_refusals_and_live_counts():
    import bwgr_amd
    X, Y = _tpod(), _tpod_traits()
    live = bwgr_amd.debug_live()
    for fn, npc in ((bwgr_amd.XSEMF, 5), (bwgr_amd.ZSEMF, 5), (bwgr_amd.YSEMF, 7)):
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            fn(Y, X, npc, maxit=2, tol=0)
        assert ei.value.code == 1 and "npc" in str(ei.value)
        assert bwgr_amd.debug_live() == live
    with pytest.raises(bwgr_amd.BwgrError) as ei:     # the reference's default npc = -1 needs min(n, k) >= 3
        bwgr_amd.YSEMF(Y[:, :2], X, maxit=2, tol=0)
    assert ei.value.code == 1 and bwgr_amd.debug_live() == live
    P = bwgr_amd.Panel(X)
    try:
        inside = bwgr_amd.debug_live()
        a = bwgr_amd.ZSEMF(Y, P, 2, maxit=3, tol=0)
        assert bwgr_amd.debug_live() == inside
        with pytest.raises(bwgr_amd.BwgrError):
            bwgr_amd.ZSEMF(Y, P, 9, maxit=3, tol=0)
        assert bwgr_amd.debug_live() == inside
        b = bwgr_amd.ZSEMF(Y, P, 2, maxit=3, tol=0)   # the panel stays usable, and the result is the same bits
    finally:
        P.close()
    assert bwgr_amd.debug_live() == live
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
