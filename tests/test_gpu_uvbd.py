"""GPU: the per-trait ridge fits on a small dense design (bwgr_uvbeta_dense, one workgroup per trait) against the float64 restatement
tests/uvb_restatement.py, which takes a dense design as it takes genotypes: every variant, the edges of q and n (one row per thread, several,
the last size whose residual stays in LDS and the first that does not), more workgroups than compute units, a padded Z, missingness, columns
without variance, solver1xF's threshold, per-trait stopping and frozen traits, repeatability, the refusals and the live counts.

Parity is mrr_restatement.scaled_err(got, restatement) <= 1e-6 on b, mu, ve, vb, h2, cnv (NaN in the same places) and equal its.  Shapes are
the smallest that reach each path; Z is standard normal."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uvb_restatement as UR  # noqa: E402
from test_gpu_uvb import KEYS, _check, _f32  # noqa: E402

pytestmark = pytest.mark.gpu


def _case(n, q, k, seed, frac=0.1, signal=1.0):
    """Z ~ N(0, 1); Y = signal * Z beta + noise + 3 with `frac` of every trait missing."""
    rng = np.random.default_rng(seed)
    Z = np.asfortranarray(rng.normal(size=(n, q)))
    Y = signal * (Z @ rng.normal(size=(q, k))) / np.sqrt(q) + rng.normal(size=(n, k)) + 3.0
    if frac:
        Y[rng.random((n, k)) < frac] = np.nan
    return Y, Z


def _ref(Y, Z, variant, **kw):
    return UR.uvbeta(Y if variant == "D" else _f32(Y), Z, variant, **kw)


def _both(Y, Z, variant, **kw):
    import bwgr_amd
    g = bwgr_amd.uvbeta_dense(Y, Z, variant, **kw)
    _check(g, _ref(Y, Z, variant, **kw))
    return g


@functools.lru_cache(None)
def _lds_rows():
    import bwgr_amd
    return bwgr_amd.uvbd_plan(1, 4, 2)["lds_rows"]


@pytest.mark.parametrize("variant", ["D", "F", "X", "Z"])
def test_every_variant(variant):
    Y, Z = _case(196, 5, 3, seed=1)
    g = _both(Y, Z, variant, maxit=6, tol=0)
    assert g["b"].shape == (5, 3) and list(g["its"]) == [6, 6, 6] and tuple(g) == ("b", "mu", "h2", "ve", "vb", "its", "cnv")
    if variant == "X":
        assert np.all(np.isnan(g["ve"])) and np.all(np.isnan(g["vb"])) and np.all(np.isnan(g["h2"]))
    if variant != "D":   # a float flavour is the same engine on the rounded Y
        import bwgr_amd
        g2 = bwgr_amd.uvbeta_dense(_f32(Y), Z, variant, maxit=6, tol=0)
        for key in KEYS:
            assert np.array_equal(g[key], g2[key], equal_nan=True), key


@pytest.mark.parametrize("q", [1, 2, 70])
def test_q_edges(q):
    """One column, two, and more columns than a wave has lanes.  With one or two nearly orthogonal columns the fit settles at once, so those
    run two and three sweeps, where every trait's delta b is still far above the rounding of b (asserted), as test_gpu_uvb's p = 1 does."""
    Y, Z = _case(196, q, 3, seed=2)
    maxit = {1: 2, 2: 3, 70: 5}[q]
    o = UR.uvbeta(Y, Z, "D", maxit=maxit, tol=0)
    assert np.all(o["cnv"] > 2 * np.log10(1e-6 * np.abs(o["b"]).max(0)))
    _both(Y, Z, "D", maxit=maxit, tol=0)


@pytest.mark.parametrize("n", [63, 1023, 1025])
def test_row_edges(n):
    """Less than a wave; one short of a row per thread of the largest workgroup; one more, so that thread 0 carries two rows."""
    import bwgr_amd
    t = bwgr_amd.uvbd_plan(n, 4, 2)["threads"]
    assert t == {63: 64, 1023: 1024, 1025: 1024}[n]
    Y, Z = _case(n, 4, 2, seed=3)
    _both(Y, Z, "Z", maxit=4, tol=0)


@pytest.mark.parametrize("where", ["lds_rows", "lds_rows + 37"])
def test_the_last_size_in_lds_and_the_first_in_global_memory(where):
    import bwgr_amd
    n = _lds_rows() + (37 if where != "lds_rows" else 0)
    pl = bwgr_amd.uvbd_plan(n, 4, 2)
    assert pl["e_in_lds"] == (1 if where == "lds_rows" else 0) and (pl["ws_bytes"] > 0) == (where != "lds_rows")
    assert pl["lds_bytes"] <= 160 * 1024
    Y, Z = _case(n, 4, 2, seed=4)
    _both(Y, Z, "D", maxit=3, tol=0)


def test_more_workgroups_than_compute_units():
    Y, Z = _case(64, 3, 300, seed=5)
    g = _both(Y, Z, "D", maxit=4, tol=0)
    assert g["b"].shape == (3, 300) and np.all(g["its"] == 4)


def test_a_padded_design():
    """ldz > n: the first n rows of a taller column-major matrix, passed as they lie."""
    import bwgr_amd
    Y, Z = _case(196, 5, 3, seed=1)
    big = np.asfortranarray(np.full((196 + 29, 5), np.nan))
    big[:196] = Z
    view = big[:196]
    assert view.strides == (8, 8 * 225) and not view.flags.f_contiguous
    g, h = bwgr_amd.uvbeta_dense(Y, view, "D", maxit=6, tol=0), bwgr_amd.uvbeta_dense(Y, Z, "D", maxit=6, tol=0)
    for key in KEYS + ("its",):
        assert np.array_equal(g[key], h[key], equal_nan=True), key


def test_missingness():
    """A fifth of every trait missing; traits 0 and 2 share their pattern; trait 3 has no observed row."""
    import bwgr_amd
    Y, Z = _case(300, 6, 5, seed=6, frac=0.2)
    Y[np.isnan(Y[:, 0]), 2] = np.nan
    Y[~np.isnan(Y[:, 0]) & np.isnan(Y[:, 2]), 2] = 1.0
    assert np.array_equal(np.isnan(Y[:, 0]), np.isnan(Y[:, 2]))
    Y[:, 3] = np.nan
    for variant in ("D", "X"):
        g = _both(Y, Z, variant, maxit=5, tol=0)
        assert list(g["its"]) == [5, 5, 5, 0, 5] and not g["b"][:, 3].any() and g["mu"][3] == 0 and g["h2"][3] == 0
        rest = [0, 1, 2, 4]
        h = bwgr_amd.uvbeta_dense(Y[:, rest], Z, variant, maxit=5, tol=0)   # no trait sees another
        for key in KEYS + ("its",):
            assert np.array_equal(g[key][..., rest], h[key], equal_nan=True), key


def test_a_column_constant_on_one_traits_rows():
    """Column 2 is 1.5 wherever trait 1 is observed: XX = 0 exactly for that trait (1.5 n_t is exact), so its b is 0; the other traits fit it."""
    Y, Z = _case(196, 4, 3, seed=7, frac=0.2)
    Z[~np.isnan(Y[:, 1]), 2] = 1.5
    for variant in ("D", "Z", "F"):
        o = _ref(Y, Z, variant, maxit=5, tol=0)
        assert o["XX"][2, 1] == 0 and o["XX"][2, 0] > 1 and o["XX"][2, 2] > 1
        g = _both(Y, Z, variant, maxit=5, tol=0)
        assert g["b"][2, 1] == 0 and g["b"][2, 0] != 0 and g["b"][2, 2] != 0


def test_the_f_threshold():
    """solver1xF skips a column whose XX is not above 1e-5 (:1633-1635): column 1 scaled to XX = 0.8e-5 on trait 0's rows is skipped by F
    and fitted by D; scaled to 1.25e-5 it is fitted by both."""
    Y, Z = _case(196, 3, 2, seed=8, frac=0.1)
    Y = _f32(Y)
    w = ~np.isnan(Y[:, 0])
    c = Z[:, 1] - Z[w, 1].mean()
    xx = (c[w] ** 2).sum()
    for target, skipped in ((0.8e-5, True), (1.25e-5, False)):
        Zs = Z.copy(order="F")
        Zs[:, 1] = c * np.sqrt(target / xx)
        o = {v: UR.uvbeta(Y, Zs, v, maxit=4, tol=0) for v in ("D", "F")}
        assert abs(o["F"]["XX"][1, 0] / target - 1) < 1e-9
        for v in ("D", "F"):
            g = _both(Y, Zs, v, maxit=4, tol=0)
            assert (g["b"][1, 0] == 0) == (skipped and v == "F"), (target, v, g["b"][1])


@functools.lru_cache(None)
def _stopping_case():
    """Five traits whose signal grows from none to strong on 12 correlated columns: their fits need different numbers of sweeps (9, 13, 21,
    26, 30 in the restatement; the seed was picked there so that no cnv comes near log10(tol): the nearest is 0.077 away)."""
    rng = np.random.default_rng(13)
    n, q, k = 400, 12, 5
    Z = rng.normal(size=(n, q)) + 1.5 * rng.normal(size=(n, 1))
    Y = (Z @ rng.normal(size=(q, k))) * np.array([0.0, 0.1, 0.3, 1.0, 3.0]) + rng.normal(size=(n, k)) + 3.0
    Y[rng.random((n, k)) < 0.1] = np.nan
    return Y, np.asfortranarray(Z), UR.uvbeta(Y, Z, "D", maxit=100, tol=10e-7)


def test_stopping_per_trait_at_the_default_tolerance():
    """Every trait's cnv stays at least 0.02 away from log10(tol) at every sweep of the restatement (asserted), so the counts must be equal."""
    import bwgr_amd
    Y, Z, o = _stopping_case()
    near = min(abs(c - np.log10(10e-7)) for tr in o["trace"] for c in tr)
    print(list(o["its"]), near)
    assert near >= 0.02 and len(set(o["its"])) > 1 and o["its"].max() < 60
    g = bwgr_amd.uvbeta_dense(Y, Z, "D")
    _check(g, o)


def test_frozen_traits():
    """The same call with a larger maxit: no trait reaches either limit, so every trait stopped at the same sweep and is bit-equal; with maxit
    between the counts, the traits that had stopped before it are bit-equal and the others ran maxit sweeps."""
    import bwgr_amd
    Y, Z, o = _stopping_case()
    a, b = bwgr_amd.uvbeta_dense(Y, Z, "D", maxit=100), bwgr_amd.uvbeta_dense(Y, Z, "D", maxit=160)
    for key in KEYS + ("its",):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    cut = int(np.sort(o["its"])[2])
    c = bwgr_amd.uvbeta_dense(Y, Z, "D", maxit=cut)
    done = o["its"] <= cut
    assert done.any() and not done.all()
    assert np.array_equal(c["its"], np.minimum(o["its"], cut))
    for key in KEYS:
        assert np.array_equal(c[key][..., done], a[key][..., done], equal_nan=True), key
    for key in ("b", "cnv"):
        assert not np.array_equal(c[key][..., ~done], a[key][..., ~done]), key


def test_two_calls_give_the_same_bits_and_maxit_zero():
    import bwgr_amd
    Y, Z = _case(1500, 7, 4, seed=10, frac=0.2)
    a, b = bwgr_amd.uvbeta_dense(Y, Z, "Z", maxit=5, tol=0), bwgr_amd.uvbeta_dense(Y, Z, "Z", maxit=5, tol=0)
    for key in KEYS + ("its",):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    z = bwgr_amd.uvbeta_dense(Y, Z, "D", maxit=0)
    assert not z["b"].any() and not z["its"].any()
    _check(z, UR.uvbeta(Y, Z, "D", maxit=0), keys=("b", "mu", "ve", "vb", "h2"))


def test_refusals_and_live_counts():
    import bwgr_amd
    Y, Z = _case(196, 5, 3, seed=1)
    live = bwgr_amd.debug_live()
    good = bwgr_amd.uvbeta_dense(Y, Z, "D", maxit=2, tol=0)
    assert bwgr_amd.debug_live() == live

    def refused(what, *a, **kw):
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            bwgr_amd.uvbeta_dense(*a, **kw)
        assert ei.value.code == 1 and what in str(ei.value), str(ei.value)
        assert bwgr_amd.debug_live() == live
        assert np.array_equal(bwgr_amd.uvbeta_dense(Y, Z, "D", maxit=2, tol=0)["b"], good["b"])   # the device is left usable

    Y1 = Y.copy()
    Y1[:, 2] = np.nan
    Y1[37, 2] = 1.5
    refused("trait 2", Y1, Z, "Z", maxit=2)
    Zn = Z.copy(order="F")
    Zn[11, 3] = np.nan
    refused("Z[11, 3]", Y, Zn, "D", maxit=2)
    Zn[11, 3] = np.inf
    refused("not finite", Y, Zn, "D", maxit=2)
    refused("q = 0", Y, Z[:, :0], "D", maxit=2)
    for bad in (7, "Q"):
        refused("variant", Y, Z, bad, maxit=2)
    refused("maxit", Y, Z, "D", maxit=-1)
    refused("nrow", Y[:100], Z, "D")
    assert bwgr_amd.debug_live() == live
