"""GPU: the per-trait ridge fits (bwgr_uvbeta: solver1x / UVBETA, solver1xF / FUVBETA, XFUVBETA, ZFUVBETA) against the float64 restatement in
tests/uvb_restatement.py: every variant, row slabs and a short last block, the edges of the 64-trait groups, shared and sparse missingness
patterns, solver1xF's test on XX, all-NaN traits, marker-count edges, per-trait stopping and frozen traits, signed and full-range genotypes,
xb, state between calls, the refusals, and a BASELINE config-2-shaped property run.

Parity is mrr_restatement.scaled_err(got, restatement) <= 1e-6 on b, mu, ve, vb, h2, cnv (NaN in the same places) and equal its."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrr_restatement as MR  # noqa: E402
import uvb_restatement as UR  # noqa: E402
from conftest import synth_small  # noqa: E402
from test_gpu_mrr import _traits, _traits_ids  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("b", "mu", "ve", "vb", "h2", "cnv")
TOL = 1e-6


def _f32(Y):
    return np.asarray(Y, np.float64).astype(np.float32).astype(np.float64)


def _errs(g, o, keys=KEYS):
    out = {}
    for key in keys:
        a, b = np.asarray(g[key], np.float64), np.asarray(o[key], np.float64)
        assert a.shape == b.shape, (key, a.shape, b.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)), key
        out[key] = MR.scaled_err(np.nan_to_num(a), np.nan_to_num(b))
    return out


def _check(g, o, keys=KEYS, tol=TOL):
    assert np.array_equal(g["its"], o["its"]), (g["its"], o["its"])
    errs = _errs(g, o, keys)
    print(errs)
    assert all(v <= tol for v in errs.values()), errs
    return errs


def _ref(Y, X, variant, **kw):
    """the restatement on what the library's variant receives: float-rounded Y for F, X and Z"""
    return UR.uvbeta(Y if variant == "D" else _f32(Y), X, variant, **kw)


@functools.lru_cache(None)
def _tpod():
    X = np.asfortranarray(np.load(os.path.join(ROOT, "tests", "golden", "tpod.npz"))["gen"])
    X.setflags(write=False)
    return X


@functools.lru_cache(None)
def _W():
    import bwgr_amd
    return bwgr_amd.uvb_plan(700, 900, 1)["W"]


@functools.lru_cache(None)
def _slabs900():
    X, _ = synth_small(700, 900, seed=3)
    X = np.asfortranarray(X)
    X.setflags(write=False)
    return X


# ---- 1 ----
@pytest.mark.parametrize("variant", ["D", "F", "X", "Z"])
def test_tpod_k3_every_variant(variant):
    import bwgr_amd
    X = _tpod()
    assert X.shape == (196, 376)   # six blocks, the last of 56 markers
    Y = _traits(X, 3, 0.1, seed=11)
    g = bwgr_amd.uvbeta(Y, X, variant, maxit=6, tol=0)
    _check(g, _ref(Y, X, variant, maxit=6, tol=0))
    assert g["b"].shape == (376, 3) and list(g["its"]) == [6, 6, 6]
    assert tuple(g) == ("b", "mu", "h2", "ve", "vb", "its", "cnv")
    if variant == "X":
        assert np.all(np.isnan(g["ve"])) and np.all(np.isnan(g["vb"])) and np.all(np.isnan(g["h2"]))
    if variant != "D":   # a float flavour is the same engine on the rounded Y
        g2 = bwgr_amd.uvbeta(_f32(Y), X, variant, maxit=6, tol=0)
        for key in KEYS:
            assert np.array_equal(g[key], g2[key], equal_nan=True), key


def test_reference_wrappers_return_the_reference_shapes():
    import bwgr_amd
    X = _tpod()
    Y = _traits(X, 3, 0.1, seed=11)
    Y[:, 1] = np.nan
    kw = dict(maxit=100, tol=10e-7, df0=20.0)
    for fn, v in ((bwgr_amd.UVBETA, "D"), (bwgr_amd.FUVBETA, "F"), (bwgr_amd.XFUVBETA, "X")):
        assert np.array_equal(fn(Y, X), bwgr_amd.uvbeta(Y, X, v, **kw)["b"])
    z, r = bwgr_amd.ZFUVBETA(Y, X), bwgr_amd.uvbeta(Y, X, "Z", **kw)
    assert z.shape == (378, 3) and np.array_equal(z[0], r["h2"]) and np.array_equal(z[1], r["mu"]) and np.array_equal(z[2:], r["b"])
    assert not z[:, 1].any() and z[:, 0].any()   # the all-NaN trait's column is zero
    y = Y[:, 0]
    r0 = bwgr_amd.solver1x(y, X)
    assert r0.shape == (376,) and np.array_equal(r0, bwgr_amd.uvbeta(y, X, "D", **kw)["b"][:, 0])
    assert np.array_equal(bwgr_amd.solver1xF(y, X, maxit=7), bwgr_amd.uvbeta(y, X, "F", maxit=7)["b"][:, 0])


# ---- 2 ----
def test_three_slabs_and_a_short_last_block():
    """700 x 900 with nwg = 3: three row slabs, a last block of 4 markers; five traits: four patterns and one fully observed trait."""
    import bwgr_amd
    X = _slabs900()
    Y = _traits(X, 5, 0, seed=5, patterns=[0.1, 0.0, 0.25, 0.05, 0.4])
    assert not np.isnan(Y[:, 1]).any()
    P = bwgr_amd.Panel(X, nwg=3)
    try:
        assert P.ld >= 3 * 128 and P.n == 700 and P.nwg == 3
        g = {v: bwgr_amd.uvbeta(Y, P, v, maxit=6, tol=0) for v in ("D", "Z")}
    finally:
        P.close()
    for v in g:
        _check(g[v], _ref(Y, X, v, maxit=6, tol=0))


# ---- 3 ----
@functools.lru_cache(None)
def _group_edge_case():
    X = _slabs900()
    k = 2 * _W() + 3
    Y = _traits(X, k, 0.15, seed=31)   # one pattern per trait
    assert len({np.isnan(Y[:, t]).tobytes() for t in range(k)}) == k
    return Y, UR.uvbeta(Y, X, "D", maxit=5, tol=0)


@pytest.mark.parametrize("kk", ["1", "W-1", "W", "W+1", "2W+3"])
def test_group_edges(kk):
    """The last group is partly padding, the first is full.  The traits do not couple, so the first k columns of one restatement serve every k."""
    import bwgr_amd
    W = _W()
    k = {"1": 1, "W-1": W - 1, "W": W, "W+1": W + 1, "2W+3": 2 * W + 3}[kk]
    X = _slabs900()
    Y, o = _group_edge_case()
    P = bwgr_amd.Panel(X, nwg=3)
    try:
        g = bwgr_amd.uvbeta(Y[:, :k], P, "D", maxit=5, tol=0)
    finally:
        P.close()
    assert g["b"].shape == (900, k)
    _check(g, {key: (o[key][:, :k] if key == "b" else o[key][:k]) for key in KEYS + ("its",)})


# ---- 4 ----
def test_shared_patterns_and_awkward_rows():
    """Traits share patterns (pt[t] != t), four rows are missing for every trait, and one pattern is observed on five rows spread over the
    three slabs, so that many markers are monomorphic for it.  Y is float-representable: D and F are then one computation."""
    import bwgr_amd
    X = _slabs900()
    ids = (0, 1, 0, 2, 1, 3, 2, 3, 0)
    five = (5, 130, 300, 450, 690)
    Y = _f32(_traits_ids(X, ids, 0.2, seed=41, all_missing=(10, 200, 400, 650), sparse=(3, five)))
    assert np.isnan(Y[[10, 200, 400, 650]]).all() and np.sum(~np.isnan(Y[:, 5])) == 5
    assert len({np.isnan(Y[:, t]).tobytes() for t in range(len(ids))}) == 4
    P = bwgr_amd.Panel(X, nwg=3)
    try:
        R = P.ld // 3
        assert len({r // R for r in five}) == 3
        g = {v: bwgr_amd.uvbeta(Y, P, v, maxit=6, tol=0) for v in ("D", "F")}
    finally:
        P.close()
    o = {v: UR.uvbeta(Y, X, v, maxit=6, tol=0) for v in ("D", "F")}
    assert np.sum(o["D"]["XX"][:, 5] == 0) > 100   # many markers are monomorphic on the five rows
    for v in ("D", "F"):
        _check(g[v], o[v])
    errs = _errs(g["F"], g["D"])
    assert all(v <= 1e-9 for v in errs.values()), errs
    assert np.array_equal(g["F"]["its"], g["D"]["its"])


# ---- 5 ----
def test_the_f_guard_on_purpose():
    """Column 7 is zero except on two rows; trait 1 is missing on exactly those rows, so the marker is monomorphic among its rows."""
    import bwgr_amd
    X = np.array(_tpod(), order="F")
    X[:, 7] = 0
    X[3, 7], X[150, 7] = 1, 2
    Y = _f32(_traits(X, 2, 0.0, seed=51))
    Y[[3, 150], 1] = np.nan
    o = {v: UR.uvbeta(Y, X, v, maxit=6, tol=0) for v in ("D", "F")}
    for v in ("D", "F"):
        assert o[v]["XX"][7, 1] == 0 and o[v]["XX"][7, 0] > 0
        g = bwgr_amd.uvbeta(Y, X, v, maxit=6, tol=0)
        _check(g, o[v])
        if v == "F":
            assert g["b"][7, 1] == 0 and g["b"][7, 0] != 0


# ---- 6 ----
@pytest.mark.parametrize("variant", ["D", "X"])
def test_an_all_nan_trait_among_normal_ones(variant):
    import bwgr_amd
    X = _tpod()
    Y = _traits(X, 4, 0.1, seed=61)
    Y[:, 2] = np.nan
    g = bwgr_amd.uvbeta(Y, X, variant, maxit=5, tol=0)
    assert not g["b"][:, 2].any() and list(g["its"]) == [5, 5, 0, 5]
    _check(g, _ref(Y, X, variant, maxit=5, tol=0))
    rest = [0, 1, 3]
    h = bwgr_amd.uvbeta(Y[:, rest], X, variant, maxit=5, tol=0)
    for key in KEYS + ("its",):
        assert np.array_equal(g[key][..., rest], h[key], equal_nan=True), key


# ---- 7 ----
@pytest.mark.parametrize("kk", ["3", "W+1"])
@pytest.mark.parametrize("p", [1, 63, 64, 65])
def test_marker_count_edges(p, kk):
    import bwgr_amd
    k = 3 if kk == "3" else _W() + 1
    X = np.asfortranarray(_tpod()[:, :p])
    assert X[:, 0].std() > 0
    Y = _traits(_tpod(), k, 0.1, seed=71)
    # With one marker the fit settles at once: after five sweeps sum (Delta b)^2 is rounding noise (cnv down to -36) and no fair subject of a
    # 1e-6 comparison.  p = 1 therefore runs two sweeps, where every trait's Delta b is still far above the rounding of b (asserted).
    maxit = 2 if p == 1 else 5
    o = UR.uvbeta(Y, X, "D", maxit=maxit, tol=0)
    assert np.all(o["cnv"] > 2 * np.log10(1e-6 * np.abs(o["b"]).max(0)))
    g = bwgr_amd.uvbeta(Y, X, "D", maxit=maxit, tol=0)
    _check(g, o)
    assert g["b"].shape == (p, k)


def test_maxit_zero():
    import bwgr_amd
    X = _tpod()
    g = bwgr_amd.uvbeta(_traits(X, 3, 0.1, seed=11), X, "D", maxit=0, xb=True)
    assert not g["b"].any() and not g["its"].any() and not g["xb"].any()


# ---- 8, 9 ----
@functools.lru_cache(None)
def _stopping_case(variant):
    X = _tpod()
    Y = _traits(X, 6, 0.1, seed=11)
    return Y, _ref(Y, X, variant, maxit=100, tol=10e-7)


@pytest.mark.parametrize("variant", ["D", "X", "Z"])
def test_stopping_per_trait_at_the_default_tolerance(variant):
    """Every trait's cnv stays at least 0.02 away from log10(tol) at every sweep of the restatement (measured with real orders: D sweeps 10,
    8, 8, 9, 8, 10, nearest approach 0.045; X 12, 11, 11, 11, 11, 12, 0.072; Z 9, 8, 8, 9, 9, 9, 0.063), so the sweep counts must be equal."""
    import bwgr_amd
    X = _tpod()
    Y, o = _stopping_case(variant)
    near = min(abs(c - np.log10(10e-7)) for tr in o["trace"] for c in tr)
    print(variant, list(o["its"]), near)
    assert near >= 0.02 and len(set(o["its"])) > 1 and o["its"].max() < 100
    g = bwgr_amd.uvbeta(Y, X, variant, maxit=100, tol=10e-7)
    _check(g, o)


def test_frozen_traits_and_independence():
    """Each trait of the stopping case fitted alone agrees with its column of the joint fit: a stopped trait is not touched by the sweeps its
    group still runs, and no trait sees another."""
    import bwgr_amd
    X = _tpod()
    Y, o = _stopping_case("D")
    P = bwgr_amd.Panel(X)
    try:
        g = bwgr_amd.uvbeta(Y, P, "D", maxit=100, tol=10e-7)
        alone = [bwgr_amd.uvbeta(Y[:, t], P, "D", maxit=100, tol=10e-7) for t in range(6)]
    finally:
        P.close()
    assert len(set(g["its"])) > 1
    for t, a in enumerate(alone):
        assert a["its"][0] == g["its"][t]
        errs = _errs(a, {key: g[key][..., t:t + 1] for key in KEYS})
        assert all(v <= 1e-9 for v in errs.values()), (t, errs)


# ---- 10 ----
def test_signed_genotypes_match_the_shifted_panel():
    import bwgr_amd
    X = _tpod()
    Xs = np.asfortranarray((X.astype(np.int16) - 1).astype(np.int8))
    assert Xs.min() == -1 and Xs.max() == 1
    Y = _traits(X, 4, 0.1, seed=81)
    g = bwgr_amd.uvbeta(Y, Xs, "D", maxit=6, tol=0)
    _check(g, UR.uvbeta(Y, Xs, "D", maxit=6, tol=0))
    g0 = bwgr_amd.uvbeta(Y, X, "D", maxit=6, tol=0)
    _check(g0, UR.uvbeta(Y, X, "D", maxit=6, tol=0))
    errs = _errs(g, g0)
    assert all(v <= 1e-9 for v in errs.values()), errs


def test_full_range_int8_panel():
    import bwgr_amd
    rng = np.random.default_rng(91)
    X = rng.integers(-128, 128, size=(300, 200)).astype(np.int8)
    X[0, 0], X[1, 0] = -128, 127
    X = np.asfortranarray(X)
    Y = _traits(X, 5, 0.1, seed=92)
    _check(bwgr_amd.uvbeta(Y, X, "D", maxit=6, tol=0), UR.uvbeta(Y, X, "D", maxit=6, tol=0))


# ---- 11 ----
def test_xb_is_the_product_on_every_row():
    import bwgr_amd
    X = _slabs900()
    k = _W() + 1
    Y = _traits(X, k, 0.3, seed=95)
    P = bwgr_amd.Panel(X, nwg=3)
    try:
        g = bwgr_amd.uvbeta(Y, P, "Z", maxit=3, tol=0, xb=True)
    finally:
        P.close()
    assert g["xb"].shape == (700, k) and tuple(g)[-1] == "xb"
    assert MR.scaled_err(g["xb"], X.astype(np.float64) @ g["b"]) <= 1e-12


# ---- 12 ----
def test_state_between_calls():
    import bwgr_amd
    X = _tpod()
    W = _W()
    Y3, Yw = _traits(X, 3, 0.1, seed=121), _traits(X, W + 1, 0.1, seed=122)
    P = bwgr_amd.Panel(X)
    try:
        a = bwgr_amd.uvbeta(Y3, P, "D", maxit=5, tol=0, xb=True)
        b = bwgr_amd.uvbeta(Yw, P, "D", maxit=5, tol=0, xb=True)
        c = bwgr_amd.uvbeta(Y3, P, "D", maxit=5, tol=0, xb=True)
        P.set_centred(True)
        e = bwgr_amd.uvbeta(Y3, P, "D", maxit=5, tol=0, xb=True)
        P.set_centred(False)
    finally:
        P.close()
    P = bwgr_amd.Panel(X)
    try:
        d = bwgr_amd.uvbeta(Yw, P, "D", maxit=5, tol=0, xb=True)
    finally:
        P.close()
    for key in a:
        assert np.array_equal(a[key], c[key]), key
        assert np.array_equal(b[key], d[key]), key
        assert np.array_equal(a[key], e[key]), key


# ---- 13 ----
def test_refusals_leave_the_device_usable():
    import bwgr_amd
    X = _tpod()
    Y = _traits(X, 4, 0.1, seed=61)
    good = bwgr_amd.uvbeta(Y, X, "D", maxit=2, tol=0)

    def usable():
        again = bwgr_amd.uvbeta(Y, X, "D", maxit=2, tol=0)
        assert np.array_equal(again["b"], good["b"])

    P = bwgr_amd.Panel(X.astype(np.float32) + 0.5)
    try:
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            bwgr_amd.uvbeta(Y, P, "D", maxit=2)
    finally:
        P.close()
    assert ei.value.code == 1 and "fp32" in str(ei.value)
    usable()
    for bad in (7, "Q"):
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            bwgr_amd.uvbeta(Y, X, bad, maxit=2)
        assert ei.value.code == 1 and "variant" in str(ei.value)
    usable()
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.uvbeta(Y, X, "D", maxit=-1)
    assert ei.value.code == 1 and "maxit" in str(ei.value)
    usable()
    Y1 = Y.copy()
    Y1[:, 2] = np.nan
    Y1[37, 2] = 1.5
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.uvbeta(Y1, X, "Z", maxit=2)
    assert ei.value.code == 1 and "trait 2" in str(ei.value)
    usable()


def test_int32_gram_bound():
    """Columns of +-127 and a fully observed trait: its pattern's Gram diagonal is n 127^2 in every block.  At the largest n the host accepts
    (n max|x|^2 < 2^31) the fit matches; one more row is refused."""
    import bwgr_amd
    n = ((1 << 31) - 1) // (127 * 127)
    assert n * 127 * 127 < (1 << 31) <= (n + 1) * 127 * 127
    rng = np.random.default_rng(101)
    X = np.asfortranarray(np.where(rng.random((n + 1, 70)) < 0.5, -127, 127).astype(np.int8))
    Y = _traits(X[:n], 2, 0, seed=102, patterns=[0.0, 0.1])
    assert np.sum(~np.isnan(Y[:, 0])) == n and np.sum(np.isnan(Y[:, 1])) > 0
    P = bwgr_amd.Panel(X[:n], block=16)
    try:
        g = bwgr_amd.uvbeta(Y, P, "D", maxit=2, tol=0)
    finally:
        P.close()
    _check(g, UR.uvbeta(Y, X[:n], "D", maxit=2, tol=0))
    Y1 = _traits(X, 2, 0.1, seed=103)
    with pytest.raises(bwgr_amd.BwgrError) as ei:      # (refused where the panel's own Gram arrays are built: before uvbeta sees the panel)
        bwgr_amd.uvbeta(Y1, X, "D", maxit=2, tol=0, block=16)
    assert ei.value.code == 1 and "int32 Gram" in str(ei.value)
    X2 = _tpod()
    Y2 = _traits(X2, 2, 0.1, seed=104)
    assert bwgr_amd.uvbeta(Y2, X2, "D", maxit=1)["its"].tolist() == [1, 1]   # the device is left usable


# ---- 14 ----
def test_config2_shape_properties():
    """n = 5 000 x p = 50 000 synthetic int8 panel (BASELINE config 2's shape), k = 24, 20 % missing, variant D, six sweeps: properties only."""
    import torch
    import bwgr_amd
    from bwgr_amd import synth
    n, p, k = 5000, 50000, 24
    Xd = synth.genotypes(n, p)
    gen = torch.Generator(device=Xd.device); gen.manual_seed(5)
    B = torch.randn(p, k, generator=gen, device=Xd.device, dtype=torch.float64) / np.sqrt(p)

    def product(Bd):   # X Bd in fp64 on the device, 2 000 markers at a time
        acc = torch.zeros(n, Bd.shape[1], device=Xd.device, dtype=torch.float64)
        for j in range(0, p, 2000):
            acc += Xd[j:j + 2000, :n].to(torch.float64).T @ Bd[j:j + 2000]
        return acc

    G = product(B).cpu().numpy()
    rng = np.random.default_rng(7)
    Y = (G - G.mean(0)) / G.std(0) + rng.normal(size=(n, k)) + 3.0
    miss = rng.random((n, k)) < 0.2
    Y[miss] = np.nan
    P = bwgr_amd.Panel(Xd, n=n)
    try:
        g = bwgr_amd.uvbeta(Y, P, "D", maxit=6, tol=0, xb=True)
        ref = product(torch.from_numpy(np.ascontiguousarray(g["b"])).to(Xd.device)).cpu().numpy()
    finally:
        P.close()
        del Xd, B
        torch.cuda.empty_cache()
    for key in KEYS + ("xb",):
        assert np.all(np.isfinite(g[key])), key
    assert np.all(g["its"] == 6)
    assert MR.scaled_err(g["xb"], ref) <= 1e-10
    cors = [np.corrcoef(g["xb"][~miss[:, t], t], Y[~miss[:, t], t])[0, 1] for t in range(k)]
    print(min(cors), max(cors))
    assert min(cors) > 0.9, cors
