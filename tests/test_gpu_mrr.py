"""GPU: mrr / mrr_float (MRR3 / MRR3F) against the float64 restatement in tests/mrr_restatement.py, the refusals, and a
BASELINE config-2-shaped property run; then the promised range -- k up to 16, shared missingness patterns, every layout of the solve's LDS
plan (tests/mrr_cases.py), marker-count edges, signed and full-range genotypes, the int32 Gram bound -- against the same restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrr_cases  # noqa: E402
import mrr_restatement as MR  # noqa: E402
from conftest import synth_small  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("b", "hat", "mu", "vb", "ve", "GC", "h2", "MSx", "cnvB")
TOL = 1e-6


def _traits(X, k, frac, seed, patterns=None):
    rng = np.random.default_rng(seed)
    Xf = X.astype(np.float64)
    n, p = X.shape
    B = rng.normal(size=(p, k)) * (1.0 / np.sqrt(p))
    G = (Xf - Xf.mean(0)) @ B
    Y = G / G.std(0) + rng.normal(size=(n, k)) + 3.0
    if patterns is None:
        Y[rng.random((n, k)) < frac] = np.nan
    else:
        for t, fr in enumerate(patterns):
            if fr > 0:
                Y[rng.random(n) < fr, t] = np.nan
    return Y


def _tpod():
    d = np.load(os.path.join(ROOT, "tests", "golden", "tpod.npz"))
    return np.asfortranarray(d["gen"])


def _check(g, o, keys=KEYS, tol=TOL):
    assert g["Its"] == o["Its"]
    errs = {k: MR.scaled_err(g[k], o[k]) for k in keys}
    assert all(v <= tol for v in errs.values()), errs
    assert tuple(g) == ("mu", "b", "hat", "h2", "GC", "vb", "ve", "MSx", "cnvB", "cnvH2", "cnvV", "b_Weights", "Its")
    return errs


def test_tpod_k3_defaults():
    import bwgr_amd
    X = _tpod()
    Y = _traits(X, 3, 0.1, seed=11)
    g = bwgr_amd.mrr(Y, X, maxit=30, tol=0)
    o = MR.mrr(Y, X, maxit=30, tol=0)
    _check(g, o)
    assert np.all(np.isfinite(g["hat"])) and g["b"].shape == (X.shape[1], 3) and g["hat"].shape == (X.shape[0], 3)
    # mrr_float: the same engine on the float-rounded inputs
    gf = bwgr_amd.mrr_float(Y, X, maxit=30, tol=0)
    of = MR.mrr(Y.astype(np.float32).astype(np.float64), X, maxit=30, tol=0)
    _check(gf, of)


def test_slabs_partial_block_patterns_k5():
    """three row slabs, 900 markers (a partial last block of 4), five traits: four missingness patterns and one fully observed trait."""
    import bwgr_amd
    X, _ = synth_small(700, 900, seed=3)
    X = np.asfortranarray(X)
    Y = _traits(X, 5, 0, seed=5, patterns=[0.1, 0.0, 0.25, 0.05, 0.4])
    P = bwgr_amd.Panel(X, nwg=3)
    try:
        assert P.ld >= 3 * 128 and P.n == 700
        g = bwgr_amd.MRR3(Y, P, maxit=10, tol=0)
    finally:
        P.close()
    o = MR.mrr(Y, X, maxit=10, tol=0)
    _check(g, o)


@pytest.mark.parametrize("opt", [dict(TH=True), dict(HCS=True), dict(XFA=True, NumXFA=2), dict(ACS=True, NumXFA=2), dict(OneVarB=True),
                                 dict(OneVarE=True), dict(updateMu=True), dict(weight_prior_h2=0.0, weight_prior_gc=0.0)],
                         ids=["TH", "HCS", "XFA", "ACS", "OneVarB", "OneVarE", "updateMu", "no_priors"])
def test_options(opt):
    import bwgr_amd
    X = _tpod()
    Y = _traits(X, 3, 0.1, seed=21)
    g = bwgr_amd.MRR3(Y, X, maxit=12, tol=0, **opt)
    o = MR.mrr(Y, X, maxit=12, tol=0, **opt)
    _check(g, o)


def test_single_trait():
    import bwgr_amd
    X = _tpod()
    y = np.load(os.path.join(ROOT, "tests", "golden", "tpod.npz"))["y"].astype(np.float64)
    g = bwgr_amd.mrr(y, X, maxit=15, tol=0)
    o = MR.mrr(y, X, maxit=15, tol=0)
    _check(g, o)
    assert g["b"].shape == (X.shape[1], 1)


def test_bending_branch():
    import bwgr_amd
    X = _tpod()
    Y = _traits(X, 3, 0.0, seed=3)
    Y[:, 1] = Y[:, 0] + 1e-3 * Y[:, 1]
    Y[:, 2] = -Y[:, 0] + 1e-3 * Y[:, 2]
    kw = dict(maxit=4, tol=0, XFA=True, NumXFA=1, weight_prior_gc=0)
    o = MR.mrr(Y, X, trace=True, **kw)
    assert any(t["bent"] for t in o["trace"])
    g = bwgr_amd.MRR3(Y, X, **kw)
    _check(g, o)


def test_convergence_at_default_tol():
    import bwgr_amd
    X = _tpod()
    Y = _traits(X, 2, 0.1, seed=31)
    g = bwgr_amd.mrr(Y, X)
    o = MR.mrr(Y, X)
    assert 1 < o["Its"] < 500
    assert abs(g["Its"] - o["Its"]) <= 1
    m = min(g["Its"], o["Its"])
    assert np.allclose(g["cnvB"][:m], o["cnvB"][:m], rtol=0, atol=1e-3)
    assert MR.scaled_err(g["b"], o["b"]) < 1e-4


def test_centred_panel_gives_the_same_result():
    """Chosen behaviour: a panel switched to implicit centring is accepted and gives the same fit (mrr centres X itself)."""
    import bwgr_amd
    X = _tpod()
    Y = _traits(X, 3, 0.1, seed=41)
    P = bwgr_amd.Panel(X)
    try:
        a = bwgr_amd.mrr(Y, P, maxit=8, tol=0)
        P.set_centred(True)
        b = bwgr_amd.mrr(Y, P, maxit=8, tol=0)
    finally:
        P.close()
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("opt", [dict(InnerGS=True), dict(NoInv=True), dict(NLfactor=0.5), dict(PenCor=1.0), dict(MinCor=0.5),
                                 dict(uncorH2below=0.1), dict(roundGCupFrom=0.9), dict(roundGCupTo=0.9), dict(roundGCdownFrom=0.1),
                                 dict(roundGCdownTo=0.1), dict(bucketGCfrom=0.2), dict(bucketGCto=0.8), dict(DeflateBy=0.1)],
                         ids=lambda d: list(d)[0])
def test_refused_options(opt):
    import bwgr_amd
    X = _tpod()
    Y = _traits(X, 2, 0.0, seed=1)
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.MRR3(Y, X, maxit=2, **opt)
    assert ei.value.code == 1 and list(opt)[0].split("_")[0] in str(ei.value)
    # the device is left usable: a valid call right after
    assert bwgr_amd.MRR3(Y, X, maxit=1)["Its"] == 1


def test_refused_k_and_float_panel():
    import bwgr_amd
    X = _tpod()
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.MRR3(_traits(X, 17, 0.0, seed=2), X, maxit=2)
    assert ei.value.code == 1
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.MRR3(_traits(X, 2, 0.0, seed=2), X.astype(np.float32) + 0.5, maxit=2)
    assert ei.value.code == 1
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.MRR3(_traits(X, 2, 0.0, seed=2), X, maxit=2, XFA=True, NumXFA=3)   # NumXFA > k
    assert ei.value.code == 1


def test_config2_shape_properties():
    """n = 5 000 x p = 50 000 synthetic int8 panel (BASELINE config 2's shape), k = 4, about 20 % missing, 20 iterations."""
    import torch
    import bwgr_amd
    from bwgr_amd import synth
    n, p, k = 5000, 50000, 4
    Xd = synth.genotypes(n, p)
    G = np.stack([synth.phenotype(Xd, n, seed=100 + t).cpu().numpy() for t in range(k)], 1)
    rng = np.random.default_rng(7)
    G = (G - G.mean(0)) / G.std(0)
    mix = np.linalg.cholesky(np.array([[1, .6, .3, .1], [.6, 1, .4, .2], [.3, .4, 1, .5], [.1, .2, .5, 1]]))
    Y = G @ mix.T + rng.normal(size=(n, k))
    miss = rng.random((n, k)) < 0.2
    Y[miss] = np.nan
    P = bwgr_amd.Panel(Xd, n=n)
    try:
        g = bwgr_amd.mrr(Y, P, maxit=20, tol=0)
    finally:
        P.close()
        del Xd
        torch.cuda.empty_cache()
    for key in ("mu", "b", "hat", "h2", "GC", "vb", "ve", "MSx", "cnvB", "cnvH2"):
        assert np.all(np.isfinite(g[key])), key
    assert g["Its"] == 20
    assert np.linalg.eigvalsh(g["vb"]).min() >= -1e-12 * np.abs(g["vb"]).max()
    assert np.allclose(np.diag(g["GC"]), 1.0, atol=1e-12)
    for t in range(k):
        obs = ~miss[:, t]
        assert np.corrcoef(g["hat"][obs, t], Y[obs, t])[0, 1] > 0.5   # the fit explains the observed records
        assert np.all(np.isfinite(g["hat"][~obs, t]))


# ---- the promised range: 1 <= k <= 16, any missingness, every layout of the solve's LDS plan (tests/mrr_cases.py) ----

def _traits_ids(X, ids, frac, seed, all_missing=(), sparse=None):
    """len(ids) traits; the traits that share an id are NaN in exactly the same rows (one random mask per id, `frac` missing).
    all_missing: rows NaN for every trait; sparse = (id, rows): that pattern is observed on `rows` alone."""
    Y = _traits(X, len(ids), 0.0, seed)
    miss = np.random.default_rng(seed + 1).random((X.shape[0], max(ids) + 1)) < frac
    miss[list(all_missing), :] = True
    if sparse is not None:
        miss[:, sparse[0]] = True
        miss[list(sparse[1]), sparse[0]] = False
    for t, g in enumerate(ids):
        Y[miss[:, g], t] = np.nan
    return Y


def _npat(Y):
    return len({np.isnan(Y[:, t]).tobytes() for t in range(Y.shape[1])})


def _regime(k, npat):
    _, linv, ngl, _, _ = mrr_cases.plan(k, npat)
    return mrr_cases.regime(linv, ngl, npat)


@pytest.fixture(scope="module")
def slabs900():
    """synth_small(700, 900) for a panel of three 256-row slabs (nwg=3): 15 marker blocks, the last of 4 markers."""
    X, _ = synth_small(700, 900, seed=3)
    return np.asfortranarray(X)


def _three_slabs(X):
    import bwgr_amd
    P = bwgr_amd.Panel(X, nwg=3)
    assert P.nwg == 3 and P.ld == 3 * P.slab_rows and P.ld // 64 == 12
    return P


@pytest.mark.parametrize("k,npat", mrr_cases.K_SWEEP, ids=["k%d_npat%d" % c for c in mrr_cases.K_SWEEP])
def test_k_sweep_across_the_solve_plan(k, npat, slabs900):
    import bwgr_amd
    X = slabs900
    Y = _traits_ids(X, [t % npat for t in range(k)], 0.1, seed=100 + k + npat)
    assert _npat(Y) == npat
    P = _three_slabs(X)
    try:
        g = bwgr_amd.MRR3(Y, P, maxit=6, tol=0)
    finally:
        P.close()
    o = MR.mrr(Y, X, maxit=6, tol=0)
    _check(g, o)


def test_mrr_float_k16(slabs900):
    import bwgr_amd
    X = slabs900
    Y = _traits(X, 16, 0.1, seed=116)
    assert _npat(Y) == 16 and _regime(16, 16) == 5
    P = _three_slabs(X)
    try:
        g = bwgr_amd.mrr_float(Y, P, maxit=5, tol=0)
    finally:
        P.close()
    o = MR.mrr(Y.astype(np.float32).astype(np.float64), X, maxit=5, tol=0)
    _check(g, o)


@pytest.mark.parametrize("ids", mrr_cases.SHARED, ids=["k%d" % len(i) for i in mrr_cases.SHARED])
def test_shared_missingness_patterns(ids, slabs900):
    """pt[t] != t with 1 < npat < k: the column set-up reads pattern bits, the pass and the solve trait bits / pt.  Rows missing for
    every trait (their hat must match too) and one pattern observed on five rows spread over the three slabs."""
    import bwgr_amd
    X = slabs900
    all_missing = [5, 260, 261, 699]
    sparse_rows = [17, 200, 301, 480, 650]
    Y = _traits_ids(X, ids, 0.15, seed=7 + len(ids), all_missing=all_missing, sparse=(max(ids), sparse_rows))
    assert _npat(Y) == len(set(ids)) and np.all(np.isnan(Y[all_missing]))
    assert np.sum(~np.isnan(Y[:, ids.index(max(ids))])) == 5
    P = _three_slabs(X)
    try:
        assert len({r // P.slab_rows for r in sparse_rows}) == 3
        g = bwgr_amd.MRR3(Y, P, maxit=6, tol=0)
    finally:
        P.close()
    o = MR.mrr(Y, X, maxit=6, tol=0)
    _check(g, o)
    assert MR.scaled_err(g["hat"][all_missing], o["hat"][all_missing]) <= TOL


def test_refuses_a_trait_with_one_observed_row():
    import bwgr_amd
    X = _tpod()
    Y = _traits(X, 4, 0.1, seed=61)
    Y1 = Y.copy()
    Y1[:, 2] = np.nan
    Y1[37, 2] = 1.5
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.MRR3(Y1, X, maxit=2)
    assert ei.value.code == 1 and "trait 2" in str(ei.value)
    assert bwgr_amd.MRR3(Y, X, maxit=1)["Its"] == 1   # the device is left usable


@pytest.mark.parametrize("nwg", [0, 5], ids=["default_slabs", "nwg5"])
def test_several_tiles_per_pass_workgroup(nwg):
    """n = 4100 rows: at least 65 tiles of 64 rows for the pass's 32 workgroups, so each accumulates its dots over several tiles."""
    import bwgr_amd
    X, _ = synth_small(4100, 300, seed=9)
    Y = _traits(X, 4, 0, seed=13, patterns=[0.1, 0.2, 0.05, 0.3])
    assert _npat(Y) == 4
    P = bwgr_amd.Panel(X, nwg=nwg, block=16 if nwg else 0)   # (five slabs of 896 rows need the smaller sweep block)
    try:
        assert P.ld // 64 >= 65 and (nwg == 0 or P.nwg == nwg)
        g = bwgr_amd.MRR3(Y, P, maxit=6, tol=0)
    finally:
        P.close()
    o = MR.mrr(Y, X, maxit=6, tol=0)
    _check(g, o)


@pytest.mark.parametrize("k", mrr_cases.EDGE_K)
@pytest.mark.parametrize("p", mrr_cases.EDGE_P)
def test_marker_count_edges(p, k):
    import bwgr_amd
    X = np.asfortranarray(_tpod()[:, :p])
    assert X[:, 0].std() > 0
    Y = _traits(X, k, 0.1, seed=200 + p + k)
    g = bwgr_amd.mrr(Y, X, maxit=6, tol=0)
    o = MR.mrr(Y, X, maxit=6, tol=0)
    _check(g, o)
    assert g["b"].shape == (p, k)


def test_maxit_zero():
    import bwgr_amd
    X = _tpod()
    Y = _traits(X, 3, 0.1, seed=71)
    g = bwgr_amd.mrr(Y, X, maxit=0, tol=0)
    o = MR.mrr(Y, X, maxit=0, tol=0)
    assert g["Its"] == 0 and o["Its"] == 0
    assert np.all(g["b"] == 0)
    for key in ("cnvB", "cnvH2", "cnvV"):
        assert g[key].shape == (0,), key
    assert np.array_equal(g["hat"], np.broadcast_to(g["mu"], g["hat"].shape))
    _check(g, o, keys=tuple(key for key in KEYS if key != "cnvB"))


def test_signed_genotypes_match_the_shifted_panel():
    """gen - 1 (values -1 / 0 / 1): the signed int8 unpacking and MFMA.  The column means are removed first, so the fit equals the one on
    gen up to rounding."""
    import bwgr_amd
    X = _tpod()
    Xs = np.asfortranarray((X.astype(np.int16) - 1).astype(np.int8))
    assert Xs.min() == -1 and Xs.max() == 1
    Y = _traits(X, 4, 0.1, seed=81)
    g = bwgr_amd.mrr(Y, Xs, maxit=8, tol=0)
    _check(g, MR.mrr(Y, Xs, maxit=8, tol=0))
    g0 = bwgr_amd.mrr(Y, X, maxit=8, tol=0)
    assert g["Its"] == g0["Its"]
    errs = {key: MR.scaled_err(g[key], g0[key]) for key in KEYS}
    assert all(v <= 1e-9 for v in errs.values()), errs


def test_full_range_int8_panel():
    import bwgr_amd
    rng = np.random.default_rng(91)
    X = rng.integers(-128, 128, size=(300, 200)).astype(np.int8)
    X[0, 0], X[1, 0] = -128, 127
    X = np.asfortranarray(X)
    Y = _traits(X, 5, 0.1, seed=92)
    g = bwgr_amd.mrr(Y, X, maxit=6, tol=0)
    o = MR.mrr(Y, X, maxit=6, tol=0)
    _check(g, o)


def test_int32_gram_bound():
    """Columns of +-127 and a fully observed trait: the diagonal of that trait's pattern Gram is n 127^2 in every block.  At the largest
    n the host accepts (n max|x|^2 < 2^31) the int32 Gram is exact and the fit matches; one more row is refused -- where the panel's own Gram
    arrays are built, so before mrr sees the panel."""
    import bwgr_amd
    n = ((1 << 31) - 1) // (127 * 127)
    assert n * 127 * 127 < (1 << 31) <= (n + 1) * 127 * 127
    rng = np.random.default_rng(101)
    X = np.asfortranarray(np.where(rng.random((n + 1, 70)) < 0.5, -127, 127).astype(np.int8))
    Y = _traits(X[:n], 2, 0, seed=102, patterns=[0.0, 0.1])
    assert np.sum(~np.isnan(Y[:, 0])) == n and np.sum(np.isnan(Y[:, 1])) > 0   # pattern 0 spans all n rows
    assert np.all((X[:n].astype(np.int64) ** 2).sum(0) == n * 127 * 127)
    P = bwgr_amd.Panel(X[:n], block=16)   # (n rows need the smaller sweep block's taller slabs)
    try:
        g = bwgr_amd.mrr(Y, P, maxit=2, tol=0)
    finally:
        P.close()
    o = MR.mrr(Y, X[:n], maxit=2, tol=0)
    _check(g, o)
    Y1 = _traits(X, 2, 0.1, seed=103)
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.mrr(Y1, X, maxit=2, tol=0, block=16)
    assert ei.value.code == 1 and "int32 Gram" in str(ei.value)


@pytest.mark.parametrize("opt", [dict(TH=True), dict(HCS=True), dict(XFA=True, NumXFA=mrr_cases.OPTIONS_K), dict(ACS=True, NumXFA=3),
                                 dict(OneVarB=True), dict(updateMu=True)],
                         ids=["TH", "HCS", "XFA_NumXFA_k", "ACS", "OneVarB", "updateMu"])
def test_options_at_large_k(opt):
    import bwgr_amd
    k = mrr_cases.OPTIONS_K
    X = _tpod()
    Y = _traits(X, k, 0.1, seed=111)
    assert _npat(Y) == k and _regime(k, k) == 2
    g = bwgr_amd.MRR3(Y, X, maxit=8, tol=0, **opt)
    o = MR.mrr(Y, X, maxit=8, tol=0, **opt)
    _check(g, o)


def test_state_between_calls():
    """k = 3, 16, 3 on one panel: the host sets the kernels' LDS attributes and allocates scratch per call; nothing may carry over."""
    import bwgr_amd
    X = _tpod()
    Y3, Y16 = _traits(X, 3, 0.1, seed=121), _traits(X, 16, 0.1, seed=122)
    P = bwgr_amd.Panel(X)
    try:
        a = bwgr_amd.mrr(Y3, P, maxit=5, tol=0)
        b = bwgr_amd.mrr(Y16, P, maxit=5, tol=0)
        c = bwgr_amd.mrr(Y3, P, maxit=5, tol=0)
    finally:
        P.close()
    P = bwgr_amd.Panel(X)
    try:
        d = bwgr_amd.mrr(Y16, P, maxit=5, tol=0)
    finally:
        P.close()
    for key in bwgr_amd.api.MRR_KEYS:
        assert np.array_equal(a[key], c[key]), key
        assert np.array_equal(b[key], d[key]), key
