"""GPU: mrr / mrr_float (MRR3 / MRR3F) against the float64 restatement in tests/mrr_restatement.py, the refusals, and a
BASELINE config-2-shaped property run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
