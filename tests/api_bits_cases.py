"""The calls whose output bits tests/golden/api_parent_digests.txt records (tools/family_digest.py --cases api_bits_cases writes the table,
tests/test_gpu_api_parent_bits.py compares against it): the entries of the Python layer that tests/sampler_bits_cases.py and
tests/uvb_bits_cases.py do not already drive -- the multi-trait fits, the EM family, wgr, KMUP, fit_many, mcmcCV, the latent-space fits and
the founder-by-sample kernels -- each through its public function, so the table holds every byte the layer hands to the library and the
order of its calls.  Inputs come from seeded numpy generators, tests/golden/tpod.npz (196 rows, its first 128 markers) and the smallest cases
of the families' own case modules.

CASES maps a name to a function that runs the call and returns a dict of results."""
import functools
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mkr_cases as MK  # noqa: E402
import pegs_cases as PG  # noqa: E402
import pegs_sparse_cases as PS  # noqa: E402
import sem2_cases as S2  # noqa: E402
from sampler_bits_cases import _bw, read_table, switches  # noqa: E402,F401  (torch before the library)

SIX = dict(maxit=6, tol=0)


@functools.lru_cache(None)
def tp():
    """(X, y, Y): tpod's first 128 markers as int8, its phenotype, and three traits with a tenth of the records missing"""
    X = np.asfortranarray(S2.tpod()[:, :128]).astype(np.int8)
    y = np.load(os.path.join(S2.ROOT, "tests", "golden", "tpod.npz"))["y"].astype(np.float64)
    Y = S2.traits(X, 3, 0.1, seed=11)
    for a in (X, y, Y):
        a.setflags(write=False)
    return X, y, Y


@functools.lru_cache(None)
def real_design():
    X = MK.real_design(196, 70, 31)
    return X, MK.traits(X, 3, 41, frac=0.1)


def _mrr_dense_device():
    import torch
    X, Y = real_design()
    return _bw().mrr(Y, _bw().dense(torch.as_tensor(np.ascontiguousarray(X), device="cuda")), maxit=6)


def _mkr():
    K = MK.grm(MK.genotypes(150, 128, 7))
    return _bw().mkr(MK.traits(K, 3, 21, frac=0.15), K, maxit=6)


def _pegs():
    Y, effects = PG.by_id("tpod_k3_defaults")["data"]()
    return _bw().PEGS(Y, np.asfortranarray(effects[0][1][:, :128]), maxit=6, logtol=PG.NOSTOP)


def _pegs_sparse(id_):
    return lambda: PS.run(PS.by_id(id_), maxit=6)


def _em(name, **kw):
    return lambda: getattr(_bw(), name)(tp()[1], tp()[0], maxit=6, **kw)


def _eigK(n):
    """a kernel's spectrum as wgr takes it: five of the falling values hold 95 % (the columns need not be orthonormal for the call to run)"""
    g = np.random.default_rng(301)
    return {"values": n * 0.5 ** np.arange(1, n + 1), "vectors": g.standard_normal((n, n)) / np.sqrt(n)}


def _wgr(nan_y=False, eig=False, **kw):
    def run():
        X, y, _ = tp()
        if nan_y:
            y = y.copy(); y[[3, 77, 190]] = np.nan
        return _bw().wgr(y, X, it=30, bi=10, seed=5, **(dict(kw, eigK=_eigK(X.shape[0])) if eig else kw))
    return run


def _kmup_inputs(P):
    g = np.random.default_rng(311)
    return g.standard_normal(P.p) * 0.05, (g.random(P.p) < 0.5).astype(np.float64), P.stats()[0], tp()[1] - tp()[1].mean(), np.full(P.p, 2.0)


def _kmup():
    P = _bw().Panel(tp()[0])
    try:
        b, d, xx, e, L = _kmup_inputs(P)
        return _bw().KMUP(P, b, d, xx, e, L, 1.0, 0.5, seed=3, it=2)
    finally:
        P.close()


def _kmup2():
    bw = _bw()
    P = bw.Panel(tp()[0])
    try:
        b, d, xx, e, L = _kmup_inputs(P)
        return bw.KMUP2(P, bw.sample_rows(7, 1, P.n, 150), b, d, xx, e, L, 1.0, 0.5, seed=3, it=2)
    finally:
        P.close()


def _fit_many():
    X, y, _ = tp()
    jobs = [dict(model="BayesB", y=y, it=20, bi=5, pi=0.9, seed=21), dict(model="BayesC", y=y, it=20, bi=5, seed=22),
            dict(model="BayesRR", y=y, it=20, bi=5, seed=23)]
    return {"job%d" % i: r for i, r in enumerate(_bw().fit_many(X, jobs))}


def _sem(name):
    return lambda: getattr(_bw(), name)(tp()[2], tp()[0], **SIX)


def _split():
    X = tp()[0]
    return np.ascontiguousarray(X[:130]), np.ascontiguousarray(X[130:])


CASES = {
    "MRR3 tpod k3": lambda: _bw().MRR3(tp()[2], tp()[0], maxit=6),
    "MRR3F tpod k3": lambda: _bw().MRR3F(tp()[2], tp()[0], maxit=6),
    "mrr dense host": lambda: _bw().mrr(real_design()[1], _bw().dense(real_design()[0]), maxit=6),
    "mrr dense device": _mrr_dense_device,
    "mkr grm150": _mkr,
    "PEGS tpod k3": _pegs,
    "PEGSZ panel sparse dense": _pegs_sparse("pz_mixed4_k3"),
    "PEGS_sparse inc12": _pegs_sparse("ps_inc12_k3"),
    "PEGSZ_sparse two inc": _pegs_sparse("pzs_two_inc_k3"),
    "PEGSX inc12 cnv_trace": _pegs_sparse("px_inc12_k3"),
    "emRR": _em("emRR"), "emBB": _em("emBB"), "emBCpi": _em("emBCpi"), "lasso": _em("lasso"),
    "emML D": lambda: _bw().emML(tp()[1], tp()[0], D=np.linspace(0.5, 1.5, 128), maxit=6),
    "wgr": _wgr(), "wgr eigK": _wgr(eig=True), "wgr bag rp": _wgr(bag=0.8, rp=True), "wgr nan y": _wgr(nan_y=True),
    "KMUP": _kmup, "KMUP2": _kmup2, "fit_many": _fit_many,
    "mcmcCV": lambda: _bw().mcmcCV(tp()[1], tp()[0], k=2, n=1, it=20, bi=5, seed=9),
    "XSEMF": _sem("XSEMF"), "ZSEMF": _sem("ZSEMF"), "YSEMF": _sem("YSEMF"), "MEGA": _sem("MEGA"), "GSEM": _sem("GSEM"),
    "ZFUVBETA": lambda: {"out": _bw().ZFUVBETA(tp()[2], tp()[0], **SIX)},
    "solver1xF": lambda: {"b": _bw().solver1xF(tp()[1], tp()[0], maxit=6, tol=0)},
    "solver2x": lambda: {"out": _bw().solver2x(tp()[1], S2.dense(196, 2, 222), tp()[0], maxit=6, tol=0)},
    "EigenArcZ parts": lambda: _bw().EigenArcZ(*_split(), parts=True),
    "crossprod2 device_out": lambda: {"out": _bw().crossprod2(*_split(), device_out=True)},
    "GRM device_out": lambda: {"K": _bw().GRM(tp()[0], device_out=True)},
}


def _flat(prefix, v, out):
    if isinstance(v, dict):
        for k, w in v.items():
            _flat("%s / %s" % (prefix, k), w, out)
    elif isinstance(v, (list, tuple)) and v and not np.isscalar(v[0]):
        for i, w in enumerate(v):
            _flat("%s[%d]" % (prefix, i), w, out)
    else:
        if hasattr(v, "data_ptr"):
            v = v.cpu().numpy()
        a = np.ascontiguousarray(np.asarray(v, np.float64) if np.isscalar(v) or isinstance(v, (list, tuple, bool)) else v)
        out.append((prefix, hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()))


def digests(name):
    """[(entry, sha256)] of one case: one per output array (the entries of a list and of a nested dict each get their own)."""
    out = []
    with switches():       # (no BWGR_* switch of the environment reaches a panel: the table was recorded with none set)
        _flat(name, CASES[name](), out)
    return out
