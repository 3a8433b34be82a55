"""The cases of the mkr / mrr(Y, dense(X)) tests, in one place: tests/test_gpu_mkr.py fits them on the GPU against tests/mrr_restatement.py, and
tests/test_mkr_cpu.py checks on the CPU that the restatement alone stays finite and runs at least three sweeps on each, and that the library's
plan (bwgr_debug_mrr_dense_plan) gives each the blocks, edge widths, row-tile trips and ngl < npat it is there for.

A case is (Y, X, opts): Y n x k with NaN = missing, X the n x r float64 design fed alike to the library and to the restatement."""
import numpy as np


def genotypes(n, p, seed):
    return np.random.default_rng(seed).integers(0, 3, size=(n, p)).astype(np.float64)


def grm(Z):
    """the centred genomic relationship matrix of a 0/1/2 matrix, Zc Zc' / sum_j var(z_j) (the restated GRM; rank n - 1)"""
    Zc = Z - Z.mean(0)
    return (Zc @ Zc.T) / Zc.var(0).sum()


def grm150():
    return grm(genotypes(150, 400, 7))


def traits(X, k, seed, frac=0.0, patterns=None):
    """k correlated traits with signal in the columns of X; `frac`: every record missing with that chance (k distinct patterns);
    `patterns`: per trait, the chance of its own missing rows (0: fully observed)."""
    rng = np.random.default_rng(seed)
    n, r = X.shape
    Xc = X - X.mean(0)
    G = Xc @ (rng.normal(size=(r, k)) / np.sqrt(r))
    sd = G.std(0)
    Y = G / np.where(sd > 0, sd, 1.0) + rng.normal(size=(n, k)) + 3.0
    if patterns is not None:
        for t, fr in enumerate(patterns):
            if fr > 0:
                Y[rng.random(n) < fr, t] = np.nan
    elif frac > 0:
        Y[rng.random((n, k)) < frac] = np.nan
    return Y


def real_design(n, r, seed):
    """real-valued columns of unequal scale and non-zero means"""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.normal(size=(n, r)) * rng.uniform(0.5, 2.0, size=r) + rng.normal(size=r))


def npat(Y):
    """the distinct missingness patterns of Y's traits"""
    obs = ~np.isnan(Y if Y.ndim == 2 else Y[:, None])
    return len({obs[:, t].tobytes() for t in range(obs.shape[1])})


# name -> (n, r, k, settings).  The plan facts a case is there for are asserted in tests/test_mkr_cpu.py.
def case(name):
    import bwgr_amd
    if name == "grm150":             # r = 149: blocks of 64, 64, 21; 150 rows: tiles of 64, 64, 22 (and one of padding); the defaults
        X = bwgr_amd.K2X(grm150())
        return traits(X, 3, 21, frac=0.15), X, {}
    if name.startswith("r"):         # r1, r64, r65, r130 at n = 200
        r = int(name[1:])
        X = real_design(200, r, 30 + r)
        return traits(X, 3, 40 + r, frac=0.1), X, dict(maxit=20)
    if name == "tall":               # 2 304 padded rows = 36 tiles on 32 workgroups: a second trip
        X = real_design(2200, 70, 51)
        return traits(X, 2, 52, frac=0.1), X, dict(maxit=10)
    if name == "k1":
        X = real_design(200, 70, 61)
        return traits(X, 1, 62, frac=0.2)[:, 0], X, dict(maxit=20)
    if name == "k16":                # sixteen distinct patterns: ngl < npat, the inverses from global memory
        X = real_design(200, 70, 63)
        return traits(X, 16, 64, frac=0.1), X, dict(maxit=10)
    if name == "k4full":             # no missing record: one pattern
        X = real_design(200, 70, 65)
        return traits(X, 4, 66), X, dict(maxit=20)
    if name in ("TH", "updateMu", "XFA"):
        X = real_design(200, 130, 71)
        opt = {"TH": dict(TH=True), "updateMu": dict(updateMu=True), "XFA": dict(XFA=True, NumXFA=2)}[name]
        Y = traits(X, 4, 72, patterns=[0.1, 0.0, 0.3, 0.0])
        Y[np.isnan(Y[:, 0]), 3] = np.nan          # traits 0 and 3 share a pattern: three patterns for four traits
        return Y, X, dict(maxit=20, **opt)
    if name == "int012":             # the design both engines take: 300 x 500 0/1/2
        X = np.asfortranarray(genotypes(300, 500, 81))
        return traits(X, 3, 82, frac=0.1), X, dict(maxit=15)
    raise KeyError(name)


CASES = ["grm150", "r1", "r64", "r65", "r130", "tall", "k1", "k16", "k4full", "TH", "updateMu", "XFA", "int012"]
