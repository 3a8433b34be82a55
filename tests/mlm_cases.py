"""The cases of MLM's tests (tests/test_mlm_cpu.py, tests/test_gpu_mlm.py), their data and their restatement, computed once per process.

The recipe: genotypes binomial(2, fr) with fr uniform in 0.1 .. 0.9; X an intercept, then up to four dummy columns of one factor, then normal
covariates, rounded to float; traits with a correlated genetic part plus X beta plus noise, rounded to float; 20 % of the records missing, per
trait or shared by all traits.  One departure: k2_f256 (n = 330, f = 256) can lose at most n - f - 17 = 57 records per trait (17 %) if
n_t - f >= 17 is to hold, so its missing records are capped there.

  k3_p65_f1     second 64-column block of one column; 64-row tile edge; intercept only
  k4_p130_f3    third block; row padding past 128
  k1_p64_f2     k = 1; exactly one block
  k16_p200_f5   16 traits, 16 patterns
  k6_p400_f17   second group of 16 in Z'X
  k2_f256       the f limit, four f-pieces; bends in almost every sweep
  k5_shared_f4  one shared pattern
  k2_conv_verb  the stopping rule: with verb=True the restatement stops long before maxit
  dense_k3      a real-valued dense(Z) (dosages: genotypes plus noise, rounded to float)
  two_slabs     a panel whose rows span two slabs (nwg = 2)
"""
import functools

import numpy as np

import mlm_restatement as LR

CASES = {
    "k3_p65_f1":    dict(n=66,  p=65,  k=3,  f=1,   maxit=30, seed=4101),
    "k4_p130_f3":   dict(n=131, p=130, k=4,  f=3,   maxit=30, seed=4102),
    "k1_p64_f2":    dict(n=65,  p=64,  k=1,  f=2,   maxit=30, seed=4103),
    "k16_p200_f5":  dict(n=150, p=200, k=16, f=5,   maxit=30, seed=4104),
    "k6_p400_f17":  dict(n=300, p=400, k=6,  f=17,  maxit=30, seed=4105),
    "k2_f256":      dict(n=330, p=100, k=2,  f=256, maxit=20, seed=4106),
    "k5_shared_f4": dict(n=120, p=350, k=5,  f=4,   maxit=29, seed=4107, shared=True),     # (not 30: the smallest ve falls to 0.2192 in sweep 30, below the 0.22 the cases keep)
    "k2_conv_verb": dict(n=200, p=60,  k=2,  f=2,   maxit=500, seed=4108, verb=True),
    "dense_k3":     dict(n=100, p=70,  k=3,  f=3,   maxit=30, seed=4109, dense=True),
    "two_slabs":    dict(n=300, p=130, k=3,  f=3,   maxit=30, seed=4110, panel_kw=dict(nwg=2)),
}
OTHER_SLABS = (dict(nwg=3), dict(block=16))      # two_slabs' rows in slabs of another height: three of 128 rows, one of 384
TABLE = ("k3_p65_f1", "k4_p130_f3", "k1_p64_f2", "k16_p200_f5", "k6_p400_f17", "k2_f256", "k5_shared_f4", "k2_conv_verb")
MISSING = 0.2
KEYS = ("b", "u", "hat", "h2", "GC", "vb", "ve", "cnv")


def design(rng, n, f):
    """n x f: an intercept, min(4, f - 1) dummy columns of one factor (its first level is the baseline), normal covariates; float-rounded"""
    nd = min(4, f - 1)
    cols = [np.ones(n)]
    if nd:
        lev = rng.permutation(np.arange(n) % (nd + 1))
        cols += [(lev == l + 1).astype(np.float64) for l in range(nd)]
    cols += [rng.normal(size=n) for _ in range(f - 1 - nd)]
    return LR.f32(np.column_stack(cols))


@functools.lru_cache(maxsize=None)
def data(name):
    """(Y, X, Z) of a case: Y n x k float-rounded with NaN, X n x f float-rounded, Z int8 (or float-rounded real values for a dense case)"""
    c = CASES[name]
    n, p, k, f = c["n"], c["p"], c["k"], c["f"]
    rng = np.random.default_rng(c["seed"])
    fr = rng.uniform(0.1, 0.9, p)
    Z = rng.binomial(2, fr, size=(n, p)).astype(np.int8)
    if c.get("dense"):
        Z = LR.f32(Z + rng.normal(scale=0.1, size=(n, p)))
    X = design(rng, n, f)
    Rg = np.full((k, k), 0.5) + 0.5 * np.eye(k)
    B = rng.normal(size=(p, k)) @ np.linalg.cholesky(Rg).T
    g = (Z - Z.mean(0)) @ B
    g /= g.std(0)
    Y = g + X @ rng.normal(size=(f, k)) + rng.normal(size=(n, k))
    nmiss = min(int(round(MISSING * n)), n - f - 17)
    if c.get("shared"):
        Y[rng.choice(n, nmiss, replace=False)] = np.nan
    else:
        for t in range(k):
            Y[rng.choice(n, nmiss, replace=False), t] = np.nan
    Y = LR.f32(Y)
    for a in (Y, X, Z):
        a.setflags(write=False)
    return Y, X, Z


def fit_kw(name):
    c = CASES[name]
    return dict(maxit=c["maxit"], verb=bool(c.get("verb", False)))


@functools.lru_cache(maxsize=None)
def ref(name, trace=False):
    """the restatement's list for a case (shared by the tests: do not write into it)"""
    Y, X, Z = data(name)
    return LR.fit(Y, X, Z.astype(np.float64), trace=trace, **fit_kw(name))


def npat(Y):
    return len({tuple(np.isnan(Y[:, t])) for t in range(Y.shape[1])})


def slab_rows(n, p, block=0, nwg=0):
    """the slab height bwgr_panel_create would pick for an int8 panel (bwgr_debug_panel_plan, host arithmetic)"""
    import ctypes as C
    from bwgr_amd import _lib
    out = (C.c_int64 * 25)()
    _lib.check(_lib.lib().bwgr_debug_panel_plan(0, n, p, block, nwg, 0, -1, 0, out))
    return int(out[2])
