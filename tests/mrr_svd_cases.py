"""The cases of mrr_svd and of the transpose product X'A, shared by tests/test_mrr_svd_cpu.py (their soundness, the rank rule, the plan's edges)
and the GPU files tests/test_gpu_mrr_svd.py and tests/test_gpu_xta.py.

FIT: genotypes binomial(2, f) with f uniform in 0.1 .. 0.9, traits with a correlated genetic part, 20 % of the records missing (a pattern per
trait, or one shared by all).  maxit is capped at 30 .. 40 except where the fit converges: run to convergence, the wider cases lose a
trait's residual variance or bend in almost every sweep, and their restatement is no longer stable against a perturbation of 2^-40.
  r = 64, 65, 128, 129: the edges of the train's 64-column blocks; k = 1 and k = 16; p < n (r = p, n - p null directions dropped).
XTA: the shapes of tests/test_gpu_xta.py, with what each one is there for."""
import ctypes as C
import functools

import numpy as np

import mrr_svd_restatement as SR

FIT = {
    # name: n, p, k, seed, maxit, shared pattern
    "k3_r65": dict(n=66, p=400, k=3, seed=1, maxit=30),
    "k16_r149": dict(n=150, p=400, k=16, seed=4, maxit=30),
    "k16_p_lt_n": dict(n=400, p=300, k=16, seed=7, maxit=30),
    "k16_r299": dict(n=300, p=700, k=16, seed=8, maxit=40),
    "k6_r129": dict(n=130, p=500, k=6, seed=2, maxit=30),
    "k5_shared": dict(n=120, p=350, k=5, seed=9, maxit=30, shared=True),
    "k2_converges": dict(n=200, p=60, k=2, seed=15, maxit=500),
    "k4_r128_converges": dict(n=129, p=129, k=4, seed=6, maxit=500),
    "k1_r64_converges": dict(n=65, p=300, k=1, seed=5, maxit=500),
}
DRIVER = ("k3_r65", "k16_p_lt_n", "k2_converges", "k1_r64_converges", "k5_shared")      # mrr_svd(Y, W) end to end


def data(name):
    """(W int8 n x p, Y n x k float-rounded with NaN)"""
    c = FIT[name]
    n, p, k = c["n"], c["p"], c["k"]
    rng = np.random.default_rng(c["seed"])
    f = rng.uniform(0.1, 0.9, p)
    W = rng.binomial(2, f, (n, p)).astype(np.int8)
    L = rng.normal(size=(k, k)) * 0.6 + np.eye(k)
    g = (W - W.mean(0)) @ rng.normal(size=(p, k)) / np.sqrt(p) @ L
    Y = g / g.std(0) + rng.normal(size=(n, k))
    Y = Y.astype(np.float32).astype(np.float64)
    if c.get("shared"):
        Y[rng.uniform(size=n) < 0.2, :] = np.nan
    else:
        Y[rng.uniform(size=(n, k)) < 0.2] = np.nan
    return W, Y


def npat(Y):
    return len({tuple(np.isnan(Y[:, t])) for t in range(Y.shape[1])})


@functools.lru_cache(maxsize=None)
def engine_ref(name):
    """(Y, X = the restatement's own eigh design, its fit with trace) -- made once, shared, never written into"""
    W, Y = data(name)
    D = SR.design_eigh(W)
    X = np.asfortranarray(D["X"])
    return Y, X, SR.fit(Y, X, maxit=FIT[name]["maxit"], trace=True)


@functools.lru_cache(maxsize=None)
def driver_ref(name):
    """(W, Y, the restatement's mrr_svd on numpy's SVD of the centred matrix)"""
    W, Y = data(name)
    return W, Y, SR.mrr_svd(Y, W, maxit=FIT[name]["maxit"])


# ---- X'A ----
XTA = {
    # n, p, block (0: the default), codes: "012" or "int8" (-128 .. 127 with constant columns), what it is there for
    "two_slabs": dict(n=300, p=700, block=0, codes="012"),       # n no multiple of 64, two slabs; p = 10 * 64 + 60
    "tall_slab": dict(n=2000, p=300, block=16, codes="012"),     # R = 1024: a second slab of a tall geometry
    "padded_slab": dict(n=1100, p=300, block=16, codes="012"),   # one slab, padded
    "two_trips": dict(n=70, p=65600, block=0, codes="012"),      # more column blocks than the grid: a second trip of 1 block
    "int8_codes": dict(n=200, p=130, block=0, codes="int8"),     # the whole int8 range, constant columns (-128, 127, 0 among them)
}
XTA_K = (1, 16, 17, 33)


def xta_W(name):
    c = XTA[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if c["codes"] == "012":
        return rng.binomial(2, rng.uniform(0.05, 0.95, c["p"]), (c["n"], c["p"])).astype(np.int8)
    W = rng.integers(-128, 128, (c["n"], c["p"])).astype(np.int8)
    W[:, 0], W[:, 1], W[:, 2], W[:, 64], W[:, 129] = -128, 127, 0, 5, -1
    W[0, 3], W[1, 3] = -128, 127
    return W


def xta_A(name, k, seed=0):
    rng = np.random.default_rng(1000 + seed + k)
    return np.asfortranarray(rng.normal(size=(XTA[name]["n"], k)) * np.exp(rng.normal(size=k)))


def slab_rows(n, p, block=0, nwg=0):
    """the slab height bwgr_panel_create would pick for an int8 panel (bwgr_debug_panel_plan, host arithmetic)"""
    from bwgr_amd import _lib
    out = (C.c_int64 * 25)()
    _lib.check(_lib.lib().bwgr_debug_panel_plan(0, n, p, block, nwg, 0, -1, 0, out))
    return int(out[2])
