"""The inputs of every GPU case of tests/test_gpu_sem2.py, shared with tests/test_sem2_cpu.py (which asserts the cases' preconditions on the
restatement) and the restatement's results on them, computed once per session and left unchanged.

An engine case is dict(Y, Z, X, kw): uvbeta2(Y, Z, X, **kw).  A driver case is dict(Y, X, npc, kw): MEGA / GSEM(Y, X, npc, **kw)."""
import functools
import os

import numpy as np

import sem2_restatement as S2
from conftest import synth_small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = dict(maxit=6, tol=0)


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def tpod():
    """196 x 376: six 64-marker blocks, the last of 56 markers."""
    return _ro(np.asfortranarray(np.load(os.path.join(ROOT, "tests", "golden", "tpod.npz"))["gen"]))


@functools.lru_cache(None)
def slabs900():
    """700 x 900: three row slabs with nwg = 3."""
    return _ro(np.asfortranarray(synth_small(700, 900, seed=3)[0]))


def traits(X, k, frac, seed, patterns=None):
    """test_gpu_mrr._traits: a polygenic signal plus noise around 3; `frac` of the records missing, or patterns[t] of trait t's."""
    rng = np.random.default_rng(seed)
    Xf = X.astype(np.float64)
    n, p = X.shape
    B = rng.normal(size=(p, k)) * (1.0 / np.sqrt(p))
    G = (Xf - Xf.mean(0)) @ B
    sd = G.std(0)
    Y = G / np.where(sd > 0, sd, 1.0) + rng.normal(size=(n, k)) + 3.0
    if patterns is None:
        Y[rng.random((n, k)) < frac] = np.nan
    else:
        for t, fr in enumerate(patterns):
            if fr > 0:
                Y[rng.random(n) < fr, t] = np.nan
    return Y


def dense(n, q, seed):
    """A latent-like design: columns on falling scales, off-centre."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, q)) * (4.0 / (1.0 + np.arange(q))) + rng.normal(size=q)


def _genotypes(n, p, seed):
    return np.asfortranarray(np.random.default_rng(seed).integers(0, 3, size=(n, p)).astype(np.int8))


def _tp(k, q, seed, frac=0.1, p=None, **kw):
    X = tpod() if p is None else np.asfortranarray(tpod()[:, :p])
    return dict(Y=traits(tpod(), k, frac, seed)[:, :k], Z=dense(196, q, seed + 1), X=X, kw=dict(kw or SIX))


def _one_pattern():
    c = _tp(5, 3, 31, frac=0.0)
    miss = np.random.default_rng(32).random((196, 2)) < 0.15
    for t, g in enumerate((0, 1, 0, 1, 0)):        # traits 0, 2, 4 share their rows, and so do 1 and 3
        c["Y"][miss[:, g], t] = np.nan
    return c


def _full_and_masked():
    c = _tp(3, 2, 33)
    c["Y"] = traits(tpod(), 3, 0.0, 33, patterns=(0.2, 0.0, 0.3))
    return c


def _all_nan():
    c = _tp(4, 3, 35)
    c["Y"][:, 2] = np.nan
    return c


def _xx1_zero():
    """Column 1 of Z is constant (0.75: every partial sum is exact) on trait 0's rows and varies on the others': XX1 = 0 for that trait only."""
    c = _tp(3, 3, 37, frac=0.2)
    c["Z"][~np.isnan(c["Y"][:, 0]), 1] = 0.75
    return c


def _trx1_zero():
    """Every column of Z is constant on trait 1's rows: TrXSX1 = 0 there, the dense design is skipped for that trait."""
    c = _tp(3, 3, 39, frac=0.2)
    c["Z"][~np.isnan(c["Y"][:, 1])] = np.array([0.5, -1.25, 2.0])
    return c


def _slabs_defaults():
    """The reference's defaults on three slabs.  cnv is an absolute measure (sum (delta b)^2), so traits on smaller scales stop sooner: the
    four scales make the traits stop at four different sweeps (33, 7, 19, 4), with steps of cnv large enough that none comes nearer than
    0.04 to log10(tol) (seed 57, picked on the CPU; tests/test_sem2_cpu.py asserts both)."""
    X = slabs900()
    Y = (traits(X, 4, 0.1, 57) - 3.0) * np.array([0.3, 0.03, 0.1, 0.01]) + 3.0
    return dict(Y=Y, Z=dense(700, 3, 43), X=X, kw={}, nwg=3)


def residual_path(n):
    """A narrow tall panel for the leg's two residual paths (n below / above the plan's lds_rows)."""
    X = _genotypes(n, 130, 51)
    return dict(Y=traits(X, 2, 0.1, 52), Z=dense(n, 2, 53), X=X, kw=dict(maxit=2, tol=0))


ENGINE = {
    "k3_q3": lambda: _tp(3, 3, 11),
    "q1": lambda: _tp(3, 1, 13),
    "q7_beyond_k": lambda: _tp(3, 7, 15),
    "k17_two_solve_workgroups": lambda: _tp(17, 2, 17),
    "k65_two_groups": lambda: _tp(65, 2, 19, maxit=3, tol=0),
    "p1": lambda: _tp(3, 2, 21, p=1, maxit=4, tol=0),
    "p63": lambda: _tp(3, 2, 23, p=63, maxit=4, tol=0),
    "p64": lambda: _tp(3, 2, 25, p=64, maxit=4, tol=0),
    "p65": lambda: _tp(3, 2, 27, p=65, maxit=4, tol=0),
    "one_pattern": _one_pattern,
    "full_and_masked": _full_and_masked,
    "all_nan_trait": _all_nan,
    "xx1_zero": _xx1_zero,
    "trx1_zero": _trx1_zero,
    "maxit0": lambda: _tp(3, 2, 45, maxit=0, tol=0),
    "maxit1": lambda: _tp(3, 2, 45, maxit=1, tol=0),
    "slabs_defaults": _slabs_defaults,
}


@functools.lru_cache(None)
def engine(name):
    c = ENGINE[name]()
    for key in ("Y", "Z"):
        _ro(c[key])
    return c


@functools.lru_cache(None)
def engine_ref(name):
    c = engine(name)
    return S2.uvbeta2(c["Y"], c["Z"], c["X"], **c["kw"])


# ---- the drivers ----
def f32(Y):
    return np.asarray(Y, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(None)
def tpod_traits():
    """The seed-227 traits of tests/test_gpu_sem.py."""
    return _ro(f32(traits(tpod(), 4, 0.1, seed=227)))


@functools.lru_cache(None)
def slab_traits():
    """Three traits for the drivers' default stopping on the 700 x 900 panel: a polygenic signal plus noise that the traits share in part
    (correlated traits: the singular values of MEGA's standardised Y2 lie apart, gap 0.165; GSEM's G: 0.373), on the scales 0.01, 0.02, 0.04
    (cnv is absolute: small scales stop within a few sweeps, by large steps; no cnv of any stage comes nearer than 0.04 to log10(tol)).
    10 % missing.  Seed 333, picked on the CPU; tests/test_sem2_cpu.py asserts the figures."""
    X = slabs900()
    rng = np.random.default_rng(333)
    Xf = X.astype(np.float64)
    n, p = X.shape
    g = (Xf - Xf.mean(0)) @ (rng.normal(size=(p, 3)) / np.sqrt(p))
    g = g / g.std(0) * 0.5
    c = rng.normal(size=n)
    E = np.stack([c + 0.5 * rng.normal(size=n), c - 0.9 * rng.normal(size=n), 0.4 * c + 1.3 * rng.normal(size=n)], 1)
    Y = (g + E) * np.array([0.01, 0.02, 0.04]) + 3.0
    Y[rng.random((n, 3)) < 0.1] = np.nan
    return _ro(Y)


@functools.lru_cache(None)
def nan_trait_traits():
    Y = np.array(tpod_traits())
    Y[:, 2] = np.nan
    return _ro(Y)


DRIVER = {
    "tpod_npc0": lambda: dict(Y=tpod_traits(), X=tpod(), npc=0, kw=SIX),
    "tpod_npc-1": lambda: dict(Y=tpod_traits(), X=tpod(), npc=-1, kw=SIX),
    "tpod_npc2": lambda: dict(Y=tpod_traits(), X=tpod(), npc=2, kw=SIX),
    "slabs_defaults": lambda: dict(Y=slab_traits(), X=slabs900(), npc=-1, kw={}, nwg=3),
    "nan_trait": lambda: dict(Y=nan_trait_traits(), X=tpod(), npc=3, kw=SIX),       # GSEM only: MEGA refuses it
}
DRIVER_CASES = [(name, case) for case in DRIVER for name in ("MEGA", "GSEM") if not (name == "MEGA" and case == "nan_trait")]


@functools.lru_cache(None)
def driver_ref(name, case, flip=None):
    c = DRIVER[case]()
    return getattr(S2, name)(c["Y"], c["X"], c["npc"], flip=flip, **c["kw"])


def stages(name, o):
    """The fits a driver's restatement ran, for the preconditions on cnv."""
    return [o["BETA"], o["fit"]] + ([o["LSB"]] if name == "MEGA" else [])
