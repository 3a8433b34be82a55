"""The shapes of the fp64 families' parity tests on tall panels, other slab heights and wide panels (tests/test_gpu_tall.py), kept in one
place so that tests/test_tall_cases_cpu.py can check, without a GPU, that every shape still reaches the code it is listed for under the
library's own host arithmetic: bwgr_debug_panel_plan (K, R, ld), bwgr_debug_uvb_plan (the pass's grid), bwgr_debug_xxt_plan (T, tiles,
pieces) and bwgr_debug_launch_plan (the grids of the tail, product and finish kernels).

Every kernel named here strides over its rows, markers or entries by its grid, so "a second trip" means: more work than one grid of
workgroups covers.  The trips, from the plans (256 threads per workgroup):
  uvb_pass   ceil((ld / 64) / pass workgroups): 64-row tiles of k_uvb_pass; dacc, eacc and the staged dBl carry across a workgroup's tiles
  uvb_rows   ceil(ld / (UVB_NP x 256)): k_uvb_rows
  mrr_ey     ceil(ld / (NP x 256)): k_mrr_ey
  mrr_tilde  ceil(p / (NP x 256)): k_mrr_tilde
  mrr_setup  ceil(p / (workgroups x 4)): k_mrr_setup_cols, one marker per wave
  kfin_apply ceil(n^2 / (workgroups x 256)): k_kfin_apply;  xxt_zero likewise for k_xxt_zero, which is launched only when a tile has several
             workgroups (accumulate).  At n >= 725 the plan splits a chunk only from about 2 000 markers on, a shape whose restatements take
             too long for this suite; so kern1100 reaches k_xxt_zero with three forced chunks (kchunk: BWGR_KCHUNK when the panel is made;
             forced_chunks as the plan then reports them), which integer sums make bit-equal to the one-chunk product
  pxb        (row tiles, 16-column slices, marker chunks, markers per chunk) of k_pxb; pxb_cross: a 1 024-row tile that spans two slabs

The two-design fits -- uvbeta2, MEGA, GSEM -- run on tall9k and slab1280 through the same pass, row reduction and panel_xb; their inputs and
the restatement's results on them are at the end of this file.  The two-panel shapes are in tests/pair_cases.py.
"""
import ctypes as C
import functools

import numpy as np

from conftest import synth_small
import driver_cases as dc

# tag -> n, p, block (0 = the default), seed of the genotypes
CASES = {
    "tall9k":     dict(n=9000,  p=200,   block=0,  seed=2900),
    "tall16k":    dict(n=16500, p=130,   block=0,  seed=2901),
    "slab1280":   dict(n=5000,  p=200,   block=16, seed=2902),
    "slab1024":   dict(n=2000,  p=300,   block=16, seed=2903),
    "kern1100":   dict(n=1100,  p=300,   block=0,  seed=2904),
    "kern1100s":  dict(n=1100,  p=300,   block=16, seed=2904),     # the same genotypes in ONE slab of 1 152 rows: another R, but the slab base
                                                                   # r0 / R is always 0 -- among the kernel shapes only slab1024 addresses a second slab
    "wide33k":    dict(n=200,   p=33000, block=0,  seed=2905),
    "xbwide":     dict(n=300,   p=9000,  block=0,  seed=2906),
}

# What each shape is there for, as the plans must report it (see the module's docstring for the names).  pad: ld - n; last64: markers of the
# last 64-marker block of mrr and uvbeta; pxb: (tiles, slices, chunks, chunk) for the k given as pxb_k; pxb_last: markers of the last chunk.
EXPECT = {
    "tall9k":    dict(K=36, R=256, ld=9216, pad=216, uvb_pass_wg=64, uvb_pass=3, uvb_rows=2, pxb_k=17, pxb=(9, 2, 2, 128), pxb_last=72),
    "tall16k":   dict(K=65, R=256, ld=16640, mrr_ey=2, uvb_rows=3, last64=2),
    "slab1280":  dict(K=4, R=1280, ld=5120, pad=120, uvb_pass=2, uvb_rows=1, mrr_ey=1, pxb_k=1, pxb=(5, 1, 2, 128), pxb_last=72, pxb_cross=True),
    "slab1024":  dict(K=2, R=1024, ld=2048, uvb_pass=1, pxb_k=17, pxb=(2, 2, 3, 128), pxb_last=44, pxb_cross=False),
    "kern1100":  dict(K=5, R=256, ld=1280, T=9, tiles=45, kfin_apply=2, accumulate=False, kchunk=100, forced_chunks=3, xxt_zero=3),
    "kern1100s": dict(K=1, R=1152, ld=1152, T=9, tiles=45, kfin_apply=2, accumulate=False),
    "wide33k":   dict(K=1, ld=256, mrr_tilde=3, mrr_setup=2, last64=40),
    "xbwide":    dict(ld=512, pxb_k=1, pxb=(1, 1, 36, 256), pxb_last=40, pxb_cap=True),
}

LAUNCH_FIELDS = ("mrr_np", "mrr_setup_wg", "mrr_pass_wg", "uvb_np", "uvb_pass_wg", "uvb_shift_wg", "uvb_xb_wg", "pxb_rows", "pxb_tiles",
                 "pxb_slices", "pxb_chunks", "pxb_chunk", "pxb_finish_wg", "xxt_zero_wg", "kfin_apply_wg", "threads", "pxb_chunks_max", "pxb_mt")
XXT_FIELDS = ("chunk", "nchunks", "tiles", "wgs", "ws_bytes", "T", "sub", "piece")


def launch_plan(n, ld, p, k=1):
    """(status, dict) of bwgr_debug_launch_plan (host arithmetic, no GPU)."""
    from bwgr_amd import _lib
    out = (C.c_int64 * len(LAUNCH_FIELDS))(*([-1] * len(LAUNCH_FIELDS)))
    rc = _lib.lib().bwgr_debug_launch_plan(int(n), int(ld), int(p), int(k), out)
    return rc, dict(zip(LAUNCH_FIELDS, (int(v) for v in out)))


def xxt_plan(n, p, xmax=2, kchunk=0):
    from bwgr_amd import _lib
    out = (C.c_int64 * len(XXT_FIELDS))()
    rc = _lib.lib().bwgr_debug_xxt_plan(int(n), int(p), int(xmax), int(kchunk), out)
    assert rc == 0, _lib.lib().bwgr_last_error().decode()
    return dict(zip(XXT_FIELDS, (int(v) for v in out)))


def _ceil(a, b):
    return -(-a // b)


def plans(tag, k=None):
    """Everything EXPECT speaks of, for one shape: the panel's geometry, the grids and the trips they give."""
    import bwgr_amd
    c = CASES[tag]
    n, p = c["n"], c["p"]
    pl = dc.panel_plan(0, n, p, c["block"])
    ld, R = pl["ld"], pl["R"]
    k = EXPECT[tag].get("pxb_k", 1) if k is None else k
    rc, lp = launch_plan(n, ld, p, k)
    assert rc == 0
    t = lp["threads"]
    pl.update(lp)
    pl["pad"] = ld - n
    pl["last64"] = p - (_ceil(p, 64) - 1) * 64
    up = bwgr_amd.uvb_plan(n, p, 3)
    if ld == _ceil(n, 128) * 128:       # (bwgr_debug_uvb_plan pads the rows to 128; a taller slab pads further)
        assert up["pass_wg"] == lp["uvb_pass_wg"]
    pl["uvb_pass"] = _ceil(ld // 64, lp["uvb_pass_wg"])
    pl["uvb_rows"] = _ceil(ld, lp["uvb_np"] * t)
    pl["mrr_ey"] = _ceil(ld, lp["mrr_np"] * t)
    pl["mrr_tilde"] = _ceil(p, lp["mrr_np"] * t)
    pl["mrr_setup"] = _ceil(p, lp["mrr_setup_wg"] * (t // 64))
    pl["kfin_apply"] = _ceil(n * n, lp["kfin_apply_wg"] * t)
    xp = xxt_plan(n, p)
    pl["T"], pl["tiles"], pl["accumulate"] = xp["T"], xp["tiles"], xp["nchunks"] * xp["sub"] > 1
    pl["kchunk"] = EXPECT[tag].get("kchunk", 0)
    fp = xxt_plan(n, p, kchunk=pl["kchunk"])
    pl["forced_chunks"] = fp["nchunks"]
    pl["xxt_zero"] = _ceil(n * n, lp["xxt_zero_wg"] * t) if fp["nchunks"] * fp["sub"] > 1 else 0      # (0: not launched)
    pl["pxb"] = (lp["pxb_tiles"], lp["pxb_slices"], lp["pxb_chunks"], lp["pxb_chunk"])
    pl["pxb_last"] = p - (lp["pxb_chunks"] - 1) * lp["pxb_chunk"]
    rows = lp["pxb_rows"]
    pl["pxb_cross"] = any((i * rows) // R != (min((i + 1) * rows, ld) - 1) // R for i in range(lp["pxb_tiles"]))
    # the chunk rule before it rounds the chunk up to whole staged tiles of B: min(cap, tiles of B, what fills the chip)
    fill = max(1, _ceil(1024, lp["pxb_tiles"] * lp["pxb_slices"]))
    pl["pxb_cap"] = min(_ceil(p, lp["pxb_mt"]), fill) >= lp["pxb_chunks_max"]
    return pl


def panel_kw(tag):
    return {"block": CASES[tag]["block"]} if CASES[tag]["block"] else {}


# ---- the two-design fits on these shapes: uvbeta2 (solver2x per trait), MEGA and GSEM ----
# tag -> how the drivers run there and the seed of their traits (tests/test_tall_cases_cpu.py asserts the preconditions and states the
# figures).  slab1280: six sweeps per stage; tall9k: the reference's defaults, every stage stopping by its own test.
SEM2_DRIVERS = {"slab1280": dict(kw=dict(maxit=6, tol=0), seed=3001), "tall9k": dict(kw={}, seed=3011)}
SEM2_ENGINE = {("tall9k", 3): 3100, ("slab1280", 3): 3110, ("slab1280", 65): 3120}      # (tag, k) -> the seed of Y; Z's is the next
SEM2_ENGINE_KW = dict(maxit=6, tol=0)


@functools.lru_cache(maxsize=None)
def uvb2_case(tag, k):
    """uvbeta2's inputs: k traits with 10 % of the records missing, q = 3 dense columns on falling scales, the shape's genotypes"""
    import sem2_cases as S2C
    X, seed = data(tag), SEM2_ENGINE[(tag, k)]
    Y, Z = S2C.traits(X, k, 0.1, seed), S2C.dense(X.shape[0], 3, seed + 1)
    Y.setflags(write=False); Z.setflags(write=False)
    return dict(Y=Y, Z=Z, X=X, kw=dict(SEM2_ENGINE_KW))


@functools.lru_cache(maxsize=None)
def uvb2_ref(tag, k):
    import sem2_restatement as S2
    c = uvb2_case(tag, k)
    return S2.uvbeta2(c["Y"], c["Z"], c["X"], **c["kw"])


@functools.lru_cache(maxsize=None)
def driver_traits(tag):
    """tests/sem2_cases.py's slab_traits on this shape: three correlated traits -- a polygenic signal plus noise the traits share in part, so
    that the singular values of MEGA's Y2 and of GSEM's G lie apart -- on the scales 0.01, 0.02, 0.04 (cnv is absolute: small scales stop
    within a few sweeps, by large steps), 10 % missing."""
    X = data(tag)
    rng = np.random.default_rng(SEM2_DRIVERS[tag]["seed"])
    Xf = X.astype(np.float64)
    n, p = X.shape
    g = (Xf - Xf.mean(0)) @ (rng.normal(size=(p, 3)) / np.sqrt(p))
    g = g / g.std(0) * 0.5
    c = rng.normal(size=n)
    E = np.stack([c + 0.5 * rng.normal(size=n), c - 0.9 * rng.normal(size=n), 0.4 * c + 1.3 * rng.normal(size=n)], 1)
    Y = (g + E) * np.array([0.01, 0.02, 0.04]) + 3.0
    Y[rng.random((n, 3)) < 0.1] = np.nan
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=None)
def driver_ref(name, tag):
    """the restatement's MEGA / GSEM (npc = -1) on the shape, computed once per session and left unchanged"""
    import sem2_restatement as S2
    return getattr(S2, name)(driver_traits(tag), data(tag), -1, **SEM2_DRIVERS[tag]["kw"])


@functools.lru_cache(maxsize=None)
def data(tag):
    """The genotypes (int8, codes 0 / 1 / 2, column-major, read-only) from the shape's seed."""
    c = CASES[tag]
    X = np.asfortranarray(synth_small(c["n"], c["p"], seed=c["seed"])[0])
    X.setflags(write=False)
    return X
