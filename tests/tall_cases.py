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
the restatement's results on them follow the plans.  The two-panel shapes are in tests/pair_cases.py.

PEGS, PEGSZ and PEGSX (the last section; bwgr_debug_pegs_launch_plan, bwgr_debug_pegsx_plan, bwgr_debug_pegs_plan) run mrr's launch train
uncentred on wide33k, tall16k, slab1280 and slab1024, and their own kernels beside it.  Their trips:
  trace      ceil(ceil(m / 4) / (workgroups x 4)): k_pegsx_trace_panel / _dense, a wave four columns of the effect at once; the per-wave totals
             carry across a wave's trips, and k_mrr_finish adds as many partials as there are workgroups (1 024 at the cap)
  dsetup     ceil(q / (workgroups x 4)): k_pegs_dense_setup, one column per wave
  rows       ceil(n / threads): the row loops of k_pegs_dense_leg and k_pegsx_fixed (1 024 threads from 961 rows on)
  fixed_cols ceil(f / (threads / 64)): the fixed step's column loop, one wave per column of X;  quad  ceil(f / 64): the trace's quadratic form
  sparse_hat ceil(n / 256): the workgroups of k_pegs_sparse_hat, one thread per row, its rows of stride n against the engine's stride ld

tall9k_sparse and slab1280_sparse put sparse effects (csrc/pegs_sparse.hip.h) beside those panels: the sparse kernels index the residual by
the panel's ld (216 and 120 rows past n, R = 256 and 1 280), a level longer than 4 096 rows spans slab edges, and the rows of PEGS_MISSING
lie on both sides of one.
"""
import ctypes as C
import functools

import numpy as np

from conftest import synth_small
import driver_cases as dc
import pegs_cases as PC
import pegs_sparse_cases as SC
import pegsx_cases as XC

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


# ---- PEGS / PEGSZ / PEGSX ----
# rows missing in every trait (uvbeta's own traits use the first three entries as they stand): in the first and the last slab and on both
# sides of a slab boundary; on tall16k the last lies beyond k_mrr_ey's first trip
ALL_MISSING = {"tall9k": (7, 4095, 4096, 8500), "slab1280": (7, 1279, 1280, 4990), "slab1024": (7, 1023, 1024, 1990)}
# PEGS' traits on tall9k also miss the four rows 4096 .. 4099, which one lane of the trace kernels loads as one quad at the start of the 17th
# slab: the whole-quad skip of the trace and the unobserved-row skip of the fixed step happen at a slab edge
PEGS_MISSING = dict(ALL_MISSING, tall9k=(7, 4095, 4096, 4097, 4098, 4099, 8500), tall16k=(7, 8191, 8192, 16400))

# job -> the panel's shape tag (None: no panel; "slabs900": tests/pegs_cases.py's 700 x 900 panel in three slabs, not on CASES because no
# other family needs it here), k, f (PEGSX), maxit, the effects in list order ("panel", the q of a dense gauss(n, q, 503), or a sparse effect
# of tests/pegs_sparse_cases.py's builders: ("inc", q), an incidence of q levels, or ("overlap", q, density)), the seed of the traits (the
# shape's seed + 70) and the entries that run it ("PEGSZ_sparse": text 2, which takes the same list).  PEGS takes one design: on tall9k and slab1280 it runs the panel alone.
# dense16501 is a TrZSZ-only job (maxit = 0): 33 000 and 16 500 are multiples of four, so no other job has a partial last group of columns.
PEGS_JOBS = {
    "wide33k":    dict(tag="wide33k",  k=3, f=3,   maxit=2, effects=("panel",),    entries=("PEGS", "PEGSZ", "PEGSX")),
    "tall16k":    dict(tag="tall16k",  k=4, f=3,   maxit=3, effects=("panel",),    entries=("PEGS", "PEGSZ", "PEGSX")),
    "tall9k":     dict(tag="tall9k",   k=3, f=3,   maxit=3, effects=("panel", 5),  entries=("PEGS", "PEGSZ", "PEGSX")),
    "tall9k_rev": dict(tag="tall9k",   k=3, f=3,   maxit=3, effects=(5, "panel"),  entries=("PEGSZ",)),
    "slab1280":   dict(tag="slab1280", k=3, f=17,  maxit=3, effects=("panel", 5),  entries=("PEGS", "PEGSZ", "PEGSX")),
    "slab1024":   dict(tag="slab1024", k=3, f=3,   maxit=3, effects=("panel",),    entries=("PEGS", "PEGSZ", "PEGSX")),
    "dense16500": dict(tag=None, n=196, seed=2907, k=3, f=3, maxit=2, effects=(16500,), entries=("PEGSZ", "PEGSX")),
    "dense16501": dict(tag=None, n=196, seed=2907, k=3, f=3, maxit=0, effects=(16501,), entries=("PEGSX",)),
    "f256":       dict(tag="slabs900", k=3, f=256, maxit=4, effects=("panel",),    entries=("PEGSX",)),
    "tall9k_sparse":   dict(tag="tall9k",   k=3, f=3, maxit=3, effects=("panel", ("inc", 2), ("overlap", 30, 0.05)), entries=("PEGSZ", "PEGSX")),
    "slab1280_sparse": dict(tag="slab1280", k=3, f=3, maxit=3, effects=("panel", ("inc", 40)), entries=("PEGSZ", "PEGSX", "PEGSZ_sparse")),
}
TRZSZ_ALONE = ("wide33k", "dense16500", "dense16501", "f256")     # a maxit = 0 run that checks TrZSZ by itself
NORMAL_EQUATIONS = ("tall9k", "slab1280", "tall9k_sparse", "slab1280_sparse")
SAME_LEVEL = {"tall9k_sparse": (4095, 4096)}      # rows on both sides of a slab edge that the job's incidence puts on one level

# What each job is there for, as pegs_plans must report it.  m: the columns of the effect the trace figures speak of; trace_last: the trip
# (1-based) on which the last group of four columns runs; trace_tail: columns of that group.  dsetup = 1 on dense16500: k_pegs_dense_setup
# covers 32 768 columns per trip, twice the trace kernels' 16 384, and the job is not grown for it.
PEGS_EXPECT = {
    "wide33k":    dict(m=33000, trace_wg=1024, trace=3, trace_last=3, trace_tail=4, mrr_tilde=3, mrr_setup=2, last64=40, K=1),
    "tall16k":    dict(mrr_ey=2, K=65, R=256, last64=2, npat=4),
    "tall9k":     dict(ld=9216, ld128=9088, pad=216, leg_threads=1024, fixed_threads=1024, rows=9, npat=3),
    "tall9k_rev": dict(ld=9216, ld128=9088, pad=216, leg_threads=1024, rows=9),
    "slab1280":   dict(R=1280, K=4, ld=5120, fixed_threads=1024, fixed_cols=2, rows=5),
    "slab1024":   dict(R=1024, K=2, ld=2048, rows=2),
    "dense16500": dict(m=16500, trace_wg=1024, trace=2, trace_last=2, trace_tail=4, dsetup=1, dsetup_wg=4125, ld=256),
    "dense16501": dict(m=16501, trace_wg=1024, trace=2, trace_last=2, trace_tail=1, dsetup=1),
    "f256":       dict(K=3, R=256, ld=768, quad=4, lds_trace=33280, lds_fixed=4096, fixed_threads=704, fixed_cols=24),
    "tall9k_sparse":   dict(K=36, R=256, ld=9216, ld128=9088, pad=216, rows=9, sparse_hat=36, sparse_legs=("disjoint", "serial"), npat=3),
    "slab1280_sparse": dict(K=4, R=1280, ld=5120, ld128=5120, pad=120, rows=5, sparse_hat=20, sparse_legs=("disjoint",), npat=3),
}


def _pegs_shape(job):
    """n, the genotypes (or None), the seed of the shape and the panel's kwargs"""
    j = PEGS_JOBS[job]
    if j["tag"] is None:
        return j["n"], None, j["seed"], {}
    if j["tag"] == "slabs900":
        Z = XC.slabs900()
        return Z.shape[0], Z, 3, dict(nwg=3)
    return CASES[j["tag"]]["n"], data(j["tag"]), CASES[j["tag"]]["seed"], panel_kw(j["tag"])


@functools.lru_cache(maxsize=None)
def _pegs_dense(n, q):
    Z = PC.gauss(n, q, 503)
    Z.setflags(write=False)
    return Z


def _pegs_sparse(job, n, e, i):
    """effect i of a job, ("inc", q) or ("overlap", q, density), through the builders of tests/pegs_sparse_cases.py"""
    if e[0] == "inc":
        A = SC.incidence(n, e[1], 505 + i)
        for a, b in (SAME_LEVEL[job],) if job in SAME_LEVEL else ():
            A[b] = A[a]
        out = ("sparse", A)
    else:
        assert e[0] == "overlap"
        out = ("sparse",) + SC.overlapping(n, e[1], 505 + i, density=e[2])
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _pegs_effect(job, n, Z, kw, e, i):
    if e == "panel":
        return ("panel", Z, kw)
    return _pegs_sparse(job, n, e, i) if isinstance(e, tuple) else ("dense", _pegs_dense(n, e))


@functools.lru_cache(maxsize=None)
def pegs_data(job):
    """(Y, effects) of a job in the form of tests/pegs_cases.py: the traits of the issue -- k traits, each its own missingness pattern, on
    the job's first design -- with the rows of PEGS_MISSING missing in every trait"""
    j = PEGS_JOBS[job]
    n, Z, seed, kw = _pegs_shape(job)
    effects = [_pegs_effect(job, n, Z, kw, e, i) for i, e in enumerate(j["effects"])]
    lead = Z if Z is not None else effects[0][1]
    Y = PC.traits(lead, j["k"], 0, seed=seed + 70, patterns=[0.1, 0.0, 0.25, 0.05][:j["k"]])
    if j["tag"] in PEGS_MISSING:
        Y[list(PEGS_MISSING[j["tag"]])] = np.nan
    assert len({np.isnan(Y[:, t]).tobytes() for t in range(j["k"])}) == j["k"], job
    Y.setflags(write=False)
    return Y, effects


@functools.lru_cache(maxsize=None)
def _pegsx_data(job):
    j = PEGS_JOBS[job]
    Y, effects = pegs_data(job)
    X = XC.fixed(Y.shape[0], j["f"] - 1, 501)
    Yx = XC.with_fixed(Y, X, 502)
    Yx.setflags(write=False); X.setflags(write=False)
    return Yx, X, effects


@functools.lru_cache(maxsize=None)
def pegs_case(entry, job):
    """the job as a case of tests/pegs_cases.py (PEGS, PEGSZ) or tests/pegsx_cases.py (PEGSX), so that their restate() computes its
    restatement once per process and the guards of tests/test_pegs_cpu.py / tests/test_pegsx_cpu.py run on it as they stand"""
    j = PEGS_JOBS[job]
    assert entry in j["entries"], (entry, job)
    kw = dict(maxit=j["maxit"], logtol=PC.NOSTOP)
    if entry == "PEGSX":
        return dict(id="tall/PEGSX/" + job, job=job, data=lambda: _pegsx_data(job), kw=kw)

    def data():
        Y, effects = pegs_data(job)
        return Y, effects[:1] if entry == "PEGS" else effects
    if entry == "PEGS":
        assert j["effects"][0] == "panel"
    return dict(id="tall/%s/%s" % (entry, job), job=job, entry=entry, data=data, kw=kw)


def gpu_effects(effects, panels):
    """a job's effects as the entries take them: `panels` (one per panel effect, in order) for the panels, dense(Z), sparse(S) in CSC"""
    import bwgr_amd
    panels = list(panels)
    return [panels.pop(0) if e[0] == "panel" else bwgr_amd.dense(e[1]) if e[0] == "dense" else SC.gpu_effects([e])[0] for e in effects]


def pegs_jobs(entry):
    return [job for job, j in PEGS_JOBS.items() if entry in j["entries"]]


def _panel_plan(n, p, block, nwg):
    """K, R, ld of bwgr_debug_panel_plan for an int8 main panel made with these block / nwg arguments"""
    from bwgr_amd import _lib
    out = (C.c_int64 * 25)()
    rc = _lib.lib().bwgr_debug_panel_plan(0, int(n), int(p), int(block), int(nwg), 0, -1, 1, out)
    assert rc == 0, _lib.lib().bwgr_last_error().decode()
    return dict(K=int(out[1]), R=int(out[2]), ld=int(out[3]))


def pegs_plans(job):
    """Everything PEGS_EXPECT speaks of, for one job, from the library's own host arithmetic."""
    import bwgr_amd
    j = PEGS_JOBS[job]
    n, Z, _, kw = _pegs_shape(job)
    k, f = j["k"], j["f"]
    ms = [Z.shape[1] if e == "panel" else e[1] if isinstance(e, tuple) else e for e in j["effects"]]
    pl = dict(n=n, ld128=_ceil(n, 128) * 128)
    if Z is not None:
        pp = _panel_plan(n, Z.shape[1], kw.get("block", 0), kw.get("nwg", 0))
        pl.update(K=pp["K"], R=pp["R"], ld=pp["ld"])
        p = Z.shape[1]
        rc, lp = launch_plan(n, pl["ld"], p, k)
        assert rc == 0
        t = lp["threads"]
        pl["mrr_ey"] = _ceil(pl["ld"], lp["mrr_np"] * t)
        pl["mrr_tilde"] = _ceil(p, lp["mrr_np"] * t)
        pl["mrr_setup"] = _ceil(p, lp["mrr_setup_wg"] * (t // 64))
        pl["last64"] = p - (_ceil(p, 64) - 1) * 64
    else:
        pl["ld"] = pl["ld128"]          # (a dense effect alone pads its rows to 128)
    pl["pad"] = pl["ld"] - n
    m = pl["m"] = max(ms)
    xp = bwgr_amd.pegsx_plan(n, f, k)
    gp = bwgr_amd.pegs_launch_plan(n, m)
    assert gp["fixed_threads"] == xp["threads"] and gp["leg_threads"] == bwgr_amd.pegs_plan(n, 1, k)["threads"]
    assert gp["trace_cols"] == gp["trace_wg"] * 4 * xp["jc"] and gp["setup_cols"] == gp["setup_wg"] * 4
    ngrp = _ceil(m, xp["jc"])
    pl.update(trace_wg=gp["trace_wg"], trace=_ceil(m, gp["trace_cols"]), trace_last=(ngrp - 1) // (gp["trace_wg"] * 4) + 1,
              trace_tail=m - (ngrp - 1) * xp["jc"], dsetup_wg=gp["setup_wg"], dsetup=_ceil(m, gp["setup_cols"]),
              leg_threads=gp["leg_threads"], fixed_threads=gp["fixed_threads"], rows=_ceil(n, gp["fixed_threads"]),
              fixed_cols=_ceil(f, gp["fixed_threads"] // 64), quad=_ceil(f, 64), lds_trace=xp["trace_lds_bytes"], lds_fixed=xp["lds_bytes"])
    Y, effects = pegs_data(job)
    pl["npat"] = len({np.isnan(Y[:, t]).tobytes() for t in range(k)})
    # the sparse effects: the leg each takes under bwgr_debug_pegs_sparse_plan, and k_pegs_sparse_hat's workgroups (a thread per row)
    legs = []
    for e in effects:
        if e[0] == "sparse":
            stored = e[2] if len(e) > 2 else e[1] != 0
            sp = bwgr_amd.pegs_sparse_plan(n, e[1].shape[1], int(stored.sum()), int(stored.sum(0).max()), k, SC.SR.row_disjoint(e[1]))
            legs.append(sp["leg"])
    pl["sparse_legs"] = tuple(legs)
    pl["sparse_hat"] = _ceil(n, 256) if legs else 0
    return pl


# ---- the handle table's PEGS / PEGSZ / PEGSX calls (tests/test_gpu_handles.py), on the 700 x 900 three-slab panel ----
# k = 3 (10 % / 0 / 25 % missing), four sweeps; PEGSZ and PEGSX with a dense effect of five columns behind the panel, PEGSX with f = 3;
# PEGSZ2: the panel's columns split 500 / 400 into two panels; PEGSZ_S and PEGSX_S (f = 3): [panel, a sparse incidence of 12 levels, a sparse
# overlapping design of 25 columns], whose legs MtFit::sweep_effect launches between host-to-device copies of the order and of iG.
# tests/test_tall_cases_cpu.py runs the branch guards on them too.
HANDLE_ENTRIES = ("PEGS", "PEGSZ", "PEGSX", "PEGSZ2", "PEGSZ_S", "PEGSX_S")


@functools.lru_cache(maxsize=None)
def _handle_data(entry):
    Z = XC.slabs900()
    n = Z.shape[0]
    Y = PC.traits(Z, 3, 0, seed=5, patterns=[0.1, 0.0, 0.25])
    D = PC.gauss(n, 5, 504)
    kw = dict(nwg=3)
    if entry == "PEGSZ2":
        effects = [("panel", np.asfortranarray(Z[:, :500]), kw), ("panel", np.asfortranarray(Z[:, 500:]), kw)]
    elif entry in ("PEGSZ_S", "PEGSX_S"):
        effects = [("panel", Z, kw), ("sparse", SC.incidence(n, 12, 506)), ("sparse",) + SC.overlapping(n, 25, 507)]
    else:
        effects = [("panel", Z, kw)] + ([] if entry == "PEGS" else [("dense", D)])
    if not entry.startswith("PEGSX"):
        Y.setflags(write=False)
        return Y, effects
    X = XC.fixed(n, 2, 501)
    Yx = XC.with_fixed(Y, X, 502)
    Yx.setflags(write=False); X.setflags(write=False)
    return Yx, X, effects


@functools.lru_cache(maxsize=None)
def handle_case(entry):
    kw = dict(maxit=4, logtol=PC.NOSTOP)
    if entry.startswith("PEGSX"):
        return dict(id="handles/" + entry, data=lambda: _handle_data(entry), kw=kw)
    return dict(id="handles/" + entry, entry="PEGS" if entry == "PEGS" else "PEGSZ", data=lambda: _handle_data(entry), kw=kw)
