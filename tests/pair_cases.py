"""The two-panel shapes of tests/test_gpu_pairs.py (crossprod2, Panel.kernel2, EigenArcZ / EigenGauZ), in the style of tests/tall_cases.py and
kept in one place so that tests/test_pair_cases_cpu.py can check, without a GPU, that every shape and orientation still reaches the code it
is listed for under the library's own host arithmetic: bwgr_debug_panel_plan (both panels' K, R, ld), bwgr_debug_xyt_plan (T_r, T_c, tiles,
chunks), bwgr_debug_xxt_plan (K_ff's own, symmetric product) and bwgr_debug_launch_plan (the grids of k_kfin2_apply and k_xxt_zero).

A pair is (founders, samples); "swapped" is the same two panels the other way round.  The trips, from the plans (256 threads per workgroup):
  apply_ff  ceil(n_f^2 / (kfin_apply_wg x 256)): k_kfin2_apply over K_ff
  apply_fs  ceil(n_f n_s / (kfin_apply_wg x 256)): k_kfin2_apply over K_fs
  zero_fs   ceil(n_f n_s / (xxt_zero_wg x 256)): k_xxt_zero(upper = 0) over the rectangular product, launched only when a tile has several
            workgroups; no plan splits a chunk of 300 markers, so pair1100 reaches it with three forced chunks (kchunk: BWGR_KCHUNK when the
            founders' panel is made; forced_chunks as bwgr_debug_xyt_plan then reports them), which integer sums make bit-equal
  sumd      ceil(n_f^2 / (1 024 x 256)): k_kfin_sumd_stage1 under GAU (XXT_SUMD_PARTS workgroups, not reported by a hook)
  rows_s    (row workgroups, slabs) of k_kfin2_rowsq and of k_kfin_xs over the samples: ld_s / 128 workgroups of 128 rows in K_s slabs
"""
import ctypes as C
import functools

import numpy as np

from conftest import synth_small
import driver_cases as dc
import tall_cases as tc

P = 300
# tag -> the two panels: "tall" names a shape of tests/tall_cases.py (its genotypes, its block), the other is n x 300 from its own seed
CASES = {
    "pair1100": dict(a=dict(tall="kern1100"), b=dict(n=1000, block=0, seed=2914)),
    "pair1024": dict(a=dict(tall="slab1024"), b=dict(n=700, block=0, seed=2913)),
}
ORIENTATIONS = [(tag, swapped) for tag in CASES for swapped in (False, True)]

# What each orientation is there for, as the plans must report it.  f, s: (n, K, R, ld) of the founders and of the samples.
EXPECT = {
    ("pair1100", False): dict(f=(1100, 5, 256, 1280), s=(1000, 4, 256, 1024), Tr=9, Tc=8, tiles=72, apply_ff=2, apply_fs=2, sumd=5, rows_s=(8, 4),
                              accumulate=False, kchunk=100, forced_chunks=3, zero_fs=3),
    ("pair1100", True):  dict(f=(1000, 4, 256, 1024), s=(1100, 5, 256, 1280), Tr=8, Tc=9, tiles=72, apply_ff=1, apply_fs=2, sumd=4, rows_s=(10, 5),
                              accumulate=False, kchunk=100, forced_chunks=3, zero_fs=3),
    ("pair1024", False): dict(f=(2000, 2, 1024, 2048), s=(700, 3, 256, 768), Tr=16, Tc=6, tiles=96, apply_ff=4, apply_fs=2, sumd=16, rows_s=(6, 3),
                              accumulate=False),
    ("pair1024", True):  dict(f=(700, 3, 256, 768), s=(2000, 2, 1024, 2048), Tr=6, Tc=16, tiles=96, apply_ff=1, apply_fs=2, sumd=2, rows_s=(16, 2),
                              accumulate=False),
}
XYT_FIELDS = ("chunk", "nchunks", "tiles", "wgs", "ws_bytes", "Tr", "Tc", "sub", "piece")
SUMD_PARTS = 1024      # XXT_SUMD_PARTS of kernels_host.hip.h: the fixed grid of k_kfin_sumd_stage1


def xyt_plan(nf, ns, p, kchunk=0, xmax=2):
    from bwgr_amd import _lib
    out = (C.c_int64 * len(XYT_FIELDS))()
    rc = _lib.lib().bwgr_debug_xyt_plan(int(nf), int(ns), int(p), int(xmax), int(xmax), int(kchunk), out)
    assert rc == 0, _lib.lib().bwgr_last_error().decode()
    return dict(zip(XYT_FIELDS, (int(v) for v in out)))


def _shape(side):
    if "tall" in side:
        c = tc.CASES[side["tall"]]
        assert c["p"] == P
        return c["n"], c["block"]
    return side["n"], side["block"]


def sides(tag, swapped=False):
    """(founders, samples): the two entries of CASES[tag] in this orientation"""
    c = CASES[tag]
    return (c["b"], c["a"]) if swapped else (c["a"], c["b"])


def panel_kw(side):
    block = _shape(side)[1]
    return {"block": block} if block else {}


@functools.lru_cache(maxsize=None)
def _data(tag, which):
    side = CASES[tag][which]
    if "tall" in side:
        return tc.data(side["tall"])
    X = np.asfortranarray(synth_small(side["n"], P, seed=side["seed"])[0])
    X.setflags(write=False)
    return X


def data(tag, swapped=False):
    """(X_f, X_s): int8, codes 0 / 1 / 2, column-major, read-only"""
    a, b = _data(tag, "a"), _data(tag, "b")
    return (b, a) if swapped else (a, b)


def _ceil(a, b):
    return -(-a // b)


def plans(tag, swapped=False):
    """Everything EXPECT speaks of, for one orientation of one pair."""
    f, s = sides(tag, swapped)
    (nf, bf), (ns, bs) = _shape(f), _shape(s)
    pf, ps = dc.panel_plan(0, nf, P, bf), dc.panel_plan(0, ns, P, bs)
    rc, lp = tc.launch_plan(nf, pf["ld"], P, 1)
    assert rc == 0
    per_apply, per_zero = lp["kfin_apply_wg"] * lp["threads"], lp["xxt_zero_wg"] * lp["threads"]
    pl = dict(f=(nf, pf["K"], pf["R"], pf["ld"]), s=(ns, ps["K"], ps["R"], ps["ld"]))
    xp = xyt_plan(nf, ns, P)
    sym = tc.xxt_plan(nf, P)
    pl.update(Tr=xp["Tr"], Tc=xp["Tc"], tiles=xp["tiles"], accumulate=xp["nchunks"] * xp["sub"] > 1 or sym["nchunks"] * sym["sub"] > 1)
    pl["apply_ff"], pl["apply_fs"] = _ceil(nf * nf, per_apply), _ceil(nf * ns, per_apply)
    pl["sumd"] = _ceil(nf * nf, SUMD_PARTS * lp["threads"])
    pl["rows_s"] = (ps["ld"] // 128, ps["K"])
    pl["kchunk"] = EXPECT[(tag, swapped)].get("kchunk", 0)
    fp = xyt_plan(nf, ns, P, kchunk=pl["kchunk"])
    pl["forced_chunks"] = fp["nchunks"] if pl["kchunk"] else 0
    pl["zero_fs"] = _ceil(nf * ns, per_zero) if pl["kchunk"] and fp["nchunks"] * fp["sub"] > 1 else 0      # (0: not launched)
    return pl
