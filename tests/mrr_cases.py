"""The (k, npat) cases of the mrr GPU parity tests (tests/test_gpu_mrr.py), kept in one place so that tests/test_mrr_cpu.py can check,
under the library's LDS plan (bwgr_debug_mrr_plan), that they still reach every layout k_mrr_solve has.

k_mrr_solve keeps the markers' k x k inverses (Linv) in LDS when they fit, then stages ngl of the block's npat per-pattern Gram matrices
in LDS and reads the rest from global memory.  Its five regimes:
  1  Linv in LDS,   ngl = npat
  2  Linv in LDS,   0 < ngl < npat
  3  Linv in LDS,   ngl = 0
  4  Linv global,   ngl = npat
  5  Linv global,   ngl < npat
"""
import ctypes as C

# k sweep on synth_small(700, 900) with nwg=3 (three slabs, a last block of 4 markers): (k, npat)
K_SWEEP = [
    (6, 6),     # at the cap, every Gram in LDS
    (7, 7),     # two patterns from global
    (9, 9),     # pass lanes t >= 8; Gram grid.y = 3
    (13, 13),   # lanes t = 12; grid.y = 4
    (15, 15),   # ngl = 0: every Gram from global
    (15, 1),    # ngl = 0 with one shared pattern
    (16, 16),   # Linv from global; nine patterns from global
    (16, 5),    # Linv from global; every Gram in LDS
]
# traits sharing missingness patterns: the pattern id of each trait, numbered in order of first appearance (as the host numbers them)
SHARED = [
    [0, 1, 0, 2, 1, 0, 2, 2],
    [0, 1, 0, 2, 1, 3, 3, 0, 4, 5, 6, 7, 8, 4, 9, 0],   # npat = 10 > ngl
]
EDGE_P = [1, 63, 64, 65]   # marker counts: a single marker, one partial block, exactly one block, a last block of one marker
EDGE_K = [3, 16]
OPTIONS_K = 12             # the options run where ngl < npat


def plan(k, npat):
    """(status, linv_lds, ngl, solve LDS bytes, k_mrr_linv LDS bytes) of bwgr_debug_mrr_plan (host arithmetic, no GPU)."""
    from bwgr_amd import _lib
    linv, ngl, sb, lb = C.c_int(-1), C.c_int(-1), C.c_int64(-1), C.c_int64(-1)
    rc = _lib.lib().bwgr_debug_mrr_plan(int(k), int(npat), C.byref(linv), C.byref(ngl), C.byref(sb), C.byref(lb))
    return rc, linv.value, ngl.value, sb.value, lb.value


def regime(linv_lds, ngl, npat):
    if linv_lds:
        return 3 if ngl == 0 else (1 if ngl == npat else 2)
    return 4 if ngl == npat else 5
