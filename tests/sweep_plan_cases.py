"""The sweeps whose plans tests/golden/sweep_plan_parent.txt records (tools/sweep_plan_table.py writes the table, tests/
test_sweep_plan_cpu.py compares against it): plan_sweep through bwgr_debug_sweep_plan, host arithmetic that needs no GPU.  Every shape is
the smallest at which its branch is taken; the two at the 32-bit edge of the DMA streamers' offsets are large, which costs nothing here.

A case is (shape, flags, mode, state, switch); key() names it, plan() asks the library.  table() runs them all: {key: FIELDS-tuple, or
None where the library refuses the combination}."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bwgr_amd.api import SWEEP_PLAN_FIELDS as FIELDS   # noqa: E402  (the hook's fields, in order: include/bwgr.h)

MAIN, ROWS, EM = 0, 1, 2
# the sweep's flags (csrc/sweep.hip.h)
SELECT, MH, VB_VEC, EM_SEL, SERIAL, CENTRE = 1, 4, 16, 128, 1 << 19, 1 << 21
ALONE, REDO, PAIR = 0, 1, 2
# the handle's state bits
CLONES, IS_CLONE, CROWDED, WITHHELD = 1, 2, 4, 8

# the instantiations plan_sweep can name, by the hook's number
KERNELS = ("k_sweep<int8_t, true>", "k_sweep<int8_t, false>", "k_sweep<float, true>", "k_sweep<float, false>", "k_sweep2<int8_t, true>",
           "k_sweep2<int8_t, false>", "k_sweep2<int8_t, true, uint16_t>", "k_sweep2<float, true>", "k_sweep2<float, false>", "k_sweep2w<true>",
           "k_sweep2w<false>", "k_sweep3<uint16_t, false>", "k_sweep3<int32_t, false>", "k_sweep3<uint16_t, true>", "k_sweep3<int32_t, true>",
           "k_sweep3p<uint16_t>", "k_sweep3p<int32_t>", "k_sweep3f")
K_SWEEP3P = (15, 16)
DMA4, DMA3 = 1 << 22, 1 << 23      # dbg3's two DMA streamer bits (S3_DMA4 / S3_DMA3 of csrc/sweep3.hip.h)

# name -> (is_f32, n, p, block, nwg, kind, xmax, gram16, blk_begin, blk_end)
SHAPES = {
    "i8 300x1000 nwg3 b64": (0, 300, 1000, 64, 3, MAIN, 2, 1, 0, 0),             # the digest tool's panel: R = 128
    "i8 300x1000 nwg3 b64 blocks 2..9": (0, 300, 1000, 64, 3, MAIN, 2, 1, 2, 9),
    "i8 300x1000 nwg3 b64 gram32": (0, 300, 1000, 64, 3, MAIN, 100, 0, 0, 0),    # the 16-bit copies are not exact: 32-bit staging
    "i8 512x2048": (0, 512, 2048, 0, 0, MAIN, 2, 1, 0, 0),                       # the default geometry, 128-marker blocks: k_sweep3f's shape, R % 256 == 0
    "i8 33280x256 nwg130": (0, 33280, 256, 0, 130, MAIN, 2, 1, 0, 0),            # 2 * K3 + 1 > 256: no solo streamers
    "f32 200x300": (1, 200, 300, 0, 0, MAIN, 0, 0, 0, 0),
    "i8 150x1000 b64 rows": (0, 150, 1000, 64, 0, ROWS, 2, 1, 0, 0),
    "i8 300x1000 nwg3 b64 em": (0, 300, 1000, 64, 3, EM, 2, 1, 0, 0),
    "i8 512x16777215 nwg2": (0, 512, (1 << 24) - 1, 0, 2, MAIN, 2, 1, 0, 0),     # p * R = 2^32 - 256: the DMA streamers' 32-bit offsets reach
    "i8 512x16777216 nwg2": (0, 512, 1 << 24, 0, 2, MAIN, 2, 1, 0, 0),           # p * R = 2^32: they do not
}
FLAGS = {"affine": 0, "select": SELECT, "select centre": SELECT | CENTRE, "select vb": SELECT | VB_VEC, "select mh": SELECT | MH, "em": EM_SEL, "serial": SERIAL}
MODES = {"alone": ALONE, "redo": REDO, "pair": PAIR}
STATES = {"alone": 0, "clones": CLONES, "clone": CLONES | IS_CLONE, "crowded": CROWDED, "withheld": WITHHELD}
SWITCHES = [None, ("BWGR_SWEEP", "1"), ("BWGR_SWEEP", "2"), ("BWGR_LAG", "2"), ("BWGR_LAG", "3"), ("BWGR_LAG", "4"), ("BWGR_STREAM3", "reg"),
            ("BWGR_WINV", "0"), ("BWGR_WFX", "0"), ("BWGR_ENG3_THR", "1"), ("BWGR_SOLO3", "0"), ("BWGR_PF3", "0"), ("BWGR_PF3", "1"), ("BWGR_FIXED3", "0"),
            ("BWGR_R3", "128")]
# every switch the plans read: unset around each call, but for the case's own
ALL_SWITCHES = ("BWGR_SWEEP", "BWGR_LAG", "BWGR_SOLO3", "BWGR_STREAM3", "BWGR_PF3", "BWGR_R3", "BWGR_D3", "BWGR_NFEED", "BWGR_ENG3_THR", "BWGR_PF3B",
                "BWGR_DRAWS", "BWGR_GRAM16", "BWGR_FIXED3", "BWGR_WINV", "BWGR_WFX", "BWGR_WPF", "BWGR_WAHEAD", "BWGR_WNQ", "BWGR_WLAG", "BWGR_DEBUG_SH_ADD",
                "BWGR_DBG3", "BWGR_NO_RECOVER", "BWGR_WLAG_TIMING")


def cases():
    """Every shape and flag set under every mode and handle state with no switch set; under every switch, alone and as a pair on a handle alone."""
    for shape in SHAPES:
        for flags in FLAGS:
            for mode in MODES:
                for state in STATES:
                    yield shape, flags, mode, state, None
            for sw in SWITCHES[1:]:
                for mode in ("alone", "pair"):
                    yield shape, flags, mode, "alone", sw


def key(shape, flags, mode, state, sw):
    return " | ".join((shape, flags, mode, state, "%s=%s" % sw if sw else "-"))


def plan(shape, flags, mode, state, sw):
    """The hook's fields for one case, or None where the library refuses it (BWGR_EINVAL)."""
    import bwgr_amd
    f32, n, p, block, nwg, kind, xmax, gram16, b0, b1 = SHAPES[shape]
    saved = {k: os.environ.pop(k) for k in ALL_SWITCHES if k in os.environ}
    if sw:
        os.environ[sw[0]] = sw[1]
    try:
        pl = bwgr_amd.sweep_plan(f32, n, p, block, nwg, kind, xmax, gram16, FLAGS[flags], b0, b1, MODES[mode], STATES[state])
    except bwgr_amd.BwgrError as e:
        assert e.code == 1, e          # BWGR_EINVAL
        return None
    finally:
        if sw:
            del os.environ[sw[0]]
        os.environ.update(saved)
    return tuple(pl[f] for f in FIELDS)


def table():
    return {key(*c): plan(*c) for c in cases()}


def _groups():
    """the cases in order, by line of the table: (shape | flags | which, [case])"""
    out = {}
    for c in cases():
        out.setdefault(" | ".join((c[0], c[1], "modes x states" if c[4] is None else "switches x alone, pair")), []).append(c)
    return out


def write_table(path, tab, commit):
    """The distinct plans once, numbered in order of first use; then one line per shape, flag set and half of cases(): its cases' plan numbers."""
    plans = list(dict.fromkeys(v for v in tab.values() if v is not None))
    with open(path, "w") as f:
        f.write("# every field of bwgr_debug_sweep_plan (tests/sweep_plan_cases.py: FIELDS) for its cases, recorded with tools/sweep_plan_table.py from "
                "plan_sweep as it stood at commit %s\n" % commit)
        f.write("# `P<k>  <fields>`: the distinct plans; `<shape> | <flags> | <which>  <k or -, one per case in the order of cases()>`: -: refused, "
                "the combination is not one the library plans\n")
        for k, v in enumerate(plans):
            f.write("P%d  %s\n" % (k, " ".join(str(x) for x in v)))
        for g, cs in _groups().items():
            f.write("%s  %s\n" % (g, " ".join("-" if tab[key(*c)] is None else str(plans.index(tab[key(*c)])) for c in cs)))


def read_table(path):
    """{key: FIELDS-tuple or None} in the order of the table's lines"""
    plans, out, groups = {}, {}, _groups()
    with open(path) as f:
        for line in f:
            if not line.strip() or line.startswith("#"):
                continue
            k, v = line.rstrip("\n").split("  ", 1)
            if k not in groups:
                assert k == "P%d" % len(plans), k
                plans[len(plans)] = tuple(int(x) for x in v.split())
                continue
            assert len(v.split()) == len(groups[k]), k
            for c, tok in zip(groups[k], v.split()):
                out[key(*c)] = None if tok == "-" else plans[int(tok)]
    return out
