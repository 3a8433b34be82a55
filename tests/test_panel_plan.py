"""What a panel is -- block and slab geometry, engines, Gram arrays -- as plan_panel / plan_panel3 decide it (bwgr_debug_panel_plan: host
arithmetic, no GPU).

The expected geometry is the previous implementation's, tabulated on the CPU from its own panel_alloc / sweep3_build arithmetic and the
kernels' LDS-size functions before the decision was gathered into plan_panel; none of it was taken from plan_panel's output.  Which arrays a
panel carries restates that implementation's allocation conditions: distance-2 cross blocks on a pipelined panel of more than two blocks,
distance-3 ones on an int8 panel of more than three whose geometry fits the lag-4 streamer (unless BWGR_LAG=2|3), 16-bit copies on every
pipelined int8 panel, byte planes for the affine engine as far as those arrays reach and -- main panels only -- to distance BWGR_WLAG - 1;
bwgr_em's scratch panel stops at distance 1 without 16-bit copies, and only a main panel attempts k_sweep3."""
import ctypes as C

import pytest

from bwgr_amd import _lib

FIELDS = ("m", "K", "R", "ld", "nblocks", "pstride", "nfeed", "lag4_ok", "lds", "lds2", "ldsw", "x_bytes", "gram_bytes", "pipelined",
          "xdist", "has16", "wdist", "try3", "fits3", "R3", "sub3", "K3", "D", "lds3", "solo3")
MAIN, ROWS, EM = 0, 1, 2
EINVAL = 1
SWITCHES = ("BWGR_SWEEP", "BWGR_LAG", "BWGR_NFEED", "BWGR_WINV", "BWGR_WLAG", "BWGR_R3", "BWGR_D3", "BWGR_SOLO3")


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def plan(f32, n, p, block=0, nwg=0, kind=MAIN, xmax=-1, gram16=1):
    """(status, {field: value}, message)"""
    out = (C.c_int64 * len(FIELDS))()
    L = _lib.lib()
    rc = L.bwgr_debug_panel_plan(int(f32), int(n), int(p), int(block), int(nwg), int(kind), int(xmax), int(gram16), out)
    return rc, dict(zip(FIELDS, (int(v) for v in out))), L.bwgr_last_error().decode()


def test_hook_writes_every_field():
    assert _lib.lib().bwgr_debug_panel_plan.argtypes[-1] == C.POINTER(C.c_int64)
    rc, pl, _ = plan(0, 10000, 1000000)
    assert rc == 0 and len(pl) == 25


# (f32, n, p, block, nwg) -> m, K, R, nblocks, pipelined, nfeed, lag4_ok, lds2
GEOMETRY = [
    ((0, 10000, 1000000, 0, 0), (128, 40, 256, 7813, 1, 2, 1, 162368)),    # c4
    ((0, 10000, 500000, 0, 0), (128, 40, 256, 3907, 1, 2, 1, 162368)),     # c3
    ((0, 5000, 50000, 0, 0), (128, 20, 256, 391, 1, 2, 1, 162368)),        # c2
    ((0, 50000, 1000000, 0, 0), (128, 196, 256, 7813, 1, 6, 1, 162368)),   # c5
    ((0, 196, 376, 0, 0), (128, 1, 256, 3, 1, 2, 1, 162368)),              # the suites' small shapes
    ((0, 196, 376, 16, 1), (16, 1, 256, 24, 1, 2, 1, 42528)),
    ((0, 196, 376, 64, 1), (64, 1, 256, 6, 1, 2, 1, 90688)),
    ((0, 900, 700, 64, 4), (64, 4, 256, 11, 1, 2, 1, 90688)),
    ((0, 700, 1400, 128, 3), (128, 3, 256, 11, 1, 2, 1, 162368)),
    ((0, 130, 9, 16, 0), (16, 1, 256, 1, 1, 2, 1, 42528)),
    ((0, 20000, 640, 0, 0), (128, 79, 256, 5, 1, 3, 1, 162368)),
    ((0, 50000, 384, 0, 0), (128, 196, 256, 3, 1, 6, 1, 162368)),
    # the largest slab the pipelined engine fits is preferred over the first engine's larger one
    ((0, 2000, 300, 16, 0), (16, 2, 1024, 19, 1, 2, 1, 142912)),
    # ... unless the caller fixes the slab count: the first-generation engine, for want of LDS
    ((0, 2000, 300, 16, 1), (16, 1, 2048, 19, 0, 2, 0, 249152)),
    ((0, 1000, 300, 32, 1), (32, 1, 1024, 10, 0, 2, 0, 176192)),
    ((0, 1000, 300, 16, 1), (16, 1, 1024, 19, 1, 2, 1, 142912)),
    ((0, 600, 300, 32, 1), (32, 1, 640, 10, 1, 2, 1, 132672)),
    ((0, 500, 300, 64, 1), (64, 1, 512, 5, 1, 2, 0, 140864)),
    ((0, 300, 200, 64, 1), (64, 1, 384, 4, 1, 2, 1, 132672)),
    # ... or for want of workgroups: K + 1 + nfeed <= 256
    ((0, 63744, 300, 0, 0), (128, 249, 256, 3, 1, 6, 1, 162368)),
    ((0, 64000, 300, 0, 0), (128, 250, 256, 3, 0, 6, 1, 162368)),
    ((0, 65000, 300, 0, 0), (128, 254, 256, 3, 0, 6, 1, 162368)),
    ((0, 65536, 300, 0, 256), (128, 256, 256, 3, 0, 6, 1, 162368)),
    # float panels
    ((1, 500, 300, 0, 0), (64, 4, 128, 5, 1, 2, 0, 111680)),
    ((1, 10000, 2000, 0, 0), (64, 79, 128, 32, 1, 3, 0, 111680)),
    ((1, 250, 300, 16, 1), (16, 1, 256, 19, 1, 2, 0, 61248)),
    ((1, 32000, 300, 0, 0), (64, 250, 128, 5, 0, 6, 0, 111680)),
    ((1, 32768, 300, 0, 0), (64, 256, 128, 5, 0, 6, 0, 111680)),
]


@pytest.mark.parametrize("shape,want", GEOMETRY, ids=lambda v: "-".join(map(str, v)) if len(v) == 5 else "")
def test_geometry(shape, want):
    f32, n, p, block, nwg = shape
    rc, pl, msg = plan(f32, n, p, block, nwg)
    assert rc == 0, msg
    got = tuple(pl[k] for k in ("m", "K", "R", "nblocks", "pipelined", "nfeed", "lag4_ok", "lds2"))
    print(shape, got)
    assert got == want
    m, esz = pl["m"], 4 if f32 else 1
    assert pl["ld"] == pl["K"] * pl["R"] and pl["ld"] >= n
    assert pl["pstride"] == (m * (m - 1) // 2 + 7) // 8 * 8
    assert pl["x_bytes"] == pl["ld"] * p * esz and pl["gram_bytes"] == pl["nblocks"] * m * m * (8 if f32 else 4)
    assert pl["lds"] <= 160 * 1024                                       # the slab limit is the first engine's LDS
    assert (pl["ldsw"] > 0) == (not f32)


def test_sweep_1_forces_the_first_engine(monkeypatch):
    monkeypatch.setenv("BWGR_SWEEP", "1")
    rc, pl, _ = plan(0, 10000, 1000000)
    assert rc == 0
    assert [pl[k] for k in ("m", "K", "R", "nblocks", "pipelined", "nfeed", "lag4_ok", "lds2")] == [128, 40, 256, 7813, 0, 2, 1, 162368]
    assert [pl[k] for k in ("xdist", "has16", "wdist", "try3")] == [1, 0, 0, 0]
    # and takes the first engine's own largest slab where the pipelined one would have taken a smaller
    rc, pl, _ = plan(0, 2000, 300, 16, 0)
    assert rc == 0 and (pl["K"], pl["R"], pl["pipelined"]) == (1, 2048, 0)


def test_nfeed_switch(monkeypatch):
    monkeypatch.setenv("BWGR_NFEED", "4")
    assert plan(0, 10000, 1000000)[1]["nfeed"] == 4
    monkeypatch.setenv("BWGR_NFEED", "7")   # out of range: ignored
    assert plan(0, 10000, 1000000)[1]["nfeed"] == 2


REFUSALS = [
    ((0, 70000, 384, 0, 0), "panel_create: n=70000 needs 274 slab workgroups of 256 rows (limits: 256 workgroups, 256 rows)"),
    ((0, 100000, 384, 0, 0), "panel_create: n=100000 needs 391 slab workgroups of 256 rows (limits: 256 workgroups, 256 rows)"),
    ((0, 5000, 300, 0, 1), "panel_create: n=5000 needs 1 slab workgroups of 5120 rows (limits: 256 workgroups, 256 rows)"),
    ((0, 2000, 300, 0, 1), "panel_create: n=2000 needs 1 slab workgroups of 2048 rows (limits: 256 workgroups, 256 rows)"),
    ((0, 3000, 300, 32, 1), "panel_create: n=3000 needs 1 slab workgroups of 3072 rows (limits: 256 workgroups, 1024 rows)"),
    ((0, 4096, 300, 16, 1), "panel_create: n=4096 needs 1 slab workgroups of 4096 rows (limits: 256 workgroups, 2176 rows)"),
    ((1, 3000, 300, 32, 1), "panel_create: n=3000 needs 1 slab workgroups of 3072 rows (limits: 256 workgroups, 256 rows)"),
    ((1, 1000, 300, 16, 1), "panel_create: n=1000 needs 1 slab workgroups of 1024 rows (limits: 256 workgroups, 512 rows)"),
    ((1, 10000, 2000, 128, 0), "panel_create: block 128 > 64 (limit for this genotype type)"),
    ((0, 1000, 300, 200, 0), "panel_create: block 200 > 128 (limit for this genotype type)"),
    ((0, 1, 5, 0, 0), "panel: need n >= 2, p >= 1 (n=1 p=5)"),
    ((0, 5, 0, 0, 0), "panel: need n >= 2, p >= 1 (n=5 p=0)"),
    ((0, 0x7FFFFF01, 5, 0, 0), "panel: n and p must fit 31 bits"),
    ((0, 200, 0x7FFFFF00, 16, 0), "panel_create: 134217712 marker blocks; the delta granules carry a 24-bit block epoch"),
    # in the order they are checked: the range before the block, the block before the slabs
    ((1, 1, 5, 128, 0), "panel: need n >= 2, p >= 1 (n=1 p=5)"),
    ((0, 70000, 384, 200, 0), "panel_create: block 200 > 128 (limit for this genotype type)"),
]


@pytest.mark.parametrize("shape,message", REFUSALS, ids=lambda v: "-".join(map(str, v)) if len(v) == 5 else "")
def test_refusals(shape, message):
    for kind in (MAIN, ROWS, EM):
        rc, _, msg = plan(*shape, kind=kind)
        assert rc == EINVAL and msg == message, (kind, rc, msg)


def test_bad_kind_is_refused():
    assert plan(0, 500, 300, kind=3)[0] == EINVAL and plan(0, 500, 300, kind=-1)[0] == EINVAL


def carried(*a, **k):
    rc, pl, msg = plan(*a, **k)
    assert rc == 0, msg
    return tuple(pl[f] for f in ("xdist", "has16", "wdist", "try3"))


def test_what_a_main_panel_carries(monkeypatch):
    assert carried(0, 10000, 1000000) == (3, 1, 3, 1)           # c4: distances 1-3, 16-bit copies, planes to BWGR_WLAG's default 4 - 1, k_sweep3
    assert carried(0, 196, 376) == (2, 1, 2, 1)                 # three blocks: nothing at distance 3
    assert carried(0, 700, 300, 128, 3) == (2, 1, 2, 1)
    assert carried(0, 700, 256, 128, 3) == (1, 1, 1, 1)         # two blocks
    assert carried(0, 130, 9, 16, 0) == (1, 1, 0, 1)            # one block: the distance-1 array is allocated, never filled; no planes
    assert carried(0, 500, 300, 64, 1) == (2, 1, 2, 1)          # five blocks, but the lag-4 streamer does not fit: no distance 3
    assert carried(1, 500, 300) == (2, 0, 0, 0)                 # float: fp64 cross blocks to distance 2, nothing else
    assert carried(0, 64000, 300) == (1, 0, 0, 0)               # the first engine: distance 1 only
    assert carried(0, 2000, 300, 16, 1) == (1, 0, 0, 0)
    for lag in "23":
        monkeypatch.setenv("BWGR_LAG", lag)
        assert carried(0, 10000, 1000000) == (2, 1, 2, 1)
    monkeypatch.setenv("BWGR_LAG", "4")
    assert carried(0, 10000, 1000000) == (3, 1, 3, 1)
    monkeypatch.delenv("BWGR_LAG")
    monkeypatch.setenv("BWGR_SWEEP", "2")                       # keeps k_sweep2: no k_sweep3, everything else as before
    assert carried(0, 10000, 1000000) == (3, 1, 3, 0)
    monkeypatch.delenv("BWGR_SWEEP")
    monkeypatch.setenv("BWGR_WINV", "0")                        # no affine product sequencer: no planes
    assert carried(0, 10000, 1000000) == (3, 1, 0, 1)


def test_far_byte_planes_follow_wlag_on_main_panels_only(monkeypatch):
    for wlag, far in (("2", 3), ("3", 3), ("4", 3), ("5", 4), ("6", 5), ("7", 3)):   # (near distances are built whatever the cap; 7: ignored)
        monkeypatch.setenv("BWGR_WLAG", wlag)
        assert carried(0, 10000, 1000000) == (3, 1, far, 1), wlag
        assert carried(0, 5000, 10000, nwg=0, kind=ROWS) == (3, 1, 3, 0), wlag
    monkeypatch.setenv("BWGR_WLAG", "6")
    assert carried(0, 20000, 640) == (3, 1, 4, 1)               # five blocks: distance 4 is the farthest there is
    assert carried(0, 196, 376) == (2, 1, 2, 1)
    monkeypatch.setenv("BWGR_LAG", "3")                         # no distance-3 array: the planes stop with the arrays
    assert carried(0, 10000, 1000000) == (2, 1, 2, 1)


@pytest.mark.parametrize("shape", [(0, 10000, 1000000, 0, 0), (0, 5000, 50000, 128, 0), (0, 196, 376, 16, 1), (0, 900, 700, 64, 4),
                                   (0, 20000, 640, 0, 0), (1, 500, 300, 0, 0), (0, 2000, 300, 16, 1), (0, 130, 9, 16, 0)])
def test_scratch_kinds(shape, monkeypatch):
    """The row-subset panel carries what a main panel carries except k_sweep3 and the distance-4 / 5 planes; the EM scratch panel carries
    distance 1 only and no 16-bit copies; the geometry does not depend on the kind."""
    monkeypatch.setenv("BWGR_WLAG", "6")
    rc, main, _ = plan(*shape, kind=MAIN)
    rc1, rows, _ = plan(*shape, kind=ROWS)
    rc2, em, _ = plan(*shape, kind=EM)
    assert rc == rc1 == rc2 == 0
    geometry = FIELDS[:14]
    assert [rows[k] for k in geometry] == [main[k] for k in geometry] == [em[k] for k in geometry]
    assert (rows["xdist"], rows["has16"]) == (main["xdist"], main["has16"])
    assert rows["wdist"] == min(main["wdist"], 3) and rows["try3"] == 0
    assert (em["xdist"], em["has16"], em["wdist"], em["try3"]) == (1, 0, 0, 0)
    for kind in (ROWS, EM):   # no k_sweep3 whatever the data says
        q = plan(*shape, kind=kind, xmax=2, gram16=1)[1]
        assert q["fits3"] == 0 and q["solo3"] == 1


# (n, p, block, nwg, xmax, gram16, BWGR_D3, BWGR_R3) -> fits, R3, sub3, K3, D, lds3, solo3
SWEEP3 = [
    ((10000, 1000000, 0, 0, 2, 1, 0, 0), (1, 256, 1, 40, 12, 159488, 1)),     # c4
    ((10000, 1000000, 0, 0, 2, 0, 0, 0), (1, 256, 1, 40, 12, 138304, 1)),     # ... on 32-bit Gram entries
    ((10000, 1000000, 0, 0, 127, 1, 0, 0), (1, 256, 1, 40, 12, 159488, 1)),
    ((50000, 1000000, 0, 0, 2, 1, 0, 0), (1, 256, 1, 196, 12, 159488, 1)),    # c5
    ((50000, 1000000, 0, 0, 127, 1, 0, 0), (1, 256, 1, 196, 12, 159488, 1)),
    ((5000, 50000, 0, 0, 2, 1, 0, 0), (1, 256, 1, 20, 12, 159488, 1)),        # c2
    ((196, 376, 0, 0, 2, 1, 0, 0), (1, 256, 1, 1, 3, 159488, 1)),             # tpod's three blocks
    ((196, 376, 16, 1, 2, 1, 0, 0), (1, 256, 1, 1, 12, 159488, 1)),
    ((700, 1400, 128, 3, 2, 1, 5, 0), (1, 256, 1, 3, 5, 159488, 1)),
    ((700, 1400, 128, 3, 2, 1, 16, 0), (1, 256, 1, 3, 11, 159488, 1)),        # eleven blocks
    ((700, 1400, 128, 3, 2, 1, 0, 64), (1, 64, 4, 12, 11, 159488, 0)),        # an explicit height: no solo streamers
    ((700, 1400, 128, 3, 2, 0, 3, 128), (1, 128, 2, 6, 3, 118528, 0)),
    ((600, 300, 32, 1, 2, 1, 0, 0), (1, 128, 5, 5, 10, 159488, 1)),           # 640-row slabs: 128-row streamers
    ((1000, 300, 16, 1, 2, 1, 0, 0), (1, 256, 4, 4, 12, 159488, 1)),
    ((300, 200, 64, 1, 2, 1, 0, 0), (1, 128, 3, 3, 4, 159488, 1)),
    ((63744, 300, 0, 0, 2, 1, 0, 0), (1, 256, 1, 249, 3, 159488, 1)),
    ((63744, 300, 0, 0, 2, 1, 0, 128), (0, 128, 2, 498, 3, 159488, 0)),       # K3 > 255: no k_sweep3
]


@pytest.mark.parametrize("case,want", SWEEP3, ids=lambda v: "-".join(map(str, v)) if len(v) == 8 else "")
def test_sweep3_geometry(case, want, monkeypatch):
    n, p, block, nwg, xmax, gram16, d3, r3 = case
    if d3:
        monkeypatch.setenv("BWGR_D3", str(d3))
    if r3:
        monkeypatch.setenv("BWGR_R3", str(r3))
    rc, pl, msg = plan(0, n, p, block, nwg, MAIN, xmax, gram16)
    assert rc == 0, msg
    got = tuple(pl[k] for k in ("fits3", "R3", "sub3", "K3", "D", "lds3", "solo3"))
    print(case, got)
    assert got == want
    assert pl["sub3"] * pl["R3"] == pl["R"] and pl["K3"] == pl["K"] * pl["sub3"]


def test_sweep3_is_not_planned_without_the_data_or_off_main_int8_pipelined_panels(monkeypatch):
    unplanned = (0, 0, 0, 0, 0, 0, 1)
    f3 = ("fits3", "R3", "sub3", "K3", "D", "lds3", "solo3")
    assert tuple(plan(0, 10000, 1000000)[1][k] for k in f3) == unplanned                       # xmax < 0
    assert tuple(plan(1, 500, 300, xmax=0)[1][k] for k in f3) == unplanned                     # float
    assert tuple(plan(0, 64000, 300, xmax=2)[1][k] for k in f3) == unplanned                   # the first engine
    monkeypatch.setenv("BWGR_SWEEP", "2")
    assert tuple(plan(0, 10000, 1000000, xmax=2)[1][k] for k in f3) == unplanned


def test_solo3_switch(monkeypatch):
    monkeypatch.setenv("BWGR_SOLO3", "0")
    assert plan(0, 10000, 1000000, xmax=2)[1]["solo3"] == 0
    monkeypatch.setenv("BWGR_SOLO3", "1")
    monkeypatch.setenv("BWGR_R3", "128")    # an explicit BWGR_SOLO3 outranks what an explicit height implies
    q = plan(0, 10000, 1000000, xmax=2)[1]
    assert (q["fits3"], q["R3"], q["K3"], q["solo3"]) == (1, 128, 80, 1)
