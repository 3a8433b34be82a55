"""CPU: the table of tests/tall_cases.py under the library's own host arithmetic (bwgr_debug_panel_plan, bwgr_debug_uvb_plan,
bwgr_debug_xxt_plan, bwgr_debug_launch_plan: no GPU).  Every shape of tests/test_gpu_tall.py reaches the loop trip, slab height or chunk
rule it is listed for; a change of a grid or of a plan rule that moves a shape out of its regime fails here instead of silently dropping
that code from what the GPU suite compares with a reference."""
import pytest

import tall_cases as tc

EINVAL = 1


def test_hook_writes_every_field_and_refuses_nonsense():
    rc, pl = tc.launch_plan(700, 768, 900, 5)
    assert rc == 0 and all(pl[f] >= 1 for f in tc.LAUNCH_FIELDS), pl
    for n, ld, p, k in [(0, 128, 10, 1), (700, 640, 10, 1), (700, 700, 10, 1), (700, 768, 0, 1), (700, 768, 10, 0), (-5, 128, 10, 1)]:
        assert tc.launch_plan(n, ld, p, k)[0] == EINVAL, (n, ld, p, k)


def test_launch_plan_is_the_documented_rule():
    """include/bwgr.h, restated: the caps of the grids, and panel_xb's chunks -- as many as bring the grid to about four workgroups per
    compute unit (1 024), at most 64 and never shorter than one staged tile of B; every marker belongs to a chunk and no chunk is empty."""
    for n, ld in ((1, 128), (196, 256), (700, 768), (5000, 5120), (9000, 9216), (70000, 70400), (300000, 300032)):
        for p in (1, 127, 128, 129, 900, 8191, 8192, 9000, 33000, 70000):
            for k in (1, 16, 17, 300):
                rc, pl = tc.launch_plan(n, ld, p, k)
                assert rc == 0
                assert pl["threads"] == 256 and pl["mrr_np"] == 64 and pl["uvb_np"] == 32 and pl["pxb_rows"] == 1024
                assert pl["xxt_zero_wg"] == 2048 and pl["kfin_apply_wg"] == 4096 and pl["pxb_chunks_max"] == 64 and pl["pxb_mt"] == 128
                assert pl["mrr_setup_wg"] == min(-(-p // 4), 8192)
                assert pl["mrr_pass_wg"] == min(ld // 64, 32) and pl["uvb_pass_wg"] == min(ld // 64, 64)
                assert pl["uvb_shift_wg"] == min(-(-n // 256), 1024) and pl["uvb_xb_wg"] == -(-n // 256)
                assert pl["pxb_finish_wg"] == min(-(-n * k // 256), 4096)
                tiles, slices = -(-ld // 1024), -(-k // 16)
                assert (pl["pxb_tiles"], pl["pxb_slices"]) == (tiles, slices)
                want = min(64, -(-p // 128), max(1, -(-1024 // (tiles * slices))))
                chunk = -(-(-(-p // want)) // 128) * 128
                assert pl["pxb_chunk"] == chunk and pl["pxb_chunks"] == -(-p // chunk) <= want, (n, p, k, pl)
                assert chunk * (pl["pxb_chunks"] - 1) < p <= chunk * pl["pxb_chunks"]


@pytest.mark.parametrize("tag", list(tc.CASES))
def test_case_reaches_what_it_is_listed_for(tag):
    pl = tc.plans(tag)
    got = {k: pl[k] for k in tc.EXPECT[tag] if k != "pxb_k"}
    want = {k: v for k, v in tc.EXPECT[tag].items() if k != "pxb_k"}
    assert got == want, (tag, pl)


def test_cases_reach_every_regime_together():
    pls = {tag: tc.plans(tag) for tag in tc.CASES}
    # uvbeta: a workgroup of the pass takes a second and a third tile; the row reduction takes a second trip; whole padding tiles; R != 256
    uvb = [pls[t] for t in ("tall9k", "slab1280", "slab1024")]
    assert max(pl["uvb_pass"] for pl in uvb) >= 3 and max(pl["uvb_rows"] for pl in uvb) >= 2
    assert any(pl["pad"] >= 64 for pl in uvb) and {pl["R"] for pl in uvb} >= {256, 1024, 1280}
    # mrr: second trips of the row reduction, of the marker reduction and of the column set-up; R != 256; a short last block
    mrr = [pls[t] for t in ("tall16k", "slab1280", "wide33k")]
    assert max(pl["mrr_ey"] for pl in mrr) >= 2 and max(pl["mrr_tilde"] for pl in mrr) >= 2 and max(pl["mrr_setup"] for pl in mrr) >= 2
    assert any(pl["R"] != 256 for pl in mrr) and any(pl["last64"] < 64 for pl in mrr)
    # panel_xb: several row tiles, one of them across two slabs; w = r0 / R with R != 256; the cap of the chunk rule; a short last chunk
    xb = [pls[t] for t in ("tall9k", "slab1280", "slab1024", "xbwide")]
    assert max(pl["pxb_tiles"] for pl in xb) >= 9 and any(pl["pxb_cross"] for pl in xb) and any(pl["pxb_cap"] for pl in xb)
    assert any(pl["R"] == 1024 and pl["pxb_tiles"] == pl["K"] == 2 for pl in xb)      # one row tile per slab
    assert all(pl["pxb_last"] < pl["pxb_chunk"] for pl in xb)
    # the relationship kernels: second trips of both element-wise kernels, at R = 256 and at another height
    kern = [pls[t] for t in ("kern1100", "kern1100s", "slab1024")]
    assert all(pl["kfin_apply"] >= 2 for pl in kern) and any(pl["xxt_zero"] >= 2 for pl in kern)
    assert {pl["R"] for pl in kern} >= {256, 1024} and len({pl["R"] for pl in kern}) == 3 and any(pl["R"] != 256 and pl["K"] > 1 for pl in kern)


@pytest.mark.parametrize("name", ["MEGA", "GSEM"])
@pytest.mark.parametrize("tag", list(tc.SEM2_DRIVERS))
def test_two_design_driver_cases_are_well_posed(tag, name):
    """Preconditions on the inputs of test_gpu_tall's MEGA / GSEM cases, as tests/test_sem2_cpu.py states them, asserted on the restatement:
    every output finite (GSEM may diverge on a trait; here it does not), neighbouring singular values of the decomposed matrix (Y2 for MEGA,
    G for GSEM) at least 5 % of the largest apart, and npc = 3.  slab1280 / seed 3001: gaps 0.173 (Y2) and 0.226 (G), six sweeps in every
    stage.  tall9k / seed 3011 at the reference's defaults: 0.180 and 0.354; every stage stops by its own test after 2 to 6 sweeps, and no cnv
    of any stage comes nearer than 0.02 to log10(tol) (the nearest is 0.115 for MEGA and 0.112 for GSEM), so the sweep counts are not a
    matter of rounding."""
    import numpy as np
    import sem2_cases as S2C
    o = tc.driver_ref(name, tag)
    s = o["s"]
    gap = float(np.min(-np.diff(s)) / s[0])
    stages = S2C.stages(name, o)
    print(name, tag, gap, [list(d["its"]) for d in stages])
    assert gap >= 0.05 and o["npc"] == 3 == len(s), (gap, s)
    for key in ("mu", "b", "hat", "BETA1", "BETA2") + (("LS", "LS_BETA", "gebv") if name == "MEGA" else ()):
        assert np.all(np.isfinite(o[key])), key
    if tc.SEM2_DRIVERS[tag]["kw"]:
        assert all((d["its"] == 6).all() for d in stages)
    else:
        logtol = np.log10(10e-7)
        near = min(abs(c - logtol) for d in stages for tr in d["trace"] for c in tr)
        print(near)
        assert near >= 0.02 and all(0 < d["its"].min() and d["its"].max() < 100 for d in stages)


def test_two_design_engine_cases_are_what_they_say():
    """uvbeta2 on tall9k and slab1280: 10 % missing in every trait, each trait its own rows, q = 3; k = 65 is two groups of traits (the
    second of one trait).  The restatement makes six sweeps and gives finite results on both k = 3 cases (asserted here); the 65-trait
    restatement takes seconds and is run by the GPU test alone, which asserts the library's six sweeps per trait against it."""
    import numpy as np
    for (tag, k) in tc.SEM2_ENGINE:
        c = tc.uvb2_case(tag, k)
        n = tc.CASES[tag]["n"]
        miss = np.isnan(c["Y"]).mean(0)
        assert c["Y"].shape == (n, k) and c["Z"].shape == (n, 3) and c["kw"] == dict(maxit=6, tol=0)
        assert miss.min() > 0.08 and miss.max() < 0.12 and len({np.isnan(c["Y"][:, t]).tobytes() for t in range(k)}) == k
    for tag in ("tall9k", "slab1280"):
        o = tc.uvb2_ref(tag, 3)
        assert list(o["its"]) == [6, 6, 6] and all(np.isfinite(o[key]).all() for key in ("b1", "b2", "mu", "h2", "ve", "vb1", "vb2", "cnv")), tag
    import bwgr_amd
    pl = bwgr_amd.uvb_plan(5000, 200, 65)
    assert pl["groups"] == 2 and pl["W"] == 64


def test_the_old_shapes_did_not_reach_them():
    """What the issue is about, pinned: on tpod (196 x 376), the 700 x 900 three-slab panel and mrr's 4 100 rows every one of these kernels
    makes a single trip, and k_pxb runs one row tile."""
    for n, ld, p in ((196, 256, 376), (700, 768, 900), (4100, 4224, 130)):
        rc, pl = tc.launch_plan(n, ld, p, 17)
        assert rc == 0
        t = pl["threads"]
        assert ld <= pl["uvb_np"] * t and ld <= pl["mrr_np"] * t and p <= pl["mrr_np"] * t and p <= pl["mrr_setup_wg"] * 4
        if n <= 700:
            assert n * n <= pl["kfin_apply_wg"] * t and n * n <= pl["xxt_zero_wg"] * t and pl["pxb_tiles"] == 1
        assert ld // 64 <= pl["uvb_pass_wg"] or n == 4100      # (mrr's pass did take a second tile there; uvbeta never ran on it)
