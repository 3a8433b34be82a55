"""CPU: the table of tests/pair_cases.py under the library's own host arithmetic (bwgr_debug_panel_plan, bwgr_debug_xyt_plan,
bwgr_debug_xxt_plan, bwgr_debug_launch_plan: no GPU).  Every orientation of every pair of tests/test_gpu_pairs.py reaches the loop trips, slab
heights and chunks it is listed for; a change of a grid or of a plan rule that moves a pair out of its regime fails here instead of silently
dropping that code from what the GPU suite compares with a reference.

Two figures of the table are the exception: `sumd` and `rows_s` restate constants that no hook reports -- XXT_SUMD_PARTS = 1 024 workgroups of
k_kfin_sumd_stage1 and the 128 rows per workgroup of kfin_rows_grid (kernels_host.hip.h) -- so a change of either would leave them as they are.
They record what the shapes were chosen for; test_the_unreported_constants_are_the_sources reads the two constants from the source text, which
is as near as a test without a hook comes."""
import numpy as np
import pytest

import pair_cases as pc
import tall_cases as tc


@pytest.mark.parametrize("tag,swapped", pc.ORIENTATIONS, ids=["%s%s" % (t, "-swapped" if s else "") for t, s in pc.ORIENTATIONS])
def test_pair_reaches_what_it_is_listed_for(tag, swapped):
    pl = pc.plans(tag, swapped)
    want = pc.EXPECT[(tag, swapped)]
    assert {k: pl[k] for k in want} == want, (tag, swapped, pl)


def test_pairs_reach_every_regime_together():
    pls = {o: pc.plans(*o) for o in pc.ORIENTATIONS}
    # the finish: later trips over K_ff and over K_fs, and one call whose K_ff fits one trip while its K_fs does not
    assert max(pl["apply_ff"] for pl in pls.values()) >= 4 and all(pl["apply_fs"] >= 2 for pl in pls.values())
    assert any(pl["apply_ff"] == 1 and pl["apply_fs"] >= 2 for pl in pls.values())
    # the rectangular zeroing kernel: later trips, n_r != n_c, both ways round
    zero = [pl for pl in pls.values() if pl["zero_fs"]]
    assert len(zero) == 2 and all(pl["zero_fs"] >= 3 and pl["forced_chunks"] == 3 and pl["f"][0] != pl["s"][0] for pl in zero)
    # pair1024: the slab heights differ, the 1 024-row panel has a second slab, and it is operand A in one orientation and operand B in the other
    a, b = pls[("pair1024", False)], pls[("pair1024", True)]
    assert a["f"][2] == 1024 and a["f"][1] == 2 and a["s"][2] != 1024 and b["s"][2] == 1024 and b["s"][1] == 2 and b["f"] == a["s"]
    assert b["rows_s"] == (16, 2) and a["sumd"] >= 2
    # the grid of the product is rectangular, T_r != T_c, everywhere
    assert all(pl["Tr"] != pl["Tc"] and pl["tiles"] == pl["Tr"] * pl["Tc"] for pl in pls.values())


def test_the_unreported_constants_are_the_sources():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwgr_amd", "csrc", "kernels_host.hip.h")).read()
    assert int(re.search(r"constexpr int XXT_SUMD_PARTS = (\d+);", src).group(1)) == pc.SUMD_PARTS
    grid = src[src.index("static inline dim3 kfin_rows_grid"):]
    assert "return dim3((unsigned)(ld / 128)," in grid[:grid.index("\n}")]
    assert "dim3(XXT_SUMD_PARTS), dim3(256), 0, st, G, ldg, diag_d" in src      # the grid k_kfin_sumd_stage1 is launched with


def test_the_old_pairs_did_not_reach_them():
    """What the table is for, pinned: the pairs of tests/test_gpu_kernels2.py -- 300 x 200, 700 x 300, 130 x 66 -- give every one of these
    kernels a single trip, and the largest forced-chunk product there (300 x 200) a single trip of k_xxt_zero."""
    for nf, ns, p in ((300, 200, 900), (700, 300, 900), (300, 700, 900), (130, 66, 376)):
        rc, lp = tc.launch_plan(nf, -(-nf // 128) * 128, p, 1)
        assert rc == 0
        assert nf * max(nf, ns) <= lp["kfin_apply_wg"] * lp["threads"] and nf * max(nf, ns) <= lp["xxt_zero_wg"] * lp["threads"]


def test_the_panels_of_a_pair_are_different_genotypes():
    for tag in pc.CASES:
        F, S = pc.data(tag)
        Sf, Ss = pc.data(tag, swapped=True)
        assert F.dtype == S.dtype == np.int8 and F.shape[1] == S.shape[1] == pc.P and F.shape[0] != S.shape[0]
        assert Sf is S and Ss is F and not np.array_equal(F[:100], S[:100])
        assert set(np.unique(F)) == set(np.unique(S)) == {0, 1, 2}
