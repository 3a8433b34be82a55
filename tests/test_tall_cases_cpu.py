"""CPU: the table of tests/tall_cases.py under the library's own host arithmetic (bwgr_debug_panel_plan, bwgr_debug_uvb_plan,
bwgr_debug_xxt_plan, bwgr_debug_launch_plan, bwgr_debug_pegs_launch_plan, bwgr_debug_pegsx_plan, bwgr_debug_pegs_plan: no GPU).  Every shape
of tests/test_gpu_tall.py reaches the loop trip, slab height or chunk rule it is listed for; a change of a grid or of a plan rule that moves
a shape out of its regime fails here instead of silently dropping that code from what the GPU suite compares with a reference.  The PEGS /
PEGSZ / PEGSX jobs also pass, on their restatements, the branch guards that tests/test_pegs_cpu.py and tests/test_pegsx_cpu.py hold their own
cases to."""
import numpy as np
import pytest

import tall_cases as tc
import test_pegs_cpu as TPC
import test_pegsx_cpu as TXC

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


# ---- PEGS / PEGSZ / PEGSX ----
PEGS_RUNS = [(entry, job) for entry in ("PEGS", "PEGSZ", "PEGSX", "PEGSZ_sparse") for job in tc.pegs_jobs(entry)]


def test_pegs_launch_plan_is_the_documented_rule():
    """include/bwgr.h, restated: the trace kernels take a workgroup per sixteen columns up to 1 024, k_pegs_dense_setup one per four columns
    up to 8 192, the dense leg and the fixed step a thread per row in whole waves up to 1 024 -- and the hook refuses nonsense."""
    import bwgr_amd
    for n in (1, 64, 65, 196, 700, 960, 961, 1024, 1500, 9000, 300000):
        for m in (1, 4, 5, 16, 17, 900, 16384, 16385, 32768, 32769, 33000, 10 ** 6):
            pl = bwgr_amd.pegs_launch_plan(n, m)
            assert pl["trace_wg"] == min(-(-(-(-m // 4)) // 4), 1024) and pl["trace_cols"] == 16 * pl["trace_wg"]
            assert pl["setup_wg"] == min(-(-m // 4), 8192) and pl["setup_cols"] == 4 * pl["setup_wg"]
            assert pl["leg_threads"] == pl["fixed_threads"] == min(1024, -(-n // 64) * 64)
            assert pl["fixed_threads"] == bwgr_amd.pegsx_plan(n, 1, 1)["threads"] and pl["leg_threads"] == bwgr_amd.pegs_plan(n, 1, 1)["threads"]
    for n, m in ((0, 5), (5, 0), (-1, 5), (5, -1)):
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            bwgr_amd.pegs_launch_plan(n, m)
        assert ei.value.code == EINVAL and "pegs launch plan" in str(ei.value)


@pytest.mark.parametrize("job", list(tc.PEGS_JOBS))
def test_pegs_job_reaches_what_it_is_listed_for(job):
    pl = tc.pegs_plans(job)
    print(job, pl)
    assert {k: pl[k] for k in tc.PEGS_EXPECT[job]} == tc.PEGS_EXPECT[job], (job, pl)


def test_pegs_jobs_reach_every_regime_together():
    import bwgr_amd
    pls = {job: tc.pegs_plans(job) for job in tc.PEGS_JOBS}
    J = tc.PEGS_JOBS
    # the trace kernels: a third trip on the panel kernel and a second on the dense one, both at the cap of the grid (1 024 partials for
    # k_mrr_finish); a last group of fewer than four columns on a later trip; every slab height, and a second slab of another height than 256
    assert pls["wide33k"]["trace"] >= 3 and pls["dense16500"]["trace"] >= 2 and J["wide33k"]["effects"] == ("panel",) and J["dense16500"]["tag"] is None
    assert pls["wide33k"]["trace_wg"] == pls["dense16500"]["trace_wg"] == 1024
    assert any(pl["trace_tail"] < 4 and pl["trace_last"] >= 2 for pl in pls.values())
    x = [pls[j] for j in tc.pegs_jobs("PEGSX") if J[j]["tag"]]
    assert {pl["R"] for pl in x} >= {256, 1024, 1280} and any(pl["R"] != 256 and pl["K"] > 1 for pl in x)
    # the uncentred train: second trips of the marker reductions and of the row reduction, R != 256, a short last block -- under every entry
    for entry in ("PEGS", "PEGSZ", "PEGSX"):
        t = [pls[j] for j in tc.pegs_jobs(entry) if J[j]["tag"] in tc.CASES]
        assert max(pl["mrr_tilde"] for pl in t) >= 3 and max(pl["mrr_setup"] for pl in t) >= 2 and max(pl["mrr_ey"] for pl in t) >= 2
        assert {pl["R"] for pl in t} >= {256, 1024, 1280} and min(pl["last64"] for pl in t) == 2
    # a dense effect beside a panel that pads further than the dense effect alone would; in both orders under PEGSZ
    both = [j for j in J if len(J[j]["effects"]) == 2]
    assert any(pls[j]["ld"] != pls[j]["ld128"] for j in both) and {J[j]["effects"][0] for j in both if "PEGSZ" in J[j]["entries"]} == {"panel", 5}
    # row loops past one trip at the widest workgroup, under every entry with a dense effect; the fixed step's column loop wraps there
    for entry in ("PEGSZ", "PEGSX"):
        assert any(pls[j]["leg_threads"] == 1024 and pls[j]["rows"] >= 5 for j in both if entry in J[j]["entries"])
    assert any(pls[j]["fixed_cols"] >= 2 and pls[j]["rows"] >= 5 and pls[j]["fixed_threads"] == 1024 for j in tc.pegs_jobs("PEGSX"))
    # f at the cap: four 64-lane trips of the quadratic form, and one more column is refused
    assert J["f256"]["f"] == 256 and pls["f256"]["quad"] == 4 and pls["f256"]["lds_trace"] == 8 * (4 * 4 * 256 + 4 * 16) <= 64 * 1024
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.pegsx_plan(700, 257, 3)
    assert ei.value.code == EINVAL
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.PEGSX(np.zeros((8, 2)), np.ones((8, 257)), [bwgr_amd.dense(np.ones((8, 3)))])
    assert ei.value.code == EINVAL and "f = 257" in str(ei.value)
    assert set(tc.TRZSZ_ALONE) <= set(tc.pegs_jobs("PEGSX")) and set(tc.NORMAL_EQUATIONS) <= set(tc.pegs_jobs("PEGSX"))


def test_pegs_traits_miss_what_they_say():
    """every trait its own pattern; the rows of PEGS_MISSING missing in every trait, on tall9k a whole quad at a slab edge"""
    for job, j in tc.PEGS_JOBS.items():
        Y, effects = tc.pegs_data(job)
        k = j["k"]
        assert Y.shape[1] == k and len({np.isnan(Y[:, t]).tobytes() for t in range(k)}) == k == tc.pegs_plans(job)["npat"]
        rows = tc.PEGS_MISSING.get(j["tag"], ())
        assert np.isnan(Y[list(rows)]).all() and int(np.isnan(Y[:, 1]).sum()) == len(rows)      # (trait 1 misses nothing else)
        assert [e[0] for e in effects] == ["panel" if e == "panel" else "sparse" if isinstance(e, tuple) else "dense" for e in j["effects"]]
        if j["tag"] in tc.PEGS_MISSING:
            R = tc.pegs_plans(job)["R"]
            assert any(r % R == 0 and r > 0 for r in rows) and any((r + 1) % R == 0 for r in rows)
    rows = tc.PEGS_MISSING["tall9k"]
    assert {4096, 4097, 4098, 4099} <= set(rows) and 4096 % 256 == 0 and 4096 % 4 == 0
    assert np.isnan(tc.pegs_case("PEGSX", "tall9k")["data"]()[0][4096:4100]).all()


def test_sparse_jobs_put_the_sparse_kernels_beside_tall_and_other_slab_panels():
    """tall9k_sparse and slab1280_sparse: the residual's stride is the panel's ld, far from n and on slabs of 256 and of 1 280 rows; a level
    longer than 4 096 rows that spans slab edges, two rows on both sides of an edge on one level, all-missing rows on both sides of an edge
    inside a level; both legs; more workgroups of k_pegs_sparse_hat than any case of tests/pegs_sparse_cases.py has (nine at n = 2 100)."""
    from pegs_sparse_cases import SR
    J = tc.PEGS_JOBS
    jobs = [job for job in J if any(isinstance(e, tuple) for e in J[job]["effects"])]
    assert jobs == ["tall9k_sparse", "slab1280_sparse"]
    pls = {job: tc.pegs_plans(job) for job in jobs}
    assert {pls[j]["R"] for j in jobs} == {256, 1280} and all(pls[j]["K"] > 1 and pls[j]["pad"] >= 120 and pls[j]["sparse_hat"] > 9 for j in jobs)
    assert {leg for j in jobs for leg in pls[j]["sparse_legs"]} == {"disjoint", "serial"}
    assert "PEGSZ_sparse" in J["slab1280_sparse"]["entries"] and all({"PEGSZ", "PEGSX"} <= set(J[j]["entries"]) for j in jobs)
    for job in jobs:
        Y, effects = tc.pegs_data(job)
        R, n = pls[job]["R"], Y.shape[0]
        rows = tc.PEGS_MISSING[J[job]["tag"]]
        assert np.isnan(Y[list(rows)]).all()
        for e in effects[1:]:
            assert e[0] == "sparse" and e[1].shape[0] == n and np.array_equal(e[1], SR.f32(e[1]))
        inc = effects[1][1]
        assert SR.row_disjoint(inc) and (inc.sum(1) == 1).all() and (inc.sum(0) > 0).all()
        edge = [r for r in rows if r % R == 0 and r > 0][0]
        assert edge - 1 in rows                                                # all-missing rows on both sides of a slab edge ...
        lev = inc.argmax(1)
        big = int(np.argmax(inc.sum(0)))
        assert len({r // R for r in np.flatnonzero(lev == big)}) == pls[job]["K"]      # ... and the largest level has rows in every slab
    Y, effects = tc.pegs_data("tall9k_sparse")
    inc = effects[1][1]
    a, b = tc.SAME_LEVEL["tall9k_sparse"]
    assert inc.shape[1] == 2 and inc.sum(0).max() > 4096 and (a + 1) % 256 == 0 and b == a + 1 and np.array_equal(inc[a], inc[b])
    assert not SR.row_disjoint(effects[2][1]) and effects[2][1].shape[1] == 30 and 0.04 < effects[2][2].mean() < 0.06
    assert tc.pegs_data("slab1280_sparse")[1][1][1].shape[1] == 40


@pytest.mark.parametrize("entry,job", PEGS_RUNS, ids=["%s-%s" % r for r in PEGS_RUNS])
def test_pegs_job_is_away_from_the_discontinuous_branches(entry, job):
    """The guards of tests/test_pegs_cpu.py / tests/test_pegsx_cpu.py as they stand, on the job's restatement: |MinDVb - covMinEv| >= 1e-3
    covMinEv in every sweep and effect, no floor active, every kept eigenvalue ratio of M'M at least 1e-3 and none dropped, its == maxit."""
    case = tc.pegs_case(entry, job)
    if case["kw"]["maxit"] == 0:      # a TrZSZ-only job: there is no sweep to guard, only the rank decision of M'M and the start values
        fit = tc.XC.restate(case)[3]
        assert fit["its"] == 0 and not fit["floors0"] and all(m["kept"].min() >= 1e-3 and m["dropped"].size == 0 for m in fit["mm"])
        return
    if entry == "PEGSX":
        TXC.test_case_is_away_from_the_discontinuous_branches(case)
        fit = tc.XC.restate(case)[3]
        print(entry, job, "min |MinDVb - cm| / cm", min(abs(r["MinDVb"] - 1e-3) / 1e-3 for recs in fit["trace"] for r in recs),
              "min kept", min(m["kept"].min() for m in fit["mm"]))
        assert fit["its"] == case["kw"]["maxit"]
    else:
        TPC.test_case_is_away_from_the_discontinuous_branches(case)
        fit = tc.PC.restate(case)[2]
        print(entry, job, "min |MinDVb - cm| / cm", min(abs(r["MinDVb"] - 1e-3) / 1e-3 for recs in fit["trace"] for r in recs))
        assert fit["numit"] == case["kw"]["maxit"]


@pytest.mark.parametrize("entry", tc.HANDLE_ENTRIES)
def test_handle_table_pegs_calls_are_away_from_the_discontinuous_branches(entry):
    """the same guards on the inputs of tests/test_gpu_handles.py's PEGS, PEGSZ and PEGSX entries, of its two-panel PEGSZ call and of the two
    entries with sparse effects"""
    case = tc.handle_case(entry)
    (TXC if entry.startswith("PEGSX") else TPC).test_case_is_away_from_the_discontinuous_branches(case)
    if entry.endswith("_S"):
        effects = case["data"]()[-1]
        assert [e[0] for e in effects] == ["panel", "sparse", "sparse"] and [e[1].shape for e in effects] == [(700, 900), (700, 12), (700, 25)]
        assert tc.SC.SR.row_disjoint(effects[1][1]) and not tc.SC.SR.row_disjoint(effects[2][1])        # both legs
        assert entry != "PEGSX_S" or case["data"]()[1].shape == (700, 3)


def test_the_old_pegs_cases_did_not_reach_them():
    """What the PEGS section is about, pinned: on tpod, the 700 x 900 panel and the dense 1 500 x 20 and 196 x 70 effects of
    tests/pegs_cases.py and tests/pegsx_cases.py the trace kernels and the dense set-up make one trip with at most 57 workgroups, no dense
    effect sits beside a panel that pads further than it would, and only the dense-only n = 1 500 case (k = 3, f = 3) takes a second row trip."""
    import bwgr_amd
    for n, m in ((196, 376), (700, 900), (196, 70), (700, 70), (1500, 20)):
        pl = bwgr_amd.pegs_launch_plan(n, m)
        assert m <= pl["trace_cols"] and m <= pl["setup_cols"] and pl["trace_wg"] <= 57
        assert (n > pl["fixed_threads"]) == (n == 1500)
    assert -(-196 // 128) * 128 == 256 and -(-700 // 128) * 128 == 768      # the panels' own ld there (tests/test_panel_plan.py)
    assert max(c["data"]()[1].shape[1] for c in tc.XC.CASES) == 70
