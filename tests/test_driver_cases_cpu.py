"""CPU: the table of tests/driver_cases.py under the library's own host arithmetic (bwgr_debug_panel_plan, bwgr_debug_aux_plan: no GPU).

* Every shape reaches the launch regime it is listed for, and together they reach every path of the row gather, every kind of subsample
  geometry and both kinds of product (one chunk; several chunks, a short last one, several row workgroups) on int8 and on float panels.  A
  change of a rule that moves a shape out of its regime fails here instead of silently dropping that branch from the GPU suite.
* Input selection for the inclusion decisions.  tests/test_gpu_drivers.py asserts EQUAL decisions between GPU and oracle.  A near-tie in
  u < p_include would fail such a test on a correct kernel; the reference side can see a near-tie alone: its two flavours ("w": double
  accumulators, "f": the float-faithful restatement) differ by summation order only, so a setting is committed only if both give identical d.
"""
import numpy as np
import pytest

import driver_cases as dc

EINVAL = 1


def test_hook_writes_every_field_and_refuses_nonsense():
    rc, pl = dc.aux_plan(0, 1300, 1536)
    assert rc == 0 and all(pl[k] >= 0 for k in dc.AUX_FIELDS)
    for f32, p, ld in [(0, 0, 1536), (0, 10, 0), (0, 10, 100), (1, 10, -128)]:
        assert dc.aux_plan(f32, p, ld)[0] == EINVAL, (f32, p, ld)


@pytest.mark.parametrize("f32", [0, 1])
def test_aux_plan_is_the_documented_rule(f32):
    """include/bwgr.h and DESIGN.md section 3, restated: chunks = min(512 | 64, max(1, p div 512)), columns per chunk rounded UP (every column
    belongs to a chunk, the last one may be short but never empty), 256 threads x (16 | 4) rows per row workgroup; the gather's path."""
    for p in (1, 15, 511, 512, 1023, 1024, 1031, 1300, 1537, 32768, 70000, 262144, 300000):
        for ld in (128, 1024, 1152, 4096, 4224, 9216, 16384, 16512, 32768, 32896, 65536, 65664, 131072):
            rc, pl = dc.aux_plan(f32, p, ld)
            assert rc == 0
            chunks = min(64 if f32 else 512, max(1, p // 512))
            assert pl["chunks"] == chunks and pl["cpc"] == -(-p // chunks), (p, ld, pl)
            assert pl["cpc"] * (chunks - 1) < p <= pl["cpc"] * chunks, (p, pl)
            rows_per_wg = 256 * (4 if f32 else 16)
            assert pl["row_wgs"] == -(-ld // rows_per_wg), (ld, pl)
            mpw = 0 if (f32 or ld > 65536) else max(1, min(8, 32768 // ld))
            assert pl["gather"] == mpw and pl["gather_lds"] == mpw * ld <= 65536, (ld, pl)


@pytest.mark.parametrize("tag", list(dc.CASES))
def test_case_reaches_its_regime(tag):
    pl = dc.plans(tag)
    got = {k: pl[k] for k in dc.EXPECT[tag]}
    assert got == dc.EXPECT[tag], (tag, pl)


def test_cases_reach_every_regime_together():
    pls = {tag: dc.plans(tag) for tag in dc.CASES}
    f32 = {tag: dc.CASES[tag]["f32"] for tag in dc.CASES}
    # the row gather, over the shapes KMUP2 and wgr(bag=) run on
    paths = set()
    for tag in set(dc.KMUP2_TAGS) | {t for _, t, _ in dc.BAG_JOBS}:
        pl = pls[tag]
        if f32[tag]:
            paths.add("float")
        elif pl["gather"] == 0:
            assert pl["ld"] > 65536
            paths.add("element-wise")
        elif pl["gather"] == 1:
            assert 32768 < pl["ld"] <= 65536 and pl["gather_lds"] == pl["ld"]
            paths.add("mpw 1")
        elif pl["gather"] == 8 and pl["ragged"]:
            paths.add("mpw 8 ragged")
        elif 1 < pl["gather"] < 8 and pl["ragged"]:
            paths.add("1 < mpw < 8 ragged")
    assert paths == {"float", "element-wise", "mpw 1", "mpw 8 ragged", "1 < mpw < 8 ragged"}, paths
    # the product behind hat and wgr's residual, over the shapes whose hat is compared
    hat_tags = {t for _, t, _ in dc.WGR_JOBS} | {t for t, _ in dc.CHAIN_JOBS} | {t for _, t, _ in dc.BAG_JOBS}
    for kind in (0, 1):
        seen = set()
        for tag in hat_tags:
            if f32[tag] != kind:
                continue
            pl = pls[tag]
            if pl["chunks"] == 1:
                seen.add("1 chunk")
            if pl["chunks"] >= 2 and pl["last_chunk"] < pl["cpc"]:
                seen.add("short last chunk")
            if pl["chunks"] >= 2:
                seen.add("chunks")
            if pl["row_wgs"] >= 2:
                seen.add("row workgroups")
        if kind == 1:      # the one-chunk float product of this table: the two-effect samplers' second panel (hat = X1 b1 + X2 b2 + mu)
            X2 = dc.bayes2_inputs()[1]
            assert X2.dtype == np.float32 and dc.aux_plan(1, X2.shape[1], dc.plans("mid")["ld"])[1]["chunks"] == 1
            seen.add("1 chunk")
        assert seen >= {"1 chunk", "short last chunk", "chunks", "row workgroups"}, (kind, seen)
    assert pls["wide"]["chunks"] > 64 and dc.CASES["wide"]["p"] > 65536
    assert any(pls[t]["K"] > 1 and dc.CASES[t]["n"] > 1024 for t in dc.KMUP_TAGS)


def test_subsample_panels_have_their_own_geometry():
    kinds = set()
    for (tag, rows), want in dc.SUBSAMPLES.items():
        c = dc.CASES[tag]
        base = dc.plans(tag)
        sub = dc.panel_plan(c["f32"], rows, c["p"], base["m"], kind=dc.ROWS)
        assert {k: sub[k] for k in want} == want and sub["m"] == base["m"], (tag, rows, sub)
        if sub["R"] != base["R"]:
            kinds.add("other slab height")
        elif sub["K"] < base["K"]:
            kinds.add("fewer slabs")
        elif sub["K"] > base["K"]:
            kinds.add("more slabs")
        else:
            kinds.add("same K")
    assert kinds == {"other slab height", "fewer slabs", "more slabs", "same K"}
    # the rows the tests actually subsample are the rows tabulated
    for tag, rows in dc.KMUP2_ROWS.items():
        assert (tag, rows) in dc.SUBSAMPLES
    assert int(dc.CASES["mid"]["n"] * 0.5) == 750 and int(dc.CASES["mid"]["n"] * 1.5) == 2250
    for tag, rows in dc.KMUP2_ROWS.items():
        assert (tag, dc.kmup2_use(tag, "most").size) in dc.SUBSAMPLES
        assert dc.kmup2_use(tag, "over").size > dc.CASES[tag]["n"]
        u = dc.kmup2_use(tag, "unsorted")
        assert np.any(np.diff(u) < 0) and u.size == rows
        assert np.unique(dc.kmup2_use(tag, "sorted")).size == rows and np.unique(dc.kmup2_use(tag, "repeats")).size < rows


@pytest.mark.parametrize("which", list(dc.EIGK_PK))
def test_eigk_truncations(which):
    """pk = 239: four float blocks of 64 (twelve slabs); 36: less than one block; 5: less than the smallest block of 16."""
    eig, vark, pk = dc.eigk_case(which)
    from oracle import oracle as O
    assert pk == dc.EIGK_PK[which] == O.eigk_truncate(eig, vark)[2]
    pl = dc.panel_plan(1, dc.CASES["mid"]["n"], pk)
    assert (pl["nblocks"], pl["K"]) == {"0.5": (4, 12), "0.1": (1, 12), "pk5": (1, 3)}[which], pl


# ---- input selection: both flavours of the reference take the same decisions ----------------------------------------------------------------
def _same_decisions(call, keys=("d",)):
    w, f = call("w"), call("f")
    for k in keys:
        assert np.array_equal(w[k], f[k]), (k, int(np.sum(w[k] != f[k])), float(np.max(np.abs(w[k] - f[k]))))
    return w


@pytest.mark.parametrize("name,tag,args", [j for j in dc.WGR_JOBS + dc.BAG_JOBS if j[2].get("pi", 0) > 0], ids=lambda v: v if isinstance(v, str) else "")
def test_wgr_settings_decide_alike_in_both_flavours(name, tag, args):
    from oracle import oracle as O
    X, y = dc.data(tag)
    _same_decisions(lambda fl: O.wgr(y, X, flavour=fl, **args))


@pytest.mark.parametrize("which", list(dc.EIGK_PK))
def test_wgr_eigk_settings_decide_alike_in_both_flavours(which):
    from oracle import oracle as O
    X, y = dc.data("mid")
    eig, vark, _ = dc.eigk_case(which)
    args = dict(dc.EIGK_BASE); args.update(dc.EIGK_SETTINGS["BayesB"])
    _same_decisions(lambda fl: O.wgr(y, X, eigK=eig, VarK=vark, flavour=fl, **args))


@pytest.mark.parametrize("tag", dc.KMUP_TAGS)
def test_kmup_inputs_decide_alike_in_both_flavours(tag):
    from oracle import oracle as O
    k = dc.kmup_inputs(tag)
    X = dc.data(tag)[0]
    _same_decisions(lambda fl: O.kmup(X, k["b"], k["d"], k["xx"], k["e"], k["L"], dc.KMUP_VE, 0.3, seed=77, it=3, flavour=fl))


@pytest.mark.parametrize("variant", dc.KMUP2_VARIANTS)
@pytest.mark.parametrize("tag", dc.KMUP2_TAGS)
def test_kmup2_inputs_decide_alike_in_both_flavours(tag, variant):
    from oracle import oracle as O
    k = dc.kmup2_inputs(tag, variant)
    X = dc.data(tag)[0]
    _same_decisions(lambda fl: O.kmup2(X, k["Use"], k["b"], k["d"], k["xx"], k["E"], k["L"], dc.KMUP_VE, 0.3, seed=dc.kmup2_seed(tag, variant), it=4, flavour=fl))


@pytest.mark.parametrize("tag,model", [j for j in dc.CHAIN_JOBS if j[1] in dc.SELECTION])
def test_chain_settings_decide_alike_in_both_flavours(tag, model):
    """... and the strongly causal marker is in the model in every iteration the reference keeps.  The reference keeps it - bi - 1 iterations
    (`i > bi`, src/Rcpp20260726ai.cpp:624) and divides by it - bi (:626), so the largest D it can return is 1 - 1 / (it - bi), not 1: PVAL =
    -log(1 - D) is largest there and stays finite for every whole it and bi."""
    from oracle import oracle as O
    X = dc.data(tag)[0]
    y = dc.chain_y(tag)
    kw = dc.chain_kw(tag, model)
    w = _same_decisions(lambda fl: O.bayes(model, y, X, flavour=fl, **kw))
    mc = kw["it"] - kw["bi"]
    top = np.float32(mc - 1) / np.float32(mc)
    assert w["d"].max() == top and 0 < np.sum(w["d"] == top) < X.shape[1] // 2
    if tag != "wide":      # (with 233 markers per row no single marker is sure of its place)
        assert w["d"][dc.CAUSAL] == top
    if "PVAL" in w:
        assert np.all(np.isfinite(w["PVAL"])) and abs(w["PVAL"].max() - np.log(mc)) < 1e-5 * np.log(mc)


@pytest.mark.parametrize("model,pi,seed", dc.CENTRED_JOBS)
def test_centred_chain_settings_decide_alike_in_both_flavours(model, pi, seed):
    from oracle import oracle as O
    X, y = dc.data("mid")
    Xc = dc.centred_f32(X)
    _same_decisions(lambda fl: O.bayes(model, y, Xc, pi=pi, seed=seed, flavour=fl, **dc.CENTRED_KW))


def test_two_effect_setting_decides_alike_in_both_flavours():
    from oracle import oracle as O
    X1, X2, y = dc.bayes2_inputs()
    _same_decisions(lambda fl: O.bayes2("BayesB2", y, X1, X2, pi=dc.BAYES2_PI, flavour=fl, **dc.BAYES2_KW), keys=("d1", "d2"))


def test_oracle_wgr_with_more_rows_than_the_panel():
    """bag > 1 with replacement: KMUP2 returns n * bag > n residuals (R/wgr.R:88).  The oracle once kept them in a buffer of n (glibc aborted the
    process at free); both flavours must run it and return finite, repeatable lists."""
    from oracle import oracle as O
    X, y = dc.data("mid")
    args = [a for name, _, a in dc.BAG_JOBS if name == "mid-bag_over"][0]
    assert args["bag"] > 1 and args["rp"]
    for fl in ("w", "f"):
        a, b = O.wgr(y, X, flavour=fl, **args), O.wgr(y, X, flavour=fl, **args)
        for k in a:
            assert np.all(np.isfinite(a[k])) and np.array_equal(a[k], b[k]), (fl, k)
