"""CPU: the table of tests/code_cases.py under the library's own host arithmetic (bwgr_debug_panel_plan: no GPU) and the oracle's two flavours.

* Every case reaches the plan it is listed for, with its own largest |x|: a change of a rule that moves a case out of its regime fails here
  instead of silently dropping that regime from tests/test_gpu_codes.py.
* Input selection for the inclusion decisions, as in tests/test_driver_cases_cpu.py: tests/test_gpu_codes.py asserts EQUAL decisions between GPU and
  oracle, so a job is admitted only if the oracle's flavours ("w": double accumulators, "f": the float-faithful restatement) decide alike on it.
  A job that does not gets another seed, never another assertion.
"""
import numpy as np
import pytest

from conftest import scaled_err
import code_cases as cc


@pytest.mark.parametrize("tag", list(cc.CASES))
def test_case_reaches_its_plan(tag):
    pl = cc.plan(tag)
    assert {k: pl[k] for k in cc.EXPECT[tag]} == cc.EXPECT[tag], (tag, pl)


def test_the_generator_gives_the_codes_each_case_is_there_for():
    for tag, c in cc.CASES.items():
        if c["n"] > 1500 and tag != "edge":
            continue      # (tall: as full; over: as edge with a row more)
        X, y = cc.data(tag)
        Xi = X.astype(np.int64)
        assert X.dtype == np.int8 and X.flags.f_contiguous and X.shape == (c["n"], c["p"]) and y.shape == (c["n"],)
        assert int(np.abs(Xi).max()) == cc.XMAX[tag] and Xi.min() == (-128 if c["hold"] else c["lo"])
        for j in c["hold"]:
            assert np.all(X[:, j] == -128)
    xbits = lambda xmax: int(np.ceil(np.log2(max(xmax, 1))))
    assert [xbits(cc.XMAX[t]) for t in ("c15", "c16", "c17", "pm1", "s127", "full", "dos100")] == [4, 4, 5, 0, 7, 7, 7]
    # the 16-bit verdict: every Gram entry in 0 .. 65 535, or not
    for tag in ("c16", "c17", "pm1", "s127", "dos100"):
        Xd = cc.data(tag)[0].astype(np.float64)
        G = Xd.T @ Xd
        assert (G.min() >= 0 and G.max() <= 65535) == bool(cc.GRAM16.get(tag, 0)), (tag, G.min(), G.max())
    assert 200 * 16 * 16 == 51200 and 200 * 17 * 17 == 57800 <= 65535


def test_tall_is_the_largest_sweep3_geometry():
    c = cc.CASES["tall"]
    pl = cc.plan("tall")
    assert (pl["K3"], pl["R3"], pl["fits3"], pl["pipelined"], pl["ld"]) == (249, 256, 1, 1, 63744)
    more = cc.panel_plan(c["n"] + cc.TALL_STEP, c["p"], 128, 0)
    assert (more["K"], more["pipelined"], more["fits3"]) == (250, 0, 0), more      # a slab more: the first engine
    assert cc.panel_plan(c["n"] + cc.TALL_STEP - 1, c["p"], 128, 0)["fits3"] == 1


def test_edge_and_over_sit_either_side_of_the_int32_gram():
    e, o = cc.CASES["edge"], cc.CASES["over"]
    assert e["n"] * 128 * 128 == 2 ** 31 - 16384 and o["n"] * 128 * 128 == 2 ** 31
    X = cc.data("edge")[0]
    g = int((X[:, 0].astype(np.int64) * X[:, 1].astype(np.int64)).sum())
    assert g == 2 ** 31 - 16384 and g == int((X[:, 0].astype(np.int64) ** 2).sum())      # the Gram entries (0, 0), (0, 1), (1, 1)
    Xo, k = cc.kmup2_over_inputs()
    assert Xo.shape[0] * 128 * 128 < 2 ** 31 <= k["Use"].size * 128 * 128 and np.all(Xo[:, 0] == -128)
    assert k["Use"].min() >= 0 and k["Use"].max() < Xo.shape[0]


# ---- input selection: both flavours of the reference take the same decisions --------------------------------------------------------------
def _same_decisions(call):
    w, f = call("w"), call("f")
    assert np.array_equal(w["d"], f["d"]), (int(np.sum(w["d"] != f["d"])), float(np.max(np.abs(w["d"] - f["d"]))))
    if "last" in w:
        assert np.array_equal(w["last"]["d"], f["last"]["d"])
    return w, f


@pytest.mark.parametrize("tag,model", cc.DECIDE_JOBS)
def test_chain_jobs_decide_alike_in_both_flavours(tag, model):
    """... and the flavours lie within the project's 1e-6 of one another on b and hat (1.4e-7 .. 6.7e-7 measured): a bound that means something on
    these inputs."""
    from oracle import oracle as O
    X, y = cc.data(tag)
    w, f = _same_decisions(lambda fl: O.bayes(model, y, X, flavour=fl, **cc.CHAIN_KW))
    assert 0 < w["last"]["d"].sum() < X.shape[1]
    assert scaled_err(f["b"], w["b"]) < 1e-6 and scaled_err(f["hat"], w["hat"]) < 1e-6


@pytest.mark.parametrize("seed", sorted({s for m, s in cc.TALL_JOBS if m in cc.SELECTION}))
def test_tall_jobs_decide_alike_in_both_flavours(seed):
    """37 to 53 markers in the model.  Seeds 21 and 34 decide alike in every iteration.  Seed 33 is kept because it is a listed case, for what
    holds of it: the flavours agree on the chain's state after its three iterations, which is what the GPU is compared on at this size (as
    test_large_n_against_oracle), though they part on marker 30 in the second iteration and meet again in the third.  The float flavour is
    1.5e-6 .. 3.3e-6 from the wide one here, so the GPU is compared with the wide one only."""
    from oracle import oracle as O
    X, y = cc.data("tall")
    if seed in cc.TALL_ALIKE_ON_STATE_ONLY:
        w, f = (O.bayes("BayesB", y, X, seed=seed, flavour=fl, **cc.TALL_KW) for fl in "wf")
        assert np.array_equal(w["last"]["d"], f["last"]["d"])
    else:
        w, _ = _same_decisions(lambda fl: O.bayes("BayesB", y, X, seed=seed, flavour=fl, **cc.TALL_KW))
    assert 30 <= w["last"]["d"].sum() <= 60


@pytest.mark.parametrize("tag,model,pi", cc.CENTRED_JOBS)
def test_centred_jobs_decide_alike_in_both_flavours(tag, model, pi):
    from oracle import oracle as O
    X, y = cc.data(tag)
    Xc = cc.centred_f32(X)
    _same_decisions(lambda fl: O.bayes(model, y, Xc, it=cc.CHAIN_KW["it"], bi=cc.CHAIN_KW["bi"], pi=pi, seed=cc.CENTRED_SEED, flavour=fl))


def test_edge_job_decides_alike_in_both_flavours():
    from oracle import oracle as O
    X, y = cc.data("edge")
    _same_decisions(lambda fl: O.bayes("BayesB", y, X, pi=0.8, flavour=fl, **cc.EDGE_KW))


@pytest.mark.parametrize("tag", cc.KMUP_TAGS)
def test_kmup_inputs_decide_alike_in_both_flavours(tag):
    from oracle import oracle as O
    X = cc.data(tag)[0]
    k = cc.kmup_inputs(tag)
    _same_decisions(lambda fl: O.kmup(X, k["b"], k["d"], k["xx"], k["e"], k["L"], cc.KMUP_VE, 0.3, seed=cc.KMUP_SEED, it=3, flavour=fl))
    for escale in (0.0, 1e-12):
        t = cc.kmup_tiny_inputs(tag, escale)
        _same_decisions(lambda fl: O.kmup(X, t["b"], t["d"], t["xx"], t["e"], t["L"], t["Ve"], 0.3, seed=t["seed"], it=t["it"], flavour=fl))


@pytest.mark.parametrize("zero_e", [False, True])
@pytest.mark.parametrize("variant", ["half", "over"])
@pytest.mark.parametrize("tag", cc.KMUP2_TAGS)
def test_kmup2_inputs_decide_alike_in_both_flavours(tag, variant, zero_e):
    from oracle import oracle as O
    X = cc.data(tag)[0]
    k = cc.kmup2_inputs(tag, variant, zero_e)
    n = X.shape[0]
    assert k["Use"].size == (n // 2 if variant == "half" else n + n // 2) and np.all(np.diff(k["Use"]) >= 0)
    assert (np.unique(k["Use"]).size < k["Use"].size) == (variant == "over")
    _same_decisions(lambda fl: O.kmup2(X, k["Use"], k["b"], k["d"], k["xx"], k["E"], k["L"], cc.KMUP_VE, 0.3, seed=cc.KMUP2_SEED, it=4, flavour=fl))


@pytest.mark.parametrize("name", [k for k, v in cc.WGR_SETTINGS.items() if v.get("pi", 0) > 0])
@pytest.mark.parametrize("tag", cc.WGR_TAGS)
def test_wgr_settings_decide_alike_in_both_flavours(tag, name):
    from oracle import oracle as O
    X, y = cc.data(tag)
    args = dict(cc.WGR_BASE); args.update(cc.WGR_SETTINGS[name])
    _same_decisions(lambda fl: O.wgr(y, X, flavour=fl, **args))
