"""GPU: the samplers on int8 codes beyond 0/1/2 -- 0..16, 0..17, dosage x 100, -1..1, -127..127, the whole byte range -- and the int32 Gram bound
(tests/code_cases.py; which plan each case reaches, and that the oracle decides every selection job alike in both flavours, is checked without a
GPU in tests/test_code_cases_cpu.py).

A panel's largest |x| sizes the fixed-point grid of k_sweep3 / k_sweep3f / k_sweep3p and of k_sweep2w's fixed-point streamers (k_escale), and the size
and sign of its Gram entries pick the uint16 or int32 staging and the affine sweeps' engine; the rest of the suite runs all of that at |x| <= 2.

Every comparison is the GPU against the oracle's "w" flavour on the same seeded inputs at the tolerances tests/test_gpu_parity*.py use: TOL = 1e-6
through scaled_err on vectors and _rel on scalars, np.array_equal on the decisions.  Each test prints what it measured (engine, Gram bits, kernel,
redo count, largest error) in a line that starts with "codes:".
"""
import ctypes as C

import numpy as np
import pytest

from conftest import scaled_err
import code_cases as cc

pytestmark = pytest.mark.gpu
TOL = 1e-6
GENERIC, FIXED = 1, 2      # bwgr_debug_sweep3_kernel


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def _which(P):
    from bwgr_amd import _lib
    w = C.c_int(-1)
    _lib.check(_lib.lib().bwgr_debug_sweep3_kernel(P._h, C.byref(w)))
    return w.value


def _run(X, y, model, kw, centred=False):
    """One chain on a fresh panel: what the panel reports, the chain's state and result, its redo count."""
    import bwgr_amd
    P = bwgr_amd.Panel(X)
    try:
        if centred:
            P.set_centred(True)
        info = {"sel": P.pipeline(True), "aff": P.pipeline(False), "which": _which(P), "stats": P.stats() if centred else None}
        ch = bwgr_amd.Chain(P, model, y, **kw)
        try:
            ch.run(kw["it"])
            info["state"], info["result"], info["nredo"] = ch.state(), ch.result(), ch.redo_count()
        finally:
            ch.close()
    finally:
        P.close()
    return info


def _check_chain(what, model, info, o, mu_scale=None):
    """State (b, e, ve, d) and result (b, hat, mu[, d]) against the oracle's; returns the largest error."""
    st, g, ol = info["state"], info["result"], o["last"]
    err = {"st.b": scaled_err(st["b"], ol["b"]), "st.e": scaled_err(st["e"], ol["e"]), "st.ve": _rel(st["ve"], ol["ve"]),
           "b": scaled_err(g["b"], o["b"]), "hat": scaled_err(g["hat"], o["hat"]),
           "mu": _rel(g["mu"], o["mu"]) if mu_scale is None else abs(float(g["mu"]) - float(o["mu"])) / mu_scale}
    gen = info["sel" if model in cc.SELECTION else "aff"]
    print("codes: %s %s generation=%d lag=%d gram_bits=%d kernel=%d nredo=%d max_err=%.2e (%s)" % (
        what, model, gen["generation"], gen["lag"], gen["gram_bits"], info["which"], info["nredo"], max(err.values()),
        " ".join("%s=%.1e" % kv for kv in err.items())))
    if model in cc.SELECTION:
        assert np.array_equal(st["d"], ol["d"]) and np.array_equal(g["d"], o["d"])
    for k, v in err.items():
        assert v < TOL, (what, model, k, v, err)
    return max(err.values())


def _check_pipeline(tag, info, env):
    """What Panel.pipeline() must report for the case under these switches."""
    sel, aff = info["sel"], info["aff"]
    if env.get("BWGR_SWEEP") == "1":
        assert sel["generation"] == 1 and aff["generation"] == 1
        return
    bits = 16 if tag in ("c15", "c16", "c17") else 32      # (dos100: entries beyond 65 535; the rest: negative entries)
    assert sel["gram_bits"] == bits and aff["gram_bits"] == bits, (tag, sel, aff)
    assert sel["generation"] == (2 if env.get("BWGR_SWEEP") == "2" else 3), (tag, sel)
    assert aff["generation"] == (4 if bits == 16 and env.get("BWGR_WINV") != "0" else 2), (tag, aff)


# ---- chains -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", cc.ALL_MODELS)
@pytest.mark.parametrize("tag", cc.CHAIN_TAGS)
def test_chains(tag, model, engine_threshold):
    """The seven samplers, eight iterations, under both engine gates: k_sweep3 (k_sweep3f on c16 / c17) and, at the shipped gate, k_sweep2 for the
    sweeps above 3 % inclusion; k_sweep2w for the affine models on c16 / c17, k_sweep2 on the signed cases and dos100.  The largest |x| exists to
    keep an ordinary chain inside the fixed-point range: no sweep is redone."""
    X, y = cc.data(tag)
    info = _run(X, y, model, cc.CHAIN_KW)
    _check_pipeline(tag, info, {})
    if tag in ("c16", "c17"):
        assert info["which"] == FIXED
    _check_chain("%s[%s]" % (tag, engine_threshold), model, info, cc.oracle_chain(tag, model, **cc.CHAIN_KW))
    assert info["nredo"] == 0


# (BWGR_WINV switches the affine sweeps' sequencer only)
OTHER_ENGINES = [(tag, model, env) for tag in cc.CHAIN_TAGS for model in cc.ALL_MODELS for env in ({"BWGR_SWEEP": "2"}, {"BWGR_SWEEP": "1"}, {"BWGR_WINV": "0"})
                 if "BWGR_WINV" not in env or model not in cc.SELECTION]


@pytest.mark.parametrize("tag,model,env", OTHER_ENGINES, ids=["%s-%s-%s" % (t, m, "-".join("%s=%s" % kv for kv in e.items())) for t, m, e in OTHER_ENGINES])
def test_chains_on_the_other_engines(tag, model, env, monkeypatch):
    """The same chains on k_sweep2 (BWGR_SWEEP=2: 16-bit staging on c16 / c17, the generic sequencer elsewhere), on the first engine k_sweep
    (BWGR_SWEEP=1) and, for the affine models, on the serial sequencer (BWGR_WINV=0)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    X, y = cc.data(tag)
    info = _run(X, y, model, cc.CHAIN_KW)
    _check_pipeline(tag, info, env)
    _check_chain("%s[%s]" % (tag, ",".join("%s=%s" % kv for kv in env.items())), model, info, cc.oracle_chain(tag, model, **cc.CHAIN_KW))
    assert info["nredo"] == 0


@pytest.mark.parametrize("model", ["BayesB", "BayesC", "BayesDpi"])
def test_c17_runs_the_fixed_kernel_and_the_generic_one_to_the_same_bits(model, monkeypatch):
    """0..17: the largest codes at which 200 rows still give 16-bit Gram entries, so k_sweep3f as shipped and k_sweep3<uint16_t> with BWGR_FIXED3=0."""
    X, y = cc.data("c17")
    monkeypatch.delenv("BWGR_FIXED3", raising=False)
    f = _run(X, y, model, cc.CHAIN_KW)
    monkeypatch.setenv("BWGR_FIXED3", "0")
    g = _run(X, y, model, cc.CHAIN_KW)
    assert (f["which"], g["which"]) == (FIXED, GENERIC) and f["sel"] == g["sel"] and f["sel"]["generation"] == 3 and f["sel"]["gram_bits"] == 16
    for part in ("state", "result"):
        for k in f[part]:
            assert np.array_equal(np.asarray(f[part][k]), np.asarray(g[part][k])), (part, k)
    assert f["nredo"] == 0 and g["nredo"] == 0


@pytest.mark.parametrize("model,seed", cc.TALL_JOBS)
def test_tall(model, seed):
    """63 700 x 260 on the whole byte range with a column held at -128: 249 streamers of 256 rows plus sequencer and prefetcher, the largest
    geometry k_sweep3 takes (45 rows more and the panel is the first engine's), int32 staging; the affine model's sweeps are k_sweep2's on 249
    slabs.  Compared on the chain's state, as test_large_n_against_oracle.  (n = 63 700 as listed: the occupancy guard accepts the launch.)"""
    X, y = cc.data("tall")
    kw = dict(cc.TALL_KW, seed=seed)
    import bwgr_amd
    from oracle import oracle as O
    P = bwgr_amd.Panel(X)
    try:
        sel, aff = P.pipeline(True), P.pipeline(False)
        assert P.nwg == 249 and sel["generation"] == 3 and sel["gram_bits"] == 32 and aff["generation"] == 2, (P.nwg, sel, aff)
        ch = bwgr_amd.Chain(P, model, y, **kw)
        try:
            ch.run(kw["it"])
            st, nredo = ch.state(), ch.redo_count()
        finally:
            ch.close()
    finally:
        P.close()
    o = O.bayes(model, y, X, **kw)["last"]
    err = {"b": scaled_err(st["b"], o["b"]), "e": scaled_err(st["e"], o["e"]), "ve": _rel(st["ve"], o["ve"])}
    print("codes: tall %s seed=%d generation=%d gram_bits=%d nredo=%d max_err=%.2e" % (model, seed, (sel if model in cc.SELECTION else aff)["generation"],
                                                                                       sel["gram_bits"], nredo, max(err.values())))
    if model in cc.SELECTION:
        assert np.array_equal(st["d"], o["d"])
    assert max(err.values()) < TOL, err
    assert nredo == 0


# ---- range recovery ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,model", cc.REDO_JOBS)
def test_a_sweep_that_leaves_the_range_is_redone_on_large_codes(tag, model, monkeypatch):
    """test_a_sweep_that_leaves_the_fixed_point_range_is_redone on codes up to 17 and +-127: with fourteen bits less headroom every sweep of a
    fixed-point engine (k_sweep3; k_sweep2w's fixed-point streamers, which serve the affine models on c17) leaves its range and is redone on
    the fp64 residual; the chain is still the oracle's.  On s127 the affine sweeps are k_sweep2's (negative Gram entries): fp64 throughout, no
    range to leave, so nothing is redone there."""
    monkeypatch.setenv("BWGR_DEBUG_SH_ADD", "14")
    X, y = cc.data(tag)
    info = _run(X, y, model, cc.CHAIN_KW)
    gen = info["sel" if model in cc.SELECTION else "aff"]["generation"]
    assert gen == (3 if model in cc.SELECTION else 4 if tag == "c17" else 2)
    _check_chain("%s[sh_add=14]" % tag, model, info, cc.oracle_chain(tag, model, **cc.CHAIN_KW))
    want = cc.CHAIN_KW["it"] if gen in (3, 4) else 0
    assert info["nredo"] == want, "every sweep of a fixed-point engine was meant to leave the range and be redone (%d of %d were)" % (info["nredo"], want)


# ---- KMUP, KMUP2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", [0.0, 0.3])
@pytest.mark.parametrize("residual", ["tpod", 0.0, 1e-12])
@pytest.mark.parametrize("tag", cc.KMUP_TAGS)
def test_kmup(tag, residual, pi, engine_threshold):
    """One sweep with the residual of test_kmup_sweep_tpod, and with test_kmup_with_a_zero_or_tiny_residual's: there the grid is sized by the
    steps times the largest |x| alone."""
    import bwgr_amd
    from oracle import oracle as O
    X = cc.data(tag)[0]
    if residual == "tpod":
        k = dict(cc.kmup_inputs(tag), Ve=cc.KMUP_VE, seed=cc.KMUP_SEED, it=3)
    else:
        k = cc.kmup_tiny_inputs(tag, residual)
    g = bwgr_amd.KMUP(X, k["b"], k["d"], k["xx"], k["e"], k["L"], k["Ve"], pi, seed=k["seed"], it=k["it"])
    nredo = cc.last_redo()
    o = O.kmup(X, k["b"], k["d"], k["xx"], k["e"], k["L"], k["Ve"], pi, seed=k["seed"], it=k["it"])
    eb, ee = scaled_err(g["b"], o["b"]), scaled_err(g["e"], o["e"])
    print("codes: kmup %s residual=%s pi=%g [%s] nredo=%d max_err=%.2e" % (tag, residual, pi, engine_threshold, nredo, max(eb, ee)))
    assert eb < TOL and ee < TOL
    assert np.array_equal(g["d"], o["d"])
    assert nredo == 0      # (the grid is sized for the steps times the panel's largest |x|: the sweep stays in range)


@pytest.mark.parametrize("pi", [0.0, 0.3])
@pytest.mark.parametrize("zero_e", [False, True], ids=["E", "E0"])
@pytest.mark.parametrize("variant", ["half", "over"])
@pytest.mark.parametrize("tag", cc.KMUP2_TAGS)
def test_kmup2(tag, variant, zero_e, pi):
    """KMUP2 sweeps a row-subset scratch panel -- half the rows, and one and a half times the rows with repeats -- which carries its parent's
    largest |x|: the fixed-point streamers of the affine sweeps on c17 run on the main panel's grid."""
    import bwgr_amd
    from oracle import oracle as O
    X = cc.data(tag)[0]
    k = cc.kmup2_inputs(tag, variant, zero_e)
    E0 = np.array(k["E"], np.float32)
    E = E0.copy()
    g = bwgr_amd.KMUP2(X, k["Use"], k["b"], k["d"], k["xx"], E, k["L"], cc.KMUP_VE, pi, seed=cc.KMUP2_SEED, it=4)
    nredo = cc.last_redo()
    o = O.kmup2(X, k["Use"], k["b"], k["d"], k["xx"], E0, k["L"], cc.KMUP_VE, pi, seed=cc.KMUP2_SEED, it=4)
    assert g["e"].shape == (k["Use"].size,)
    eb, ee = scaled_err(g["b"], o["b"]), scaled_err(g["e"], o["e"])
    print("codes: kmup2 %s %s E0=%d pi=%g nredo=%d max_err=%.2e" % (tag, variant, zero_e, pi, nredo, max(eb, ee)))
    assert eb < TOL and ee < TOL
    assert np.array_equal(g["d"], o["d"])
    assert np.array_equal(E, E0)
    assert nredo == 0      # (the scratch panel sweeps on its parent's grid)


# ---- wgr, the EM family -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.WGR_SETTINGS))
@pytest.mark.parametrize("tag", cc.WGR_TAGS)
def test_wgr(tag, name):
    """test_gpu_drivers.py's assertions: plain, with selection, and bagged -- half the rows, and one and a half times the rows with replacement,
    a scratch panel refilled every iteration."""
    import bwgr_amd
    from oracle import oracle as O
    X, y = cc.data(tag)
    args = dict(cc.WGR_BASE); args.update(cc.WGR_SETTINGS[name])
    g = bwgr_amd.wgr(y, X, **args)
    nredo = cc.last_redo()
    o = O.wgr(y, X, **args)
    assert list(g.keys()) == list(o.keys()) == ["mu", "b", "Vb", "d", "Ve", "hat", "cxx"]
    err = {"b": scaled_err(g["b"], o["b"]), "hat": scaled_err(g["hat"], o["hat"]), "Vb": scaled_err(np.atleast_1d(g["Vb"]), np.atleast_1d(o["Vb"])),
           "Ve": _rel(g["Ve"], o["Ve"]), "mu": _rel(g["mu"], o["mu"]), "cxx": _rel(g["cxx"], o["cxx"]), "d": scaled_err(g["d"], o["d"])}
    print("codes: wgr %s %s nredo=%d max_err=%.2e (%s)" % (tag, name, nredo, max(err.values()), " ".join("%s=%.1e" % kv for kv in err.items())))
    assert nredo == 0
    assert err["b"] < TOL and err["hat"] < TOL, err
    assert err["Vb"] < 5 * TOL, err
    assert err["Ve"] < TOL and err["mu"] < TOL and err["cxx"] < 1e-12, err
    assert err["d"] < 1e-12, err


@pytest.mark.parametrize("model", cc.EM_MODELS)
@pytest.mark.parametrize("tag", cc.EM_TAGS)
def test_em_family(tag, model):
    """test_em_family_matches_oracle's runs (seven sweeps, and the default length with the convergence test): the shuffled copy is a scratch panel too."""
    import bwgr_amd
    from oracle import oracle as O
    X = cc.data(tag)[0]
    y = cc.em_y(tag)
    worst = 0.0
    P = bwgr_amd.Panel(X)
    try:
        for maxit in (7, 0):
            got = getattr(bwgr_amd, model)(y, P, maxit=maxit)
            ref = O.em(model, y, X, maxit=maxit)
            assert list(got) == [k for k in ref if k != "iters"], (model, list(got))
            for k in got:
                g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
                assert np.all(np.isfinite(r)), (model, k)
                e = scaled_err(g, r) if g.ndim else _rel(g, r) / 10
                worst = max(worst, e)
                assert e < TOL, (model, maxit, k, e)      # (scalars at 10 * TOL, as _em_check)
    finally:
        P.close()
    print("codes: em %s %s max_err=%.2e" % (tag, model, worst))


# ---- implicit centring ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,model,pi", cc.CENTRED_JOBS)
def test_implicit_centring(tag, model, pi, engine_threshold):
    """test_implicit_centring_is_the_chain_on_the_centred_columns with column sums up to 1.5e5 and sums of squares up to 1.5e7: against the oracle
    on the explicitly centred float matrix."""
    from oracle import oracle as O
    X, y = cc.data(tag)
    kw = dict(it=cc.CHAIN_KW["it"], bi=cc.CHAIN_KW["bi"], pi=pi, seed=cc.CENTRED_SEED)
    info = _run(X, y, model, kw, centred=True)
    xx, vx, msx = info["stats"]
    oxx, ovx, omsx = O.stats(cc.centred_f32(X))
    assert scaled_err(xx, oxx) < 2e-7 and _rel(msx, omsx) < 1e-6
    assert info["sel"]["generation"] == 3
    o = cc.oracle_centred_chain(tag, model, pi)
    # (on centred columns the intercept is the mean of y: compared on the scale of y, as the test this mirrors does)
    _check_chain("%s[centred,%s]" % (tag, engine_threshold), model, info, o, mu_scale=max(abs(float(o["mu"])), float(np.std(y))))
    assert info["nredo"] == 0


# ---- pairs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", cc.PAIR_TAGS)
def test_pairs(tag, monkeypatch):
    """bwgr_chain_run_pair (k_sweep3p, the other digit split of the slab-dot words): BayesB and BayesC on one set of streamers are, bit for bit,
    the chains they are alone."""
    import bwgr_amd
    monkeypatch.setenv("BWGR_ENG3_THR", "1")
    X, y = cc.data(tag)
    it = cc.CHAIN_KW["it"]
    P = bwgr_amd.Panel(X)
    Q = P.clone()
    try:
        solo = []
        for h, mdl, seed in ((P, "BayesB", 3), (Q, "BayesC", 4)):
            ch = bwgr_amd.Chain(h, mdl, y, **dict(cc.CHAIN_KW, seed=seed))
            ch.run(it)
            solo.append(ch.state()); ch.close()
        c0 = bwgr_amd.Chain(P, "BayesB", y, **dict(cc.CHAIN_KW, seed=3))
        c1 = bwgr_amd.Chain(Q, "BayesC", y, **dict(cc.CHAIN_KW, seed=4))
        try:
            c0.run_pair(c1, it)
            s0, s1 = c0.state(), c1.state()
        finally:
            c0.close(); c1.close()
    finally:
        Q.close(); P.close()
    for got, want in ((s0, solo[0]), (s1, solo[1])):
        assert np.array_equal(got["d"], want["d"]) and np.array_equal(got["b"], want["b"]) and np.array_equal(got["e"], want["e"])
        assert got["ve"] == want["ve"]
    assert 0 < s0["d"].sum() < X.shape[1]


# ---- stats, and the int32 Gram bound ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["full", "edge"])
def test_stats(tag):
    """xx, vx, MSx as test_panel_stats_tpod; on `edge` two columns' sums of squares are 2^31 - 16 384."""
    import bwgr_amd
    from oracle import oracle as O
    X = cc.data(tag)[0]
    P = bwgr_amd.Panel(X)
    try:
        xx, vx, msx = P.stats()
    finally:
        P.close()
    oxx, ovx, omsx = O.stats(X)
    assert np.array_equal(xx, oxx)
    if tag == "edge":
        assert xx[0] == xx[1] == np.float32(2 ** 31 - 16384)
    assert scaled_err(vx, ovx) < 1e-7
    assert _rel(msx, omsx) < 1e-7


@pytest.mark.parametrize("model,pi", cc.EDGE_JOBS)
def test_the_last_panel_the_int32_gram_holds(model, pi):
    """131 071 rows with two columns held at -128: the Gram entries (0, 0), (0, 1), (1, 1) are 2^31 - 16 384, the largest an int8 panel may have."""
    X, y = cc.data("edge")
    kw = dict(cc.EDGE_KW, pi=pi)
    info = _run(X, y, model, kw)
    assert info["sel"]["gram_bits"] == 32 and info["sel"]["generation"] == 2 and info["aff"]["generation"] == 2      # (32-marker blocks: no k_sweep3)
    _check_chain("edge", model, info, cc.oracle_chain("edge", model, **kw))
    assert info["nredo"] == 0


def test_a_panel_beyond_the_int32_gram_is_refused():
    """One row more: n * max|x|^2 = 2^31.  Refused on the host with BWGR_EINVAL; the device is left usable."""
    import bwgr_amd
    from oracle import oracle as O
    X = cc.data("over")[0]
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.Panel(X)
    assert ei.value.code == 1 and "int32 Gram" in str(ei.value)
    Xs = cc.data("c17")[0]
    P = bwgr_amd.Panel(Xs)
    try:
        assert np.array_equal(P.stats()[0], O.stats(Xs)[0])
    finally:
        P.close()


def test_kmup2_on_more_rows_than_the_int32_gram_holds_is_refused():
    """A scratch panel may have more rows than its parent: 140 000 repeated rows of a 70 000-row panel with a column at -128 are refused the same
    way (the parent itself is within the bound)."""
    import bwgr_amd
    from oracle import oracle as O
    X, k = cc.kmup2_over_inputs()
    n = X.shape[0]
    P = bwgr_amd.Panel(X)
    try:
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            bwgr_amd.KMUP2(P, k["Use"], k["b"], k["d"], k["xx"] * (k["Use"].size / n), k["E"], k["L"], cc.KMUP_VE, 0.0, seed=cc.KMUP2_SEED, it=4)
        assert ei.value.code == 1 and "int32 Gram" in str(ei.value)
        half = k["Use"][::2]      # ... and a subsample within the bound -- as many rows as the panel has -- goes through on the same panel
        assert half.size == n and np.unique(half).size < n
        g = bwgr_amd.KMUP2(P, half, k["b"], k["d"], k["xx"], k["E"], k["L"], cc.KMUP_VE, 0.0, seed=cc.KMUP2_SEED, it=4)
    finally:
        P.close()
    o = O.kmup2(X, half, k["b"], k["d"], k["xx"], k["E"], k["L"], cc.KMUP_VE, 0.0, seed=cc.KMUP2_SEED, it=4)
    assert scaled_err(g["b"], o["b"]) < TOL and scaled_err(g["e"], o["e"]) < TOL
