"""GPU parity of the drivers around the sweep -- wgr (plain, bagged, with a polygenic term, with missing data), KMUP, KMUP2, the chains' return
lists, the EM family, the two-effect samplers, staging and stats -- on multi-slab, multi-chunk panels (tests/driver_cases.py; what regime
each shape is there for is checked without a GPU in tests/test_driver_cases_cpu.py).

Every assertion is the GPU against the oracle's "w" flavour on the same seeded inputs, with the tolerance the existing test of the same entry
point uses (tests/test_gpu_parity.py, test_gpu_parity2.py): TOL = 1e-6 on b, hat, e; 5 * TOL on u, Vb / vb / h2; 1e-12 on wgr's d and cxx;
np.array_equal on the chains' and the sweeps' decisions.  The float panel `flt` inherits the int8 tolerances of each entry point; the one
exception is emBCpi, whose existing float-panel test (test_em_family_other_shapes) already uses 5e-6.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import scaled_err
import driver_cases as dc

pytestmark = pytest.mark.gpu
TOL = 1e-6


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def _ids(jobs):
    return [j[0] for j in jobs]


# ---- wgr ------------------------------------------------------------------------------------------------------------------------------------
def _check_wgr(g, o, extra=()):
    assert list(g.keys()) == list(o.keys()) == ["mu", "b", "Vb", "d", "Ve", "hat"] + list(extra) + ["cxx"]
    err = {"b": scaled_err(g["b"], o["b"]), "hat": scaled_err(g["hat"], o["hat"]), "Vb": scaled_err(np.atleast_1d(g["Vb"]), np.atleast_1d(o["Vb"])),
           "Ve": _rel(g["Ve"], o["Ve"]), "mu": _rel(g["mu"], o["mu"]), "cxx": _rel(g["cxx"], o["cxx"]), "d": scaled_err(g["d"], o["d"])}
    if "u" in extra:
        err["u"] = scaled_err(g["u"], o["u"]); err["Vk"] = _rel(g["Vk"], o["Vk"])
    print("wgr errors:", " ".join("%s=%.2e" % kv for kv in err.items()))
    assert err["b"] < TOL and err["hat"] < TOL, err
    assert err["Vb"] < 5 * TOL, err
    assert err["Ve"] < TOL and err["mu"] < TOL and err["cxx"] < 1e-12, err
    assert err["d"] < 1e-12, err
    if "u" in extra:
        assert err["u"] < 5 * TOL and err["Vk"] < TOL, err


@pytest.mark.parametrize("name,tag,args", dc.WGR_JOBS, ids=_ids(dc.WGR_JOBS))
def test_wgr(name, tag, args, engine_threshold):
    """wgr() rebuilds its residual with the two-stage product every iteration and returns hat from it: two chunks (`mid`, `flt`, `signed` with
    a short last one), 136 chunks and a strided column sum (`wide`), two row workgroups (`flt`), n above one workgroup of 1024 (`mid`, `flt`)."""
    import bwgr_amd
    from oracle import oracle as O
    X, y = dc.data(tag)
    g = bwgr_amd.wgr(y, X, **args, **dc.panel_kw(tag))
    _check_wgr(g, O.wgr(y, X, **args))


@pytest.mark.parametrize("name,tag,args", dc.BAG_JOBS, ids=_ids(dc.BAG_JOBS))
def test_wgr_bagging(name, tag, args):
    """wgr(bag != 1): every iteration gathers sort(sample(n, n * bag, rp)) rows into a scratch panel with its own slab count and (block 16) slab
    height -- through every path of the gather: float, 8 / 3 / 1 columns per workgroup in LDS with a ragged last group, element-wise int8."""
    import bwgr_amd
    from oracle import oracle as O
    X, y = dc.data(tag)
    g = bwgr_amd.wgr(y, X, **args, **dc.panel_kw(tag))
    _check_wgr(g, O.wgr(y, X, **args))


@pytest.mark.parametrize("setting", list(dc.EIGK_SETTINGS))
@pytest.mark.parametrize("which", list(dc.EIGK_PK))
def test_wgr_polygenic_term(which, setting):
    """wgr(eigK=): the eigenvectors are a float panel of n x pk swept each iteration -- four blocks over twelve slabs (pk = 239), one block (36),
    fewer columns than the smallest block (5)."""
    import bwgr_amd
    from oracle import oracle as O
    X, y = dc.data("mid")
    eig, vark, pk = dc.eigk_case(which)
    args = dict(dc.EIGK_BASE); args.update(dc.EIGK_SETTINGS[setting])
    g = bwgr_amd.wgr(y, X, eigK=eig, VarK=vark, **args)
    o = O.wgr(y, X, eigK=eig, VarK=vark, **args)
    assert pk == dc.EIGK_PK[which]
    _check_wgr(g, o, extra=("u", "Vk"))


def test_wgr_missing_phenotypes_and_genotypes():
    """Rows with missing y are dropped on both sides of slab boundaries and still predicted; missing genotypes are mean-imputed first, which
    makes the panel a float one (test_wgr_missing_phenotypes_are_dropped_and_predicted's assertions on `mid`)."""
    import bwgr_amd
    from oracle import oracle as O
    y, X, Xi, keep = dc.missing_case()
    g = bwgr_amd.wgr(y, X, **dc.MISSING_KW)
    o = O.wgr(y[keep], Xi[keep], **dc.MISSING_KW)
    assert scaled_err(g["b"], o["b"]) < TOL and abs(g["mu"] - o["mu"]) <= TOL * max(1.0, abs(o["mu"]))
    assert g["hat"].shape == (y.size,)
    assert scaled_err(g["hat"][keep], o["hat"]) < TOL
    assert scaled_err(g["hat"][~keep], o["mu"] + Xi[~keep] @ o["b"]) < TOL


# ---- KMUP, KMUP2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", [0.0, 0.3])
@pytest.mark.parametrize("tag", dc.KMUP_TAGS)
def test_kmup_sweep(tag, pi, engine_threshold):
    import bwgr_amd
    from oracle import oracle as O
    X = dc.data(tag)[0]
    k = dc.kmup_inputs(tag)
    g = bwgr_amd.KMUP(X, k["b"], k["d"], k["xx"], k["e"], k["L"], dc.KMUP_VE, pi, seed=77, it=3, **dc.panel_kw(tag))
    o = O.kmup(X, k["b"], k["d"], k["xx"], k["e"], k["L"], dc.KMUP_VE, pi, seed=77, it=3)
    print("kmup errors: b=%.2e e=%.2e" % (scaled_err(g["b"], o["b"]), scaled_err(g["e"], o["e"])))
    assert scaled_err(g["b"], o["b"]) < TOL
    assert scaled_err(g["e"], o["e"]) < TOL
    assert np.array_equal(g["d"], o["d"])


@pytest.mark.parametrize("pi", [0.0, 0.3])
@pytest.mark.parametrize("variant", dc.KMUP2_VARIANTS)
@pytest.mark.parametrize("tag", dc.KMUP2_TAGS)
def test_kmup2(tag, variant, pi):
    """KMUP2 on rows in the caller's order (include/bwgr.h): sorted without repeats, with repeats, UNSORTED, more rows than the panel has, and
    nearly all of them (a scratch panel of the base panel's own geometry).  e_out, b, d as test_kmup2_tpod; E is not modified."""
    import bwgr_amd
    from oracle import oracle as O
    X = dc.data(tag)[0]
    k = dc.kmup2_inputs(tag, variant)
    E0 = np.array(k["E"], np.float32)
    E = E0.copy()
    seed = dc.kmup2_seed(tag, variant)
    g = bwgr_amd.KMUP2(X, k["Use"], k["b"], k["d"], k["xx"], E, k["L"], dc.KMUP_VE, pi, seed=seed, it=4, **dc.panel_kw(tag))
    o = O.kmup2(X, k["Use"], k["b"], k["d"], k["xx"], E0, k["L"], dc.KMUP_VE, pi, seed=seed, it=4)
    assert g["e"].shape == (k["Use"].size,)
    print("kmup2 errors: b=%.2e e=%.2e" % (scaled_err(g["b"], o["b"]), scaled_err(g["e"], o["e"])))
    assert scaled_err(g["b"], o["b"]) < TOL and scaled_err(g["e"], o["e"]) < TOL
    assert np.array_equal(g["d"], o["d"])
    assert np.array_equal(E, E0)


# ---- the chains' return lists -----------------------------------------------------------------------------------------------------------
def _check_list(g, o):
    """Every key of the reference's list: names and order, then values."""
    assert list(g.keys()) == [k for k in o.keys() if k != "last"]
    err = {}
    for k in g:
        if k in ("b", "hat", "PVAL"):
            fin = np.isfinite(o[k])
            assert np.array_equal(np.isfinite(g[k]), fin) and np.array_equal(g[k][~fin], o[k][~fin]), k   # infinities (and nothing else) at the same markers
            err[k] = scaled_err(g[k][fin], o[k][fin])
        elif k == "vb":
            err[k] = scaled_err(np.atleast_1d(g[k]), np.atleast_1d(o[k]))
        elif k != "d":
            err[k] = _rel(g[k], o[k])
    print("list errors:", " ".join("%s=%.2e" % kv for kv in err.items()))
    if "d" in g:
        assert np.array_equal(g["d"], o["d"])
    for k, v in err.items():
        bound = {"vb": 5 * TOL, "h2": 5 * TOL, "MSx": 1e-7}.get(k, TOL)     # (MSx: test_panel_stats_tpod's)
        assert v < bound, (k, v, err)


@pytest.mark.parametrize("tag,model", dc.CHAIN_JOBS)
def test_chain_return_list(tag, model):
    """result() of a chain: mu, b, d, hat, vb, ve, h2, MSx or pi and PVAL -- hat through two (`mid`, `signed`, `flt`) and 136 (`wide`) chunks,
    PVAL through k_final_markers, vb's sum through sum_floats -- and a second call, which divides nothing again, returns the same bits.  One
    marker is in the model in every kept iteration: D takes its largest value 1 - 1 / (it - bi) there (the reference keeps one iteration fewer
    than it divides by, so D = 1 and an infinite PVAL cannot occur: tests/test_driver_cases_cpu.py)."""
    import bwgr_amd
    from oracle import oracle as O
    X = dc.data(tag)[0]
    y = dc.chain_y(tag)
    kw = dc.chain_kw(tag, model)
    P = bwgr_amd.Panel(X, **dc.panel_kw(tag))
    try:
        ch = bwgr_amd.Chain(P, model, y, **kw)
        ch.run(kw["it"])
        g = ch.result(); again = ch.result()
        ch.close()
    finally:
        P.close()
    o = O.bayes(model, y, X, **kw)
    for k in g:
        assert np.array_equal(np.asarray(g[k]), np.asarray(again[k])), k
    _check_list(g, o)
    if "d" in g:
        mc = kw["it"] - kw["bi"]
        assert g["d"].max() == np.float32(mc - 1) / np.float32(mc)
        if "PVAL" in g:
            assert np.all(np.isfinite(g["PVAL"])) and int(np.argmax(g["PVAL"])) == int(np.argmax(o["PVAL"]))


@pytest.mark.parametrize("model,pi,seed", dc.CENTRED_JOBS)
def test_centred_chain_return_list(model, pi, seed):
    """An implicitly centred int8 panel against the oracle on the explicitly centred float matrix, as
    test_implicit_centring_is_the_chain_on_the_centred_columns, on `mid`: hat = X B - sum_j mean_j B_j over two chunks."""
    import bwgr_amd
    from oracle import oracle as O
    X, y = dc.data("mid")
    Xc = dc.centred_f32(X)
    kw = dict(dc.CENTRED_KW, pi=pi, seed=seed)
    P = bwgr_amd.Panel(X).set_centred(True)
    try:
        assert P.centred()
        xx, vx, msx = P.stats()
        oxx, ovx, omsx = O.stats(Xc)
        assert scaled_err(xx, oxx) < 2e-7 and _rel(msx, omsx) < 1e-6
        ch = bwgr_amd.Chain(P, model, y, **kw)
        ch.run(kw["it"])
        g = ch.result(); st = ch.state()
        ch.close()
    finally:
        P.close()
    o = O.bayes(model, y, Xc, **kw)
    assert np.array_equal(g["d"], o["d"]) and np.array_equal(st["d"], o["last"]["d"])
    assert scaled_err(g["b"], o["b"]) < TOL and scaled_err(g["hat"], o["hat"]) < TOL
    assert _rel(g["ve"], o["ve"]) < TOL and abs(float(g["mu"]) - float(o["mu"])) < TOL * max(abs(float(o["mu"])), float(np.std(y)))
    assert scaled_err(st["e"], o["last"]["e"]) < TOL and scaled_err(st["b"], o["last"]["b"]) < TOL
    assert _rel(g["h2"], o["h2"]) < 5 * TOL and scaled_err(np.atleast_1d(g["vb"]), np.atleast_1d(o["vb"])) < 5 * TOL


# ---- the EM family --------------------------------------------------------------------------------------------------------------------------
def _em_check(model, got, ref, tol=TOL):
    assert list(got) == [k for k in ref if k != "iters"], (model, list(got))
    for k in got:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        if g.ndim:
            assert scaled_err(g, r) < tol, (model, k, scaled_err(g, r))
        else:
            assert _rel(g, r) < 10 * tol, (model, k, float(g), float(r))


@pytest.mark.parametrize("model,maxit", [("emRR", 25), ("emBC", 25), ("emEN", 25), ("lasso", 25), ("emDE", 25), ("emRR", 0)])
def test_em_family_mid(model, maxit):
    """bwgr_em on six slabs: the shuffled copy (k_permute_cols moves 16-byte pieces per slab), its scratch panel, hat through two chunks;
    maxit = 0: the reference's default length with its convergence test."""
    import bwgr_amd
    from oracle import oracle as O
    X, y = dc.data("mid")
    y = y.astype(np.float32)
    _em_check(model, getattr(bwgr_amd, model)(y, X, maxit=maxit), O.em(model, y, X, maxit=maxit))


@pytest.mark.parametrize("model", ["emRR", "emBCpi"])
def test_em_family_flt(model):
    """... and on the float panel (eleven slabs of 128): emBCpi at the 5e-6 test_em_family_other_shapes uses for it on a float panel; emRR has no
    float-panel test yet, so it keeps its only existing bound, TOL."""
    import bwgr_amd
    from oracle import oracle as O
    X, y = dc.data("flt")
    y = y.astype(np.float32)
    _em_check(model, getattr(bwgr_amd, model)(y, X, maxit=25, as_int8=False), O.em(model, y, X, maxit=25), tol=5e-6 if model == "emBCpi" else TOL)


# ---- two-effect samplers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["BayesA2", "BayesB2", "BayesRR2"])
def test_two_effect_samplers(model):
    """test_two_effect_samplers' assertions with `mid`'s genotypes as X1 (int8) and 200 float columns as X2: hat = X1 b1 + X2 b2 + mu over
    two panels of different type, the first with two chunks."""
    import bwgr_amd
    from oracle import oracle as O
    X1, X2, y = dc.bayes2_inputs()
    kw = dict(dc.BAYES2_KW)
    if model == "BayesB2":
        kw["pi"] = dc.BAYES2_PI
    g = getattr(bwgr_amd, model)(y, X1, X2, block=64, **kw)
    o = O.bayes2(model, y, X1, X2, **kw)
    assert list(g.keys()) == [k for k in o.keys() if k != "last"]
    for k in ("b1", "b2", "hat"):
        assert scaled_err(g[k], o[k]) < TOL, k
    for k in ("mu", "ve", "h2"):
        assert abs(g[k] - o[k]) <= TOL * max(1.0, abs(o[k])), k
    if model == "BayesRR2":
        assert abs(g["vb1"] - o["vb1"]) <= TOL * abs(o["vb1"]) and abs(g["vb2"] - o["vb2"]) <= TOL * abs(o["vb2"])
    else:
        assert scaled_err(g["vb1"], o["vb1"]) < TOL and scaled_err(g["vb2"], o["vb2"]) < TOL
    if model == "BayesB2":
        assert np.array_equal(g["d1"], o["d1"]) and np.array_equal(g["d2"], o["d2"])


# ---- staging and stats ------------------------------------------------------------------------------------------------------------------
def _raw_panel(ptr, xtype, memloc, n, p, ldx, block=0):
    """bwgr_panel_create through ctypes (bwgr_amd.Panel always passes ldx = n for a host matrix)."""
    from bwgr_amd import _lib, api
    P = api.Panel.__new__(api.Panel)
    P._h = C.c_void_p(); P._keep = None
    _lib.check(_lib.lib().bwgr_panel_create(C.byref(P._h), ptr, xtype, memloc, n, p, ldx, 0, block, 0))
    info = (C.c_int64 * 8)()
    _lib.check(_lib.lib().bwgr_panel_info(P._h, info))
    P.n, P.p, P.ld, P.block, P.nwg, P.slab_rows, P.x_bytes, P.gram_bytes = [int(v) for v in info]
    P.device = 0
    return P


def _stats_and_state(P, y):
    import bwgr_amd
    xx, vx, msx = P.stats()
    ch = bwgr_amd.Chain(P, "BayesB", y, it=3, bi=0, pi=0.8, seed=8)
    ch.run(3)
    st = ch.state()
    ch.close()
    return xx, vx, msx, st


@pytest.mark.parametrize("source", ["host_i8", "host_f32", "host_f64", "device_i8", "device_f32"])
def test_staging_with_a_leading_dimension_beyond_n(source):
    """bwgr_panel_create from a matrix whose columns are ldx = n + 7 apart, the seven rows between them full of garbage: the panel's stats and a
    three-iteration BayesB state are bit for bit the contiguous panel's (k_convert must zero from row n on, not copy)."""
    import bwgr_amd
    from bwgr_amd import api
    tag = "mid" if source.endswith("i8") else "flt"
    X, y = dc.data(tag)
    n, p = X.shape
    dtype = {"i8": np.int8, "f32": np.float32, "f64": np.float64}[source.split("_")[1]]
    xtype = {"i8": api.X_I8, "f32": api.X_F32, "f64": api.X_F64}[source.split("_")[1]]
    ldx = n + 7
    padded = np.full((p, ldx), 99 if dtype == np.int8 else 77.25, dtype)     # row j = column j of X, then garbage
    padded[:, :n] = X.T.astype(dtype)
    ref = bwgr_amd.Panel(X.astype(dtype), as_int8=(dtype == np.int8))
    try:
        want = _stats_and_state(ref, y)
    finally:
        ref.close()
    if source.startswith("host"):
        flat = padded.reshape(-1)[:(p - 1) * ldx + n].copy()      # the last column may end at row n (include/bwgr.h)
        P = _raw_panel(flat.ctypes.data_as(C.c_void_p), xtype, api.HOST, n, p, ldx)
    else:
        import torch
        t = torch.from_numpy(padded).cuda()
        torch.cuda.synchronize()
        P = _raw_panel(C.c_void_p(t.data_ptr()), xtype, api.DEVICE, n, p, ldx)
    try:
        assert (P.ld, P.block, P.nwg, P.slab_rows) == (ref.ld, ref.block, ref.nwg, ref.slab_rows)
        got = _stats_and_state(P, y)
    finally:
        P.close()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    for k in ("b", "d", "e", "vb"):
        assert np.array_equal(got[3][k], want[3][k]), k
    assert got[3]["ve"] == want[3]["ve"] and got[3]["mu"] == want[3]["mu"]


@pytest.mark.parametrize("tag", ["mid", "signed", "flt", "tall40k"])
def test_panel_stats(tag):
    """xx, vx, MSx against the oracle as test_panel_stats_tpod: integer sums of squares exact on int8; k_stats over several slabs."""
    import bwgr_amd
    from oracle import oracle as O
    X = dc.data(tag)[0]
    P = bwgr_amd.Panel(X, **dc.panel_kw(tag))
    try:
        xx, vx, msx = P.stats()
    finally:
        P.close()
    oxx, ovx, omsx = O.stats(X)
    if dc.CASES[tag]["f32"]:
        assert scaled_err(xx, oxx) < 2e-7      # (float columns: test_implicit_centring_is_the_chain_on_the_centred_columns' bound on their norms)
    else:
        assert np.array_equal(xx, oxx)
    assert scaled_err(vx, ovx) < 1e-7
    assert _rel(msx, omsx) < 1e-7
