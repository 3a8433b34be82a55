"""CPU: the tests' numpy restatement of solver2x / MEGA / GSEM (tests/sem2_restatement.py) pinned by the properties it must have, the
preconditions of the GPU cases (tests/sem2_cases.py) asserted on it, and the public surface of the two-design entries."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrr_restatement as MR  # noqa: E402
import sem2_cases as C  # noqa: E402
import sem2_restatement as S2  # noqa: E402
import uvb_restatement as UR  # noqa: E402

E = inspect.Parameter.empty
MEGA_KEYS = ("mu", "b", "hat", "LS", "LS_BETA", "BETA1", "BETA2", "gebv")
GSEM_KEYS = ("mu", "b", "hat")


def _small(seed=5, p=40, q=3):
    X = C.tpod()[:, :p].astype(np.float64)
    Y = C.traits(C.tpod(), 1, 0.2, seed)[:, 0]
    w = ~np.isnan(Y)
    return Y[w], C.dense(196, q, seed + 1)[w], X[w]


# ---- the restatement ----
def test_solver2x_reaches_the_ridge_solution_of_the_stacked_design():
    """Fixed lambdas, far past convergence: Gauss-Seidel's fixed point is the solution of ([Z X]c'[Z X]c + diag(lambda_1 I, lambda_2 I)) b
    = [Z X]c'y on the rows given, both designs centred by their means over those rows.  This pins the yardstick, not the feature."""
    Y, Z, X = _small()
    lam = (3.0, 40.0)
    r = S2.solver2x(Y, Z, X, maxit=4000, tol=1e-30, lam=lam)
    W = np.hstack([Z - Z.mean(0), X - X.mean(0)])
    D = np.diag([lam[0]] * Z.shape[1] + [lam[1]] * X.shape[1])
    b = np.linalg.solve(W.T @ W + D, W.T @ (Y - Y.mean()))
    assert r["its"] < 4000 and MR.scaled_err(np.concatenate([r["b1"], r["b2"]]), b) <= 1e-9
    assert abs(r["mu"] - Y.mean()) <= 1e-9 * abs(Y.mean())          # the designs are centred: the intercept is the mean


def test_a_dense_design_constant_on_the_rows_leaves_solver1x():
    """Departure 2: with TrXSX1 = 0 the dense design is skipped and the panel runs as if alone -- bit for bit uvb_restatement's solver D."""
    Y, Z, X = _small(seed=9)
    Z[:] = np.array([0.5, -1.25, 2.0])
    for kw in (dict(maxit=5, tol=0), dict()):
        r, o = S2.solver2x(Y, Z, X, **kw), UR.solver(Y, X, "D", **kw)
        assert np.array_equal(r["b2"], o["b"]) and r["mu"] == o["mu"] and r["trace"] == o["trace"] and r["its"] == o["its"]
        assert not r["b1"].any() and np.isnan(r["vb1"]) and np.isnan(r["lam1"]) and r["vb2"] == o["vb"] and r["ve"] == o["ve"]
    Xc = np.ones_like(X)                                            # and the other way round: the panel constant, the dense design alone
    r, o = S2.solver2x(Y, Z + C.dense(Y.shape[0], 3, 1), Xc, maxit=5, tol=0), UR.solver(Y, Z + C.dense(Y.shape[0], 3, 1), "D", maxit=5, tol=0)
    assert np.array_equal(r["b1"], o["b"]) and r["mu"] == o["mu"] and not r["b2"].any() and np.isnan(r["vb2"])


def test_a_column_with_xx_zero_gets_exactly_zero():
    Y, Z, X = _small(seed=13)
    Z[:, 1] = 0.75
    X[:, 7] = 2.0
    r = S2.solver2x(Y, Z, X, maxit=4, tol=0)
    assert r["XX1"][1] == 0 and r["b1"][1] == 0 and r["b1"][0] != 0 and r["XX2"][7] == 0 and r["b2"][7] == 0
    assert np.isfinite(r["b1"]).all() and np.isfinite(r["b2"]).all() and np.isfinite(r["cnv"])


FLIP = (1, -1, -1, 1)


@pytest.mark.parametrize("name", ["MEGA", "GSEM"])
def test_invariant_outputs_do_not_change_under_a_flip(name):
    """Flipping a singular pair flips LS's column, LS_BETA's (or V's) column and BETA1's row together -- exactly: x -> -x commutes with every
    rounding, and XX, lambda, e and cnv do not see the sign.  So mu, b, hat, gebv and BETA2 are the same bits."""
    a, f = C.driver_ref(name, "tpod_npc0"), C.driver_ref(name, "tpod_npc0", FLIP)
    sg = np.array(FLIP, np.float64)
    assert tuple(a)[:len(MEGA_KEYS if name == "MEGA" else GSEM_KEYS)] == (MEGA_KEYS if name == "MEGA" else GSEM_KEYS)
    for key in ("mu", "b", "hat", "BETA2") + (("gebv",) if name == "MEGA" else ()):
        assert np.array_equal(f[key], a[key]), key
    assert np.array_equal(f["BETA1"], a["BETA1"] * sg[:, None])
    if name == "MEGA":
        assert np.array_equal(f["LS"], a["LS"] * sg) and np.array_equal(f["LS_BETA"], a["LS_BETA"] * sg)
    else:
        assert np.array_equal(f["LS"], a["LS"] * sg) and np.array_equal(f["V"], a["V"] * sg)
    assert [list(t) for t in f["fit"]["trace"]] == [list(t) for t in a["fit"]["trace"]]


def test_gsem_with_every_component_equals_the_whole_v():
    """:1609 multiplies by the whole V; with npc = min(n, k) V.leftCols(npc) is V."""
    c = C.DRIVER["tpod_npc0"]()
    a = C.driver_ref("GSEM", "tpod_npc0")
    w = S2.GSEM(c["Y"], c["X"], 0, whole_v=True, **c["kw"])
    assert a["npc"] == 4 == min(c["Y"].shape) and np.array_equal(a["b"], w["b"])
    with pytest.raises(ValueError):       # fewer components: the line as written is not conformable
        S2.GSEM(c["Y"], c["X"], 2, whole_v=True, **c["kw"])


def test_mega_shapes_and_its_imputed_records():
    c = C.DRIVER["tpod_npc2"]()
    o = C.driver_ref("MEGA", "tpod_npc2")
    assert o["LS"].shape == (196, 2) and o["LS_BETA"].shape == (376, 2) and o["BETA1"].shape == (2, 4) and o["BETA2"].shape == (376, 4)
    assert o["b"].shape == (376, 4) and o["hat"].shape == o["gebv"].shape == (196, 4) and o["mu"].shape == (4,)
    Y2 = S2.imputed_y(c["Y"], o["G"])
    w = ~np.isnan(c["Y"])
    assert np.array_equal(Y2[~w], o["G"][~w]) and np.allclose(np.where(w, Y2, 0).sum(0), 0, atol=1e-10)
    assert np.allclose((o["Y2"] ** 2).sum(0), 195.0)                  # :1533-1534
    assert np.array_equal(o["LS"], C.driver_ref("MEGA", "tpod_npc0")["LS"][:, :2])
    with pytest.raises(ValueError):
        S2.MEGA(C.nan_trait_traits(), c["X"], 2, maxit=1, tol=0)


def test_uvbeta2_of_a_trait_without_rows():
    o = C.engine_ref("all_nan_trait")
    assert not o["b1"][:, 2].any() and not o["b2"][:, 2].any() and o["its"][2] == 0 and o["mu"][2] == 0 and o["h2"][2] == 0
    assert all(np.isnan(o[key][2]) for key in ("ve", "vb1", "vb2", "cnv"))


# ---- preconditions on the cases, not tolerances ----
@pytest.mark.parametrize("name,case", C.DRIVER_CASES)
def test_driver_cases_are_well_posed(name, case):
    """Neighbouring singular values of the decomposed matrix (Y2 for MEGA, G for GSEM) differ by at least 5 % of the largest; where default
    stopping is used no cnv of any stage comes within 0.02 of log10(tol).  Seeds were picked so that both hold: tpod / seed 227: gaps 0.063
    (Y2) and 0.145 (G); the 700 x 900 panel / seed 333: 0.165 and 0.373, nearest cnv 0.040."""
    o = C.driver_ref(name, case)
    s = o["s"]
    rank = 3 if case == "nan_trait" else len(s)
    gap = float(np.min(-np.diff(s[:rank])) / s[0])
    print(name, case, gap, [list(d["its"]) for d in C.stages(name, o)])
    assert gap >= 0.05, (gap, s)
    if case == "nan_trait":
        assert s[3] <= 1e-12 * s[0] and o["npc"] == 3
    if not C.DRIVER[case]()["kw"]:
        logtol = np.log10(10e-7)
        near = min(abs(c - logtol) for d in C.stages(name, o) for tr in d["trace"] for c in tr)
        print(near)
        assert near >= 0.02 and o["npc"] == 3
    else:
        assert all((d["its"][d["its"] > 0] == 6).all() for d in C.stages(name, o))


def test_engine_default_case_stops_each_trait_at_its_own_sweep():
    o = C.engine_ref("slabs_defaults")
    logtol = np.log10(10e-7)
    near = min(abs(c - logtol) for tr in o["trace"] for c in tr)
    print(o["its"], near)
    assert len(set(o["its"])) == 4 and o["its"].max() < 100 and near >= 0.02


def test_degenerate_cases_are_what_they_say():
    c, o = C.engine("xx1_zero"), C.engine_ref("xx1_zero")
    assert o["b1"][1, 0] == 0 and o["b1"][1, 1] != 0 and o["b1"][1, 2] != 0 and np.isfinite(o["vb1"]).all()
    c, o = C.engine("trx1_zero"), C.engine_ref("trx1_zero")
    assert not o["b1"][:, 1].any() and np.isnan(o["vb1"][1]) and o["b1"][:, 0].all() and o["b1"][:, 2].all()
    d = UR.uvbeta(c["Y"], c["X"], "D", **c["kw"])
    assert np.array_equal(o["b2"][:, 1], d["b"][:, 1]) and o["mu"][1] == d["mu"][1] and o["its"][1] == d["its"][1]
    c = C.engine("one_pattern")
    w = ~np.isnan(c["Y"])
    assert np.array_equal(w[:, 0], w[:, 2]) and np.array_equal(w[:, 1], w[:, 3]) and not np.array_equal(w[:, 0], w[:, 1]) and not w.all()
    w = ~np.isnan(C.engine("full_and_masked")["Y"])
    assert w[:, 1].all() and not w[:, 0].all() and not w[:, 2].all()
    assert C.engine("k65_two_groups")["Y"].shape[1] == 65 and C.engine("q7_beyond_k")["Z"].shape[1] == 7


# ---- surface ----
def _params(fn, kind):
    return [(q.name, q.default) for q in inspect.signature(fn).parameters.values() if q.kind == kind]


def test_signatures_and_key_order_match_the_reference():
    """R/RcppExports.R:200, 208, 212 -- names, order and defaults; the solvers' maxit, tol, df0 keyword-only on the drivers."""
    import bwgr_amd as B
    P, K = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    for fn in (B.MEGA, B.GSEM):
        assert _params(fn, P) == [("Y", E), ("X", E), ("npc", -1)]
        assert _params(fn, K) == [("maxit", 100), ("tol", 10e-7), ("df0", 20.0)]
    assert _params(B.solver2x, P) == [("Y", E), ("X1", E), ("X2", E), ("maxit", 100), ("tol", 10e-7), ("df0", 20.0)]
    assert _params(B.uvbeta2, P) == [("Y", E), ("Z", E), ("X", E), ("maxit", 100), ("tol", 10e-7), ("df0", 20.0)]
    assert "dense X2 is not taken" in B.solver2x.__doc__
    from bwgr_amd import api
    assert api.UVB2_KEYS == ("b1", "b2", "mu", "h2", "ve", "vb1", "vb2", "its", "cnv")
    src = open(os.path.join(ROOT, "bwgr_amd", "uvfit.py")).read()   # the return lists, in the reference's order (:1571-1578, :1608-1610)
    assert '("mu", "b", "hat", "LS", "LS_BETA", "BETA1", "BETA2", "gebv")' in src and '("mu", "b", "hat"), (mu, b, hat)' in src
    rsrc = open(os.path.join(ROOT, "rshim", "bwgr_hip.R")).read()
    for fn in ("MEGA <- function(Y, X, npc = -1L", "GSEM <- function(Y, X, npc = -1L", "solver2x <- function(Y, X1, X2, maxit = 100L, tol = 10e-7, df0 = 20.0"):
        assert fn in rsrc, fn


def test_exports_header_and_shim():
    from bwgr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bwgr.h")).read()
    assert "bwgr_uvbeta2" in _lib.EXPORTS and hasattr(_lib.lib(), "bwgr_uvbeta2") and re.search(r"\bint bwgr_uvbeta2\(", hdr)
    assert _lib.lib().bwgr_abi_version() == 1
    doc = hdr[hdr.index("two designs in one sweep"):hdr.index("int bwgr_uvbeta2(")]
    for word in ("Departures", "TrXSX_i is 0", "1 - ve / vy", "solver2xF", "bwgr_debug_uvbd_plan"):
        assert word in doc, word
    src = open(os.path.join(ROOT, "rshim", "bwgr_shim.c")).read()
    assert re.search(r'\{"bwgrhip_uvbeta2",\s*\(DL_FUNC\)\s*&bwgrhip_uvbeta2,\s*6\}', src)


def test_no_gpu_gives_enodev():
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    rng = np.random.default_rng(0)
    Y = rng.normal(size=(16, 3))
    X = (rng.random((16, 8)) < 0.5).astype(np.int8)
    for call in (lambda: bwgr_amd.uvbeta2(Y, rng.normal(size=(16, 2)), X, maxit=2), lambda: bwgr_amd.solver2x(Y[:, 0], rng.normal(size=(16, 2)), X),
                 lambda: bwgr_amd.MEGA(Y, X), lambda: bwgr_amd.GSEM(Y, X, 2)):
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            call()
        assert ei.value.code == 5   # BWGR_ENODEV
