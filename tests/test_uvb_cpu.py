"""CPU: the tests' numpy restatement of the per-trait ridge solvers (tests/uvb_restatement.py) pinned against the ridge system it must solve,
the host arithmetic of bwgr_uvbeta's plan, and the public surface of the UVBETA / FUVBETA family."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrr_restatement as MR  # noqa: E402
import uvb_restatement as UR  # noqa: E402

E = inspect.Parameter.empty


def _tpod():
    return np.load(os.path.join(ROOT, "tests", "golden", "tpod.npz"))["gen"]


def _traits(X, k, frac, seed):
    """test_gpu_mrr._traits: a polygenic signal plus noise, `frac` of the records missing."""
    rng = np.random.default_rng(seed)
    Xf = X.astype(np.float64)
    n, p = X.shape
    B = rng.normal(size=(p, k)) * (1.0 / np.sqrt(p))
    G = (Xf - Xf.mean(0)) @ B
    Y = G / G.std(0) + rng.normal(size=(n, k)) + 3.0
    Y[rng.random((n, k)) < frac] = np.nan
    return Y


def test_restatement_solves_the_ridge_system_on_the_traits_rows():
    """Variant X at a fixed lambda, run far past convergence: Gauss-Seidel's fixed point is (Xc'Xc + lambda I)^-1 Xc'y on the trait's own
    rows, Xc centred by the means over those rows.  This pins the yardstick, not the feature."""
    X = _tpod()
    Y = _traits(X, 2, 0.2, seed=7)
    lam = 40.0
    for t in range(2):
        w = ~np.isnan(Y[:, t])
        assert 0 < (~w).sum() < len(w)
        r = UR.solver(Y[w, t], X[w], "X", maxit=400, tol=1e-300, lam=lam)
        assert r["its"] == 400
        Xc = X[w].astype(np.float64); Xc -= Xc.mean(0)
        y = Y[w, t] - Y[w, t].mean()
        b = np.linalg.solve(Xc.T @ Xc + lam * np.eye(X.shape[1]), Xc.T @ y)
        assert MR.scaled_err(r["b"], b) <= 1e-10


@pytest.mark.parametrize("variant", ["D", "F", "X", "Z"])
def test_restatement_is_shift_invariant(variant):
    """The column means are removed per trait, over the trait's rows: gen - 1 gives the fit of gen."""
    X = _tpod()
    Y = _traits(X, 3, 0.1, seed=11)
    a = UR.uvbeta(Y, X, variant, maxit=6, tol=0)
    b = UR.uvbeta(Y, X.astype(np.int16) - 1, variant, maxit=6, tol=0)
    assert list(a["its"]) == [6, 6, 6] == list(b["its"])
    for key in ("b", "mu", "cnv") + (() if variant == "X" else ("ve", "vb", "h2")):
        assert MR.scaled_err(b[key], a[key]) <= 1e-9, key


def test_restatement_all_nan_trait_and_maxit_zero():
    X = _tpod()[:, :40]
    Y = _traits(X, 3, 0.1, seed=2)
    Y[:, 1] = np.nan
    r = UR.uvbeta(Y, X, "Z", maxit=3, tol=0)
    assert list(r["its"]) == [3, 0, 3] and not r["b"][:, 1].any() and r["b"][:, 0].any()
    z = UR.uvbeta(Y, X, "D", maxit=0)
    assert not z["b"].any() and not z["its"].any()


# ---- the plan (bwgr_debug_uvb_plan) ----
def test_plan_groups_and_lds():
    import bwgr_amd
    W = bwgr_amd.uvb_plan(700, 900, 1)["W"]
    assert W >= 32
    for k in (1, W, W + 1, 1000):
        pl = bwgr_amd.uvb_plan(5000, 50000, k)
        assert pl["W"] == W and pl["groups"] == -(-k // W), (k, pl)
        assert 0 < pl["solve_lds"] <= 160 * 1024 and 0 < pl["pass_lds"] <= 160 * 1024, pl
        assert 1 <= pl["ngl"] <= pl["solve_traits"] and W % pl["solve_traits"] == 0, pl
        # the solve's LDS, restated from its carve-up: ngl Gram matrices of 64 x 64 int32 (four words apart), u [64][traits] and sum e [traits]
        # in doubles, the block's marker ids
        st = pl["solve_traits"]
        assert pl["solve_lds"] == pl["ngl"] * (64 * 64 + 4) * 4 + 8 * (64 * st + st) + 4 * 64, pl
        assert pl["solve_lds"] + (64 * 64 + 4) * 4 > 160 * 1024 or pl["ngl"] == st, pl     # as many Gram matrices as fit
        assert 1 <= pl["pass_wg"] <= -(-5000 // 64) + 1, pl
        # the workspace holds at least the gathered panel, y and e, and the four p x W arrays of every group
        assert pl["ws_bytes"] >= 5000 * 50000 + 8 * pl["groups"] * W * (2 * 5000 + 4 * 50000), pl
    assert bwgr_amd.uvb_plan(100, 10, 3)["ws_bytes"] < bwgr_amd.uvb_plan(100, 10, 3 * W)["ws_bytes"]


def test_plan_refuses_nonsense():
    import bwgr_amd
    for n, p, k in [(0, 10, 1), (10, 0, 1), (10, 10, 0), (-5, 10, 3), (10, 10, -1)]:
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            bwgr_amd.uvb_plan(n, p, k)
        assert ei.value.code == 1, (n, p, k)   # BWGR_EINVAL


# ---- surface ----
def _pos(fn):
    return [(q.name, q.default) for q in inspect.signature(fn).parameters.values() if q.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]


def test_signatures_match_the_reference():
    """R/RcppExports.R:196-238 -- names, order and defaults."""
    import bwgr_amd as B
    for f in (B.solver1x, B.solver1xF):
        assert _pos(f) == [("Y", E), ("X", E), ("maxit", 100), ("tol", 10e-7), ("df0", 20.0)]
    for f in (B.UVBETA, B.FUVBETA, B.XFUVBETA, B.ZFUVBETA):
        assert _pos(f) == [("Y", E), ("X", E)]
    assert _pos(B.uvbeta) == [("Y", E), ("X", E), ("variant", "D"), ("maxit", 100), ("tol", 10e-7), ("df0", 20.0), ("xb", False)]
    assert B.api.UVB_KEYS == ("b", "mu", "h2", "ve", "vb", "its", "cnv")


def test_variants_match_the_header():
    from bwgr_amd import api
    src = open(os.path.join(ROOT, "include", "bwgr.h")).read()
    for name, v in api.UVB_VARIANTS.items():
        assert re.search(r"BWGR_UVB_%s = %d\b" % (name, v), src), name
    assert re.search(r"#define BWGR_UVB_PLAN_NOUT 8\b", src)


def test_shim_registers_the_entries():
    src = open(os.path.join(ROOT, "rshim", "bwgr_shim.c")).read()
    for name, nargs in (("bwgrhip_solver1x", 6), ("bwgrhip_UVBETA", 3)):
        assert re.search(r'\{"%s",\s*\(DL_FUNC\)\s*&%s,\s*%d\}' % (name, name, nargs), src), name
    rsrc = open(os.path.join(ROOT, "rshim", "bwgr_hip.R")).read()
    for fn in ("solver1x <- function(Y, X, maxit = 100L, tol = 10e-7, df0 = 20.0)", "solver1xF <- function(Y, X, maxit = 100L, tol = 10e-7, df0 = 20.0)",
               "UVBETA <- function(Y, X)", "FUVBETA <- function(Y, X)", "XFUVBETA <- function(Y, X)", "ZFUVBETA <- function(Y, X)"):
        assert fn in rsrc, fn


def test_no_gpu_gives_enodev():
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    Y = np.random.default_rng(0).normal(size=(16, 3))
    X = np.ones((16, 8), np.int8)
    for call in (lambda: bwgr_amd.UVBETA(Y, X), lambda: bwgr_amd.ZFUVBETA(Y, X), lambda: bwgr_amd.solver1x(Y[:, 0], X, maxit=2),
                 lambda: bwgr_amd.uvbeta(Y, X, "X", xb=True)):
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            call()
        assert ei.value.code == 5   # BWGR_ENODEV
