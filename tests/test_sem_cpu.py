"""CPU: the tests' numpy restatement of XSEMF / ZSEMF / YSEMF (tests/sem_restatement.py) pinned by the properties it must have, the host
arithmetic of bwgr_uvbeta_dense's plan, and the public surface of the latent-space fits (uvbeta_dense, panel_xb, uvbd_plan, the drivers)."""
import functools
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrr_restatement as MR  # noqa: E402
import sem_restatement as SR  # noqa: E402
from test_uvb_cpu import _tpod, _traits  # noqa: E402

E = inspect.Parameter.empty
OUT = {"XSEMF": ("b", "GC", "hat"), "ZSEMF": ("mu", "b", "hat", "h2", "GC"), "YSEMF": ("mu", "b", "hat", "h2", "GC")}


def _f32(Y):
    return np.asarray(Y, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(None)
def _case(name, flip=None):
    X = _tpod()[:, :120]
    Y = _f32(_traits(X, 4, 0.1, seed=227))
    return X, Y, getattr(SR, name)(Y, X, 0, maxit=4, tol=0, flip=flip)


# ---- the restatement ----
@pytest.mark.parametrize("name", ["XSEMF", "ZSEMF", "YSEMF"])
def test_outputs_do_not_depend_on_the_signs_of_the_singular_pairs(name):
    """Flipping a pair flips Z's column, V's column and the second stage's coefficient together -- exactly, in IEEE arithmetic: x -> -x
    commutes with every rounding, a column's mean and centred column flip with it, and XX, lambda, e and cnv do not see the sign."""
    _, _, a = _case(name)
    _, _, f = _case(name, (1, -1, -1, 1))
    assert np.array_equal(f["Z"], a["Z"] * np.array([1.0, -1.0, -1.0, 1.0]))
    assert np.array_equal(f["second"]["b"], a["second"]["b"] * np.array([1.0, -1.0, -1.0, 1.0])[:, None])
    for key in OUT[name]:
        assert MR.scaled_err(f[key], a[key]) <= 1e-12, key
    assert tuple(a)[:len(OUT[name])] == OUT[name]


@pytest.mark.parametrize("name", ["XSEMF", "ZSEMF", "YSEMF"])
def test_gc_is_a_correlation_matrix(name):
    _, _, a = _case(name)
    GC = a["GC"]
    assert GC.shape == (4, 4) and np.allclose(np.diag(GC), 1.0, atol=1e-12) and np.allclose(GC, GC.T, atol=1e-14)
    assert np.all(np.abs(GC) <= 1 + 1e-12)
    if name == "XSEMF":   # hat is the standardised X b
        assert np.allclose(a["hat"].mean(0), 0, atol=1e-12) and np.allclose((a["hat"] ** 2).mean(0), 1.0, atol=1e-12)
    else:
        assert a["hat"].shape == (196, 4) and a["mu"].shape == (4,) and a["h2"].shape == (4,)


def test_gc_of_a_zero_column_is_nan():
    G = np.random.default_rng(0).normal(size=(30, 3))
    G[:, 1] = 0
    g = SR.gc(G)
    assert np.isnan(g["GC"][1]).all() and np.isnan(g["GC"][:, 1]).all() and np.isfinite(g["GC"][[0, 2]][:, [0, 2]]).all()
    assert np.isnan(g["hat"][:, 1]).all()


def test_xsemf_b_lies_in_the_column_space_of_beta():
    _, _, a = _case("XSEMF")
    B = a["BETA"]["b"]
    proj = B @ np.linalg.lstsq(B, a["b"], rcond=None)[0]
    assert MR.scaled_err(proj, a["b"]) <= 1e-10
    assert a["G"].shape == (196, 4) and a["Z"].shape == (196, 4) and a["second"]["b"].shape == (4, 4)


def test_npc_rules():
    """:1760-1761 -- npc < 0: round(2 sqrt(m)); 0: m; leftCols(npc) beyond m is refused."""
    assert [SR.n_components(-1, m) for m in (3, 4, 9, 10, 16, 100)] == [3, 4, 6, 6, 8, 20]
    assert [SR.n_components(0, m) for m in (1, 4, 7)] == [1, 4, 7]
    assert SR.n_components(2, 4) == 2 and SR.n_components(4, 4) == 4
    for npc, m in ((5, 4), (-1, 1), (-1, 2)):   # (2 sqrt(m) > m for m < 4: the reference's default leaves the matrix there)
        with pytest.raises(ValueError):
            SR.n_components(npc, m)
    for m in range(1, 2000):   # no tie: 2 sqrt(m) is never a half-integer
        assert abs(2 * np.sqrt(m) % 1 - 0.5) > 1e-9
    X, Y, a = _case("ZSEMF")
    two = SR.ZSEMF(Y, X, 2, maxit=4, tol=0)
    assert two["Z"].shape == (196, 2) and np.array_equal(two["Z"], a["Z"][:, :2]) and two["second"]["b"].shape == (2, 4)
    assert SR.YSEMF(Y, X, maxit=1, tol=0)["npc"] == 4


# ---- the plan (bwgr_debug_uvbd_plan) ----
def test_plan_arithmetic():
    import bwgr_amd
    pl = bwgr_amd.uvbd_plan(5000, 64, 64)
    assert tuple(pl) == ("lds_rows", "e_in_lds", "threads", "lds_bytes", "ws_bytes")
    L = pl["lds_rows"]
    overhead = pl["lds_bytes"] - 8 * 5000
    assert pl["e_in_lds"] == 1 and overhead >= 0 and pl["ws_bytes"] == 0
    assert 8 * L + overhead <= 160 * 1024 < 8 * (L + 1) + overhead        # the largest n that fits
    for q, k in ((1, 1), (4, 2), (64, 300)):
        at, over = bwgr_amd.uvbd_plan(L, q, k), bwgr_amd.uvbd_plan(L + 1, q, k)
        assert at["lds_rows"] == L == over["lds_rows"]
        assert at["e_in_lds"] == 1 and at["lds_bytes"] == 8 * L + overhead and at["ws_bytes"] == 0
        assert over["e_in_lds"] == 0 and over["lds_bytes"] == overhead and over["ws_bytes"] == 8 * (L + 1) * k
    for n in (1, 63, 64, 65, 196, 1023, 1024, 1025, L, L + 37):
        t = bwgr_amd.uvbd_plan(n, 5, 3)["threads"]
        assert t % 64 == 0 and 64 <= t <= 1024 and (t >= n or t == 1024), (n, t)


def test_plan_refuses_nonsense():
    import bwgr_amd
    for n, q, k in [(0, 10, 1), (10, 0, 1), (10, 10, 0), (-5, 10, 3), (10, -1, 3), (10, 10, -1)]:
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            bwgr_amd.uvbd_plan(n, q, k)
        assert ei.value.code == 1, (n, q, k)   # BWGR_EINVAL


# ---- surface ----
def _params(fn, kind):
    return [(q.name, q.default) for q in inspect.signature(fn).parameters.values() if q.kind == kind]


def test_signatures_and_key_order_match_the_reference():
    """R/RcppExports.R:232, 240, 244 -- names, order and defaults; the solvers' built-in maxit, tol, df0 as keyword-only arguments."""
    import bwgr_amd as B
    P, K = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    for fn, npc in ((B.XSEMF, 0), (B.ZSEMF, 0), (B.YSEMF, -1)):
        assert _params(fn, P) == [("Y", E), ("X", E), ("npc", npc)]
        assert _params(fn, K) == [("maxit", 100), ("tol", 10e-7), ("df0", 20.0)]
    assert _params(B.uvbeta_dense, P) == [("Y", E), ("Z", E), ("variant", "D"), ("maxit", 100), ("tol", 10e-7), ("df0", 20.0)]
    assert _params(B.uvbeta_dense, K) == [("device", 0)]
    assert _params(B.panel_xb, P) == [("X", E), ("B", E)] and _params(B.Panel.xb, P) == [("self", E), ("B", E)]
    assert _params(B.uvbd_plan, P) == [("n", E), ("q", E), ("k", E)]
    rsrc = open(os.path.join(ROOT, "rshim", "bwgr_hip.R")).read()
    for fn in ("XSEMF <- function(Y, X, npc = 0L)", "ZSEMF <- function(Y, X, npc = 0L)", "YSEMF <- function(Y, X, npc = -1L)"):
        assert fn in rsrc, fn
    api = open(os.path.join(ROOT, "bwgr_amd", "uvfit.py")).read()   # the return lists, in the reference's order (:1769, :1841-1845, :1870-1874)
    assert '("b", "GC", "hat")' in api and api.count('("mu", "b", "hat", "h2", "GC")') >= 2


def test_exports_and_header():
    from bwgr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bwgr.h")).read()
    for name in ("bwgr_uvbeta_dense", "bwgr_debug_uvbd_plan", "bwgr_panel_xb"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name) and re.search(r"\bint %s\(" % name, hdr), name
    assert re.search(r"#define BWGR_UVBD_PLAN_NOUT 5\b", hdr)
    notes = hdr[hdr.index("Not here: MEGA"):]
    assert "XSEMF" not in notes[:notes.index("sharded")]   # the out-of-scope list no longer names the latent-space fits


def test_shim_registers_the_entries():
    src = open(os.path.join(ROOT, "rshim", "bwgr_shim.c")).read()
    for name, nargs in (("bwgrhip_uvbeta_dense", 6), ("bwgrhip_panel_xb", 2)):
        assert re.search(r'\{"%s",\s*\(DL_FUNC\)\s*&%s,\s*%d\}' % (name, name, nargs), src), name


def test_no_gpu_gives_enodev():
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    rng = np.random.default_rng(0)
    Y = rng.normal(size=(16, 3))
    X = (rng.random((16, 8)) < 0.5).astype(np.int8)
    for call in (lambda: bwgr_amd.uvbeta_dense(Y, rng.normal(size=(16, 2)), "Z", maxit=2), lambda: bwgr_amd.panel_xb(X, np.ones((8, 2))),
                 lambda: bwgr_amd.XSEMF(Y, X), lambda: bwgr_amd.ZSEMF(Y, X, 2), lambda: bwgr_amd.YSEMF(Y, X)):
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            call()
        assert ei.value.code == 5   # BWGR_ENODEV
