"""CPU: the public surface of mrr / mrr_float (MRR3 / MRR3F) and the invariants of the tests' numpy restatement of them."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrr_cases  # noqa: E402
import mrr_restatement as MR  # noqa: E402

E = inspect.Parameter.empty
# R/RcppExports.R:180, :184 -- names, order and defaults
_TAIL = [("maxit", 500), ("tol", 10e-9), ("cores", 1), ("TH", False)]
_REST = [("InnerGS", False), ("NoInv", False), ("HCS", False), ("XFA", False), ("ACS", False), ("NumXFA", 3), ("R2", 0.5), ("gc0", 0.5),
         ("df0", 1.0), ("updateMu", False), ("weight_prior_h2", 0.01), ("weight_prior_gc", 0.01), ("PenCor", 0.0), ("MinCor", 1.0),
         ("uncorH2below", 0.0), ("roundGCupFrom", 1.0), ("roundGCupTo", 1.0), ("roundGCdownFrom", 1.0), ("roundGCdownTo", 0.0),
         ("bucketGCfrom", 1.0), ("bucketGCto", 1.0), ("DeflateMax", 0.9), ("DeflateBy", 0.0), ("OneVarB", False), ("OneVarE", False),
         ("verbose", False)]


def _pos(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]


def test_signatures_match_the_reference():
    import bwgr_amd as B
    assert _pos(B.MRR3) == [("Y", E), ("X", E)] + _TAIL + [("NLfactor", 0.0)] + _REST
    assert _pos(B.MRR3F) == [("Y", E), ("X", E)] + _TAIL + [("NonLinearFactor", 0.0)] + _REST
    assert _pos(B.mrr) == [("Y", E), ("X", E)]          # R/mix.R:1271: mrr = function(Y,X,...) MRR3(Y,X,...)
    assert _pos(B.mrr_float) == [("Y", E), ("X", E)]
    assert B.api.MRR_KEYS == ("mu", "b", "hat", "h2", "GC", "vb", "ve", "MSx", "cnvB", "cnvH2", "cnvV", "b_Weights", "Its")


def test_options_order_matches_the_header():
    from bwgr_amd import api
    src = open(os.path.join(ROOT, "include", "bwgr.h")).read()
    body = re.search(r"enum \{ (BWGR_MRR_MAXIT.*?)BWGR_MRR_NOPTS \}", src, re.S).group(1)
    names = [re.sub(r"\s*=.*", "", s).strip() for s in body.split(",") if s.strip()]
    assert [n.replace("BWGR_MRR_", "") for n in names] == [o.upper() for o in api._MRR_OPTS]
    defaults = re.search(r"#define BWGR_MRR_DEFAULTS \{([^}]*)\}", src).group(1).split(",")
    d = dict(_TAIL + [("NLfactor", 0.0)] + _REST)
    assert [float(v) for v in defaults] == [float(d[o]) for o in api._MRR_OPTS]


def test_shim_registers_the_entries():
    src = open(os.path.join(ROOT, "rshim", "bwgr_shim.c")).read()
    for name in ("bwgrhip_MRR3", "bwgrhip_MRR3F"):
        assert re.search(r'\{"%s",\s*\(DL_FUNC\)\s*&%s,\s*3\}' % (name, name), src), name
    rsrc = open(os.path.join(ROOT, "rshim", "bwgr_hip.R")).read()
    for fn in ("MRR3 <- function(Y, X, maxit = 500L", "MRR3F <- function(Y, X, maxit = 500L", "mrr <- function(Y, X, ...)", "mrr_float <- function(Y, X, ...)"):
        assert fn in rsrc, fn


def test_no_gpu_gives_enodev():
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    Y = np.random.default_rng(0).normal(size=(16, 3))
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.MRR3(Y, np.ones((16, 8), np.int8), maxit=2)
    assert ei.value.code == 5   # BWGR_ENODEV
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.mrr_float(Y, np.ones((16, 8), np.int8), maxit=2)
    assert ei.value.code == 5


def _tpod(k=3, frac=0.1, seed=1):
    d = np.load(os.path.join(ROOT, "tests", "golden", "tpod.npz"))
    X = d["gen"].astype(np.float64)
    rng = np.random.default_rng(seed)
    n, p = X.shape
    B = rng.normal(size=(p, k)) * 0.1
    Y = (X - X.mean(0)) @ B + rng.normal(size=(n, k))
    Y[rng.random((n, k)) < frac] = np.nan
    return Y, X


@pytest.mark.parametrize("k", [3, 16])
def test_restatement_residual_and_symmetry_invariants(k):
    Y, X = _tpod(k=k)
    r = MR.mrr(Y, X, maxit=6, tol=0, trace=True)
    assert r["Its"] == 6 and len(r["cnvB"]) == 6
    for t in r["trace"]:
        e_expect = (t["y"] - t["Xc"] @ t["b"]) * t["Z"]
        assert np.max(np.abs(t["e"] - e_expect)) < 1e-10 * np.max(np.abs(t["y"]))
    assert np.allclose(r["vb"], r["vb"].T, rtol=0, atol=1e-14 * np.abs(r["vb"]).max())
    assert np.allclose(np.diag(r["GC"]), 1.0, rtol=0, atol=1e-12)
    assert [key for key in r if key != "trace"] == ["mu", "b", "hat", "h2", "GC", "vb", "ve", "MSx", "cnvB", "cnvH2", "cnvV", "b_Weights", "Its"]


def test_restatement_k1_solves_the_ridge_system():
    d = np.load(os.path.join(ROOT, "tests", "golden", "tpod.npz"))
    X, y = d["gen"].astype(np.float64), d["y"].astype(np.float64)
    r = MR.mrr(y, X, maxit=400, tol=1e-30, trace=True)
    t = r["trace"][-1]
    Xc = X - X.mean(0)
    lam = t["ve_sweep"][0] * t["iG_sweep"][0, 0]     # ve / vb at the last sweep
    b = np.linalg.solve(Xc.T @ Xc + lam * np.eye(X.shape[1]), Xc.T @ (y - y.mean()))
    assert MR.scaled_err(r["b"][:, 0], b) < 1e-6


def test_restatement_large_k_solves_the_stacked_ridge_system():
    """k = 16 traits with missing records, run to convergence: b solves the stacked system of the last sweep's iG and ve,
    (iG (x) I_p) vec(B) + blockdiag_t(Xc' diag(z_t) Xc / ve_t) vec(B) = vec_t(Xc' (z_t o y_t) / ve_t), with Xc, Z and y built here
    from X and Y (not taken from the restatement)."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "tpod.npz"))
    X = d["gen"].astype(np.float64)[:, ::3]
    n, p = X.shape
    k = 16
    rng = np.random.default_rng(5)
    Y = (X - X.mean(0)) @ (rng.normal(size=(p, k)) * 0.1) + rng.normal(size=(n, k))
    Y[rng.random((n, k)) < 0.15] = np.nan
    r = MR.mrr(Y, X, maxit=300, tol=1e-30, trace=True)
    assert r["Its"] < 300   # stopped by the tolerance
    t = r["trace"][-1]
    iG, ve = t["iG_sweep"], t["ve_sweep"]
    Z = (~np.isnan(Y)).astype(np.float64)
    y = np.where(Z > 0, Y - np.nanmean(Y, 0), 0.0)
    Xc = X - X.mean(0)
    assert Z.min() == 0
    A = np.kron(iG, np.eye(p))
    rhs = np.empty(p * k)
    for s in range(k):
        A[s * p:(s + 1) * p, s * p:(s + 1) * p] += Xc.T @ (Z[:, s:s + 1] * Xc) / ve[s]
        rhs[s * p:(s + 1) * p] = Xc.T @ (Z[:, s] * y[:, s]) / ve[s]
    b = np.linalg.solve(A, rhs).reshape(k, p).T
    assert MR.scaled_err(r["b"], b) < 1e-6


def test_restatement_takes_the_bending_branch():
    # two traits that are one trait: GC pulled to the edge of the PD cone, XFA with one factor then
    # leaves off-diagonals above 1 once the diagonal is reset -> a negative eigenvalue
    Y, X = _tpod(k=3, frac=0.0, seed=3)
    Y[:, 1] = Y[:, 0] + 1e-3 * Y[:, 1]
    Y[:, 2] = -Y[:, 0] + 1e-3 * Y[:, 2]
    r = MR.mrr(Y, X, maxit=4, tol=0, XFA=True, NumXFA=1, weight_prior_gc=0, trace=True)
    assert any(t["bent"] for t in r["trace"])
    assert np.linalg.eigvalsh(r["GC"]).min() >= -1e-12
    assert np.allclose(np.diag(r["GC"]), 1.0, atol=1e-12)


def test_restatement_float_flavour_tracks_double():
    Y, X = _tpod()
    r64 = MR.mrr(Y, X, maxit=5, tol=0)
    r32 = MR.mrr(Y, X, maxit=5, tol=0, dtype=np.float32)
    assert MR.scaled_err(r32["b"], r64["b"]) < 1e-3


# ---- the LDS plan of k_mrr_solve / k_mrr_linv (bwgr_debug_mrr_plan) ----
LDS_MAX = 160 * 1024
GRAM_B = 64 * 64 * 4   # one block's int32 Gram matrix of one pattern
# k_mrr_solve's fixed arrays, restated from its carve-up of the dynamic LDS: dc [64][17], xx / b0 / dB [64][16] each, xbar [64],
# S [16][64], rhs [16], sum e [16] (doubles) and the block's marker ids [64] (int32)
SOLVE_FIXED = 8 * (64 * 17 + 3 * 64 * 16 + 64 + 16 * 64 + 16 + 16) + 4 * 64


def test_mrr_plan_invariants():
    for k in range(1, 17):
        linv_b = 8 * 64 * k * k   # k_mrr_linv: a[(r k + s) 64 + tid], and the solve's staged inverses [64][k][k]
        for npat in range(1, k + 1):
            rc, linv, ngl, solve, lin = mrr_cases.plan(k, npat)
            case = (k, npat, linv, ngl, solve, lin)
            assert rc == 0 and linv in (0, 1), case
            assert solve <= LDS_MAX and lin <= LDS_MAX, case
            assert lin >= linv_b, case
            assert 0 <= ngl <= npat, case
            need = ngl * GRAM_B + (linv_b if linv else 0) + SOLVE_FIXED   # what the solve indexes
            assert solve >= need, case
            assert linv or SOLVE_FIXED + linv_b > LDS_MAX, case     # the inverses are staged whenever they fit
            assert ngl == npat or need + GRAM_B > LDS_MAX, case     # as many Grams as the rest holds


def test_mrr_plan_refuses_what_the_engine_does_not_run():
    for k, npat in [(0, 1), (17, 1), (17, 17), (3, 0), (3, 4), (1, 2)]:
        assert mrr_cases.plan(k, npat)[0] == 1, (k, npat)   # BWGR_EINVAL


def test_gpu_cases_reach_every_plan_regime():
    """The GPU parity table of tests/mrr_cases.py covers all five layouts of the solve under the current plan; a change of the LDS
    budget that moves a case out of its regime fails here rather than silently dropping that layout from the GPU suite."""
    seen = {}
    for k, npat in mrr_cases.K_SWEEP:
        _, linv, ngl, _, _ = mrr_cases.plan(k, npat)
        seen.setdefault(mrr_cases.regime(linv, ngl, npat), []).append((k, npat))
    assert sorted(seen) == [1, 2, 3, 4, 5], seen
    # the shared-pattern cases: pt[t] != t with 1 < npat < k
    for ids in mrr_cases.SHARED:
        npat = len(set(ids))
        first = [g for j, g in enumerate(ids) if g not in ids[:j]]
        assert 1 < npat < len(ids) and first == list(range(npat)), ids   # numbered as the host numbers them
    k, npat = len(mrr_cases.SHARED[-1]), len(set(mrr_cases.SHARED[-1]))
    assert mrr_cases.plan(k, npat)[2] < npat        # ... one of them with patterns read from global memory
    _, linv, ngl, _, _ = mrr_cases.plan(mrr_cases.OPTIONS_K, mrr_cases.OPTIONS_K)
    assert linv and 0 < ngl < mrr_cases.OPTIONS_K   # the options run in regime 2
