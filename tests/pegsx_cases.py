"""The cases of the PEGSX tests, in one table, in the idiom of tests/pegs_cases.py (whose data makers it reuses): tests/test_gpu_pegsx.py runs
each on the GPU against tests/pegsx_restatement.py, and tests/test_pegsx_cpu.py checks on the restatement alone that none of them sits on a
discontinuous branch (MinDVb < covMinEv, a near-degenerate eigen-gap where XFA truncates, the rank decision of M'M) or on a floor.

A case: id, data() -> (Y, X, effects), kw (the fit's arguments).  An effect is ("panel", Z int8, panel kwargs) or ("dense", Z float64).  Every
case runs with logtol = -inf (every sweep) unless its kw says otherwise.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pegs_cases as PC  # noqa: E402
from pegs_cases import NOSTOP, K16_IDS, gauss, slabs900, tpod, traits, traits_ids  # noqa: E402, F401

_cache = {}


def fixed(n, ncov, seed):
    """an intercept and ncov Gaussian covariates"""
    return np.asfortranarray(np.column_stack([np.ones(n), np.random.default_rng(seed).normal(size=(n, ncov))]))


def with_fixed(Y, X, beta_seed):
    """adds X beta to the traits, so that the fixed effects have something to fit (NaN stays NaN)"""
    beta = np.random.default_rng(beta_seed).normal(size=(X.shape[1], Y.shape[1]))
    return Y + X @ beta


def _tpod_k3():
    Z = tpod()
    X = fixed(Z.shape[0], 2, 101)
    return with_fixed(traits(Z, 3, 0.1, seed=11), X, 102), X, [("panel", Z, {})]


def _f1():
    Z = tpod()
    return traits(Z, 3, 0.1, seed=11), np.ones((Z.shape[0], 1)), [("panel", Z, {})]


def _f70():
    Z = slabs900()
    X = fixed(Z.shape[0], 69, 103)
    return with_fixed(traits(Z, 5, 0, seed=5, patterns=[0.1, 0.0, 0.25, 0.05, 0.4]), X, 104), X, [("panel", Z, dict(nwg=3))]


def _k1():
    Z = tpod()
    X = fixed(Z.shape[0], 2, 105)
    return with_fixed(traits(Z, 1, 0.1, seed=13), X, 106), X, [("panel", Z, {})]


def _k16():
    Z = slabs900()
    X = fixed(Z.shape[0], 2, 107)
    return with_fixed(traits_ids(Z, K16_IDS, 0.1, seed=121), X, 108), X, [("panel", Z, dict(nwg=3))]


def _rank_deficient():
    """intercept + two complementary 0/1 dummies + one covariate: f = 4, rank 3 in every missingness pattern"""
    Z = tpod()
    n = Z.shape[0]
    rng = np.random.default_rng(109)
    d = (rng.random(n) < 0.45).astype(np.float64)
    X = np.asfortranarray(np.column_stack([np.ones(n), d, 1.0 - d, rng.normal(size=n)]))
    return with_fixed(traits(Z, 3, 0.1, seed=11), X, 110), X, [("panel", Z, {})]


def _bending():
    Y, effs = PC._bending()
    X = fixed(Y.shape[0], 1, 111)
    return Y, X, effs


def _two_panels():
    Y, effs = PC._two_panels()
    X = fixed(Y.shape[0], 2, 113)
    return with_fixed(Y, X, 114), X, effs


def _panel_dense(first):
    def data():
        Y, effs = PC._panel_dense(70, 23, first=first)()
        X = fixed(Y.shape[0], 2, 115)
        return with_fixed(Y, X, 116), X, effs
    return data


def _dense_only(n, q, seed, ncov):
    def data():
        Y, effs = PC._dense_only(n, q, seed)()
        X = fixed(n, ncov, seed + 7)
        return with_fixed(Y, X, seed + 8), X, effs
    return data


def _stop():
    """few columns and a strong prior: the sweeps barely move u, so cnv is below 0 from the start"""
    Y, effs = PC._dense_only(196, 6, 47)()
    X = fixed(196, 1, 117)
    return with_fixed(Y, X, 118), X, effs


# ---- int8 codes beyond 0 / 1 / 2 (the panels of tests/pegs_cases.py): beside PEGS's uncentred sweeps, k_pegsx_trace_panel reads the same
# bytes, and with an intercept in X TrZSZ = sum z^2 - v'A v is a difference of two large numbers once the codes have a large mean ----

def _codes(name, ncov=2, seed=131):
    def data():
        Z = PC._panel(name)
        X = fixed(Z.shape[0], ncov, seed)
        return with_fixed(traits(Z, 3, 0.1, seed=PC.CODES_SEED), X, seed + 1), X, [("panel", Z, {})]
    return data


def _codes_f70():
    Z = PC._panel("full_slabs")
    X = fixed(Z.shape[0], 69, 133)
    return with_fixed(traits(Z, 5, 0, seed=5, patterns=[0.1, 0.0, 0.25, 0.05, 0.4]), X, 134), X, [("panel", Z, dict(nwg=3))]


def _case(id_, data, **kw):
    kw.setdefault("logtol", NOSTOP)
    return dict(id=id_, data=data, kw=kw)


CASES = [
    _case("tpod_k3_defaults", _tpod_k3, maxit=12),
    _case("tpod_k3_nnc", _tpod_k3, maxit=12, NNC=True),
    _case("tpod_k3_xfa1", _tpod_k3, maxit=12, XFA=True, NumXFA=1),
    _case("tpod_k3_xfa2", _tpod_k3, maxit=12, XFA=True, NumXFA=2),
    _case("tpod_k3_xfa3", _tpod_k3, maxit=12, XFA=True, NumXFA=3),
    _case("tpod_k3_xfa_num0", _tpod_k3, maxit=12, XFA=True, NumXFA=0),
    _case("tpod_k3_df0_20", _tpod_k3, maxit=12, df0=20.0),
    _case("tpod_k3_covbend2", _tpod_k3, maxit=12, covbend=2.0),
    _case("f1_intercept", _f1, maxit=12),
    _case("f70_slabs_k5", _f70, maxit=6),
    _case("k1", _k1, maxit=12),
    _case("k16_shared_patterns", _k16, maxit=4),
    _case("rank_deficient_x", _rank_deficient, maxit=8),
    _case("bending_nnc_on", _bending, maxit=4, NNC=True),
    _case("bending_nnc_off", _bending, maxit=4, NNC=False),
    _case("two_panels", _two_panels, maxit=8),
    _case("panel_dense70", _panel_dense("panel"), maxit=8),
    _case("dense70_panel", _panel_dense("dense"), maxit=8),
    _case("dense_only_n196", _dense_only(196, 70, 41, 2), maxit=8),
    _case("dense_only_n1500", _dense_only(1500, 20, 45, 2), maxit=6),
    _case("stop_rule", _stop, maxit=50, logtol=0.0),
]
# the code-range cases: an intercept and two covariates unless the id says otherwise (const_cols: the intercept alone, which spans the
# all-2 column, so that column's share of TrZSZ is an exact 0 made of two equal sums)
CODE_CASES = [
    _case("codes_signed", _codes("signed"), maxit=8),
    _case("codes_full", _codes("full"), maxit=8),
    _case("codes_offset", _codes("offset"), maxit=8),
    _case("codes_pm127", _codes("pm127"), maxit=8),
    _case("codes_offset_xfa2", _codes("offset"), maxit=8, XFA=True, NumXFA=2),
    _case("codes_full_slabs_f70_k5", _codes_f70, maxit=6),
    _case("codes_const_cols_f1", _codes("const_cols", ncov=0), maxit=8),
]
CASES += CODE_CASES
# the restatement's trace must say that these inflated in every sweep
BENDS = ("bending_nnc_on", "bending_nnc_off", "codes_full", "codes_offset", "codes_pm127", "codes_offset_xfa2", "codes_full_slabs_f70_k5")
RANK_DEFICIENT = ("rank_deficient_x",)          # the only cases whose M'M may drop an eigenvalue
NAMED_FLOORS = {}                               # case id -> the floors it is allowed to sit on (none of the cases needs one)


def by_id(id_):
    return next(c for c in CASES if c["id"] == id_)


def designs(effects):
    return [np.asarray(e[1], np.float64) for e in effects]


def restate(case, **more):
    """the restatement's fit of a case with its trace, computed once per process"""
    import pegsx_restatement as XR
    key = ("fit", case["id"], tuple(sorted(more.items())))
    if key not in _cache:
        Y, X, effects = case["data"]()
        kw = dict(case["kw"], **more)
        _cache[key] = (Y, X, effects, XR.pegsx(Y, X, designs(effects), dense=[e[0] == "dense" for e in effects], trace=True, **kw))
    return _cache[key]
