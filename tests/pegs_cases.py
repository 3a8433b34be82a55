"""The cases of the PEGS / PEGSZ tests, in one table: tests/test_gpu_pegs.py runs each on the GPU against tests/pegs_restatement.py, and
tests/test_pegs_cpu.py checks on the restatement alone that none of them sits on the fit's only discontinuous branch (MinDVb < covMinEv) or
on a near-degenerate eigen-gap where XFA truncates -- there a difference in the last bits would flip the branch and parity would be luck.

A case: id, entry ("PEGS" / "PEGSZ"), data() -> (Y, effects), kw (the fit's arguments).  An effect is ("panel", X int8, panel kwargs) or
("dense", Z float64); tests/tall_cases.py adds ("sparse", A float64[, stored mask]), read here as its dense copy A.  Every case runs with logtol = -inf (every sweep) unless its kw says otherwise.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import synth_small  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOSTOP = float("-inf")


def traits(X, k, frac, seed, patterns=None):
    """the traits of tests/test_gpu_mrr.py: a genetic part on the centred X, unit noise, mean 3"""
    rng = np.random.default_rng(seed)
    Xf = np.asarray(X, np.float64)
    n, p = Xf.shape
    B = rng.normal(size=(p, k)) * (1.0 / np.sqrt(p))
    G = (Xf - Xf.mean(0)) @ B
    Y = G / G.std(0) + rng.normal(size=(n, k)) + 3.0
    if patterns is None:
        Y[rng.random((n, k)) < frac] = np.nan
    else:
        for t, fr in enumerate(patterns):
            if fr > 0:
                Y[rng.random(n) < fr, t] = np.nan
    return Y


def traits_ids(X, ids, frac, seed):
    """len(ids) traits; those that share an id are NaN in exactly the same rows"""
    Y = traits(X, len(ids), 0.0, seed)
    miss = np.random.default_rng(seed + 1).random((X.shape[0], max(ids) + 1)) < frac
    for t, g in enumerate(ids):
        Y[miss[:, g], t] = np.nan
    return Y


_cache = {}


def tpod():
    if "tpod" not in _cache:
        _cache["tpod"] = np.asfortranarray(np.load(os.path.join(ROOT, "tests", "golden", "tpod.npz"))["gen"])
    return _cache["tpod"]


def slabs900():
    """synth_small(700, 900): with Panel(nwg=3) three row slabs and 15 marker blocks, the last of 4 markers"""
    if "s900" not in _cache:
        _cache["s900"] = np.asfortranarray(synth_small(700, 900, seed=3)[0])
    return _cache["s900"]


def gauss(n, q, seed):
    return np.asfortranarray(np.random.default_rng(seed).normal(size=(n, q)))


def _tpod_k3():
    X = tpod()
    return traits(X, 3, 0.1, seed=11), [("panel", X, {})]


def _slabs_k5():
    X = slabs900()
    return traits(X, 5, 0, seed=5, patterns=[0.1, 0.0, 0.25, 0.05, 0.4]), [("panel", X, dict(nwg=3))]


def _k1():
    X = tpod()
    return traits(X, 1, 0.1, seed=13), [("panel", X, {})]


K16_IDS = [t % 5 for t in range(16)]   # (16, 5) of tests/mrr_cases.py: the inverses do not fit in LDS, every Gram does


def _k16():
    X = slabs900()
    return traits_ids(X, K16_IDS, 0.1, seed=121), [("panel", X, dict(nwg=3))]


def _bending():
    """the collinear traits of test_gpu_mrr.py::test_bending_branch: MinDVb is about 1e-9 and the matrix bends in every sweep"""
    X = tpod()
    Y = traits(X, 3, 0.0, seed=3)
    Y[:, 1] = Y[:, 0] + 1e-3 * Y[:, 1]
    Y[:, 2] = -Y[:, 0] + 1e-3 * Y[:, 2]
    return Y, [("panel", X, {})]


def _two_panels():
    """tpod's columns split 200 / 176, neither a multiple of 64: the residual crosses from one gathered panel's last partial block to the next
    panel's first"""
    X = tpod()
    return traits(X, 3, 0.1, seed=17), [("panel", np.asfortranarray(X[:, :200]), {}), ("panel", np.asfortranarray(X[:, 200:]), {})]


def _panel_dense(q, seed, first="panel"):
    def data():
        X = tpod()
        effs = [("panel", X, {}), ("dense", gauss(X.shape[0], q, seed))]
        return traits(X, 3, 0.1, seed=19), effs if first == "panel" else effs[::-1]
    return data


def _dense_only(n, q, seed):
    def data():
        Z = gauss(n, q, seed)
        return traits(Z, 3, 0.1, seed=seed + 1), [("dense", Z)]
    return data


def _default_logtol():
    X = tpod()
    return traits(X, 2, 0.1, seed=31), [("panel", X, {})]


# ---- int8 codes beyond 0 / 1 / 2: PEGS never centres X, so the codes' sign, range and mean reach XX, XSX, the Grams and the fitted values ----

def _i8(A):
    assert A.min() >= -128 and A.max() <= 127
    return np.asfortranarray(A.astype(np.int8))


def _panel(name):
    """signed: tpod - 1 (-1 / 0 / 1).  full: 300 x 200 uniform in -128..127, both ends in column 0.  offset: tpod + 100 (a mean 140 times the
    spread).  pm127: 500 x 70 of +-127.  const_cols: tpod with an all-0 column (XX = 0) and an all-2 column (XSX = 0 with XX > 0).
    full_slabs: 700 x 900 uniform in -128..127, for Panel(nwg=3) -- slabs900's geometry."""
    key = "codes_" + name
    if key not in _cache:
        rng = np.random.default_rng(91)
        if name == "signed":
            A = tpod().astype(np.int16) - 1
        elif name == "full":
            A = rng.integers(-128, 128, size=(300, 200))
            A[0, 0], A[1, 0] = -128, 127
        elif name == "offset":
            A = tpod().astype(np.int16) + 100
        elif name == "pm127":
            A = np.where(rng.random((500, 70)) < 0.5, -127, 127)
        elif name == "const_cols":
            A = tpod().astype(np.int16)
            A[:, 37], A[:, 301] = 0, 2
        else:
            assert name == "full_slabs"
            A = rng.integers(-128, 128, size=(700, 900))
            A[0, 0], A[1, 0] = -128, 127
        _cache[key] = _i8(A)
    return _cache[key]


CODE_PANELS = ("signed", "full", "offset", "pm127", "const_cols", "full_slabs")
CODES_SEED = 11


def _codes(name, k=3):
    def data():
        X = _panel(name)
        return traits(X, k, 0.1, seed=CODES_SEED), [("panel", X, {})]
    return data


def _codes_slabs_k5():
    X = _panel("full_slabs")
    return traits(X, 5, 0, seed=5, patterns=[0.1, 0.0, 0.25, 0.05, 0.4]), [("panel", X, dict(nwg=3))]


def _codes_k16():
    X = _panel("full")
    return traits_ids(X, K16_IDS, 0.1, seed=121), [("panel", X, {})]


def _codes_two_ranges():
    """two panels of different code ranges against one residual: tpod - 1 on the first 200 columns, tpod + 100 on the other 176"""
    A, B = _panel("signed"), _panel("offset")
    return traits(tpod(), 3, 0.1, seed=17), [("panel", np.asfortranarray(A[:, :200]), {}), ("panel", np.asfortranarray(B[:, 200:]), {})]


def _codes_full_dense():
    X = _panel("full")
    return traits(X, 3, 0.1, seed=19), [("panel", X, {}), ("dense", gauss(X.shape[0], 70, 23))]


GRAM_BOUND_N = ((1 << 31) - 1) // (127 * 127)   # 133 144: the most rows of +-127 whose column sums of squares fit the int32 Gram


def gram_bound():
    """test_gpu_mrr.py::test_int32_gram_bound's shape for PEGS and PEGSX: (X of n + 1 rows of +-127 by 70 columns, Y on the first n rows
    with trait 0 fully observed, so that its pattern's Gram diagonal is n 127^2, and Y1 on all n + 1)"""
    if "gram_bound" not in _cache:
        n = GRAM_BOUND_N
        assert n * 127 * 127 < (1 << 31) <= (n + 1) * 127 * 127
        X = np.asfortranarray(np.where(np.random.default_rng(101).random((n + 1, 70)) < 0.5, -127, 127).astype(np.int8))
        Y = traits(X[:n], 2, 0, seed=102, patterns=[0.0, 0.1])
        assert np.sum(~np.isnan(Y[:, 0])) == n and np.sum(np.isnan(Y[:, 1])) > 0
        _cache["gram_bound"] = (X, Y, traits(X, 2, 0.1, seed=103))
    return _cache["gram_bound"]


def _case(id_, entry, data, **kw):
    kw.setdefault("logtol", NOSTOP)
    return dict(id=id_, entry=entry, data=data, kw=kw)


# covMinEv: vb's eigenvalues on these traits lie within a factor two of the default 1e-3, so every case below was checked (and its
# threshold or seed chosen) so that the guards of tests/test_pegs_cpu.py hold; a case that states no covMinEv holds at the default
CASES = [
    _case("tpod_k3_defaults", "PEGS", _tpod_k3, maxit=12),
    _case("tpod_k3_xfa0", "PEGS", _tpod_k3, maxit=12, XFA=0),
    _case("tpod_k3_xfa1", "PEGS", _tpod_k3, maxit=12, XFA=1),
    _case("tpod_k3_xfa2", "PEGS", _tpod_k3, maxit=12, XFA=2),
    _case("tpod_k3_nnc_off", "PEGS", _tpod_k3, maxit=12, NNC=False),
    _case("tpod_k3_covbend2", "PEGS", _tpod_k3, maxit=12, covbend=2.0),
    _case("slabs_k5_patterns", "PEGS", _slabs_k5, maxit=6),
    _case("k1", "PEGS", _k1, maxit=12),
    _case("k16_shared_patterns", "PEGS", _k16, maxit=4),
    _case("bending_nnc_on", "PEGS", _bending, maxit=4),
    _case("bending_nnc_off", "PEGS", _bending, maxit=4, NNC=False),
    _case("pegsz_two_panels", "PEGSZ", _two_panels, maxit=8),
    _case("pegsz_panel_dense70", "PEGSZ", _panel_dense(70, 23), maxit=8),
    _case("pegsz_dense70_panel", "PEGSZ", _panel_dense(70, 23, first="dense"), maxit=8),
    _case("pegsz_panel_dense1", "PEGSZ", _panel_dense(1, 29), maxit=8),
    _case("pegsz_dense_only_n196", "PEGSZ", _dense_only(196, 70, 41), maxit=8),
    _case("pegsz_dense_only_n700", "PEGSZ", _dense_only(700, 70, 43), maxit=6),
    _case("pegs_one_effect_as_pegsz", "PEGSZ", _tpod_k3, maxit=12),
    _case("default_logtol", "PEGS", _default_logtol, logtol=-4.0),
]
# the code-range cases.  On large codes vb scales as 1 / x^2, far below the default covMinEv, so at the default these fits bend in every
# sweep; the *_unbent cases state a covMinEv below every sweep's MinDVb (chosen on the restatement) and run the other side of the branch
CODE_CASES = [
    _case("codes_signed", "PEGS", _codes("signed"), maxit=8),
    _case("codes_full", "PEGS", _codes("full"), maxit=8),
    _case("codes_offset", "PEGS", _codes("offset"), maxit=8),
    _case("codes_pm127", "PEGS", _codes("pm127"), maxit=8),
    _case("codes_const_cols", "PEGS", _codes("const_cols"), maxit=8),
    _case("codes_full_slabs_k5", "PEGS", _codes_slabs_k5, maxit=6),
    _case("codes_full_unbent", "PEGS", _codes("full"), maxit=8, covMinEv=1e-9),
    _case("codes_pm127_unbent", "PEGS", _codes("pm127"), maxit=8, covMinEv=1e-9),
    _case("codes_offset_xfa2_unbent", "PEGS", _codes("offset"), maxit=8, XFA=2, covMinEv=1e-9),
    _case("codes_full_k16", "PEGS", _codes_k16, maxit=4),
    _case("pegsz_codes_signed_offset", "PEGSZ", _codes_two_ranges, maxit=8),
    _case("pegsz_codes_full_dense70", "PEGSZ", _codes_full_dense, maxit=8),
]
CASES += CODE_CASES
# the restatement's trace must say that these inflated in every sweep
BENDS = ("bending_nnc_on", "bending_nnc_off", "codes_full", "codes_offset", "codes_pm127", "codes_full_slabs_k5", "codes_full_k16")


def by_id(id_):
    return next(c for c in CASES if c["id"] == id_)


def designs(effects):
    """the effects as float64 matrices, for the restatement"""
    return [np.asarray(e[1], np.float64) for e in effects]


def restate(case):
    """the restatement's fit of a case with its trace, computed once per process"""
    import pegs_restatement as PR
    key = ("fit", case["id"])
    if key not in _cache:
        Y, effects = case["data"]()
        if case["entry"] == "PEGSZ_sparse":        # text 2 (tests/tall_cases.py runs it beside a panel); its fit always carries the trace
            import pegs_sparse_restatement as SR
            fit = SR.pegsz_sparse(Y, designs(effects), **case["kw"])
        else:
            fit = PR.pegsz(Y, designs(effects), own_text=case["entry"] == "PEGS", trace=True, **case["kw"])
        _cache[key] = (Y, effects, fit)
    return _cache[key]
