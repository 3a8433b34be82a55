"""The cases of tests/test_mt_tight_cpu.py and tests/test_gpu_mt_tight.py: inputs on which the multi-trait fp64 fits -- mrr / mrr_float on the
int8 launch train, mrr(Y, dense(X)) and mkr on the dense train, PEGS and PEGSZ, the sparse legs, PEGSX -- are held to the bounds of tests/mt_tight.py.  They are
made by the generators of tests/test_gpu_mrr.py, tests/mkr_cases.py, tests/pegs_cases.py, tests/pegsx_cases.py and tests/pegs_sparse_cases.py, cut to the smallest shape that still reaches the path
a case is there for; every fit runs every sweep (tol = 0, logtol = -inf), three to six of them, unless the case says otherwise.

A case is dict(family, Y, kw, ...):
  "mrr"    X int8, variant "D" (mrr) or "F" (mrr_float), panel (the name of the Panel a GPU module shares between the cases of one shape) and
           panel_kw.  The int8 train centres implicitly, so its bounds carry kappa (tests/mt_tight.py).
  "dense"  X float64, fitted as mrr(Y, dense(X)); device=True: from a tensor on the device; K: fitted as mkr(Y, K) with X = K2X(K) made once
           here and handed to the restatement.
  "pegs"   entry "PEGS" / "PEGSZ" / "PEGS_sparse" / "PEGSZ_sparse" and effects as tests/pegs_cases.py writes them: ("panel", X int8, panel
           kwargs, panel name), ("dense", Z) or ("sparse", A float64 n x q[, stored mask]), which the library receives as
           bwgr_amd.sparse(...) -- with serial=True where the case says so.
  "pegsx"  the same effects beside X (n x f, its first column the intercept), fitted as PEGSX(Y, X, effects).
The panel of the int8 cases is panel132(): synth_small(700, 900) cut to 132 markers, for Panel(nwg=3): three row slabs and blocks of 64, 64
and 4 markers, so k_mrr_pass is called for a block that has both a previous and a next one."""
import functools

import numpy as np

import mkr_cases as MC
import mrr_cases
import pegs_cases as PC
import pegs_sparse_cases as SC
import pegsx_cases as XC
from conftest import synth_small
from test_gpu_mrr import _traits, _traits_ids

NWG3 = dict(nwg=3)
F01 = float(np.float32(0.01))      # mrr_float's priors as the library rounds them


@functools.lru_cache(None)
def panel132():
    return np.asfortranarray(PC.slabs900()[:, :132])


@functools.lru_cache(None)
def tpod():
    return np.array(PC.tpod(), order="F")


@functools.lru_cache(None)
def wide_freq():
    """700 x 132 codes 0/1/2 with allele frequencies from 0.05 to 0.95: columns whose mean is up to six times their spread"""
    rs = np.random.RandomState(17)
    f = rs.uniform(0.05, 0.95, 132)
    return np.asfortranarray((rs.uniform(size=(700, 132)) < f).astype(np.int8) + (rs.uniform(size=(700, 132)) < f).astype(np.int8))


@functools.lru_cache(None)
def signed132():
    return np.asfortranarray((panel132().astype(np.int16) - 1).astype(np.int8))


@functools.lru_cache(None)
def full_range():
    rng = np.random.default_rng(91)
    X = rng.integers(-128, 128, size=(300, 200)).astype(np.int8)
    X[0, 0], X[1, 0] = -128, 127
    return np.asfortranarray(X)


@functools.lru_cache(None)
def rows2200():
    return np.asfortranarray(synth_small(2200, 68, seed=9)[0])


def kappa(X):
    """max over the columns of sum x^2 / sum (x - mean)^2 over all rows, in long double"""
    X = np.asarray(X, np.longdouble)
    return float(((X ** 2).sum(0) / ((X - X.mean(0)) ** 2).sum(0)).max())


def _mrr(Y, X, panel, sweeps=3, variant="D", panel_kw=None, **kw):
    return dict(family="mrr", Y=Y, X=X, variant=variant, panel=panel, panel_kw=dict(panel_kw or {}), kw=dict(dict(maxit=sweeps, tol=0), **kw))


def _on132(Y, sweeps=3, **kw):
    return _mrr(Y, panel132(), "panel132", sweeps, panel_kw=NWG3, **kw)


# ---- mrr on the int8 train ----
REGIMES = {(6, 6): 1, (7, 7): 2, (15, 15): 3, (16, 5): 4, (16, 16): 5, (9, 9): 2}   # (k, npat) of mrr_cases.K_SWEEP -> k_mrr_solve's regime
assert set(REGIMES) <= set(mrr_cases.K_SWEEP)


def _k_sweep(k, npat):
    return _on132(_traits_ids(panel132(), [t % npat for t in range(k)], 0.1, seed=100 + k + npat))


def _shared(i):
    ids = mrr_cases.SHARED[i]
    return _on132(_traits_ids(panel132(), ids, 0.15, seed=7 + len(ids)), 4)


def _tpod_k3(variant):
    kw = dict(weight_prior_h2=F01, weight_prior_gc=F01) if variant == "F" else {}
    return _mrr(_traits(tpod(), 3, 0.1, seed=11), tpod(), "tpod", 6, variant, **kw)


OPTIONS = {"TH": dict(TH=True), "HCS": dict(HCS=True), "XFA": dict(XFA=True, NumXFA=2), "ACS": dict(ACS=True, NumXFA=2), "OneVarB": dict(OneVarB=True),
           "OneVarE": dict(OneVarE=True), "updateMu": dict(updateMu=True), "no_priors": dict(weight_prior_h2=0.0, weight_prior_gc=0.0)}


def _option(name):
    return _mrr(_traits(tpod(), 3, 0.1, seed=21), tpod(), "tpod", 4, **OPTIONS[name])


def _bending():
    """test_gpu_mrr.test_bending_branch: collinear traits, one factor, no prior on GC: GC has a negative eigenvalue and bends"""
    Y = _traits(tpod(), 3, 0.0, seed=3)
    Y[:, 1] = Y[:, 0] + 1e-3 * Y[:, 1]
    Y[:, 2] = -Y[:, 0] + 1e-3 * Y[:, 2]
    return _mrr(Y, tpod(), "tpod", 4, XFA=True, NumXFA=1, weight_prior_gc=0)


def _tpod_p(p):
    X = np.asfortranarray(tpod()[:, :p])
    return _mrr(_traits(X, 3, 0.1, seed=200 + p + 3), X, "tpod_p%d" % p, 3 if p == 1 else 6)


def _rows2200():
    """2 200 rows in the default slabs: more 64-row tiles than k_mrr_pass has workgroups"""
    X = rows2200()
    return _mrr(_traits(X, 3, 0, seed=13, patterns=[0.1, 0.2, 0.05]), X, "rows2200", 4)


AWKWARD_IDS = (0, 1, 0, 2, 1, 3, 2, 3, 0)
ALL_MISSING = (10, 200, 400, 650)
FIVE_ROWS = (5, 130, 300, 450, 690)


def _awkward_rows():
    """uvb_tight_cases._shared's layout: shared patterns, four rows nobody has, pattern 3 observed on five rows over the three slabs"""
    return _on132(_traits_ids(panel132(), AWKWARD_IDS, 0.2, seed=41, all_missing=ALL_MISSING, sparse=(3, FIVE_ROWS)), 4)


def _wide_freq():
    return _mrr(_traits(wide_freq(), 3, 0.1, seed=51), wide_freq(), "wide_freq", 4, panel_kw=NWG3)


def _signed():
    return _mrr(_traits(panel132(), 3, 0.1, seed=81), signed132(), "signed132", 4, panel_kw=NWG3)


def _full_range():
    return _mrr(_traits(full_range(), 5, 0.1, seed=92), full_range(), "full_range", 4)


STOP_TOL = 10e-9    # mrr's default


def _stopping():
    """the default tol on tpod's first 65 markers: the fit stops by its tolerance"""
    X = np.asfortranarray(tpod()[:, :65])
    return _mrr(_traits(X, 2, 0.1, seed=31), X, "tpod_p65", 500, tol=STOP_TOL)


# ---- the dense train ----
def _dense(Y, X, sweeps=4, **more):
    return dict(family="dense", Y=Y, X=X, kw=dict(maxit=sweeps, tol=0), **more)


def _dense_r(r, k=4, n=200):
    X = MC.real_design(n, r, 30 + r)
    return _dense(MC.traits(X, k, 40 + r + k, frac=0.1), X, 3 if k == 16 else 4)


def _dense_tall():
    """2 200 rows: 2 304 padded rows = 36 tiles on 32 workgroups, a second trip of k_mrrd_pass's and k_mrrd_gram's tile loops"""
    X = MC.real_design(2200, 65, 51)
    return _dense(MC.traits(X, 4, 52, frac=0.1), X, 3)


def _dense_device():
    c = _dense_r(65)
    return dict(c, device=True)


def _mkr():
    import bwgr_amd
    K = MC.grm150()
    X = bwgr_amd.K2X(K)
    return _dense(MC.traits(X, 3, 21, frac=0.15), X, 5, K=K)


# ---- PEGS / PEGSZ ----
def _pegs(entry, Y, effects, sweeps=4, **kw):
    return dict(family="pegs", entry=entry, Y=Y, effects=effects, kw=dict(dict(maxit=sweeps, logtol=PC.NOSTOP), **kw))


def _p132():
    return ("panel", panel132(), NWG3, "panel132")


def _pegs_k3(**kw):
    return _pegs("PEGS", PC.traits(panel132(), 3, 0.1, seed=11), [_p132()], **kw)


def _pegs_k5():
    return _pegs("PEGS", PC.traits(panel132(), 5, 0, seed=5, patterns=[0.1, 0.0, 0.25, 0.05, 0.4]), [_p132()])


def _pegs_k16():
    return _pegs("PEGS", PC.traits_ids(panel132(), PC.K16_IDS, 0.1, seed=121), [_p132()], 3)


def _pegsz_q(q):
    return _pegs("PEGSZ", PC.traits(panel132(), 3, 0.1, seed=19), [_p132(), ("dense", PC.gauss(700, q, 23 + q))])


def _pegsz_dense_only():
    Z = PC.gauss(196, 70, 41)
    return _pegs("PEGSZ", PC.traits(Z, 3, 0.1, seed=42), [("dense", Z)])


def _pegs_signed():
    return _pegs("PEGS", PC.traits(signed132(), 3, 0.1, seed=11), [("panel", signed132(), NWG3, "signed132")])


# ---- PEGSX: the fixed step, the three trace kernels, k_pegs_zb on the fixed design ----
def _pegsx(Y, X, effects, sweeps=4, **kw):
    return dict(family="pegsx", Y=Y, X=X, effects=effects, kw=dict(dict(maxit=sweeps, logtol=PC.NOSTOP), **kw))


def _px132(ncov, k=3, sweeps=4, Z=None, seed=300, **kw):
    """the 700 x 132 panel in three slabs beside an intercept and ncov covariates: f = ncov + 1"""
    Z = _p132() if Z is None else Z
    X = XC.fixed(700, ncov, seed + ncov)
    return _pegsx(XC.with_fixed(PC.traits(Z[1], k, 0.1, seed=seed + 50 + ncov), X, seed + 100 + ncov), X, [Z], sweeps, **kw)


def _px_f70_k5():
    """f = 70 beside five traits of five patterns: k >= 5 inflates in every sweep"""
    X = XC.fixed(700, 69, 103)
    Y = PC.traits(panel132(), 5, 0, seed=5, patterns=[0.1, 0.0, 0.25, 0.05, 0.4])
    return _pegsx(XC.with_fixed(Y, X, 104), X, [_p132()], 3)


def _px_k1():
    X = XC.fixed(700, 2, 105)
    return _pegsx(XC.with_fixed(PC.traits(panel132(), 1, 0.1, seed=13), X, 106), X, [_p132()])


def _px_k16():
    X = XC.fixed(700, 2, 107)
    return _pegsx(XC.with_fixed(PC.traits_ids(panel132(), PC.K16_IDS, 0.1, seed=121), X, 108), X, [_p132()], 3)


def _px_signed():
    """codes -1 / 0 / 1 beside an intercept and sixteen covariates (the trace's float mutant shows in the non-integer columns of X alone)"""
    return _px132(16, Z=("panel", signed132(), NWG3, "signed132"), seed=320)


def _px_dense(q, first):
    """the panel beside a dense effect of q columns (a partial PEGSX_JC group), either of them first"""
    X = XC.fixed(700, 6, 115 + q)
    effs = [_p132(), ("dense", PC.gauss(700, q, 23 + q))]
    return _pegsx(XC.with_fixed(PC.traits(panel132(), 3, 0.1, seed=19 + q), X, 116 + q), X, effs if first == "panel" else effs[::-1])


N1501 = 1501      # no multiple of 4, and more rows than k_pegsx_fixed has threads


def _px_dense_only():
    Y, X, effs = XC._dense_only(N1501, 70, 45, 2)()
    return _pegsx(Y, X, effs, 3)


def _px_inc12():
    Y, effs, X = SC._mk(SC._inc12, 3, 116, x=SC.fixed)()
    return _pegsx(Y, X, effs)


def _fixed7(n):
    return SC.fixed(n, 6)


def _px_mixed4():
    """[panel, incidence, overlapping, dense]: every kind of effect against one residual, the serial leg among them"""
    Y, effs, X = SC._mk(SC._mixed4, 3, 218, x=_fixed7)()      # (a seed of its own: the table's cache of made data does not know X)
    return _pegsx(Y, X, [e + ("sc_panel200",) if e[0] == "panel" else e for e in effs])


QUAD_ONE, QUAD_ALL = (8, 12), (256, 264)      # rows missing in trait 1 alone; rows missing in every trait


def _px_quad_missing():
    """whole aligned quads of rows without a record: in one pattern, and in all of them"""
    c = _px132(2, seed=340)
    Y = c["Y"].copy()
    Y[QUAD_ONE[0]:QUAD_ONE[1], 1] = np.nan
    Y[QUAD_ALL[0]:QUAD_ALL[1]] = np.nan
    return dict(c, Y=Y)


def _px_rank_deficient():
    """intercept + two complementary 0/1 dummies + four covariates: f = 7, rank 6 in every missingness pattern"""
    rng = np.random.default_rng(109)
    d = (rng.random(700) < 0.45).astype(np.float64)
    X = np.asfortranarray(np.column_stack([np.ones(700), d, 1.0 - d, rng.normal(size=(700, 4))]))
    return _pegsx(XC.with_fixed(PC.traits(panel132(), 3, 0.1, seed=11), X, 110), X, [_p132()])


# ---- the sparse legs: k_pegs_sparse_setup, pegs_sparse_column (serial and disjoint), k_pegs_sparse_hat ----
def _sparse(entry, build, k, seed, sweeps=4, serial=False, **kw):
    Y, effs = SC._mk(build, k, seed)()
    effs = [e + ("sc_panel200",) if e[0] == "panel" else e for e in effs]
    return dict(_pegs(entry, Y, effs, sweeps, **kw), serial=serial)


CASES = {}
for _c in REGIMES:
    CASES["mrr/k%d_npat%d" % _c] = functools.partial(_k_sweep, *_c)
for _i in (0, 1):
    CASES["mrr/shared_k%d" % len(mrr_cases.SHARED[_i])] = functools.partial(_shared, _i)
CASES["mrr/tpod_k3"] = functools.partial(_tpod_k3, "D")
CASES["mrr/tpod_k3_float"] = functools.partial(_tpod_k3, "F")
for _o in OPTIONS:
    CASES["mrr/opt_" + _o] = functools.partial(_option, _o)
CASES["mrr/bending"] = _bending
for _p in mrr_cases.EDGE_P:
    CASES["mrr/tpod_p%d" % _p] = functools.partial(_tpod_p, _p)
CASES["mrr/rows2200"] = _rows2200
CASES["mrr/awkward_rows"] = _awkward_rows
CASES["mrr/wide_freq"] = _wide_freq
CASES["mrr/signed"] = _signed
CASES["mrr/full_range_int8"] = _full_range
CASES["mrr/stopping"] = _stopping
for _r in (1, 63, 64, 65, 132):
    CASES["dense/r%d" % _r] = functools.partial(_dense_r, _r)
CASES["dense/k16"] = functools.partial(_dense_r, 65, 16)
CASES["dense/rows2200"] = _dense_tall
CASES["dense/device"] = _dense_device
CASES["dense/mkr_grm150"] = _mkr
CASES["pegs/k3"] = _pegs_k3
CASES["pegs/k5_inflated"] = _pegs_k5
CASES["pegs/k16"] = _pegs_k16
for _q in (1, 5, 70):
    CASES["pegsz/panel_dense%d" % _q] = functools.partial(_pegsz_q, _q)
CASES["pegsz/dense_only"] = _pegsz_dense_only
CASES["pegs/xfa0"] = functools.partial(_pegs_k3, XFA=0)
CASES["pegs/xfa2"] = functools.partial(_pegs_k3, XFA=2)
CASES["pegs/nnc_off"] = functools.partial(_pegs_k3, NNC=False)
CASES["pegs/signed"] = _pegs_signed
OLD_NAMES = tuple(CASES)      # the 49 cases whose bounds tests/test_mt_tight_cpu.py holds to their recorded bits
for _f, _ncov in ((1, 0), (3, 2), (17, 16)):
    CASES["pegsx/f%d" % _f] = functools.partial(_px132, _ncov)
CASES["pegsx/f70_k5_inflated"] = _px_f70_k5
CASES["pegsx/k1"] = _px_k1
CASES["pegsx/k16_shared"] = _px_k16
CASES["pegsx/signed"] = _px_signed
CASES["pegsx/panel_dense1"] = functools.partial(_px_dense, 1, "panel")
CASES["pegsx/dense5_panel"] = functools.partial(_px_dense, 5, "dense")
CASES["pegsx/dense70_n1501"] = _px_dense_only
CASES["pegsx/inc12"] = _px_inc12
CASES["pegsx/mixed4"] = _px_mixed4
CASES["pegsx/quad_missing"] = _px_quad_missing
CASES["pegsx/nnc"] = functools.partial(_px132, 2, NNC=True)
CASES["pegsx/xfa1"] = functools.partial(_px132, 2, XFA=True, NumXFA=1)
CASES["pegsx/df0_20"] = functools.partial(_px132, 2, df0=20.0)
CASES["pegsx/rank_deficient"] = _px_rank_deficient
CASES["sparse/ps_q1"] = functools.partial(_sparse, "PEGS_sparse", SC._inc1, 3, 104)
CASES["sparse/ps_q12"] = functools.partial(_sparse, "PEGS_sparse", SC._inc12, 3, 101)
CASES["sparse/ps_q70"] = functools.partial(_sparse, "PEGS_sparse", SC._inc70, 3, 105)
CASES["sparse/ps_q12_k1"] = functools.partial(_sparse, "PEGS_sparse", SC._inc12, 1, 102)
CASES["sparse/ps_q12_k5"] = functools.partial(_sparse, "PEGS_sparse", SC._inc12, 5, 103)
CASES["sparse/ps_q12_k16"] = functools.partial(_sparse, "PEGS_sparse", SC._inc12, 16, 131, 3)
CASES["sparse/ps_empty_col"] = functools.partial(_sparse, "PEGS_sparse", SC._inc_empty, 3, 107)
CASES["sparse/ps_long_cols"] = functools.partial(_sparse, "PEGS_sparse", SC._inc_long, 3, 108, 3)
CASES["sparse/ps_overlap_serial_leg"] = functools.partial(_sparse, "PEGS_sparse", SC._overlap, 3, 109)
CASES["sparse/ps_weighted"] = functools.partial(_sparse, "PEGS_sparse", SC._weighted, 3, 125)
CASES["sparse/pzs_two_inc"] = functools.partial(_sparse, "PEGSZ_sparse", SC._two_inc, 3, 110)
CASES["sparse/pz_panel_inc"] = functools.partial(_sparse, "PEGSZ", SC._panel_inc, 3, 112)
CASES["sparse/ps_q4133"] = functools.partial(_sparse, "PEGS_sparse", SC._inc_trip, 3, 106, 2)
CASES["sparse/ps_q12_forced_serial"] = functools.partial(_sparse, "PEGS_sparse", SC._inc12, 3, 101, serial=True)
NAMES = tuple(CASES)
ORDINARY_012 = ("panel132", "tpod", "tpod_p1", "tpod_p63", "tpod_p64", "tpod_p65", "rows2200")   # the panels whose kappa must stay below 4


@functools.lru_cache(None)
def case(name):
    c = CASES[name]()
    for A in [c["Y"], c.get("X"), c.get("K")] + [a for e in c.get("effects", ()) for a in e[1:3] if isinstance(a, np.ndarray)]:
        if A is not None:
            A.setflags(write=False)
    return c
