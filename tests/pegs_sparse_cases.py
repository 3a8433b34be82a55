"""The cases of the sparse-effect tests, in one table: tests/test_gpu_pegs_sparse.py runs each on the GPU against the restatements
(tests/pegs_restatement.py, tests/pegsx_restatement.py and, for PEGSZ_sparse's text, tests/pegs_sparse_restatement.py) on the dense copy of
every sparse design, and tests/test_pegs_sparse_cpu.py checks on the restatement alone that none of them sits on the fit's discontinuous
branch (MinDVb < covMinEv) or on a near-degenerate eigen-gap where XFA truncates.

A case: id, entry ("PEGS_sparse" / "PEGSZ_sparse" / "PEGSZ" / "PEGSX"), data() -> (Y, effects[, X]), kw (the fit's arguments).  An effect is
("sparse", A float64 n x q[, stored mask]), ("panel", X int8, panel kwargs) or ("dense", Z float64); the values of a sparse design are
floats already.  n = 300 (no multiple of 64) unless a case says otherwise; about 20 % of the records are missing, one trait is missing on a
whole level of the first sparse effect, and a few rows are missing for every trait.  Every case runs with logtol = -inf (every sweep).

The cases of the second round (from ps_setup_trip_k3 on) are there for one edge of the kernels each -- a second trip of the set-up kernel,
the sparse trace kernel at the cap of its grid, f past one and up to four lane strides, sixteen patterns, the serial leg's hand-off between
long columns that share rows, values other than 1 on the disjoint leg, a level without a record -- stated beside each case in the table and
asserted from the plan hooks by tests/test_pegs_sparse_cpu.py::test_second_round_cases_reach_what_they_are_listed_for.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pegs_sparse_restatement as SR  # noqa: E402

NOSTOP = float("-inf")
N = 300
TRIP_COLS = 4096          # the columns one trip of the disjoint grid covers (test_pegs_sparse_cpu.py holds it against the plan hook)
_cache = {}


def incidence(n, q, seed, member=1.0, empty=()):
    """the incidence matrix of a factor with q levels: every row belongs to one level (with probability `member`, else to none), no row to
    a level in `empty`; every other level has at least one row"""
    rng = np.random.default_rng(seed)
    live = [j for j in range(q) if j not in empty]
    lev = rng.choice(live, size=n)
    rows = rng.permutation(n)[:len(live)] if len(live) <= n else None
    if rows is not None and member == 1.0:
        lev[rows] = live                                   # no live level without a row
    A = np.zeros((n, q))
    A[np.arange(n), lev] = 1.0
    if member < 1.0:
        A[rng.random(n) >= member] = 0.0
    return A


def overlapping(n, q, seed, density=0.08):
    """normal values at `density`, negative ones among them; a few stored zeros -> (A, stored mask)"""
    rng = np.random.default_rng(seed)
    stored = rng.random((n, q)) < density
    A = SR.f32(np.where(stored, rng.normal(size=(n, q)), 0.0))
    zr, zc = np.nonzero(stored)
    pick = rng.permutation(len(zr))[:7]
    A[zr[pick], zc[pick]] = 0.0                            # stored, and zero
    assert (A < 0).any() and (stored & (A == 0)).sum() == 7 and not SR.row_disjoint(A)
    return A, stored


def panel(n, p, seed):
    return np.asfortranarray(np.random.default_rng(seed).integers(0, 3, size=(n, p)).astype(np.int8))


def gauss(n, q, seed):
    return np.asfortranarray(SR.f32(np.random.default_rng(seed).normal(size=(n, q))))


def design(eff):
    """an effect as a float64 matrix, for the restatements"""
    return np.asarray(eff[1], np.float64)


def traits(effects, k, seed, frac=0.2):
    """k traits: a part on every effect's columns (correlated over the traits), unit noise, mean 3; then the missing records"""
    rng = np.random.default_rng(seed)
    n = effects[0][1].shape[0]
    L = rng.normal(size=(k, k)) * 0.5 + np.eye(k)
    G = np.zeros((n, k))
    for eff in effects:
        D = design(eff)
        D = D - D.mean(0)
        part = D @ (rng.normal(size=(D.shape[1], k)) @ L)
        sd = part.std(0)
        G += part / np.where(sd > 0, sd, 1.0)
    Y = G + rng.normal(size=(n, k)) + 3.0
    Y[rng.random((n, k)) < frac] = np.nan
    first = next((design(e) for e in effects if e[0] == "sparse"), None)
    if first is not None:                                  # trait min(1, k - 1) has no record on a whole level of the first sparse effect
        sizes = (first != 0).sum(0)
        lvl = int(np.argsort(sizes)[len(sizes) // 2]) if first.shape[1] > 1 else None
        if lvl is not None and 0 < sizes[lvl] < n // 2:
            Y[first[:, lvl] != 0, min(1, k - 1)] = np.nan
    Y[[7, n // 2, n - 1]] = np.nan                         # rows with no record at all
    return Y


def _mk(build, k, seed, x=None):
    def data():
        key = (build.__name__, k, seed)
        if key not in _cache:
            effects = build()
            Y = traits(effects, k, seed)
            _cache[key] = (Y, effects) if x is None else (Y, effects, x(effects[0][1].shape[0]))
        return _cache[key]
    return data


def fixed(n, ncov=2):
    """PEGSX's X: an intercept and ncov covariates, rounded to float"""
    return np.asfortranarray(np.column_stack([np.ones(n), SR.f32(np.random.default_rng(77).normal(size=(n, ncov)))]))


def fixed70(n):
    return fixed(n, 69)


def _inc12(): return [("sparse", incidence(N, 12, 1))]
def _inc1(): return [("sparse", incidence(N, 1, 2, member=0.4))]
def _inc70(): return [("sparse", incidence(N, 70, 3))]
def _inc_trip(): return [("sparse", incidence(N, TRIP_COLS + 37, 4))]
def _inc_empty(): return [("sparse", incidence(N, 12, 5, empty=(4,)))]


def _inc_long():
    """n = 2100: a level of more than 1024 rows, one of more than 64, a small one"""
    lev = np.repeat([0, 1, 2, 3], [1100, 700, 250, 50])
    A = np.zeros((2100, 4))
    A[np.arange(2100), np.random.default_rng(6).permutation(lev)] = 1.0
    return [("sparse", A)]


def _overlap(): return [("sparse",) + overlapping(N, 25, 7)]
def _two_inc(): return [("sparse", incidence(N, 12, 8)), ("sparse", incidence(N, 7, 9))]
def _panel_inc(): return [("panel", panel(N, 200, 10), {}), ("sparse", incidence(N, 12, 11))]
def _panel_inc70(): return [("panel", panel(N, 200, 10), {}), ("sparse", incidence(N, 70, 12))]
def _mixed4(): return [("panel", panel(N, 200, 10), {}), ("sparse", incidence(N, 12, 13)), ("sparse",) + overlapping(N, 25, 14), ("dense", gauss(N, 9, 15))]
def _inc_overlap(): return [("sparse", incidence(N, 12, 16)), ("sparse",) + overlapping(N, 25, 17)]


# ---- the second round: every loop bound and stride of csrc/pegs_sparse.hip.h that the table above stops short of ----
SETUP_TRIP_COLS = 32768   # the columns one trip of k_pegs_sparse_setup covers (8 192 workgroups of four waves, a column each)
N2 = 700                  # rows of the cases with f = 256 or columns of three lane strides (no multiple of 64 either)


def placed(n, q, seed, last=40):
    """an incidence far wider than it is tall, which incidence() would leave empty at the far end: `last` rows (none of those that traits()
    leaves without any record) sit on the last `last` columns, one each, the other rows on random levels"""
    rng = np.random.default_rng(seed)
    lev = rng.integers(0, q - last, size=n)
    rows = np.setdiff1d(np.arange(n), [7, n // 2, n - 1])
    lev[rng.permutation(rows)[:last]] = np.arange(q - last, q)
    A = np.zeros((n, q))
    A[np.arange(n), lev] = 1.0
    return A


def weighted(n, q, seed):
    """a covariate nested in a factor: a row-disjoint matrix of float-rounded normal values, negative ones among them, and five stored zeros
    -> (A, stored mask)"""
    inc = incidence(n, q, seed)
    rng = np.random.default_rng(seed + 1000)
    A = inc * SR.f32(rng.normal(size=n))[:, None]
    stored = inc != 0
    A[rng.permutation(n)[:5]] = 0.0                        # stored, and zero
    assert SR.row_disjoint(A) and (A < 0).any() and (stored & (A == 0)).sum() == 5 and stored.sum() == n
    return A, stored


def unobserved_level(n, q, seed, level=5):
    """an incidence one level of which consists of exactly the rows that traits() leaves without a record in any trait"""
    gone = [7, n // 2, n - 1]
    rest = np.setdiff1d(np.arange(n), gone)
    A = np.zeros((n, q))
    A[np.ix_(rest, np.arange(q) != level)] = incidence(len(rest), q - 1, seed)
    A[gone, level] = 1.0
    assert SR.row_disjoint(A) and np.array_equal(np.flatnonzero(A[:, level]), gone) and (A.sum(0) > 0).all()
    return A


def unobserved_column(A, Y):
    """the one column of A that has stored entries and no record under them in any trait"""
    seen = (np.asarray(A) != 0).T.astype(float) @ (~np.isnan(Y)).any(1).astype(float)
    cols = np.flatnonzero((seen == 0) & ((np.asarray(A) != 0).sum(0) > 0))
    assert len(cols) == 1
    return int(cols[0])


def _inc_setup_trip(): return [("sparse", placed(N, SETUP_TRIP_COLS + 37, 20))]
def _inc_trace_cap(): return [("sparse", placed(N, 16501, 21))]
def _inc70_overlap(): return [("sparse", incidence(N, 70, 22)), ("sparse",) + overlapping(N, 25, 23)]
def _inc12_overlap_n700(): return [("sparse", incidence(N2, 12, 24)), ("sparse",) + overlapping(N2, 25, 25)]
def _overlap_long(): return [("sparse",) + overlapping(N2, 130, 26, density=0.25)]
def _inc12_overlap_long(): return [("sparse", incidence(N2, 12, 27))] + _overlap_long()
def _weighted(): return [("sparse",) + weighted(N, 12, 28)]
def _unobserved(): return [("sparse", unobserved_level(N, 12, 29))]


def _f256_data():
    """px_f256_k3: X and its share of Y as tests/tall_cases.py's f256 job builds them (an intercept and 255 covariates, X beta added to Y)"""
    import pegsx_cases as XC
    key = "f256"
    if key not in _cache:
        effects = _inc12_overlap_n700()
        X = XC.fixed(N2, 255, 501)
        _cache[key] = (XC.with_fixed(traits(effects, 3, 126), X, 502), effects, X)
    return _cache[key]


def _case(id_, entry, data, **kw):
    kw.setdefault("logtol", NOSTOP)
    return dict(id=id_, entry=entry, data=data, kw=kw)


CASES = [
    _case("ps_inc12_k3", "PEGS_sparse", _mk(_inc12, 3, 101), maxit=8),
    _case("ps_inc12_k1", "PEGS_sparse", _mk(_inc12, 1, 102), maxit=8),
    _case("ps_inc12_k5_xfa2", "PEGS_sparse", _mk(_inc12, 5, 103), maxit=6, XFA=2),
    _case("ps_inc12_k3_xfa0", "PEGS_sparse", _mk(_inc12, 3, 101), maxit=8, XFA=0),
    _case("ps_q1_k3", "PEGS_sparse", _mk(_inc1, 3, 104), maxit=8),
    _case("ps_inc70_k3", "PEGS_sparse", _mk(_inc70, 3, 105), maxit=8),
    _case("ps_trip_k3", "PEGS_sparse", _mk(_inc_trip, 3, 106), maxit=6),
    _case("ps_empty_col_k3", "PEGS_sparse", _mk(_inc_empty, 3, 107), maxit=8),
    _case("ps_long_cols_k3", "PEGS_sparse", _mk(_inc_long, 3, 108), maxit=6),
    _case("ps_overlap_k3", "PEGS_sparse", _mk(_overlap, 3, 109), maxit=8),
    _case("pzs_two_inc_k3", "PEGSZ_sparse", _mk(_two_inc, 3, 110), maxit=8),
    _case("pzs_inc_overlap_k5_xfa2", "PEGSZ_sparse", _mk(_inc_overlap, 5, 111), maxit=6, XFA=2),
    _case("pzs_inc12_k1", "PEGSZ_sparse", _mk(_inc12, 1, 102), maxit=8),
    _case("pz_two_inc_k3", "PEGSZ", _mk(_two_inc, 3, 110), maxit=8),
    _case("pz_panel_inc_k3", "PEGSZ", _mk(_panel_inc, 3, 112), maxit=8),
    _case("pz_panel_inc70_k16_xfa2", "PEGSZ", _mk(_panel_inc70, 16, 113), maxit=6, XFA=2),
    _case("pz_mixed4_k3", "PEGSZ", _mk(_mixed4, 3, 114), maxit=8),
    _case("pz_mixed4_k5_xfa0", "PEGSZ", _mk(_mixed4, 5, 115), maxit=6, XFA=0),
    _case("px_inc12_k3", "PEGSX", _mk(_inc12, 3, 116, x=fixed), maxit=8),
    _case("px_overlap_k1", "PEGSX", _mk(_overlap, 1, 117, x=fixed), maxit=8),
    _case("px_mixed4_k3_xfa2", "PEGSX", _mk(_mixed4, 3, 118, x=fixed), maxit=8, XFA=True, NumXFA=2, covMinEv=1e-5),   # (at the default a sweep's MinDVb comes within 0.3 % of it)
    _case("px_panel_inc70_k5", "PEGSX", _mk(_panel_inc70, 5, 119, x=fixed), maxit=6),
    # the second round; what each is there for (tests/test_pegs_sparse_cpu.py asserts it from the plan hooks):
    # a second trip of k_pegs_sparse_setup with its last column occupied, and k_mrr_tilde's second and third trips over d2
    _case("ps_setup_trip_k3", "PEGS_sparse", _mk(_inc_setup_trip, 3, 120), maxit=2),
    # k_pegsx_trace_sparse at its cap of 1 024 workgroups: four whole trips of 4 096 columns and a fifth that ends on the last column
    _case("px_trace_cap_k3", "PEGSX", _mk(_inc_trace_cap, 3, 121, x=fixed), maxit=2),
    # f > 64: a second step of both lane loops of the sparse trace; sixteen patterns in tot[g]; k = 16 on the serial leg beside a disjoint one
    _case("px_f70_k16", "PEGSX", _mk(_inc70_overlap, 16, 122, x=fixed70), maxit=4),
    # f = 256: four steps of the lane loops, the whole of a wave's LDS region
    _case("px_f256_k3", "PEGSX", _f256_data, maxit=4),
    # the serial leg's hand-off: columns of three lane strides that share rows, more columns than a wave has lanes, the shuffles for t up to 15
    _case("ps_overlap_long_k16", "PEGS_sparse", _mk(_overlap_long, 16, 123), maxit=4, XFA=2),
    _case("pzs_inc_overlap_long_k3", "PEGSZ_sparse", _mk(_inc12_overlap_long, 3, 124), maxit=4),
    # the disjoint leg on values other than 1: XX is no count, v is negative, fractional or a stored zero
    _case("ps_weighted_k3", "PEGS_sparse", _mk(_weighted, 3, 125), maxit=8),
    # a column with stored entries and XX = 0 in every trait: Linv_j is the inverse of iG alone, b_j stays 0
    _case("ps_unobserved_level_k3", "PEGS_sparse", _mk(_unobserved, 3, 127), maxit=8),
]
TRZSZ_ALONE = ("px_trace_cap_k3",)      # a maxit = 0 run that checks TrZSZ by itself
# the cases whose sparse effects are all row-disjoint: the plan takes the disjoint leg, and serial=True must give the same bits
DISJOINT = ("ps_inc12_k3", "ps_inc12_k1", "ps_inc12_k5_xfa2", "ps_inc12_k3_xfa0", "ps_q1_k3", "ps_inc70_k3", "ps_trip_k3", "ps_empty_col_k3",
            "ps_long_cols_k3", "pzs_two_inc_k3", "pzs_inc12_k1", "pz_two_inc_k3", "pz_panel_inc_k3", "pz_panel_inc70_k16_xfa2", "px_inc12_k3",
            "px_panel_inc70_k5", "ps_setup_trip_k3", "px_trace_cap_k3", "ps_weighted_k3", "ps_unobserved_level_k3")


def by_id(id_):
    return next(c for c in CASES if c["id"] == id_)


def restate(case, **more):
    """the restatement's fit of a case on the dense copies, computed once per process -> (data, fit)"""
    import pegs_restatement as PR
    import pegsx_restatement as PXR
    key = ("fit", case["id"], tuple(sorted(more.items())))
    if key not in _cache:
        data = case["data"]()
        Y, effects = data[0], data[1]
        D = [design(e) for e in effects]
        kw = dict(case["kw"], **more)
        if case["entry"] == "PEGS_sparse":
            fit = PR.pegsz(Y, D, own_text=True, trace=True, **kw)
            fit["b"], fit["GC"], fit["bend"] = fit["b"][0], fit["GC"][0], float(fit["bend"][0])      # (as PR.pegs unwraps them)
        elif case["entry"] == "PEGSZ_sparse":
            fit = SR.pegsz_sparse(Y, D, **kw)
        elif case["entry"] == "PEGSZ":
            fit = PR.pegsz(Y, D, trace=True, **kw)
        else:
            fit = PXR.pegsx(Y, data[2], D, dense=[e[0] != "panel" for e in effects], trace=True, **kw)
        _cache[key] = (data, fit)
    return _cache[key]


def gpu_effects(effects, how="sparse", serial=False):
    """the effects as the package takes them; how = "dense": every sparse design as dense(S.toarray())"""
    import bwgr_amd
    out = []
    for e in effects:
        if e[0] == "panel":
            out.append(e[1])
        elif e[0] == "dense":
            out.append(bwgr_amd.dense(e[1]))
        elif how == "dense":
            out.append(bwgr_amd.dense(e[1]))
        else:
            out.append(bwgr_amd.sparse(SR.csc(e[1], e[2] if len(e) > 2 else None), shape=e[1].shape, serial=serial))
    return out


def run(case, how="sparse", serial=False, **over):
    """the case through the package's entry -> its dict (cnv_trace included)"""
    import bwgr_amd
    data = case["data"]()
    Y, effs = data[0], gpu_effects(data[1], how, serial)
    kw = dict(case["kw"], cnv_trace=True, **over)
    if case["entry"] == "PEGS_sparse":
        return (bwgr_amd.PEGS_sparse if how == "sparse" else bwgr_amd.PEGS)(Y, effs[0], **kw)
    if case["entry"] == "PEGSZ_sparse":
        return bwgr_amd.PEGSZ_sparse(Y, effs, **kw)
    if case["entry"] == "PEGSZ":
        return bwgr_amd.PEGSZ(Y, effs, **kw)
    return bwgr_amd.PEGSX(Y, data[2], effs, **kw)


PEGS_OUT = ("mu", "b", "hat", "h2", "GC", "bend", "cnv", "cnv_trace")
PEGSX_OUT = ("TrZSZ", "b", "u", "vb_list", "GC_list", "ve", "hat", "cnv", "bend", "cnv_trace")


def outputs(case):
    return PEGSX_OUT if case["entry"] == "PEGSX" else PEGS_OUT


def pairs(a, b):
    """the arrays of one entry of two results, list or not"""
    return list(zip(a, b)) if isinstance(a, list) else [(a, b)]
