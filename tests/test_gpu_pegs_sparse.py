"""GPU: sparse effects in PEGS / PEGSZ / PEGSX, PEGS_sparse and PEGSZ_sparse (bwgr_pegs_ex, bwgr_pegsx_ex) against the float64 restatements
on the dense copy of every sparse design, on the cases of tests/pegs_sparse_cases.py (tests/test_pegs_sparse_cpu.py checks that none of
them sits on a discontinuous branch) -- then the same numbers through the dense leg, the disjoint leg against the serial one bit for bit,
PEGSZ_sparse's text against PEGSZ's, determinism, an empty column, the refusals and mrr's own results around them, and the effect order.

Parity: pegs_restatement.scaled_err <= 1e-6 on every output, equal sweep counts with logtol = -inf.  Every test prints what it measured.
Largest errors measured on an MI355X: parity 3.5e-13 (bend of the q = 1 case, which bends in every sweep), 2.1e-13 on cnv (the case of
32 805 columns; 1.2e-13 before it), at most 3.0e-14 on every other figure (vb_list at f = 256; 1.9e-14 on bend at f = 70, k = 16);
sparse(S) against dense(S.toarray()) 3.9e-14 (cnv; 2.8e-14 on bend at f = 70; TrZSZ 2.1e-16); TrZSZ alone at the cap of the sparse trace's
grid 1.3e-16; the disjoint leg against the serial leg and a run against its repeat: the same bits; PEGSZ_sparse's mu against PEGSZ's on the
same data: 1.1e-4 apart.

The second round of cases (tests/pegs_sparse_cases.py, from ps_setup_trip_k3 on) runs through the same tests: a second trip of the set-up
kernel and a third of the d2 reduction, the sparse trace at 1 024 workgroups and five trips (also alone, maxit = 0), f = 70 with sixteen
patterns and f = 256, columns of three lane strides that share rows on the serial leg at k = 16, a weighted row-disjoint matrix on the
disjoint leg, and a level whose rows have no record (test_level_without_a_record_keeps_b_zero_and_hat_at_mu)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pegs_restatement as PR  # noqa: E402
import pegs_sparse_cases as SC  # noqa: E402
import pegs_sparse_restatement as SR  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6


def _its(r):
    return r["numit"] if "numit" in r else r["its"]


def _errs(case, g, o):
    return {key: max(PR.scaled_err(a, b) for a, b in SC.pairs(g[key], o[key])) for key in SC.outputs(case)}


def _same(case, a, b):
    assert _its(a) == _its(b)
    for key in SC.outputs(case):
        for x, y in SC.pairs(a[key], b[key]):
            assert np.array_equal(x, y), (case["id"], key)


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c["id"])
def test_parity(case):
    data, o = SC.restate(case)
    g = SC.run(case)
    errs = _errs(case, g, o)
    print(case["id"], "sweeps", _its(g), {k: "%.2e" % v for k, v in errs.items()})
    assert _its(g) == _its(o) == case["kw"]["maxit"]
    assert all(v <= TOL for v in errs.values()), errs
    n, k = data[0].shape
    assert g["hat"].shape == (n, k) and np.all(np.isfinite(g["hat"]))     # a row for every individual, rows without any record included
    coef = g["u"] if case["entry"] == "PEGSX" else [g["b"]] if case["entry"] == "PEGS_sparse" else g["b"]
    assert [c.shape for c in coef] == [(e[1].shape[1], k) for e in data[1]]


LEGS = ("ps_inc12_k3", "ps_inc70_k3", "ps_trip_k3", "ps_long_cols_k3", "ps_overlap_k3", "pzs_inc_overlap_k5_xfa2", "pz_mixed4_k3", "px_inc12_k3",
        "px_overlap_k1", "px_mixed4_k3_xfa2",
        # the second round: the wide ones (dense copies of 79 MB and 40 MB), the long columns, f = 70 with sixteen patterns and f = 256
        "ps_setup_trip_k3", "px_trace_cap_k3", "ps_overlap_long_k16", "pzs_inc_overlap_long_k3", "px_f70_k16", "px_f256_k3")


@pytest.mark.parametrize("cid", LEGS)
def test_sparse_and_dense_legs_agree_on_the_same_numbers(cid):
    """sparse(S) and dense(S.toarray()): the same numbers summed over the stored entries or over every row; for PEGSX, TrZSZ comes from the
    sparse or the dense trace kernel"""
    case = SC.by_id(cid)
    _, o = SC.restate(case)
    s, d = SC.run(case), SC.run(case, how="dense")
    es, ed, sd = _errs(case, s, o), _errs(case, d, o), _errs(case, s, d)
    print(cid, "sparse vs dense", {k: "%.2e" % v for k, v in sd.items()}, "worst vs restatement: sparse %.2e dense %.2e" % (max(es.values()), max(ed.values())))
    assert _its(s) == _its(d)
    assert all(v <= TOL for v in sd.values()), sd
    assert all(v <= TOL for v in es.values()) and all(v <= TOL for v in ed.values())


@pytest.mark.parametrize("cid", SC.DISJOINT)
def test_disjoint_and_serial_legs_agree_bit_for_bit(cid):
    import bwgr_amd
    case = SC.by_id(cid)
    for e in case["data"]()[1]:
        if e[0] == "sparse":
            A = e[1]
            assert SR.row_disjoint(A)
            pl = bwgr_amd.pegs_sparse_plan(A.shape[0], A.shape[1], int((A != 0).sum()), int((A != 0).sum(0).max()), case["data"]()[0].shape[1], True)
            assert pl["leg"] == "disjoint"
    _same(case, SC.run(case), SC.run(case, serial=True))


def test_overlapping_effect_takes_the_serial_leg():
    """the plan's verdict on an overlapping matrix is the serial leg, forced or not: the same bits, and the restatement's numbers"""
    import bwgr_amd
    case = SC.by_id("ps_overlap_k3")
    A, stored = case["data"]()[1][0][1:]
    assert not SR.row_disjoint(A)
    assert bwgr_amd.pegs_sparse_plan(A.shape[0], A.shape[1], int(stored.sum()), int(stored.sum(0).max()), 3, SR.row_disjoint(A))["leg"] == "serial"
    a, b = SC.run(case), SC.run(case, serial=True)
    _same(case, a, b)
    assert max(_errs(case, a, SC.restate(case)[1]).values()) <= TOL


def test_text2_differs_from_text0_in_mu_and_each_matches_its_restatement():
    import bwgr_amd
    case = SC.by_id("pzs_two_inc_k3")
    Y, effects = case["data"]()
    D = [SC.design(e) for e in effects]
    g2 = bwgr_amd.PEGSZ_sparse(Y, SC.gpu_effects(effects), **case["kw"])
    g0 = bwgr_amd.PEGSZ(Y, SC.gpu_effects(effects), **case["kw"])
    o2, o0 = SR.pegsz_sparse(Y, D, **case["kw"]), PR.pegsz(Y, D, **case["kw"])
    diff = float(np.max(np.abs(g2["mu"] - g0["mu"])))
    print("text 2 vs text 0: max |mu2 - mu0| = %.3e (restatements: %.3e)" % (diff, float(np.max(np.abs(o2["mu"] - o0["mu"])))))
    assert diff > 1e-6
    for g, o in ((g2, o2), (g0, o0)):
        for key in ("mu", "b", "hat", "h2", "GC", "bend", "cnv"):
            assert max(PR.scaled_err(a, b) for a, b in SC.pairs(g[key], o[key])) <= TOL, key
    # PEGSZ_sparse takes what `sparse` takes: the plain arrays give the marked effects' bits
    g2b = bwgr_amd.PEGSZ_sparse(Y, D, **case["kw"])
    assert np.array_equal(g2b["hat"], g2["hat"]) and np.array_equal(g2b["mu"], g2["mu"])


@pytest.mark.parametrize("cid", ["ps_trip_k3", "ps_overlap_k3", "pz_mixed4_k3", "px_mixed4_k3_xfa2", "ps_setup_trip_k3", "px_trace_cap_k3", "px_f70_k16",
                                 "px_f256_k3", "ps_overlap_long_k16", "pzs_inc_overlap_long_k3", "ps_weighted_k3", "ps_unobserved_level_k3"])
def test_two_runs_are_bit_identical(cid):
    case = SC.by_id(cid)
    _same(case, SC.run(case), SC.run(case))


def test_empty_column_keeps_b_zero():
    case = SC.by_id("ps_empty_col_k3")
    A = SC.design(case["data"]()[1][0])
    j = int(np.flatnonzero((A != 0).sum(0) == 0)[0])
    for serial in (False, True):
        g = SC.run(case, serial=serial)
        assert np.all(g["b"][j] == 0.0) and np.all(g["b"][np.arange(A.shape[1]) != j] != 0.0)
    trip = SC.run(SC.by_id("ps_trip_k3"))           # and the thousands of empty levels of the two-trip case
    T = SC.design(SC.by_id("ps_trip_k3")["data"]()[1][0])
    assert np.all(trip["b"][(T != 0).sum(0) == 0] == 0.0)


@pytest.mark.parametrize("cid", SC.TRZSZ_ALONE)
def test_trzsz_alone(cid):
    """maxit = 0: k_pegsx_trace_sparse apart from the sweeps, at the cap of its grid (1 024 workgroups, five trips, one column in the last
    workgroup of the last), as tests/test_gpu_tall.py's test_pegsx_trzsz_alone for the panel and dense kernels; and through the dense kernel"""
    case = SC.by_id(cid)
    _, o = SC.restate(case, maxit=0)
    g, d = SC.run(case, maxit=0), SC.run(case, how="dense", maxit=0)
    err = max(PR.scaled_err(a, b) for a, b in zip(g["TrZSZ"], o["TrZSZ"]))
    between = max(PR.scaled_err(a, b) for a, b in zip(g["TrZSZ"], d["TrZSZ"]))
    print(cid, "TrZSZ alone %.2e, sparse against dense %.2e" % (err, between))
    assert g["its"] == o["its"] == 0 and g["cnv"] == 10.0 and err <= TOL and between <= TOL
    assert all(np.all(u == 0) for u in g["u"]) and PR.scaled_err(g["b"], o["b"]) <= TOL and PR.scaled_err(g["hat"], o["hat"]) <= TOL


def test_level_without_a_record_keeps_b_zero_and_hat_at_mu():
    """a column with stored entries whose rows have no record in any trait: XX_jt = 0 for every t, so Linv_j is the inverse of iG alone and
    the dots are sums of zeros -- b_j is exactly 0 on both legs, and with one effect hat on those rows is mu to the bit"""
    case = SC.by_id("ps_unobserved_level_k3")
    Y, effects = case["data"]()
    A = SC.design(effects[0])
    j = SC.unobserved_column(A, Y)
    rows = np.flatnonzero(A[:, j])
    records = (A != 0).T.astype(int) @ (~np.isnan(Y)).astype(int)              # per level and trait (one trait misses another whole level)
    assert np.all(records[j] == 0) and (records[np.arange(A.shape[1]) != j] > 0).any(1).all()
    for serial in (False, True):
        g = SC.run(case, serial=serial)
        assert np.all(g["b"][j] == 0.0) and np.all(g["b"][records > 0] != 0.0)
        assert np.array_equal(g["hat"][rows], np.tile(g["mu"], (len(rows), 1)))
        others = np.flatnonzero(np.isnan(Y).all(1) & (A[:, j] == 0))           # (rows without a record on observed levels get that level's b)
        assert len(others) and not np.array_equal(g["hat"][others], np.tile(g["mu"], (len(others), 1)))


def test_refusals_leave_the_panel_usable():
    """mrr before and after every refused call gives the same bits; then the panel fits with a sparse effect beside it"""
    import bwgr_amd
    from bwgr_amd import sparse
    Y, effects = SC.by_id("pz_panel_inc_k3")["data"]()
    X, A = effects[0][1], effects[1][1]
    data, idx, ptr = SR.csc(A)
    n, q = A.shape
    dup = idx.copy(); dup[1] = dup[0]
    nan = data.copy(); nan[5] = np.nan
    far = idx.copy(); far[-1] = n
    ptr1 = ptr.copy(); ptr1[0] = 1
    P = bwgr_amd.Panel(X)
    try:
        before = bwgr_amd.mrr(Y, P, maxit=4, tol=0)
        calls = [
            ("strictly increase", lambda: bwgr_amd.PEGSZ(Y, [P, sparse((data, dup, ptr), shape=A.shape)], maxit=2)),
            ("not finite", lambda: bwgr_amd.PEGSZ(Y, [P, sparse((nan, idx, ptr), shape=A.shape)], maxit=2)),
            ("outside [0, n)", lambda: bwgr_amd.PEGSX(Y, np.ones((n, 1)), [P, sparse((data, far, ptr), shape=A.shape)], maxit=2)),
            ("colptr[0]", lambda: bwgr_amd.PEGSZ_sparse(Y, [P, sparse((data, idx, ptr1), shape=A.shape)], maxit=2)),
            ("TrXSX", lambda: bwgr_amd.PEGSZ(Y, [P, sparse(np.ones((n, 1)))], maxit=2)),          # a constant column: found on the device
        ]
        for word, call in calls:
            with pytest.raises(bwgr_amd.BwgrError) as ei:
                call()
            assert ei.value.code == 1 and word in str(ei.value) and "effect 1" in str(ei.value), (word, str(ei.value))
            after = bwgr_amd.mrr(Y, P, maxit=4, tol=0)
            for key in bwgr_amd.api.MRR_KEYS:
                assert np.array_equal(before[key], after[key]), (word, key)
        assert bwgr_amd.PEGSZ(Y, [P, sparse(A)], maxit=1)["numit"] == 1
    finally:
        P.close()


def test_effect_order_matters_and_each_matches():
    import bwgr_amd
    case = SC.by_id("pzs_inc_overlap_k5_xfa2")
    Y, effects = case["data"]()
    kw = dict(case["kw"], XFA=-1)
    D = [SC.design(e) for e in effects]
    oa, ob = PR.pegsz(Y, D, **kw), PR.pegsz(Y, D[::-1], **kw)
    assert PR.scaled_err(oa["b"][0], ob["b"][1]) > 1e-4          # the same incidence, swept before or after the overlapping design
    ga, gb = bwgr_amd.PEGSZ(Y, SC.gpu_effects(effects), **kw), bwgr_amd.PEGSZ(Y, SC.gpu_effects(effects[::-1]), **kw)
    ea, eb = PR.scaled_err(ga["b"][0], oa["b"][0]), PR.scaled_err(gb["b"][1], ob["b"][1])
    print("effect order: %.2e %.2e, between the orders %.2e" % (ea, eb, PR.scaled_err(ga["b"][0], gb["b"][1])))
    assert ea <= TOL and eb <= TOL and PR.scaled_err(ga["b"][0], gb["b"][1]) > 1e-4
