"""GPU: PEGSX (bwgr_pegsx) against the float64 restatement in tests/pegsx_restatement.py on the cases of tests/pegsx_cases.py -- the smallest
shapes at which each piece can still go wrong (tests/test_pegsx_cpu.py checks that none of them sits on a discontinuous branch) -- then the
projected traces alone, the normal equations of the fixed step, determinism, handles and streams, other fits around a PEGSX call, and the
refusals.

Parity: scaled_err <= 1e-6 on TrZSZ, b, every u, vb_list, GC_list, ve, hat, bend and cnv, equal its with logtol = -inf.
Largest error measured over the table on an MI355X: 1.4e-10 (cnv and u of the collinear traits that bend in every sweep), 3.7e-13 elsewhere;
on the codes_* cases (int8 codes beyond 0 / 1 / 2) 8.8e-11 on tpod + 100, which is the numpy restatement's own rounding of TrZSZ where it
cancels (test_trzsz_alone_where_it_cancels holds the library to a long double reference instead), and at most 1.4e-14 on the other panels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pegsx_cases as XC  # noqa: E402
import pegsx_restatement as XR  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6
KEYS = ("TrZSZ", "b", "u", "vb_list", "GC_list", "ve", "hat", "bend", "cnv")
LISTS = ("TrZSZ", "u", "vb_list", "GC_list")
ORDER = ("TrZSZ", "b", "u", "vb_list", "GC_list", "ve", "hat", "its", "cnv", "bend")


def _open(effects):
    import bwgr_amd
    return [bwgr_amd.Panel(e[1], **e[2]) if e[0] == "panel" else bwgr_amd.dense(e[1]) for e in effects]


def _close(effs):
    import bwgr_amd
    for E in effs:
        if isinstance(E, bwgr_amd.Panel):
            E.close()


def _run(case, effs, Y, X, **more):
    import bwgr_amd
    return bwgr_amd.PEGSX(Y, X, effs, **dict(case["kw"], cnv_trace=True, **more))


def _fit(case, **more):
    Y, X, effects = case["data"]()
    effs = _open(effects)
    try:
        return _run(case, effs, Y, X, **more)
    finally:
        _close(effs)


def _errs(g, o):
    return {key: max(XR.scaled_err(a, b) for a, b in zip(g[key], o[key])) if key in LISTS else XR.scaled_err(g[key], o[key]) for key in KEYS}


def _same(a, b):
    assert a["its"] == b["its"]
    for key in KEYS + ("cnv_trace",):
        for x, y in zip(a[key], b[key]) if key in LISTS else [(a[key], b[key])]:
            assert np.array_equal(x, y), key


@pytest.mark.parametrize("case", [c for c in XC.CASES if c["kw"]["logtol"] == XC.NOSTOP], ids=lambda c: c["id"])
def test_parity(case):
    Y, X, effects, o = XC.restate(case)
    g = _fit(case)
    errs = _errs(g, o)
    print(case["id"], "its", g["its"], {k: "%.2e" % v for k, v in errs.items()})
    assert tuple(g)[:10] == ORDER
    assert g["its"] == o["its"] == case["kw"]["maxit"]
    assert all(v <= TOL for v in errs.values()), errs
    n, k = np.asarray(Y).reshape(len(Y), -1).shape
    assert g["hat"].shape == (n, k) and np.all(np.isfinite(g["hat"]))     # a row for every individual, missing records included
    assert g["b"].shape == (X.shape[1], k) and [u.shape for u in g["u"]] == [(np.asarray(e[1]).shape[1], k) for e in effects]
    if case["id"] in XC.BENDS:
        assert all(r["inflated"] for recs in o["trace"] for r in recs) and np.all(g["bend"] > 0)


@pytest.mark.parametrize("cid", ["f70_slabs_k5", "rank_deficient_x", "dense_only_n196"])
def test_trzsz_alone(cid):
    """maxit = 0: the trace kernels apart from the sweeps (f past one wave with three row slabs; a pseudo-inverse that drops a direction; the
    dense kernel)"""
    case = XC.by_id(cid)
    Y, X, effects, o = XC.restate(case, maxit=0)
    g = _fit(case, maxit=0)
    err = max(XR.scaled_err(a, b) for a, b in zip(g["TrZSZ"], o["TrZSZ"]))
    print(cid, "TrZSZ err %.2e" % err)
    assert g["its"] == 0 and g["cnv"] == 10.0 and err <= TOL
    assert all(np.all(u == 0) for u in g["u"]) and XR.scaled_err(g["b"], o["b"]) <= TOL and XR.scaled_err(g["hat"], o["hat"]) <= TOL


def _normal_equations(Y, X, hat):
    """the largest |M_t'(Y - hat)_t| over a trait's observed rows, as a fraction of ||M_t|| ||y_t||"""
    Yf, Xf = np.asarray(Y, np.float32).astype(np.float64), np.asarray(X, np.float32).astype(np.float64)
    worst = 0.0
    for t in range(Yf.shape[1]):
        w = ~np.isnan(Yf[:, t])
        M, yt = Xf[w], Yf[w, t]
        worst = max(worst, float(np.max(np.abs(M.T @ (yt - hat[w, t]))) / (np.linalg.norm(M) * np.linalg.norm(yt))))
    return worst


@pytest.mark.parametrize("cid", ["f70_slabs_k5", "dense_only_n1500", "codes_full"])
def test_normal_equations(cid):
    """M_t'(Y - hat)_t = 0 over a trait's observed rows after any fit, because the fixed step is the last thing that touches the residual:
    at most 1e-9 of ||M_t|| ||y_t||.  Independent of the restatement."""
    case = XC.by_id(cid)
    Y, X, effects = case["data"]()
    g = _fit(case)
    worst = _normal_equations(Y, X, g["hat"])
    print(cid, "normal equations %.2e" % worst)
    assert worst <= 1e-9


def test_panel_and_dense_legs_agree_on_the_same_numbers():
    """tpod as an int8 Panel and as dense(float64): the same numbers in the same column order through the int8 launch train and the panel
    trace kernel, then through k_pegs_dense_leg and the dense trace kernel.  TrZSZ alone (maxit = 0) and a six-sweep fit: the two agree to
    1e-6 on TrZSZ, u, hat, ve and vb_list, and each agrees with the restatement (which does not care how an effect is stored: 0 / 1 / 2 are
    floats already)."""
    import bwgr_amd
    Y, X, effects = XC.by_id("tpod_k3_defaults")["data"]()
    Z = effects[0][1]
    P = bwgr_amd.Panel(Z)
    try:
        for maxit in (0, 6):
            kw = dict(maxit=maxit, logtol=XC.NOSTOP)
            o = XR.pegsx(Y, X, [Z.astype(np.float64)], **kw)
            gp = bwgr_amd.PEGSX(Y, X, [P], **kw)
            gd = bwgr_amd.PEGSX(Y, X, [bwgr_amd.dense(Z.astype(np.float64))], **kw)
            assert gp["its"] == gd["its"] == o["its"] == maxit
            for key in ("TrZSZ", "u", "hat", "ve", "vb_list"):
                lst = key in LISTS
                for a, b, r in zip(*[(v[key] if lst else [v[key]]) for v in (gp, gd, o)]):
                    errs = (XR.scaled_err(a, b), XR.scaled_err(a, r), XR.scaled_err(b, r))
                    print("maxit", maxit, key, "panel/dense %.2e panel/ref %.2e dense/ref %.2e" % errs)
                    assert max(errs) <= TOL, (maxit, key, errs)
    finally:
        P.close()


def _ld_inv(A):
    """Gauss-Jordan with row pivoting in numpy.longdouble (numpy.linalg has no long double)"""
    A = np.array(A, np.longdouble)
    f = len(A)
    I = np.eye(f, dtype=np.longdouble)
    for c in range(f):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, p]], I[[c, p]] = A[[p, c]], I[[p, c]]
        piv = A[c, c]
        A[c], I[c] = A[c] / piv, I[c] / piv
        for r in range(f):
            if r != c:
                m = A[r, c]
                A[r], I[r] = A[r] - m * A[c], I[r] - m * I[c]
    return I


def test_trzsz_alone_where_it_cancels():
    """tpod + 100 beside an intercept: sum z^2 and v'A v are both about 7e8 and TrZSZ, their difference, 6e4 -- four of fp64's sixteen
    digits go, and the sums' own rounding takes some more.  Against the formula evaluated in numpy.longdouble on the host, to 1e-9 relative."""
    case = XC.by_id("codes_offset")
    Y, X, effects = case["data"]()
    g = _fit(case, maxit=0)
    Yf = np.asarray(Y, np.float32)
    Xl, Zl = np.asarray(X, np.float32).astype(np.longdouble), effects[0][1].astype(np.longdouble)
    assert np.all(Xl[:, 0] == 1) and g["its"] == 0
    for t in range(Yf.shape[1]):
        w = ~np.isnan(Yf[:, t])
        M, Zw = Xl[w], Zl[w]
        V = M.T @ Zw
        total = (Zw ** 2).sum()
        ref = total - (V * (_ld_inv(M.T @ M) @ V)).sum()
        rel = abs(float((np.longdouble(g["TrZSZ"][0][t]) - ref) / ref))
        print("trait", t, "sum z^2 %.6e TrZSZ %.6e rel err %.2e" % (float(total), float(ref), rel))
        assert total / ref > 5e3 and rel <= 1e-9, (t, rel)


@pytest.mark.parametrize("name", ["full", "offset"])
def test_panel_and_dense_legs_agree_on_other_codes(name):
    """The same on codes -128..127 and on tpod + 100 beside an intercept and two covariates: k_pegsx_trace_panel unpacks four signed rows
    from a dword where k_pegsx_trace_dense reads four doubles, and the uncentred int8 train runs against k_pegs_dense_leg.  TrZSZ alone
    (maxit = 0) and a six-sweep fit agree to 1e-9 on every output, without the restatement (which each then matches to 1e-6)."""
    import bwgr_amd
    Y, X, effects = XC.by_id("codes_" + name)["data"]()
    Z = effects[0][1]
    P = bwgr_amd.Panel(Z)
    try:
        for maxit in (0, 6):
            kw = dict(maxit=maxit, logtol=XC.NOSTOP)
            o = XR.pegsx(Y, X, [Z.astype(np.float64)], **kw)
            gp = bwgr_amd.PEGSX(Y, X, [P], **kw)
            gd = bwgr_amd.PEGSX(Y, X, [bwgr_amd.dense(Z.astype(np.float64))], **kw)
            assert gp["its"] == gd["its"] == o["its"] == maxit
            between, ep, ed = _errs(gp, gd), _errs(gp, o), _errs(gd, o)
            print(name, "maxit", maxit, {k: "%.2e" % v for k, v in between.items()}, {k: "%.2e" % v for k, v in ep.items()}, {k: "%.2e" % v for k, v in ed.items()})
            assert all(v <= 1e-9 for v in between.values()), (maxit, between)
            for errs in (ep, ed):
                assert all(v <= TOL for v in errs.values()), (maxit, errs)
    finally:
        P.close()


def test_int32_gram_bound():
    """test_gpu_mrr.py::test_int32_gram_bound through PEGSX with an intercept: at the most rows of +-127 that n max|x|^2 < 2^31 allows the fit
    and its TrZSZ (1.5e11 a trait) match; one more row is refused where the panel is made, and the refused call leaves nothing behind."""
    import bwgr_amd
    Z, Y, Y1 = XC.PC.gram_bound()
    n = XC.PC.GRAM_BOUND_N
    kw = dict(maxit=2, logtol=XC.NOSTOP)
    P = bwgr_amd.Panel(Z[:n], block=16)   # (n rows need the smaller sweep block's taller slabs)
    try:
        g = bwgr_amd.PEGSX(Y, np.ones((n, 1)), [P], **kw)
    finally:
        P.close()
    o = XR.pegsx(Y, np.ones((n, 1)), [Z[:n]], **kw)
    errs = _errs(g, o)
    print("gram bound", {k: "%.2e" % v for k, v in errs.items()})
    assert g["its"] == o["its"] == 2 and all(v <= TOL for v in errs.values()), errs
    live = bwgr_amd.debug_live()
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.PEGSX(Y1, np.ones((n + 1, 1)), [Z], block=16, **kw)
    assert ei.value.code == 1 and "int32 Gram" in str(ei.value)
    assert bwgr_amd.debug_live() == live
    case = XC.by_id("tpod_k3_defaults")
    assert all(v <= TOL for v in _errs(_fit(case), XC.restate(case)[3]).values())


def test_effect_order_matters_and_each_matches():
    a, b = XC.restate(XC.by_id("panel_dense70"))[3], XC.restate(XC.by_id("dense70_panel"))[3]
    assert XR.scaled_err(a["u"][0], b["u"][1]) > 1e-4      # the same panel, swept before or after the dense design
    ga, gb = _fit(XC.by_id("panel_dense70")), _fit(XC.by_id("dense70_panel"))
    assert XR.scaled_err(ga["u"][0], a["u"][0]) <= TOL and XR.scaled_err(gb["u"][1], b["u"][1]) <= TOL
    assert XR.scaled_err(ga["u"][0], gb["u"][1]) > 1e-4


def test_stop_rule():
    case = XC.by_id("stop_rule")
    o = XC.restate(case)[3]
    g = _fit(case)
    assert o["its"] == 5 and g["its"] == 5 and g["cnv"] == g["cnv_trace"][-1] and len(g["cnv_trace"]) == 5
    assert np.allclose(g["cnv_trace"], o["cnv_trace"], rtol=0, atol=1e-5) and np.all(g["cnv_trace"][2:] < 0.0)


def test_two_runs_are_bit_identical():
    for cid in ("panel_dense70", "f70_slabs_k5", "codes_full_slabs_f70_k5"):
        _same(_fit(XC.by_id(cid)), _fit(XC.by_id(cid)))


def test_clone_and_callers_stream_give_the_roots_result():
    import torch
    case = XC.by_id("panel_dense70")
    Y, X, effects = case["data"]()
    effs = _open(effects)
    P = effs[0]
    s = torch.cuda.Stream()
    try:
        first = _run(case, effs, Y, X)
        Q = P.clone()
        try:
            on_clone = _run(case, [Q] + effs[1:], Y, X)
        finally:
            Q.close()
        try:
            P.set_stream(s.cuda_stream)
            with torch.cuda.stream(s):
                torch.cuda._sleep(20_000_000)      # the caller's stream is busy when the call arrives
            on_stream = _run(case, effs, Y, X)
            torch.cuda.synchronize()
        finally:
            P.set_stream(0)
        back = _run(case, effs, Y, X)
    finally:
        _close(effs)
    for other in (on_clone, on_stream, back):
        _same(first, other)


def test_pegsz_and_mrr_before_and_after_a_pegsx_call():
    import bwgr_amd
    Z = XC.tpod()
    Y = XC.traits(Z, 3, 0.1, seed=61)
    X = XC.fixed(Z.shape[0], 2, 62)
    D = XC.gauss(Z.shape[0], 5, 2)
    P = bwgr_amd.Panel(Z)
    try:
        a = bwgr_amd.mrr(Y, P, maxit=5, tol=0)
        za = bwgr_amd.PEGSZ(Y, [D, P], maxit=3, logtol=XC.NOSTOP)
        bwgr_amd.PEGSX(Y, X, [P], maxit=3, logtol=XC.NOSTOP)
        bwgr_amd.PEGSX(Y, X, [D, P], maxit=3, logtol=XC.NOSTOP, XFA=True, NumXFA=1)
        b = bwgr_amd.mrr(Y, P, maxit=5, tol=0)
        zb = bwgr_amd.PEGSZ(Y, [D, P], maxit=3, logtol=XC.NOSTOP)
    finally:
        P.close()
    for key in bwgr_amd.api.MRR_KEYS:
        assert np.array_equal(a[key], b[key]), key
    for key in bwgr_amd.api.PEGS_KEYS:
        for x, y in zip(za[key], zb[key]) if isinstance(za[key], list) else [(za[key], zb[key])]:
            assert np.array_equal(x, y), key


def _refusals(P, Z, Y, X):
    import bwgr_amd
    n = Z.shape[0]
    Xnan = X.copy(); Xnan[5, 1] = np.nan
    Y1 = Y.copy(); Y1[:, 1] = np.nan; Y1[7, 1] = 1.0
    Pf = bwgr_amd.Panel(Z.astype(np.float32) + 0.5)
    Pl = bwgr_amd.Panel(Z, nwg=4)      # four slabs of 256 rows pad 700 rows to 1024, P's three to 768
    try:
        yield "InnerGS", lambda: bwgr_amd.PEGSX(Y, X, [P], maxit=2, InnerGS=True)
        yield "NoInv", lambda: bwgr_amd.PEGSX(Y, X, [P], maxit=2, NoInv=True)
        yield "not finite", lambda: bwgr_amd.PEGSX(Y, Xnan, [P], maxit=2)
        yield "rows", lambda: bwgr_amd.PEGSX(Y, X[:100], [P], maxit=2)
        yield "f = 0", lambda: bwgr_amd.PEGSX(Y, np.zeros((n, 0)), [P], maxit=2)
        yield "f = 257", lambda: bwgr_amd.PEGSX(Y, np.ones((n, 257)), [P], maxit=2)
        yield "effects", lambda: bwgr_amd.PEGSX(Y, X, [], maxit=2)
        yield "trait 1", lambda: bwgr_amd.PEGSX(Y1, X, [P], maxit=2)
        yield "fp32", lambda: bwgr_amd.PEGSX(Y, X, [Pf], maxit=2)
        assert Pl.ld != P.ld
        yield "ld =", lambda: bwgr_amd.PEGSX(Y, X, [P, Pl], maxit=2)
    finally:
        Pf.close(); Pl.close()


def test_refusals_leave_the_panel_usable():
    import bwgr_amd
    Z = XC.slabs900()
    Y = XC.traits(Z, 3, 0.1, seed=51)
    X = XC.fixed(Z.shape[0], 2, 52)
    P = bwgr_amd.Panel(Z, nwg=3)
    try:
        ref = bwgr_amd.PEGSX(Y, X, [P], maxit=2)
        seen = 0
        for word, call in _refusals(P, Z, Y, X):
            with pytest.raises(bwgr_amd.BwgrError) as ei:
                call()
            assert ei.value.code == 1 and word in str(ei.value), (word, str(ei.value))
            seen += 1
        assert seen == 10
        again = bwgr_amd.PEGSX(Y, X, [P], maxit=2)
        _same(dict(ref, cnv_trace=0), dict(again, cnv_trace=0))
    finally:
        P.close()
