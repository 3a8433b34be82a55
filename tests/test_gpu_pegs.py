"""GPU: PEGS / PEGSZ (bwgr_pegs) against the float64 restatement in tests/pegs_restatement.py on the cases of tests/pegs_cases.py -- the
smallest shapes at which each piece can still go wrong (tests/test_pegs_cpu.py checks that none of them sits on a discontinuous branch) --
then determinism, handles and streams, the refusals, and mrr's own results around a PEGS call.

Parity: scaled_err <= 1e-6 on mu, b, hat, h2, GC, bend and cnv, equal numit with logtol = -inf.
The codes_* cases run the uncentred int8 train on codes beyond 0 / 1 / 2 (signed, -128..127, a large mean, +-127, constant columns):
largest error measured on an MI355X 2.3e-13 (h2 on tpod + 100), at most 1.1e-14 on the other panels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pegs_cases as PC  # noqa: E402
import pegs_restatement as PR  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6
KEYS = ("mu", "b", "hat", "h2", "GC", "bend", "cnv")


def _open(effects):
    import bwgr_amd
    return [bwgr_amd.Panel(e[1], **e[2]) if e[0] == "panel" else bwgr_amd.dense(e[1]) for e in effects]


def _close(effs):
    import bwgr_amd
    for E in effs:
        if isinstance(E, bwgr_amd.Panel):
            E.close()


def _run(case, effs, Y, **more):
    import bwgr_amd
    kw = dict(case["kw"], cnv_trace=True, **more)
    return bwgr_amd.PEGS(Y, effs[0], **kw) if case["entry"] == "PEGS" else bwgr_amd.PEGSZ(Y, effs, **kw)


def _fit(case, **more):
    Y, effects = case["data"]()
    effs = _open(effects)
    try:
        return _run(case, effs, Y, **more)
    finally:
        _close(effs)


def _errs(g, o, entry):
    out = {}
    for key in KEYS:
        if entry == "PEGSZ" and key in ("b", "GC"):
            out[key] = max(PR.scaled_err(a, b) for a, b in zip(g[key], o[key]))
        elif entry == "PEGS" and key in ("b", "GC", "bend"):
            out[key] = PR.scaled_err(g[key], o[key][0])
        else:
            out[key] = PR.scaled_err(g[key], o[key])
    return out


def _same(a, b):
    assert a["numit"] == b["numit"]
    for key in KEYS + ("cnv_trace",):
        for x, y in zip(a[key], b[key]) if isinstance(a[key], list) else [(a[key], b[key])]:
            assert np.array_equal(x, y), key


@pytest.mark.parametrize("case", [c for c in PC.CASES if c["kw"]["logtol"] == PC.NOSTOP], ids=lambda c: c["id"])
def test_parity(case):
    Y, effects, o = PC.restate(case)
    g = _fit(case)
    errs = _errs(g, o, case["entry"])
    print(case["id"], "numit", g["numit"], {k: "%.2e" % v for k, v in errs.items()})
    assert tuple(g)[:8] == ("mu", "b", "hat", "h2", "GC", "bend", "numit", "cnv")
    assert g["numit"] == o["numit"] == case["kw"]["maxit"]
    assert all(v <= TOL for v in errs.values()), errs
    n, k = np.asarray(Y).reshape(len(Y), -1).shape
    assert g["hat"].shape == (n, k) and np.all(np.isfinite(g["hat"]))     # a row for every individual, missing records included
    bs = [g["b"]] if case["entry"] == "PEGS" else g["b"]
    assert [b.shape for b in bs] == [(np.asarray(e[1]).shape[1], k) for e in effects]
    if case["id"] in PC.BENDS:
        assert all(r["inflated"] for recs in o["trace"] for r in recs) and g["bend"] > 0


def test_effect_order_matters_and_each_matches():
    a, b = PC.restate(PC.by_id("pegsz_panel_dense70"))[2], PC.restate(PC.by_id("pegsz_dense70_panel"))[2]
    assert PR.scaled_err(a["b"][0], b["b"][1]) > 1e-4      # the same panel, swept before or after the dense design
    ga, gb = _fit(PC.by_id("pegsz_panel_dense70")), _fit(PC.by_id("pegsz_dense70_panel"))
    assert PR.scaled_err(ga["b"][0], a["b"][0]) <= TOL and PR.scaled_err(gb["b"][1], b["b"][1]) <= TOL
    assert PR.scaled_err(ga["b"][0], gb["b"][1]) > 1e-4


def test_default_logtol():
    case = PC.by_id("default_logtol")
    _, _, o = PC.restate(case)
    g = _fit(case)
    assert 1 < o["numit"] < 100 and abs(g["numit"] - o["numit"]) <= 1 and 1 < g["numit"] < 100
    m = min(g["numit"], o["numit"])
    assert np.allclose(g["cnv_trace"][:m], o["cnv_trace"][:m], rtol=0, atol=1e-3)
    assert g["cnv"] < -4.0 and g["cnv"] == g["cnv_trace"][-1]


def test_pegs_and_pegsz_agree_on_one_effect():
    import bwgr_amd
    Y, effects = PC.by_id("tpod_k3_defaults")["data"]()
    effs = _open(effects)
    try:
        a = bwgr_amd.PEGS(Y, effs[0], maxit=6, logtol=PC.NOSTOP)
        z = bwgr_amd.PEGSZ(Y, effs, maxit=6, logtol=PC.NOSTOP)
    finally:
        _close(effs)
    for key in KEYS:
        zz = z[key][0] if key in ("b", "GC", "bend") else z[key]
        assert PR.scaled_err(a[key], zz) <= 1e-9, key


def test_panel_and_dense_legs_agree_on_the_same_numbers():
    """PEGSZ(Y, [Panel(tpod)]) runs the int8 launch train, PEGSZ(Y, [dense(tpod as float64)]) k_pegs_dense_leg on the same numbers in the
    same column order; k = 3, six sweeps.  The two agree to 1e-6 on every output (b, hat, the variance components as h2 and GC, mu, bend,
    cnv), and each agrees with the restatement."""
    import bwgr_amd
    Y, effects = PC.by_id("tpod_k3_defaults")["data"]()
    Z = effects[0][1]
    kw = dict(maxit=6, logtol=PC.NOSTOP)
    o = PR.pegsz(Y, [Z.astype(np.float64)], **kw)
    P = bwgr_amd.Panel(Z)
    try:
        gp = bwgr_amd.PEGSZ(Y, [P], **kw)
    finally:
        P.close()
    gd = bwgr_amd.PEGSZ(Y, [bwgr_amd.dense(Z.astype(np.float64))], **kw)
    assert gp["numit"] == gd["numit"] == o["numit"] == 6
    between, ep, ed = _errs(gp, gd, "PEGSZ"), _errs(gp, o, "PEGSZ"), _errs(gd, o, "PEGSZ")
    print({k: "%.2e" % v for k, v in between.items()}, {k: "%.2e" % v for k, v in ep.items()}, {k: "%.2e" % v for k, v in ed.items()})
    for errs in (between, ep, ed):
        assert all(v <= TOL for v in errs.values()), errs


@pytest.mark.parametrize("name", ["full", "offset"])
def test_panel_and_dense_legs_agree_on_other_codes(name):
    """The same on codes -128..127 and on tpod + 100, where the uncentred train's sign extension, S_g and XSX = XX / n - (S / n)^2 matter:
    the int8 train against k_pegs_dense_leg on the same numbers as float64, to 1e-9 on every output and without the restatement (which
    each leg then matches to 1e-6)."""
    import bwgr_amd
    Y, effects = PC.by_id("codes_" + name)["data"]()
    Z = effects[0][1]
    kw = dict(maxit=6, logtol=PC.NOSTOP)
    o = PR.pegsz(Y, [Z.astype(np.float64)], **kw)
    P = bwgr_amd.Panel(Z)
    try:
        gp = bwgr_amd.PEGSZ(Y, [P], **kw)
    finally:
        P.close()
    gd = bwgr_amd.PEGSZ(Y, [bwgr_amd.dense(Z.astype(np.float64))], **kw)
    assert gp["numit"] == gd["numit"] == o["numit"] == 6
    between, ep, ed = _errs(gp, gd, "PEGSZ"), _errs(gp, o, "PEGSZ"), _errs(gd, o, "PEGSZ")
    print(name, {k: "%.2e" % v for k, v in between.items()}, {k: "%.2e" % v for k, v in ep.items()}, {k: "%.2e" % v for k, v in ed.items()})
    assert all(v <= 1e-9 for v in between.values()), between
    for errs in (ep, ed):
        assert all(v <= TOL for v in errs.values()), errs


def test_int32_gram_bound():
    """test_gpu_mrr.py::test_int32_gram_bound through PEGS, whose uncentred XX is the Gram's diagonal itself: at the most rows of +-127 that
    n max|x|^2 < 2^31 allows the fit matches; one more row is refused where the panel is made, and the refused call leaves nothing behind."""
    import bwgr_amd
    X, Y, Y1 = PC.gram_bound()
    n = PC.GRAM_BOUND_N
    assert np.all((X[:n].astype(np.int64) ** 2).sum(0) == n * 127 * 127)
    kw = dict(maxit=2, logtol=PC.NOSTOP)
    P = bwgr_amd.Panel(X[:n], block=16)   # (n rows need the smaller sweep block's taller slabs)
    try:
        g = bwgr_amd.PEGS(Y, P, **kw)
    finally:
        P.close()
    o = PR.pegs(Y, X[:n], **kw)
    errs = {key: PR.scaled_err(g[key], o[key]) for key in KEYS}
    print("gram bound", {k: "%.2e" % v for k, v in errs.items()})
    assert g["numit"] == o["numit"] == 2 and all(v <= TOL for v in errs.values()), errs
    live = bwgr_amd.debug_live()
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.PEGS(Y1, X, block=16, **kw)
    assert ei.value.code == 1 and "int32 Gram" in str(ei.value)
    assert bwgr_amd.debug_live() == live
    case = PC.by_id("tpod_k3_defaults")
    assert all(v <= TOL for v in _errs(_fit(case), PC.restate(case)[2], "PEGS").values())


def test_staging_rule():
    """_pegs_effect on the device: an integer-valued float matrix within int8 range (negative values included) and a bool matrix are
    staged as int8 panels, bit for bit the int8 matrix's fit; a float matrix holding 128.0 no longer fits int8 and goes to the dense leg;
    an int16 matrix holding 200 becomes an fp32 panel, which PEGS refuses, and the panel made for the call is released."""
    import bwgr_amd
    kw = dict(maxit=4, logtol=PC.NOSTOP, cnv_trace=True)
    Y, effects = PC.by_id("codes_signed")["data"]()
    S = effects[0][1]
    assert S.min() == -1
    _same(bwgr_amd.PEGS(Y, S.astype(np.float64), **kw), bwgr_amd.PEGS(Y, S, **kw))
    T = PC.tpod()
    Yt = PC.by_id("tpod_k3_defaults")["data"]()[0]
    B = T > 0
    assert B.dtype == np.bool_
    _same(bwgr_amd.PEGS(Yt, B, **kw), bwgr_amd.PEGS(Yt, B.astype(np.int8), **kw))
    Yf, effects = PC.by_id("codes_full")["data"]()
    Z = effects[0][1].astype(np.float64)
    assert Z[0, 0] == -128.0
    Z[0, 0] = 128.0
    a, d = bwgr_amd.PEGSZ(Yf, [Z], **kw), bwgr_amd.PEGSZ(Yf, [bwgr_amd.dense(Z)], **kw)
    _same(a, d)
    o = PR.pegsz(Yf, [Z], maxit=4, logtol=PC.NOSTOP)
    assert all(v <= TOL for v in _errs(a, o, "PEGSZ").values())
    A = T.astype(np.int16)
    A[0, 0] = 200
    live = bwgr_amd.debug_live()
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.PEGS(Yt, A, **kw)
    assert ei.value.code == 1 and "fp32" in str(ei.value)
    assert bwgr_amd.debug_live() == live
    case = PC.by_id("tpod_k3_defaults")
    assert all(v <= TOL for v in _errs(_fit(case), PC.restate(case)[2], "PEGS").values())


def test_two_runs_are_bit_identical():
    for cid in ("pegsz_panel_dense70", "codes_full_slabs_k5"):
        _same(_fit(PC.by_id(cid)), _fit(PC.by_id(cid)))


def test_clone_and_callers_stream_give_the_roots_result():
    import torch
    case = PC.by_id("pegsz_panel_dense70")
    Y, effects = case["data"]()
    effs = _open(effects)
    P = effs[0]
    s = torch.cuda.Stream()
    try:
        first = _run(case, effs, Y)
        Q = P.clone()
        try:
            on_clone = _run(case, [Q] + effs[1:], Y)
        finally:
            Q.close()
        try:
            P.set_stream(s.cuda_stream)
            with torch.cuda.stream(s):
                torch.cuda._sleep(20_000_000)      # the caller's stream is busy when the call arrives
            on_stream = _run(case, effs, Y)
            torch.cuda.synchronize()
        finally:
            P.set_stream(0)
        back = _run(case, effs, Y)
    finally:
        _close(effs)
    for other in (on_clone, on_stream, back):
        _same(first, other)


def _refusals(P, X, Y):
    import bwgr_amd
    n = X.shape[0]
    Z = PC.gauss(n, 4, 1)
    Zbad = Z.copy(); Zbad[3, 2] = np.inf
    Y1 = Y.copy(); Y1[:, 1] = np.nan; Y1[7, 1] = 1.0
    Pn = bwgr_amd.Panel(np.asfortranarray(X[:100]))
    Pf = bwgr_amd.Panel(X.astype(np.float32) + 0.5)
    try:
        yield "k", lambda: bwgr_amd.PEGS(PC.traits(X, 17, 0.0, seed=2), P, maxit=2)
        yield "XFA", lambda: bwgr_amd.PEGS(Y, P, maxit=2, XFA=4)
        yield "maxit", lambda: bwgr_amd.PEGS(Y, P, maxit=-1)
        yield "covbend", lambda: bwgr_amd.PEGS(Y, P, maxit=2, covbend=float("nan"))
        yield "covMinEv", lambda: bwgr_amd.PEGS(Y, P, maxit=2, covMinEv=float("inf"))
        yield "logtol", lambda: bwgr_amd.PEGS(Y, P, maxit=2, logtol=float("nan"))
        yield "trait 1", lambda: bwgr_amd.PEGS(Y1, P, maxit=2)
        yield "fp32", lambda: bwgr_amd.PEGS(Y, Pf, maxit=2)
        yield "rows", lambda: bwgr_amd.PEGSZ(Y, [P, Pn], maxit=2)
        yield "rows", lambda: bwgr_amd.PEGSZ(Y, [P, Z[:100]], maxit=2)
        yield "not finite", lambda: bwgr_amd.PEGSZ(Y, [P, Zbad], maxit=2)
        yield "TrXSX", lambda: bwgr_amd.PEGSZ(Y, [P, bwgr_amd.dense(np.ones((n, 2)))], maxit=2)
        yield "effects", lambda: bwgr_amd.PEGSZ(Y, [], maxit=2)
    finally:
        Pn.close(); Pf.close()


def test_refusals_leave_the_panel_usable():
    import bwgr_amd
    X = PC.tpod()
    Y = PC.traits(X, 3, 0.1, seed=51)
    y = np.nan_to_num(Y[:, 0], nan=3.0)
    P = bwgr_amd.Panel(X)
    try:
        ref = bwgr_amd.BayesRR(y, P, it=20, bi=5, seed=7)
        for word, call in _refusals(P, X, Y):
            with pytest.raises(bwgr_amd.BwgrError) as ei:
                call()
            assert ei.value.code == 1 and word in str(ei.value), (word, str(ei.value))
            again = bwgr_amd.BayesRR(y, P, it=20, bi=5, seed=7)
            for key in ref:
                assert np.array_equal(np.asarray(ref[key]), np.asarray(again[key])), (word, key)
        assert bwgr_amd.PEGS(Y, P, maxit=1)["numit"] == 1
    finally:
        P.close()


def test_panels_on_different_devices_are_refused():
    import bwgr_amd
    if bwgr_amd.device_count() < 2:
        pytest.skip("one device visible: two panels cannot live on different devices")
    X = PC.tpod()
    P, Q = bwgr_amd.Panel(X, device=0), bwgr_amd.Panel(X, device=1)
    try:
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            bwgr_amd.PEGSZ(PC.traits(X, 2, 0.1, seed=3), [P, Q], maxit=1)
        assert ei.value.code == 1 and "device" in str(ei.value)
    finally:
        P.close(); Q.close()


def test_mrr_before_and_after_a_pegs_call():
    import bwgr_amd
    X = PC.tpod()
    Y = PC.traits(X, 3, 0.1, seed=61)
    P = bwgr_amd.Panel(X)
    try:
        a = bwgr_amd.mrr(Y, P, maxit=5, tol=0)
        bwgr_amd.PEGS(Y, P, maxit=3, logtol=PC.NOSTOP)
        bwgr_amd.PEGSZ(Y, [PC.gauss(X.shape[0], 5, 2), P], maxit=3, logtol=PC.NOSTOP)
        b = bwgr_amd.mrr(Y, P, maxit=5, tol=0)
    finally:
        P.close()
    for key in bwgr_amd.api.MRR_KEYS:
        assert np.array_equal(a[key], b[key]), key


def test_maxit_zero():
    import bwgr_amd
    Y, effects = PC.by_id("tpod_k3_defaults")["data"]()
    g = bwgr_amd.PEGS(Y, effects[0][1], maxit=0)
    assert g["numit"] == 0 and g["cnv"] == 10.0 and np.all(g["b"] == 0) and np.allclose(g["h2"], 0.5)
    assert np.array_equal(g["hat"], np.broadcast_to(g["mu"], g["hat"].shape))
