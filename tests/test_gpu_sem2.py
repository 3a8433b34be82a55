"""GPU: solver2x for every column of Y (bwgr_uvbeta2) and the drivers MEGA / GSEM against the float64 restatement tests/sem2_restatement.py,
end to end and stage by stage.  The inputs are tests/sem2_cases.py's; tests/test_sem2_cpu.py asserts their preconditions (singular values
apart, no cnv near log10(tol)) on the restatement.

Parity is mrr_restatement.scaled_err(got, restatement) <= 1e-6 with NaN in the same places, and equal its."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrr_restatement as MR  # noqa: E402
import sem2_cases as C  # noqa: E402
import sem2_restatement as S2  # noqa: E402
import uvb_restatement as UR  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6
KEYS = ("b1", "b2", "mu", "h2", "ve", "vb1", "vb2", "its", "cnv")
MEGA_KEYS = ("mu", "b", "hat", "LS", "LS_BETA", "BETA1", "BETA2", "gebv")
GSEM_KEYS = ("mu", "b", "hat")
INVARIANT = {"MEGA": ("mu", "b", "hat", "BETA2", "gebv"), "GSEM": ("mu", "b", "hat")}


def _err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    return MR.scaled_err(np.nan_to_num(a), np.nan_to_num(b))


def _check(g, o, what=""):
    assert tuple(g) == KEYS
    assert np.array_equal(g["its"], o["its"]), (g["its"], o["its"])
    errs = {key: _err(g[key], o[key]) for key in KEYS if key != "its"}
    print(what, errs)
    assert all(v <= TOL for v in errs.values()), errs


def _same(a, b):
    assert list(a) == list(b)
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def _run(c, **panel_kw):
    import bwgr_amd
    if "nwg" in c:
        panel_kw.setdefault("nwg", c["nwg"])
    return bwgr_amd.uvbeta2(c["Y"], c["Z"], c["X"], **c["kw"], **panel_kw)


# ---- the engine ----
@pytest.mark.parametrize("name", [n for n in C.ENGINE if n != "slabs_defaults"])
def test_uvbeta2(name):
    """tpod (196 x 376: six blocks, the last of 56 markers): k = q = 3; q = 1 and q = 7 > k; k = 17 (two solve workgroups); k = 65 (two
    groups, the second with one trait); p = 1, 63, 64, 65; shared patterns, a fully observed trait, an all-NaN trait, XX1 = 0 for one trait,
    TrXSX1 = 0 for one trait; maxit = 0 and 1."""
    c, o = C.engine(name), C.engine_ref(name)
    g = _run(c)
    _check(g, o, name)
    k = c["Y"].shape[1]
    assert g["b1"].shape == (c["Z"].shape[1], k) and g["b2"].shape == (c["X"].shape[1], k)
    if name == "maxit0":
        assert not g["b1"].any() and not g["b2"].any() and not g["its"].any() and np.isnan(g["cnv"]).all()
    if name == "all_nan_trait":
        assert not g["b1"][:, 2].any() and not g["b2"][:, 2].any() and g["its"][2] == 0 and g["mu"][2] == 0 and g["h2"][2] == 0
    if name == "xx1_zero":
        assert g["b1"][1, 0] == 0 and g["b1"][1, 1] != 0
    if name == "trx1_zero":      # the dense design is skipped for trait 1: the panel runs as if alone, bit for bit
        import bwgr_amd
        d = bwgr_amd.uvbeta(c["Y"], c["X"], "D", **c["kw"])
        assert not g["b1"][:, 1].any() and np.isnan(g["vb1"][1])
        assert np.array_equal(g["b2"][:, 1], d["b"][:, 1]) and g["mu"][1] == d["mu"][1] and g["its"][1] == d["its"][1]
        assert g["vb2"][1] == d["vb"][1] and g["ve"][1] == d["ve"][1] and g["cnv"][1] == d["cnv"][1]


def test_defaults_on_three_slabs_and_frozen_traits():
    """700 x 900, nwg = 3, the reference's defaults: the four traits stop at four different sweeps.  A stopped trait is frozen through both
    legs: its columns of b1 and b2 are the same bits whether the call ends at its sweep or runs on to maxit = 100 for the others."""
    import bwgr_amd
    c, o = C.engine("slabs_defaults"), C.engine_ref("slabs_defaults")
    P = bwgr_amd.Panel(c["X"], nwg=3)
    try:
        assert P.nwg == 3
        g = bwgr_amd.uvbeta2(c["Y"], c["Z"], P)
        _check(g, o, "slabs_defaults")
        assert len(set(g["its"])) == 4
        for t in np.argsort(g["its"])[:3]:
            short = bwgr_amd.uvbeta2(c["Y"], c["Z"], P, maxit=int(g["its"][t]))
            assert short["its"][t] == g["its"][t]
            for key in ("b1", "b2"):
                assert np.array_equal(short[key][:, t], g[key][:, t]), (key, t)
            assert short["mu"][t] == g["mu"][t] and short["cnv"][t] == g["cnv"][t]
    finally:
        P.close()


@pytest.mark.parametrize("side", ["below", "above"])
def test_both_residual_paths_of_the_leg(side):
    """The trait's row of E in LDS (n <= lds_rows) and in place in global memory (n > lds_rows); the threshold is read from the plan."""
    import bwgr_amd
    L = bwgr_amd.uvbd_plan(1000, 2, 2)["lds_rows"]
    n = L - 27 if side == "below" else L + 37
    assert bwgr_amd.uvbd_plan(n, 2, 2)["e_in_lds"] == (1 if side == "below" else 0)
    c = C.residual_path(n)
    g = _run(c)
    _check(g, S2.uvbeta2(c["Y"], c["Z"], c["X"], **c["kw"]), side)


# ---- determinism, handles, state ----
def test_two_calls_implicit_centring_clone_and_stream():
    import torch
    import bwgr_amd
    c = C.engine("k3_q3")
    live = bwgr_amd.debug_live()
    P = bwgr_amd.Panel(c["X"])
    try:
        a = bwgr_amd.uvbeta2(c["Y"], c["Z"], P, **c["kw"])
        before = bwgr_amd.debug_live()
        _same(a, bwgr_amd.uvbeta2(c["Y"], c["Z"], P, **c["kw"]))
        assert bwgr_amd.debug_live() == before
        P.set_centred(True)
        _same(a, bwgr_amd.uvbeta2(c["Y"], c["Z"], P, **c["kw"]))
        P.set_centred(False)
        inside = bwgr_amd.debug_live()      # (the panel keeps what implicit centring made until it is closed)
        Q = P.clone()
        try:
            _same(a, bwgr_amd.uvbeta2(c["Y"], c["Z"], Q, **c["kw"]))
        finally:
            Q.close()
        s = torch.cuda.Stream()
        try:
            P.set_stream(s.cuda_stream)
            with torch.cuda.stream(s):
                torch.cuda._sleep(2_000_000)      # the caller's stream is busy when the call arrives
            on_stream = bwgr_amd.uvbeta2(c["Y"], c["Z"], P, **c["kw"])
            s.synchronize()
        finally:
            P.set_stream(0)
        _same(a, on_stream)
        _same(a, bwgr_amd.uvbeta2(c["Y"], c["Z"], P, **c["kw"]))
        assert bwgr_amd.debug_live() == inside
        with pytest.raises(bwgr_amd.BwgrError):
            bwgr_amd.uvbeta2(c["Y"], c["Z"], P, maxit=-1)
        assert bwgr_amd.debug_live() == inside
    finally:
        P.close()
    assert bwgr_amd.debug_live() == live
    _check(a, C.engine_ref("k3_q3"))
    v = bwgr_amd.solver2x(c["Y"][:, 0], c["Z"], c["X"], **c["kw"])      # the one-trait form: (mu, b_1, b_2)
    assert v.shape == (1 + 3 + 376,) and v[0] == a["mu"][0] and np.array_equal(v[1:4], a["b1"][:, 0]) and np.array_equal(v[4:], a["b2"][:, 0])


def test_refusals():
    import bwgr_amd
    c = C.engine("k3_q3")
    Y, Z, X = c["Y"], c["Z"], c["X"]
    live = bwgr_amd.debug_live()

    def refused(call, *words):
        with pytest.raises(bwgr_amd.BwgrError) as ei:
            call()
        assert ei.value.code == 1 and all(w in str(ei.value) for w in words), str(ei.value)
        assert bwgr_amd.debug_live() == live

    refused(lambda: bwgr_amd.uvbeta2(Y, Z, X.astype(np.float32) + 0.5), "fp32")
    Zn = np.array(Z)
    Zn[5, 1] = np.nan
    refused(lambda: bwgr_amd.uvbeta2(Y, Zn, X), "Z[5, 1]", "not finite")
    refused(lambda: bwgr_amd.uvbeta2(Y, Z[:, :0], X), "q = 0")
    Y1 = np.array(Y)
    Y1[:, 2] = np.nan
    Y1[0, 2] = 1.0
    refused(lambda: bwgr_amd.uvbeta2(Y1, Z, X), "trait 2", "one observed row")
    refused(lambda: bwgr_amd.uvbeta2(Y, Z, X, maxit=-1), "maxit = -1")
    Yd = C.tpod_traits()
    for fn in (bwgr_amd.MEGA, bwgr_amd.GSEM):
        refused(lambda: fn(Yd, X, 5, maxit=2, tol=0), "npc")
    refused(lambda: bwgr_amd.MEGA(C.nan_trait_traits(), X, 2, maxit=2, tol=0), "trait 2", "no record")


# ---- the drivers ----
def _signs(g, o):
    sign = np.sign((np.asarray(g) * np.asarray(o)).sum(0))
    assert np.all(sign != 0)
    return sign


def _check_driver(name, g, o):
    assert tuple(g) == (MEGA_KEYS if name == "MEGA" else GSEM_KEYS)
    errs = {key: _err(g[key], o[key]) for key in INVARIANT[name]}
    if name == "MEGA":      # LS, LS_BETA and BETA1 are defined up to the sign of each singular pair
        sign = _signs(g["LS"], o["LS"])
        errs.update(LS=_err(g["LS"] * sign, o["LS"]), LS_BETA=_err(g["LS_BETA"] * sign, o["LS_BETA"]), BETA1=_err(g["BETA1"] * sign[:, None], o["BETA1"]))
    print(name, errs)
    assert all(v <= TOL for v in errs.values()), errs


@pytest.mark.parametrize("name,case", [nc for nc in C.DRIVER_CASES if nc[1].startswith("tpod")])
def test_drivers_end_to_end(name, case):
    import bwgr_amd
    c, o = C.DRIVER[case](), C.driver_ref(name, case)
    assert o["npc"] == {"tpod_npc0": 4, "tpod_npc-1": 4, "tpod_npc2": 2}[case]
    g = getattr(bwgr_amd, name)(c["Y"], c["X"], c["npc"], **c["kw"])
    _check_driver(name, g, o)
    if name == "MEGA":
        assert g["LS"].shape == (196, o["npc"]) and g["LS_BETA"].shape == (376, o["npc"]) and g["BETA1"].shape == (o["npc"], 4) and g["gebv"].shape == (196, 4)


@pytest.mark.parametrize("name", ["MEGA", "GSEM"])
def test_drivers_stage_by_stage(name):
    """The stages the driver is composed of, called as the driver calls them: BETA, G, the latent design up to the sign of each column,
    MEGA's UVBETA(LS, X), and the two-design fit on the restatement's own LS."""
    import bwgr_amd
    from bwgr_amd import api
    c, o = C.DRIVER["tpod_npc0"](), C.driver_ref(name, "tpod_npc0")
    X, Y = c["X"], c["Y"]
    P = bwgr_amd.Panel(X)
    try:
        s1 = bwgr_amd.uvbeta(Y, P, "D", **c["kw"])
        G = P.xb(s1["b"])
        if name == "MEGA":
            LS = api._mega_latent(np.asarray(Y), G, 0, name)
            lsb = bwgr_amd.uvbeta(o["LS"], P, "D", **c["kw"])
        else:
            LS, V = api._sem_latent(G, 0, name)
        fit = bwgr_amd.uvbeta2(Y, o["LS"], P, **c["kw"])
    finally:
        P.close()
    assert _err(s1["b"], o["BETA"]["b"]) <= TOL and _err(G, o["G"]) <= TOL
    sign = _signs(LS, o["LS"])
    assert _err(LS * sign, o["LS"]) <= TOL
    if name == "MEGA":
        assert _err(lsb["b"], o["LS_BETA"]) <= TOL and np.array_equal(lsb["its"], o["LSB"]["its"])
    else:
        assert _err(V * sign, o["V"][:, :4]) <= TOL
    _check(fit, o["fit"], name)


@pytest.mark.parametrize("name", ["MEGA", "GSEM"])
def test_drivers_with_the_references_defaults(name):
    """maxit = 100, tol = 10e-7 on the 700 x 900 three-slab panel: every stage stops by its own test (tests/test_sem2_cpu.py asserts that no
    cnv of the restatement comes nearer than 0.02 to log10(tol)), so the sweep counts agree.  The panel that was passed in stays usable."""
    import bwgr_amd
    c, o = C.DRIVER["slabs_defaults"](), C.driver_ref(name, "slabs_defaults")
    P = bwgr_amd.Panel(c["X"], nwg=3)
    try:
        g = getattr(bwgr_amd, name)(c["Y"], P)
        again = P.xb(g["b"])
    finally:
        P.close()
    _check_driver(name, g, o)
    assert MR.scaled_err(again, c["X"].astype(np.float64) @ g["b"]) <= 1e-12
    if name == "MEGA":
        assert _err(again + g["mu"], g["gebv"]) <= 1e-12


def test_gsem_with_an_all_nan_trait():
    """Trait 2 has no record (npc = k - 1 = 3: the fourth direction of G is null): zero columns exactly where the restatement's are."""
    import bwgr_amd
    c, o = C.DRIVER["nan_trait"](), C.driver_ref("GSEM", "nan_trait")
    g = bwgr_amd.GSEM(c["Y"], c["X"], c["npc"], **c["kw"])
    _check_driver("GSEM", g, o)
    for key in ("b", "hat"):
        assert np.array_equal(g[key] == 0, o[key] == 0), key
    assert not g["b"][:, 2].any() and not g["hat"][:, 2].any() and g["mu"][2] == 0 and not o["b"][:, 2].any()
