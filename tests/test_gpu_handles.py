"""GPU: every entry point on every kind of handle -- the root panel on the default stream, a clone (its own non-blocking stream), the root on
a caller's stream (bwgr_panel_set_stream) and the root back on the default stream -- must give the same bits, and the first must pass the
entry's existing comparison with the oracle or its restatement.  tpod (196 x 376) and the 700 x 900 three-slab panel: size is not the point.

On the default (null) stream every stray hipMemcpy, hipMemset or launch on stream 0 is ordered for free; on a non-blocking stream it is a
race.  To make such a race lose, the caller's stream is kept busy: before each call on it a spin kernel (torch.cuda._sleep) is enqueued
there that lasts at least five times the entry's own time on the default stream (both measured with events and printed).  Whatever the
library issues off the caller's stream without an event dependency then runs before its inputs exist and shows as wrong bits.  The null
stream gets a filler of its own that outlasts the caller's filler and the entry together: an entry's early operations are ordered by its
own host synchronisations whatever stream they are on, but a late launch on stream 0 queues behind that filler and has not run when the
entry copies its results out with hipMemcpyAsync on the caller's stream (mrr, the uvbeta family, xb, the samplers).  The relationship
kernels hand their results out by hipMemcpy2DAsync, which on this runtime was measured to wait for stream 0 (tools/stream0_probe.py): a
late launch on stream 0 in them cannot be seen by a caller, here or anywhere else.

What this does and does not prove.  It is believed, not measured, that this runtime makes a host-to-device copy from pageable memory
host-synchronous; if so, an entry's first such copy on the caller's stream waits for the filler, and operations mis-ordered after that copy
are caught only by the natural durations of the work they race with.  These tests catch what runs on the null stream cannot catch at all;
they are not a proof of ordering.  One entry proves less than the others: with device_out=True Panel._out2d waits for the whole device before it
calls the library (the tensors it has just made must exist), which drains the filler, so kernel2_GAU_device and GRM_device are ordered
against the natural durations of their own launches only.

The two-panel entries (crossprod2, kernel2 on the 700 x 900 root and a 300 x 900 samples panel in slabs of another height) run in the table like
the others, the samples on the default stream; test_two_panel_entry_on_every_pair_of_handles then puts the founders and the samples on
different streams and clones.

PEGS, PEGSZ ([panel, dense of five columns]) and PEGSX (the same effects, f = 3), and PEGSZ_S / PEGSX_S ([panel, sparse incidence, sparse
overlapping design]) on the 700 x 900 root issue the library's longest host
sequences -- 20 to 30 copies, clears and launches per sweep on the first panel's stream -- and stand in the table like the others (their inputs,
and the branch guards on them, are tests/tall_cases.py's handle_case and tests/test_tall_cases_cpu.py);
test_two_panel_effects_of_one_pegsz_call_on_different_handles puts the two panel effects of one PEGSZ call on different handles."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernels2_restatement as K2  # noqa: E402
import kernels_restatement as KR  # noqa: E402
import mrr_restatement as MR  # noqa: E402
import pegs_cases as PC  # noqa: E402
import pegs_restatement as PR  # noqa: E402
import pegsx_cases as XC  # noqa: E402
import tall_cases as tc  # noqa: E402
import sem2_cases as C2  # noqa: E402
import sem2_restatement as S2  # noqa: E402
import sem_restatement as SR  # noqa: E402
import uvb_restatement as UR  # noqa: E402
from conftest import scaled_err, synth_small  # noqa: E402
from test_gpu_mrr import _check as _mrr_check, _traits  # noqa: E402
from test_gpu_parity import _em_check, _rel  # noqa: E402
from test_gpu_sem import _check as _sem_check, _strong, _well_posed  # noqa: E402
from test_gpu_sem2 import _check as _uvb2_check, _check_driver  # noqa: E402
from test_gpu_uvb import _check as _uvb_check, _slabs900  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-6
FILL = 5.0      # the filler lasts at least this many times the entry's own time
# While ALT["on"], every entry's call runs on other inputs (another phenotype, other traits, another B).  One such call goes before the call on
# the caller's stream: the library's freed temporaries then hold another problem's numbers, not -- from the call before -- this one's results,
# which an operation that runs too early would otherwise find ready-made.
ALT = {"on": False}


def _y():
    y = _tpod()[1]
    return 0.5 * y + 1.0 if ALT["on"] else y


def _Y(which):
    Y = _slab_traits(which)
    return np.ascontiguousarray(Y[:, ::-1]) if ALT["on"] else Y


@functools.lru_cache(None)
def _tpod():
    d = np.load(os.path.join(ROOT, "tests", "golden", "tpod.npz"))
    X = np.asfortranarray(d["gen"])
    X.setflags(write=False)
    return X, d["y"].astype(np.float64)


@functools.lru_cache(None)
def _kmup_inputs():
    """b, d, xx, e, L of test_kmup_sweep_tpod and the rows and xx of test_kmup2_tpod"""
    X, y = _tpod()
    n, p = X.shape
    rs = np.random.RandomState(5)
    Xd = X.astype(np.float64)
    xx = (Xd ** 2).sum(0)
    b = rs.normal(size=p) * 0.01
    e = y - y.mean() - Xd @ b
    L = np.full(p, 120.0) * rs.uniform(0.5, 2.0, p)
    use = np.sort(np.random.RandomState(9).choice(n, 120, replace=True)).astype(np.int32)
    return dict(b=b, d=np.ones(p), xx=xx, e=e, L=L, use=use, xx2=xx * (120.0 / n))


@functools.lru_cache(None)
def _eigk():
    Z = _tpod()[0].astype(np.float64); Z = Z - Z.mean(0)
    K = Z @ Z.T; K = K / np.mean(np.diag(K))
    w, v = np.linalg.eigh(K); o = np.argsort(-w)
    return {"values": w[o], "vectors": v[:, o]}


BAYES2_KW = dict(it=12, bi=3, pi=0.7, seed=21)


@functools.lru_cache(None)
def _x2():
    """the second, fp32 panel's matrix of BayesB2 and the phenotype that depends on it"""
    X, y = _tpod()
    X2 = np.random.default_rng(5).normal(size=(X.shape[0], 90)).astype(np.float32)
    return X2, (y + 0.7 * float(np.std(y)) * X2[:, 0]).astype(np.float32)


@functools.lru_cache(None)
def _slab_traits(which):
    X = _slabs900()
    if which == "mrr":
        return _traits(X, 3, 0, seed=5, patterns=[0.1, 0.0, 0.25])
    if which == "uvb":
        return _traits(X, 5, 0, seed=5, patterns=[0.1, 0.0, 0.25, 0.05, 0.4])
    if which == "uvb2":
        return C2.traits(X, 3, 0.1, 61)
    if which == "sem2":
        return C2.slab_traits()      # tests/sem2_cases.py's: test_sem2_cpu asserts the drivers' preconditions on it (gaps 0.165 and 0.373)
    return _strong(X, 3, seed=302)      # test_gpu_sem's: gaps 0.278 and 0.243


# ---- the entries: (panel, call(P, aux) -> dict of arrays, check(result) against the oracle or the restatement) ----
def _wgr_check(g, o):
    assert scaled_err(g["b"], o["b"]) < TOL and scaled_err(g["hat"], o["hat"]) < TOL
    assert scaled_err(np.atleast_1d(g["Vb"]), np.atleast_1d(o["Vb"])) < 5 * TOL and scaled_err(g["d"], o["d"]) < 1e-12
    assert _rel(g["Ve"], o["Ve"]) < TOL and _rel(g["mu"], o["mu"]) < TOL and _rel(g["cxx"], o["cxx"]) < 1e-12
    if "u" in o:
        assert scaled_err(g["u"], o["u"]) < 5 * TOL and _rel(g["Vk"], o["Vk"]) < TOL


def _kmup(P, aux):
    import bwgr_amd
    k = _kmup_inputs()
    return bwgr_amd.KMUP(P, k["b"], k["d"], k["xx"], k["e"] * (0.7 if ALT["on"] else 1.0), k["L"], 0.03, 0.3, seed=77, it=3)


def _kmup_ok(g):
    from oracle import oracle as O
    k = _kmup_inputs()
    o = O.kmup(_tpod()[0], k["b"], k["d"], k["xx"], k["e"], k["L"], 0.03, 0.3, seed=77, it=3)
    assert scaled_err(g["b"], o["b"]) < TOL and scaled_err(g["e"], o["e"]) < TOL and np.array_equal(g["d"], o["d"])


def _kmup2(P, aux):
    import bwgr_amd
    k = _kmup_inputs()
    return bwgr_amd.KMUP2(P, k["use"], k["b"], k["d"], k["xx2"], k["e"] * (0.7 if ALT["on"] else 1.0), k["L"], 0.03, 0.3, seed=78, it=4)


def _kmup2_ok(g):
    from oracle import oracle as O
    k = _kmup_inputs()
    o = O.kmup2(_tpod()[0], k["use"], k["b"], k["d"], k["xx2"], k["e"], k["L"], 0.03, 0.3, seed=78, it=4)
    assert scaled_err(g["b"], o["b"]) < TOL and scaled_err(g["e"], o["e"]) < TOL and np.array_equal(g["d"], o["d"])


WGR = {"wgr": dict(it=25, bi=5, seed=21), "wgr_bag": dict(it=20, bi=5, seed=17, bag=0.7, pi=0.3),
       "wgr_eigK": dict(it=25, bi=5, VarK=0.9, seed=13)}


def _wgr(name):
    def call(P, aux):
        import bwgr_amd
        return bwgr_amd.wgr(_y(), P, **WGR[name], **({"eigK": _eigk()} if name == "wgr_eigK" else {}))

    def ok(g):
        from oracle import oracle as O
        X, y = _tpod()
        _wgr_check(g, O.wgr(y, X, **WGR[name], **({"eigK": _eigk()} if name == "wgr_eigK" else {})))
    return call, ok


def _em(model):
    def call(P, aux):
        import bwgr_amd
        return getattr(bwgr_amd, model)(_y(), P)

    def ok(g):
        from oracle import oracle as O
        X, y = _tpod()
        _em_check(model, g, O.em(model, y, X), tol=2e-6 if model == "emBCpi" else TOL)      # (test_em_family_tpod_defaults' bounds)
    return call, ok


def _bayes2(P, aux):
    import bwgr_amd
    return bwgr_amd.BayesB2(_x2()[1] * np.float32(0.5 if ALT["on"] else 1.0), P, aux["P2"], **BAYES2_KW)


def _bayes2_ok(g):
    from oracle import oracle as O
    X2, y2 = _x2()
    o = O.bayes2("BayesB2", y2, _tpod()[0].astype(np.float32), X2, **BAYES2_KW)
    for k in ("b1", "b2", "hat", "vb1", "vb2", "d1", "d2"):
        assert scaled_err(g[k], o[k]) < TOL, k
    for k in ("mu", "ve", "h2"):
        assert abs(g[k] - o[k]) <= TOL * max(1.0, abs(o[k])), k


CHAIN_KW = dict(it=6, bi=1, pi=0.9, df=5, R2=0.5, seed=11)


def _chain(P, aux):
    import bwgr_amd
    ch = bwgr_amd.Chain(P, "BayesB", _y(), **CHAIN_KW)
    try:
        ch.run(6)
        out = dict(ch.result())
        out.update({"state_" + k: v for k, v in ch.state().items()})
    finally:
        ch.close()
    return out


def _chain_ok(g):
    from oracle import oracle as O
    X, y = _tpod()
    o = O.bayes("BayesB", y, X, **CHAIN_KW)
    assert scaled_err(g["b"], o["b"]) < TOL and scaled_err(g["hat"], o["hat"]) < TOL and np.array_equal(g["d"], o["d"])
    assert _rel(g["ve"], o["ve"]) < TOL and _rel(g["mu"], o["mu"]) < TOL
    assert scaled_err(g["state_e"], o["last"]["e"]) < TOL and scaled_err(g["state_b"], o["last"]["b"]) < TOL


def _stats(P, aux):
    xx, vx, msx = P.stats()
    return dict(xx=xx, vx=vx, msx=msx)


def _stats_ok(g):
    from oracle import oracle as O
    oxx, ovx, omsx = O.stats(_tpod()[0])
    assert np.array_equal(g["xx"], oxx) and scaled_err(g["vx"], ovx) < 1e-7 and _rel(g["msx"], omsx) < 1e-7


def _mrr(P, aux):
    import bwgr_amd
    return bwgr_amd.MRR3(_Y("mrr"), P, maxit=5, tol=0)


def _mrr_ok(g):
    _mrr_check(g, MR.mrr(_slab_traits("mrr"), _slabs900(), maxit=5, tol=0))


def _uvb(P, aux):
    import bwgr_amd
    return bwgr_amd.uvbeta(_Y("uvb"), P, "D", maxit=4, tol=0, xb=True)


def _uvb_ok(g):
    X = _slabs900()
    _uvb_check(g, UR.uvbeta(_slab_traits("uvb"), X, "D", maxit=4, tol=0))
    assert MR.scaled_err(g["xb"], X.astype(np.float64) @ g["b"]) <= 1e-12


@functools.lru_cache(None)
def _B():
    return np.random.default_rng(5).normal(size=(900, 17))


def _xb(P, aux):
    return dict(xb=P.xb(-1.5 * _B() if ALT["on"] else _B()))


def _xb_ok(g):
    assert MR.scaled_err(g["xb"], _slabs900().astype(np.float64) @ _B()) <= 1e-12


def _crossprod(P, aux):
    return dict(G=P.crossprod())


def _crossprod_ok(g):
    assert np.array_equal(g["G"], KR.crossprod(_slabs900()))


def _grm(device_out):
    def call(P, aux):
        K = P.kernel("GRM", device_out=device_out)
        return dict(K=K.cpu().numpy() if device_out else K)

    def ok(g):
        assert MR.scaled_err(g["K"], KR.GRM(np.ascontiguousarray(_slabs900()))) <= TOL and np.array_equal(g["K"], g["K"].T)
    return call, ok


def _zsemf(P, aux):
    import bwgr_amd
    return bwgr_amd.ZSEMF(_Y("sem"), P, 0, maxit=6, tol=0)


def _zsemf_ok(g):
    o = SR.ZSEMF(_slab_traits("sem"), _slabs900(), 0, maxit=6, tol=0)
    _well_posed(o)
    _sem_check("ZSEMF", g, o)


@functools.lru_cache(None)
def _samples900():
    """the samples of the two-panel entries: 300 x 900, other genotypes than the root's"""
    X = np.asfortranarray(synth_small(300, 900, seed=6)[0])
    X.setflags(write=False)
    return X


@functools.lru_cache(None)
def _pair_ref(kind, phi=1.0):
    """the exact product (kind None) or the restated (K_ff, K_fs) of the root and the samples, computed once"""
    F, S = np.ascontiguousarray(_slabs900()), np.ascontiguousarray(_samples900())
    return K2.crossprod2(F, S) if kind is None else K2.kernels(kind, F, S, phi)


def _crossprod2(P, aux):
    return dict(G=P.crossprod2(aux["S"]))


def _crossprod2_ok(g):
    assert g["G"].dtype == np.int64 and np.array_equal(g["G"], _pair_ref(None))


def _kernel2(kind, phi, device_out):
    def call(P, aux):
        Kff, Kfs = P.kernel2(aux["S"], kind, phi, device_out=device_out)
        return dict(Kff=Kff.cpu().numpy(), Kfs=Kfs.cpu().numpy()) if device_out else dict(Kff=Kff, Kfs=Kfs)

    def ok(g):      # test_gpu_kernels2's test_kernel2_matches_the_restatement
        rff, rfs = _pair_ref(kind, phi)
        assert g["Kff"].shape == rff.shape and g["Kfs"].shape == rfs.shape and np.all(np.isfinite(g["Kff"])) and np.all(np.isfinite(g["Kfs"]))
        assert scaled_err(g["Kff"], rff) <= TOL and scaled_err(g["Kfs"], rfs) <= TOL and np.array_equal(g["Kff"], g["Kff"].T)
    return call, ok


@functools.lru_cache(None)
def _dense():
    Z = C2.dense(700, 3, 62)
    Z.setflags(write=False)
    return Z


def _uvb2(P, aux):
    import bwgr_amd
    return bwgr_amd.uvbeta2(_Y("uvb2"), _dense(), P, **C2.SIX)


def _uvb2_ok(g):
    _uvb2_check(g, S2.uvbeta2(_slab_traits("uvb2"), _dense(), _slabs900(), **C2.SIX))


def _sem2(name):
    """MEGA / GSEM at the reference's defaults: tests/sem2_cases.py's slabs_defaults case"""
    def call(P, aux):
        import bwgr_amd
        return getattr(bwgr_amd, name)(_Y("sem2"), P)

    def ok(g):
        _check_driver(name, g, C2.driver_ref(name, "slabs_defaults"))
    return call, ok


PEGS_FLAT = {"PEGS": ("mu", "b", "hat", "h2", "GC", "bend", "cnv"), "PEGSX": ("TrZSZ", "b", "u", "vb_list", "GC_list", "ve", "hat", "bend", "cnv")}


def _flat(g, keys, its):
    """a PEGS / PEGSZ / PEGSX result as a dict of arrays: a list (one entry per effect) becomes key0, key1, ..."""
    out = {}
    for key in keys:
        for i, v in enumerate(g[key]) if isinstance(g[key], list) else [("", g[key])]:
            out["%s%s" % (key, i)] = np.asarray(v)
    out["its"] = np.array(g[its])      # (last: the table looks at an entry's first array to see that other inputs gave another result)
    return out


def _pegs_inputs(entry):
    """(Y, X or None, the effects' data) of tests/tall_cases.py's handle_case; under ALT Y's columns are reversed, as _Y does"""
    d = tc.handle_case(entry)["data"]()
    Y = np.ascontiguousarray(d[0][:, ::-1]) if ALT["on"] else d[0]
    return Y, (d[1] if entry.startswith("PEGSX") else None), d[-1]


def _pegs(entry):
    """PEGS (k = 3, four sweeps), PEGSZ ([panel, dense of five columns]) and PEGSX (the same effects, f = 3) on the slabs panel: the longest
    host sequences of the library, 20 to 30 copies, clears and launches per sweep on the first panel's stream.  PEGSZ_S and PEGSX_S: [panel,
    sparse incidence of 12 levels, sparse overlapping design]: the sparse set-up, both legs, their reduction of d2, the sparse trace and
    k_pegs_sparse_hat, launched between host-to-device copies of the order and of iG -- one of them on stream 0 would read or write beside
    the fit's stream, and the filler would show it as other bits"""
    kw = tc.handle_case(entry)["kw"]

    def call(P, aux):
        import bwgr_amd
        Y, X, effects = _pegs_inputs(entry)
        effs = tc.gpu_effects(effects, [P])
        if entry == "PEGS":
            return _flat(bwgr_amd.PEGS(Y, P, cnv_trace=True, **kw), PEGS_FLAT["PEGS"] + ("cnv_trace",), "numit")
        if entry.startswith("PEGSZ"):
            return _flat(bwgr_amd.PEGSZ(Y, effs, cnv_trace=True, **kw), PEGS_FLAT["PEGS"] + ("cnv_trace",), "numit")
        return _flat(bwgr_amd.PEGSX(Y, X, effs, cnv_trace=True, **kw), PEGS_FLAT["PEGSX"] + ("cnv_trace",), "its")

    def ok(g):
        case = tc.handle_case(entry)
        if entry.startswith("PEGSX"):
            o = _flat(XC.restate(case)[3], PEGS_FLAT["PEGSX"], "its")
        else:
            o = PC.restate(case)[2]
            if entry == "PEGS":
                o = dict(o, b=o["b"][0], GC=o["GC"][0], bend=o["bend"][0])
            o = _flat(o, PEGS_FLAT["PEGS"], "numit")
        assert g["its"] == o["its"] == kw["maxit"]
        for key in o:
            assert PR.scaled_err(g[key], o[key]) <= TOL, (entry, key)
    return call, ok


NO_INPUTS = ("stats", "crossprod", "GRM_host", "GRM_device", "crossprod2", "kernel2_ARC_host", "kernel2_GAU_device")      # nothing but the panels
ENTRIES = {
    "KMUP": ("tpod", _kmup, _kmup_ok), "KMUP2": ("tpod", _kmup2, _kmup2_ok),
    "wgr": ("tpod",) + _wgr("wgr"), "wgr_bag": ("tpod",) + _wgr("wgr_bag"), "wgr_eigK": ("tpod",) + _wgr("wgr_eigK"),
    "emRR": ("tpod",) + _em("emRR"), "emBCpi": ("tpod",) + _em("emBCpi"), "BayesB2": ("tpod2", _bayes2, _bayes2_ok),
    "chain": ("tpod", _chain, _chain_ok), "stats": ("tpod", _stats, _stats_ok),
    "mrr": ("slabs", _mrr, _mrr_ok), "uvbeta_xb": ("slabs", _uvb, _uvb_ok), "xb": ("slabs", _xb, _xb_ok),
    "crossprod": ("slabs", _crossprod, _crossprod_ok), "GRM_host": ("slabs",) + _grm(False), "GRM_device": ("slabs",) + _grm(True),
    "ZSEMF": ("slabs", _zsemf, _zsemf_ok),
    "crossprod2": ("slabs", _crossprod2, _crossprod2_ok), "kernel2_ARC_host": ("slabs",) + _kernel2("ARC", 1.0, False),
    "kernel2_GAU_device": ("slabs",) + _kernel2("GAU", 0.5, True),
    "uvbeta2": ("slabs", _uvb2, _uvb2_ok), "MEGA": ("slabs",) + _sem2("MEGA"), "GSEM": ("slabs",) + _sem2("GSEM"),
    "PEGS": ("slabs",) + _pegs("PEGS"), "PEGSZ": ("slabs",) + _pegs("PEGSZ"), "PEGSX": ("slabs",) + _pegs("PEGSX"),
    "PEGSZ_S": ("slabs",) + _pegs("PEGSZ_S"), "PEGSX_S": ("slabs",) + _pegs("PEGSX_S"),
}


def _same(a, b, what):
    assert list(a) == list(b), what
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=np.asarray(a[key]).dtype.kind == "f"), (what, key)


class _Env:
    """The two root panels, BayesB2's second panel, the caller's stream and its filler."""

    def __init__(self):
        import torch
        import bwgr_amd
        self.torch = torch
        self.live = bwgr_amd.debug_live()
        # (tpod2: BayesB2's two panels share the residual, hence the slab geometry, and an fp32 panel's slabs have at most 128 rows)
        self.P = {"tpod": bwgr_amd.Panel(_tpod()[0]), "tpod2": bwgr_amd.Panel(_tpod()[0], nwg=2), "slabs": bwgr_amd.Panel(_slabs900(), nwg=3)}
        assert self.P["slabs"].nwg == 3 and self.P["tpod2"].nwg == 2
        # (S: the two-panel entries' samples, in three slabs of 128 rows against the root's three of 256 -- left to itself a 300-row panel
        # takes 256-row slabs like the root -- so each operand's addresses come from its own slab height)
        self.aux = {"P2": bwgr_amd.Panel(_x2()[0], nwg=2), "S": bwgr_amd.Panel(_samples900(), nwg=3)}
        assert self.aux["S"].nwg == 3 and self.aux["S"].slab_rows != self.P["slabs"].slab_rows
        self.s, self.s2 = torch.cuda.Stream(), torch.cuda.Stream()
        assert self.s.cuda_stream != 0 and self.s2.cuda_stream not in (0, self.s.cuda_stream)
        self.unit_cycles = 5_000_000
        ms = []
        for _ in range(3):      # (the first launch carries the kernel's load: the shortest of the later two is the unit)
            e0, e1 = self._spin(1)
            self.s.synchronize()
            ms.append(e0.elapsed_time(e1))
        self.unit_ms = min(ms[1:])
        assert self.unit_ms > 0

    def _spin(self, units, stream=None):
        """enqueue `units` spin kernels on the caller's stream (or on `stream`) between two events"""
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.s if stream is None else stream):
            e0.record()
            for _ in range(units):
                torch.cuda._sleep(self.unit_cycles)
            e1.record()
        return e0, e1

    def timed(self, call):
        """(result, ms) of a call on the default stream, by events around it"""
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)

    def _units(self, entry_ms):
        return int(math.ceil((FILL + 1.0) * entry_ms / self.unit_ms)) + 1

    def busy(self, entry_ms, stream=None):
        """keep the caller's stream (or `stream`) busy for more than FILL times entry_ms; returns the events that time the filler"""
        return self._spin(self._units(entry_ms), stream)

    def busy_null(self, entry_ms):
        """keep the default (null) stream busy for longer than a caller's stream's filler and the entry behind it take together: twice that
        filler's spin kernels and one more.  The library has no business on the null stream while no panel of the call sits there; what it
        launches there all the same queues behind this filler, and so runs after the call has copied its results out.  (torch's streams
        are non-blocking: nothing on them waits for the null stream by itself.)"""
        return self._spin(2 * self._units(entry_ms) + 1, self.torch.cuda.default_stream())

    def close(self):
        import bwgr_amd
        for P in list(self.P.values()) + list(self.aux.values()):
            P.set_stream(0)
            P.close()
        self.s.synchronize()
        self.s2.synchronize()
        assert bwgr_amd.debug_live() == self.live


@pytest.fixture(scope="module")
def env():
    e = _Env()
    yield e
    e.close()


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_on_every_handle(env, name):
    import bwgr_amd
    which, call, ok = ENTRIES[name]
    P = env.P[which]
    first = call(P, env.aux)
    again, entry_ms = env.timed(lambda: call(P, env.aux))
    live = bwgr_amd.debug_live()      # (after the handle's first sweeps: it keeps the scratch, stream and events they made until it is closed)
    _same(first, again, "two calls on the default stream")      # the precondition of everything below
    ok(first)
    Q = P.clone()
    try:
        on_clone = call(Q, env.aux)
    finally:
        Q.close()
    ALT["on"] = True
    try:
        other = call(P, env.aux)      # (stats, the products and the kernels have no input but the panels: the same result again)
    finally:
        ALT["on"] = False
    assert name in NO_INPUTS or not np.array_equal(next(iter(other.values())), next(iter(first.values())))
    try:
        P.set_stream(env.s.cuda_stream)
        n0, n1 = env.busy_null(entry_ms)
        e0, e1 = env.busy(entry_ms)
        on_stream = call(P, env.aux)
        env.torch.cuda.synchronize()
        filler_ms, null_ms = e0.elapsed_time(e1), n0.elapsed_time(n1)
    finally:
        P.set_stream(0)
    back = call(P, env.aux)
    print("%s: entry %.3f ms on the default stream, filler %.3f ms on the caller's, %.3f ms on the null stream" % (name, entry_ms, filler_ms, null_ms))
    assert filler_ms >= FILL * entry_ms, (filler_ms, entry_ms)
    assert null_ms >= filler_ms + entry_ms, (null_ms, filler_ms, entry_ms)
    _same(first, on_clone, "clone")
    _same(first, on_stream, "caller's stream")
    _same(first, back, "back on the default stream")
    assert bwgr_amd.debug_live() == live


# founders' and samples' handle: "root" (the default stream), "s" / "s2" (the root on a caller's stream), "clone" (its own non-blocking stream)
PAIR_HANDLES = {"founders_on_a_stream": ("s", "root"), "samples_on_a_stream": ("root", "s"), "both_on_one_stream": ("s", "s"),
                "each_on_its_own_stream": ("s", "s2"), "founders_clone": ("clone", "root"), "samples_clone": ("root", "clone")}


@pytest.mark.parametrize("how", list(PAIR_HANDLES))
@pytest.mark.parametrize("name", ["crossprod2", "kernel2_ARC_host"])
def test_two_panel_entry_on_every_pair_of_handles(env, name, how):
    """The two-panel entries with the founders and the samples on different handles: every combination must give the bits of the call with
    both roots on the default stream.  The founders' stream carries the work; the library makes it wait, by an event, for what is pending on
    the samples' stream (xyt_order), a branch that two panels on one stream never enter.  Before each call every stream of the combination
    that a caller can reach -- a caller's stream, or the default stream under a root left there -- is kept busy by a filler of FILL times
    the entry's length (a clone's own stream cannot be reached), and the temporaries of the call before are overwritten by another problem's
    (the GAU kernels of the pair the other way round), so that a launch or copy off the founders' stream finds neither its inputs nor last
    time's results.  Where neither panel sits on the default stream (both on one stream, each on its own) the null stream gets a filler
    that outlasts the caller's filler and the entry together (_Env.busy_null), behind which a launch on stream 0 after the entry's host
    synchronisations -- a finish, say -- stays queued.  For these two entries that is a precaution and no detector: measured on this
    runtime, the two-dimensional copy to pageable host memory by which they hand out their results waits for stream 0 (DESIGN.md section 3,
    scratch edit (c)), so such a launch has run by then.

    What this does not prove: the samples bring nothing to the call but their resident genotypes, uploaded when the panel was made, so a
    library that left xyt_order out would pass.  The test runs the event branch (record, wait, give the event back: debug_live), on every
    kind of pair; it does not show that the wait is needed."""
    import bwgr_amd
    torch = env.torch
    _, call, ok = ENTRIES[name]
    F, S = env.P["slabs"], env.aux["S"]
    first = call(F, env.aux)
    again, entry_ms = env.timed(lambda: call(F, env.aux))
    live = bwgr_amd.debug_live()
    _same(first, again, "two calls on the default stream")
    ok(first)
    S.kernel2(F, "GAU", 0.5); F.kernel2(S, "GAU", 0.5)
    streams = {"root": None, "s": env.s, "s2": env.s2}
    hf, hs = PAIR_HANDLES[how]
    Qf, Qs = (F.clone() if hf == "clone" else F), (S.clone() if hs == "clone" else S)
    timers = []
    try:
        for Q, h in ((Qf, hf), (Qs, hs)):
            if h in ("s", "s2"):
                Q.set_stream(streams[h].cuda_stream)
        idle_null = not ({hf, hs} & {"root", "clone"})      # (a clone's partner is a root on the default stream)
        null = env.busy_null(entry_ms) if idle_null else None
        for h in sorted({hf, hs} - {"clone"}):
            timers.append(env.busy(entry_ms, torch.cuda.default_stream() if h == "root" else streams[h]))
        got = call(Qf, {"S": Qs})
        torch.cuda.synchronize()
        filler_ms = [e0.elapsed_time(e1) for e0, e1 in timers]
        null_ms = null[0].elapsed_time(null[1]) if idle_null else None
    finally:
        for Q, h in ((Qf, hf), (Qs, hs)):
            if h == "clone":
                Q.close()
            else:
                Q.set_stream(0)
    back = call(F, env.aux)
    print("%s, %s: entry %.3f ms, fillers %s ms%s" % (name, how, entry_ms, ", ".join("%.3f" % m for m in filler_ms),
                                                       ", %.3f ms on the null stream" % null_ms if idle_null else ""))
    assert filler_ms and all(m >= FILL * entry_ms for m in filler_ms), (filler_ms, entry_ms)
    assert idle_null == (how in ("both_on_one_stream", "each_on_its_own_stream")) and (not idle_null or null_ms >= max(filler_ms) + entry_ms)
    _same(first, got, how)
    _same(first, back, "back on the default stream")
    assert bwgr_amd.debug_live() == live


# the handles of the two panel effects A and B of one PEGSZ call
PEGS_PAIR_HANDLES = {"each_on_its_own_stream": ("s", "s2"), "first_clone": ("clone", "root"), "second_clone": ("root", "clone")}


def test_two_panel_effects_of_one_pegsz_call_on_different_handles(env):
    """PEGSZ(Y, [A, B]) with the 700 x 900 panel's columns split 500 / 400 into two Panels: with both roots on the default stream (which
    passes the restatement's check), with A on one caller's stream and B on another, with A a clone, with B a clone -- the bits of the first
    every time, and debug_live back to its value.  The first panel's stream carries the whole call; B brings only its resident genotypes,
    uploaded when it was made.  Before each call every stream of the combination that a caller can reach is kept busy by a filler of FILL
    times the entry's length, the null stream by a longer one where neither panel sits there (_Env.busy_null), and the temporaries of the
    call before hold another problem's numbers (the traits' columns reversed).

    What this does not prove: as with the two-panel products, a library that made no ordering between the two handles would pass, since
    nothing of B's is pending on its stream when the call arrives; what runs off A's stream without a dependency does show."""
    import bwgr_amd
    torch = env.torch
    case = tc.handle_case("PEGSZ2")
    Y, effects = case["data"]()
    kw = dict(case["kw"], cnv_trace=True)
    keys = PEGS_FLAT["PEGS"] + ("cnv_trace",)
    live0 = bwgr_amd.debug_live()
    A, B = bwgr_amd.Panel(effects[0][1], **effects[0][2]), bwgr_amd.Panel(effects[1][1], **effects[1][2])
    try:
        assert (A.p, B.p, A.ld) == (500, 400, B.ld)

        def call(a, b, Yc=Y):
            return _flat(bwgr_amd.PEGSZ(Yc, [a, b], **kw), keys, "numit")
        first = call(A, B)
        again, entry_ms = env.timed(lambda: call(A, B))
        live = bwgr_amd.debug_live()
        _same(first, again, "two calls on the default stream")
        o = _flat(PC.restate(case)[2], PEGS_FLAT["PEGS"], "numit")
        assert first["its"] == o["its"] == 4
        for key in o:
            assert PR.scaled_err(first[key], o[key]) <= TOL, key
        streams = {"s": env.s, "s2": env.s2}
        for how, (ha, hb) in PEGS_PAIR_HANDLES.items():
            other = call(A, B, np.ascontiguousarray(Y[:, ::-1]))
            assert not np.array_equal(other["hat"], first["hat"])
            Qa, Qb = (A.clone() if ha == "clone" else A), (B.clone() if hb == "clone" else B)
            timers = []
            try:
                for Q, h in ((Qa, ha), (Qb, hb)):
                    if h in streams:
                        Q.set_stream(streams[h].cuda_stream)
                idle_null = not ({ha, hb} & {"root", "clone"})
                null = env.busy_null(entry_ms) if idle_null else None
                for h in sorted({ha, hb} - {"clone"}):
                    timers.append(env.busy(entry_ms, torch.cuda.default_stream() if h == "root" else streams[h]))
                got = call(Qa, Qb)
                torch.cuda.synchronize()
                filler_ms = [e0.elapsed_time(e1) for e0, e1 in timers]
                null_ms = null[0].elapsed_time(null[1]) if idle_null else None
            finally:
                for Q, h in ((Qa, ha), (Qb, hb)):
                    if h == "clone":
                        Q.close()
                    else:
                        Q.set_stream(0)
            print("PEGSZ [A, B], %s: entry %.3f ms, fillers %s ms%s" % (how, entry_ms, ", ".join("%.3f" % m for m in filler_ms),
                                                                        ", %.3f ms on the null stream" % null_ms if idle_null else ""))
            assert filler_ms and all(m >= FILL * entry_ms for m in filler_ms), (filler_ms, entry_ms)
            assert idle_null == (how == "each_on_its_own_stream") and (not idle_null or null_ms >= max(filler_ms) + entry_ms)
            _same(first, got, how)
            assert bwgr_amd.debug_live() == live, how
        _same(first, call(A, B), "back on the default stream")
    finally:
        A.set_stream(0); B.set_stream(0)
        A.close(); B.close()
    assert bwgr_amd.debug_live() == live0


@pytest.mark.parametrize("model,pi", [("BayesB", 0.9), ("BayesRR", 0.0)])
def test_a_chain_across_stream_changes(env, model, pi):
    """three iterations on the default stream, three on the caller's: the state and the result of six uninterrupted ones"""
    import bwgr_amd
    X, y = _tpod()
    P = env.P["tpod"]
    kw = dict(it=6, bi=1, pi=pi, seed=11)
    whole = bwgr_amd.Chain(P, model, y, **kw)
    try:
        _, run_ms = env.timed(lambda: (whole.run(6), whole.sync()))
        ref = dict(whole.result(), **{"state_" + k: v for k, v in whole.state().items()})
    finally:
        whole.close()
    parts = bwgr_amd.Chain(P, model, y, **kw)
    try:
        parts.run(3); parts.sync()
        P.set_stream(env.s.cuda_stream)
        env.busy(run_ms)
        parts.run(3); parts.sync()
        got = dict(parts.result(), **{"state_" + k: v for k, v in parts.state().items()})
    finally:
        P.set_stream(0)
        parts.close()
    _same(ref, got, model)


def test_chain_inputs_already_on_the_device(env):
    """y is written by torch on the caller's stream right behind the filler, and the chain is created with that stream set and without
    waiting for the device first (wait_for_y=False): the same bits as with y from the host."""
    import torch
    import bwgr_amd
    X, y = _tpod()
    P = env.P["tpod"]
    kw = dict(it=6, bi=1, pi=0.9, seed=11)

    def finish(ch):
        ch.run(6)
        return dict(ch.result(), **{"state_" + k: v for k, v in ch.state().items()})

    host = bwgr_amd.Chain(P, "BayesB", y, **kw)
    try:
        ref, run_ms = env.timed(lambda: finish(host))
    finally:
        host.close()
    src = torch.from_numpy(y.astype(np.float32)).cuda()
    yd = torch.zeros(P.n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ch = None
    try:
        P.set_stream(env.s.cuda_stream)
        env.busy(run_ms)
        with torch.cuda.stream(env.s):
            yd.copy_(src, non_blocking=True)
        ch = bwgr_amd.Chain(P, "BayesB", yd, wait_for_y=False, **kw)
        got = finish(ch)
    finally:
        P.set_stream(0)
        if ch is not None:
            ch.close()
    _same(ref, got, "device y")
