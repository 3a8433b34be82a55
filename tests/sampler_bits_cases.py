"""The calls whose output bits tests/golden/sampler_parent_digests.txt records (tools/family_digest.py writes the table, tests/
test_gpu_sampler_parent_bits.py compares against it): the float samplers -- KMUP / KMUP2, the fused chains, the two-panel models, wgr, the EM
family, a group on one device, a chain on implicitly centred columns -- and every path of a sweep's planning and launching: pairs, clones,
block ranges, the fixed-shape k_sweep3f, the fp64 redo and the engine switches.  These families draw from a counter-based generator and reduce
in a fixed order, so equal inputs give equal bits.

The data come from seeded numpy generators.  The shapes are the smallest at which these paths leave the trivial case: an int8 panel of
300 x 1000 with three slabs and 64-marker blocks (the lag-3 / lag-4 pipelines, the byte planes and k_sweep3 are reachable), an int8 panel of
512 x 2048 in the default geometry (128-marker blocks: k_sweep3f's shape) and an fp32 panel of 200 x 300 (the fp32 instantiations).

CASES maps a name to a function that runs the calls and returns {"call / output": array}.  Every case runs with the engine switches of the
environment unset but for its own: the switches are read when a panel is made."""
import contextlib
import ctypes as C
import functools
import hashlib
import os

import numpy as np

IT, BI = 30, 10
I8_KW = dict(nwg=3, block=64)
SWITCHES = ("BWGR_SWEEP", "BWGR_LAG", "BWGR_SOLO3", "BWGR_STREAM3", "BWGR_PF3", "BWGR_PF3B", "BWGR_R3", "BWGR_D3", "BWGR_NFEED", "BWGR_ENG3_THR", "BWGR_DRAWS",
            "BWGR_GRAM16", "BWGR_FIXED3", "BWGR_WINV", "BWGR_WFX", "BWGR_WPF", "BWGR_WAHEAD", "BWGR_WNQ", "BWGR_WLAG", "BWGR_DEBUG_SH_ADD", "BWGR_OCC_GUARD")


def _bw():
    try:
        import torch  # noqa: F401  (before the library: bwgr_amd/_lib.py)
    except ImportError:
        pass
    import bwgr_amd
    return bwgr_amd


@contextlib.contextmanager
def switches(**kw):
    saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k in kw:
            os.environ.pop(k, None)
        os.environ.update(saved)


@functools.lru_cache(None)
def data(name):
    """(X, y) of one of the three panels"""
    g = np.random.default_rng({"i8": 20260726, "fixed": 20260727, "f32": 20260728}[name])
    if name == "f32":
        X = g.standard_normal((200, 300)).astype(np.float32)
    else:
        n, p = (300, 1000) if name == "i8" else (512, 2048)
        X = g.binomial(2, g.uniform(0.05, 0.5, p), size=(n, p)).astype(np.int8)
    n, p = X.shape
    beta = np.where(g.uniform(size=p) < 0.05, g.standard_normal(p), 0.0)
    y = X.astype(np.float64) @ beta
    y = y - y.mean() + g.standard_normal(n) * (y.std() + 1e-3)
    X.setflags(write=False)
    return X, y.astype(np.float32)


def _panel(name):
    return _bw().Panel(data(name)[0], **(I8_KW if name == "i8" else dict(as_int8=False) if name == "f32" else {}))


def _flat(out, call, result):
    for k, v in result.items():
        out["%s / %s" % (call, k)] = v


def _chain(P, name, model="BayesB", seed=11, pi=None):
    from bwgr_amd.api import Chain
    return Chain(P, model, data(name)[1], IT, BI, (0.95 if model in ("BayesB", "BayesC") else 0.0) if pi is None else pi, 5.0, 0.5, seed, 0)


def _run_chain(P, name, model="BayesB", seed=11):
    ch = _chain(P, name, model, seed)
    try:
        ch.run(IT)
        return ch.result()
    finally:
        ch.close()


def _which(P):
    from bwgr_amd import _lib
    w = C.c_int(-1)
    _lib.check(_lib.lib().bwgr_debug_sweep3_kernel(P._h, C.byref(w)))
    return w.value


# ---- the families' calls (the table tools/family_digest.py has printed since the samplers' host entries were split out) ----
def _samplers(name):
    def run():
        bw = _bw()
        X, y = data(name)
        g = np.random.default_rng(5)
        n, p = X.shape
        out = {}
        P = _panel(name)
        try:
            xx, vx, msx = P.stats()
            b0 = (g.standard_normal(p) * 0.01).astype(np.float32)
            d0 = (g.uniform(size=p) < 0.5).astype(np.float32)
            L = np.full(p, float(msx), np.float32)
            e0 = (y - y.mean()).astype(np.float32)
            use = np.sort(g.integers(0, n, size=n // 2)).astype(np.int32)
            use[1] = use[0]                                       # a repeated row
            for pi in (0.0, 0.7):
                _flat(out, "KMUP pi=%g" % pi, bw.KMUP(P, b0, d0, xx, e0, L, 1.0, pi, seed=3, it=2))
                _flat(out, "KMUP2 pi=%g" % pi, bw.KMUP2(P, use, b0, d0, xx, e0, L, 1.0, pi, seed=3, it=2))
            for model in ("BayesA", "BayesB", "BayesC", "BayesL", "BayesRR", "BayesCpi", "BayesDpi"):
                _flat(out, model, _run_chain(P, name, model))
            yd = y.astype(np.float64)
            _flat(out, "wgr", bw.wgr(yd, P, IT, BI, 2, seed=5))
            if name == "i8":
                _flat(out, "wgr iv", bw.wgr(yd, P, IT, BI, 2, iv=True, seed=5))
                _flat(out, "wgr de", bw.wgr(yd, P, IT, BI, 2, de=True, seed=5))
                _flat(out, "wgr pi=0.5", bw.wgr(yd, P, IT, BI, 2, pi=0.5, seed=5))
                _flat(out, "wgr bag=0.8", bw.wgr(yd, P, IT, BI, 2, bag=0.8, rp=False, seed=5))
                _flat(out, "wgr bag=0.8 rp", bw.wgr(yd, P, IT, BI, 2, bag=0.8, rp=True, seed=5))
                U = np.linalg.qr(g.standard_normal((n, 5)))[0]
                _flat(out, "wgr eigK", bw.wgr(yd, P, IT, BI, 2, eigK={"values": np.ones(5), "vectors": U}, VarK=0.9, seed=5))   # rank 5
                for fit in ("emRR", "emBA", "emBB", "emBC", "emBCpi", "emDE", "emBL", "emEN", "lasso", "emML"):
                    _flat(out, fit, getattr(bw, fit)(y, P, maxit=5))
                _flat(out, "emML D", bw.emML(y, P, D=g.uniform(0.5, 2.0, p).astype(np.float32), maxit=5))
        finally:
            P.close()
        return out
    return run


def _two_panels():
    bw = _bw()
    X, y = data("i8")
    out = {}
    for fit in ("BayesA2", "BayesB2", "BayesRR2"):                 # two panels of 600 and 400 markers on the same rows
        _flat(out, fit, getattr(bw, fit)(y, X[:, :600], X[:, 600:], IT, BI, seed=7, **I8_KW))
    return out


def _group():
    from bwgr_amd.api import Group
    _bw()
    X, y = data("i8")
    G = Group("BayesB", y, X, devices=(0,), it=IT, bi=BI, seed=9, block=64)
    try:
        G.run(IT)
        return dict(G.result())
    finally:
        G.close()


def _centred():
    P = _panel("i8")
    try:
        P.set_centred(True)
        return _run_chain(P, "i8", "BayesC", seed=13)
    finally:
        P.close()


# ---- a sweep's planning and launching, path by path ----
def _pair(name):
    """Two BayesB chains, on the root and on a clone, advanced by run_pair; then the same two chains each run alone (k_sweep3 for every sweep,
    as in a pair): `pair 0` and `alone 0`, `pair 1` and `alone 1` carry equal digests in the table itself."""
    def run():
        out = {}
        with switches(BWGR_ENG3_THR="1"):
            P = _panel(name)
        try:
            Q = P.clone()
            c0, c1 = _chain(P, name, seed=21), _chain(Q, name, seed=22)
            try:
                c0.run_pair(c1, IT)
                _flat(out, "pair 0", c0.result()); _flat(out, "pair 1", c1.result())
            finally:
                c0.close(); c1.close()
            _flat(out, "alone 0", _run_chain(P, name, seed=21)); _flat(out, "alone 1", _run_chain(Q, name, seed=22))
        finally:
            P.close()
        return out
    return run


def _clone(name):
    """a chain on a root with a live clone, so not alone on the GPU: the 256-row (register) streamers where the slab allows, no prefetch workgroup"""
    def run():
        with switches(BWGR_ENG3_THR="1"):
            P = _panel(name)
        try:
            Q = P.clone()
            out = _run_chain(P, name, seed=23)
            Q.close()
            return out
        finally:
            P.close()
    return run


def _ranges(name):
    """a chain swept in two ranges an iteration through round_sweep / round_apply, the delta passed through unchanged, then end_iteration"""
    def run():
        import torch
        with switches(BWGR_ENG3_THR="1"):
            P = _panel(name)
        try:
            ch = _chain(P, name, seed=24)
            try:
                delta = torch.empty(P.ld, dtype=torch.float64, device="cuda:%d" % P.device)
                half = ch.nblocks // 2
                for _ in range(IT):
                    for lo, hi in ((0, half), (half, ch.nblocks)):
                        ch.round_sweep(lo, hi, delta)
                        ch.round_apply(delta)
                    ch.end_iteration(None)
                return ch.result()
            finally:
                ch.close()
        finally:
            P.close()
    return run


def _fixed_shape():
    """the 512 x 2048 panel in the default geometry: k_sweep3f (2) for a chain alone, k_sweep3 (1) while a clone is alive"""
    out = {}
    with switches(BWGR_ENG3_THR="1"):
        P = _panel("fixed")
    try:
        assert _which(P) == 2, _which(P)
        _flat(out, "alone", _run_chain(P, "fixed", seed=25))
        Q = P.clone()
        assert _which(P) == 1 and _which(Q) == 1, (_which(P), _which(Q))
        _flat(out, "beside a clone", _run_chain(P, "fixed", seed=25))
        Q.close()
        assert _which(P) == 2, _which(P)
    finally:
        P.close()
    return out


def _redo(name):
    """BayesCpi with fourteen bits less headroom on the fixed-point grid: every sweep leaves its range and is redone on the fp64 engine"""
    def run():
        with switches(BWGR_ENG3_THR="1", BWGR_DEBUG_SH_ADD="14"):
            P = _panel(name)
        try:
            ch = _chain(P, name, "BayesCpi", seed=26)
            try:
                ch.run(IT)
                assert ch.redo_count() > 0
                out = dict(ch.result())
                out["redo_count"] = np.int64(ch.redo_count())
                return out
            finally:
                ch.close()
        finally:
            P.close()
    return run


def _switch(**sw):
    """a selection chain and an affine one under an engine switch"""
    def run():
        out = {}
        with switches(**sw):
            P = _panel("i8")
        try:
            _flat(out, "BayesB", _run_chain(P, "i8", "BayesB", seed=27))
            _flat(out, "BayesA", _run_chain(P, "i8", "BayesA", seed=28))
        finally:
            P.close()
        return out
    return run


CASES = {"samplers i8": _samplers("i8"), "samplers f32": _samplers("f32"), "two panels": _two_panels, "group BayesB": _group, "BayesC centred": _centred}
for _name in ("i8", "fixed"):
    CASES["pair " + _name] = _pair(_name)
    CASES["clone " + _name] = _clone(_name)
    CASES["ranges " + _name] = _ranges(_name)
    CASES["redo " + _name] = _redo(_name)
CASES["fixed shape"] = _fixed_shape
for _sw in (dict(BWGR_SWEEP="1"), dict(BWGR_SWEEP="2"), dict(BWGR_STREAM3="reg", BWGR_ENG3_THR="1"), dict(BWGR_WINV="0"), dict(BWGR_ENG3_THR="1")):
    CASES["switch " + " ".join("%s=%s" % kv for kv in _sw.items())] = _switch(**_sw)


def digest(v):
    a = np.ascontiguousarray(np.asarray(v, np.float64) if np.isscalar(v) or isinstance(v, (list, tuple, bool)) else v)
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def digests(name):
    """[(entry, sha256)] of one case: one per output array."""
    with switches():
        return [("%s / %s" % (name, key), digest(v)) for key, v in CASES[name]().items()]


def read_table(path):
    """{entry: sha256} of a table written by tools/family_digest.py (lines `sha256  case / call / output`; `#` starts a comment)."""
    out = {}
    with open(path) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                h, entry = line.rstrip("\n").split("  ", 1)
                out[entry] = h
    return out
