"""The calls whose output bits tests/golden/uvb_parent_digests.txt records (tools/uvb_digest.py writes the table, tests/
test_gpu_uvb_parent_bits.py compares against it): the per-trait fits bwgr_uvbeta / bwgr_uvbeta2 / bwgr_uvbeta_dense, bwgr_panel_xb and the
relationship kernels.  These families reduce in a fixed order and have no atomics outside the integer products, so equal inputs give equal
bits.  Everything comes from seeded numpy generators and tests/golden/tpod.npz; each case is the smallest shape that reaches its path.

CASES maps a name to a function that runs the call and returns a dict of arrays."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sem2_cases as C  # noqa: E402
from test_gpu_mrr import _traits  # noqa: E402
from test_gpu_uvb import _stopping_case  # noqa: E402


def _bw():
    import bwgr_amd
    return bwgr_amd


def _tpod_k3(variant, **kw):
    return lambda: _bw().uvbeta(_traits(C.tpod(), 3, 0.1, seed=11), C.tpod(), variant, maxit=6, tol=0, **kw)


def _p65_two_groups():
    """65 markers: the last block holds one.  k = W + 1: traits 4 and 5 share their rows, trait 9 has none, group 1 holds trait W alone."""
    bw = _bw()
    W = bw.uvb_plan(196, 65, 1)["W"]
    X = np.asfortranarray(C.tpod()[:, :65])
    Y = _traits(C.tpod(), W + 1, 0.0, seed=211)
    miss = np.random.default_rng(212).random(Y.shape) < 0.1
    miss[:, 5] = miss[:, 4]
    Y[miss] = np.nan
    Y[:, 9] = np.nan
    return bw.uvbeta(Y, X, "D", maxit=4, tol=0)


def _stopping(variant):
    def run():
        Y, _ = _stopping_case(variant)
        g = _bw().uvbeta(Y, C.tpod(), variant, maxit=100, tol=10e-7)
        assert len(set(g["its"])) > 1 and g["its"].max() < 100, g["its"]      # traits drop out at different sweeps, none at maxit
        return g
    return run


def _clone_centred_root():
    """The three-slab panel through a clone (its own stream) while the root sweeps implicitly centred columns: these fits read the raw ones."""
    bw = _bw()
    X = C.slabs900()
    Y = _traits(X, 5, 0, seed=5, patterns=[0.1, 0.0, 0.25, 0.05, 0.4])
    P = bw.Panel(X, nwg=3)
    try:
        P.set_centred(True)
        Q = P.clone()
        try:
            return bw.uvbeta(Y, Q, "D", maxit=4, tol=0)
        finally:
            Q.close()
            P.set_centred(False)
    finally:
        P.close()


def _uvbeta2(c):
    kw = {"nwg": c["nwg"]} if "nwg" in c else {}
    return _bw().uvbeta2(c["Y"], c["Z"], c["X"], **c["kw"], **kw)


def _residual(side):
    def run():
        L = _bw().uvbd_plan(1000, 2, 2)["lds_rows"]
        return _uvbeta2(C.residual_path(L - 27 if side == "below" else L + 37))
    return run


def _dense():
    Y = _traits(C.tpod(), 3, 0.1, seed=221)[:63]
    return _bw().uvbeta_dense(Y, C.dense(63, 2, 222), "D", maxit=6, tol=0)


def _panel_xb():
    X = C.slabs900()
    B = np.random.default_rng(231).normal(size=(900, 17))
    return {"xb": _bw().panel_xb(X, B, nwg=3)}


def _tpod_split():
    X = np.ascontiguousarray(C.tpod()).astype(np.int8)
    return np.ascontiguousarray(X[:130]), np.ascontiguousarray(X[130:])


def _kernel(kind, par=1.0):
    def run():
        P = _bw().Panel(_tpod_split()[0])
        try:
            return {"K": P.kernel(kind, par)}
        finally:
            P.close()
    return run


def _kernel2_arc():
    bw = _bw()
    F, S = _tpod_split()
    Pf, Ps = bw.Panel(F), bw.Panel(S)
    try:
        Kff, Kfs = Pf.kernel2(Ps, "ARC")
        return {"Kff": Kff, "Kfs": Kfs}
    finally:
        Pf.close(); Ps.close()


CASES = {"uvbeta %s tpod k3" % v: _tpod_k3(v) for v in "DFXZ"}
CASES["uvbeta D tpod k3 xb"] = _tpod_k3("D", xb=True)
CASES["uvbeta D p65 k=W+1"] = _p65_two_groups
CASES["uvbeta D stopping"] = _stopping("D")
CASES["uvbeta Z stopping"] = _stopping("Z")
CASES["uvbeta D maxit0"] = lambda: _bw().uvbeta(_traits(C.tpod(), 3, 0.1, seed=11), C.tpod(), "D", maxit=0, xb=True)
CASES["uvbeta D slabs900 clone"] = _clone_centred_root
for _name in C.ENGINE:
    CASES["uvbeta2 " + _name] = (lambda name: lambda: _uvbeta2(C.engine(name)))(_name)
CASES["uvbeta2 residual below"] = _residual("below")
CASES["uvbeta2 residual above"] = _residual("above")
CASES["uvbeta_dense D n63 q2 k3"] = _dense
CASES["panel_xb k17 slabs900"] = _panel_xb
CASES["panel_kernel GRM"] = _kernel("GRM")
CASES["panel_kernel EigenGAU"] = _kernel("EigenGAU", 0.5)
CASES["panel_kernel2 ARC"] = _kernel2_arc


def digest(v):
    import hashlib
    a = np.ascontiguousarray(v)
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def digests(name):
    """[(entry, sha256)] of one case: one per output array."""
    return [("%s / %s" % (name, key), digest(v)) for key, v in CASES[name]().items()]


def read_table(path):
    """{entry: sha256} of a table written by tools/uvb_digest.py (lines `sha256  case / key`; `#` starts a comment)."""
    out = {}
    with open(path) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                h, entry = line.rstrip("\n").split("  ", 1)
                out[entry] = h
    return out
