"""One SHA-256 per output array of the float samplers, for a fixed table of calls: KMUP / KMUP2, the fused chains, the two-panel models, wgr,
the EM family, a group on one device and a selection chain on implicitly centred columns.  These families draw from a counter-based generator
and reduce in a fixed order, so equal inputs give equal bits: two builds of the library that print the same table compute the same thing.

    python tools/family_digest.py                              # the library of this tree
    BWGR_LIB=/path/to/libbwgr_hip.so python tools/family_digest.py --out table.txt

The data come from a seeded numpy generator; nothing outside the repository is read.  The shapes are the smallest at which these paths leave
the trivial case: an int8 panel of 300 x 1000 with three slabs and 64-marker blocks (the lag-3 / lag-4 pipelines, the byte planes and k_sweep3
are reachable), and an fp32 panel of 200 x 300 in the default geometry (the fp32 instantiations)."""
import argparse
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IT, BI = 30, 10
I8_KW = dict(nwg=3, block=64)


def digest(v):
    a = np.ascontiguousarray(np.asarray(v, np.float64) if np.isscalar(v) or isinstance(v, (list, tuple, bool)) else v)
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def data():
    g = np.random.default_rng(20260726)
    Xi = g.binomial(2, g.uniform(0.05, 0.5, 1000), size=(300, 1000)).astype(np.int8)
    Xf = g.standard_normal((200, 300)).astype(np.float32)
    out = {}
    for name, X in (("i8", Xi), ("f32", Xf)):
        n, p = X.shape
        beta = np.where(g.uniform(size=p) < 0.05, g.standard_normal(p), 0.0)
        y = X.astype(np.float64) @ beta
        y = y - y.mean() + g.standard_normal(n) * (y.std() + 1e-3)
        out[name] = (X, y.astype(np.float32))
    return out, g


def calls(emit):
    import bwgr_amd as bw
    from bwgr_amd.api import Chain, Group, Panel
    D, g = data()
    for name, (X, y) in D.items():
        kw = I8_KW if name == "i8" else dict(as_int8=False)
        n, p = X.shape
        P = Panel(X, **kw)
        try:
            xx, vx, msx = P.stats()
            b0 = (g.standard_normal(p) * 0.01).astype(np.float32)
            d0 = (g.uniform(size=p) < 0.5).astype(np.float32)
            L = np.full(p, float(msx), np.float32)
            e0 = (y - y.mean()).astype(np.float32)
            use = np.sort(g.integers(0, n, size=n // 2)).astype(np.int32)
            use[1] = use[0]                                       # a repeated row
            for pi in (0.0, 0.7):
                emit("KMUP pi=%g %s" % (pi, name), bw.KMUP(P, b0, d0, xx, e0, L, 1.0, pi, seed=3, it=2))
                emit("KMUP2 pi=%g %s" % (pi, name), bw.KMUP2(P, use, b0, d0, xx, e0, L, 1.0, pi, seed=3, it=2))
            for model in ("BayesA", "BayesB", "BayesC", "BayesL", "BayesRR", "BayesCpi", "BayesDpi"):
                ch = Chain(P, model, y, IT, BI, 0.95 if model in ("BayesB", "BayesC") else 0.0, 5.0, 0.5, 11, 0)
                try:
                    ch.run(IT)
                    emit("%s %s" % (model, name), ch.result())
                finally:
                    ch.close()
            yd = y.astype(np.float64)
            emit("wgr %s" % name, bw.wgr(yd, P, IT, BI, 2, seed=5))
            if name == "i8":
                emit("wgr iv", bw.wgr(yd, P, IT, BI, 2, iv=True, seed=5))
                emit("wgr de", bw.wgr(yd, P, IT, BI, 2, de=True, seed=5))
                emit("wgr pi=0.5", bw.wgr(yd, P, IT, BI, 2, pi=0.5, seed=5))
                emit("wgr bag=0.8", bw.wgr(yd, P, IT, BI, 2, bag=0.8, rp=False, seed=5))
                emit("wgr bag=0.8 rp", bw.wgr(yd, P, IT, BI, 2, bag=0.8, rp=True, seed=5))
                U = np.linalg.qr(g.standard_normal((n, 5)))[0]
                emit("wgr eigK", bw.wgr(yd, P, IT, BI, 2, eigK={"values": np.ones(5), "vectors": U}, VarK=0.9, seed=5))   # rank 5
                for fit in ("emRR", "emBA", "emBB", "emBC", "emBCpi", "emDE", "emBL", "emEN", "lasso", "emML"):
                    emit(fit, getattr(bw, fit)(y, P, maxit=5))
                emit("emML D", bw.emML(y, P, D=g.uniform(0.5, 2.0, p).astype(np.float32), maxit=5))
        finally:
            P.close()
    X, y = D["i8"]
    for fit in ("BayesA2", "BayesB2", "BayesRR2"):                 # two panels of 600 and 400 markers on the same rows
        emit(fit, getattr(bw, fit)(y, X[:, :600], X[:, 600:], IT, BI, seed=7, **I8_KW))
    G = Group("BayesB", y, X, devices=(0,), it=IT, bi=BI, seed=9, block=64)
    try:
        G.run(IT)
        emit("Group BayesB", G.result())
    finally:
        G.close()
    P = Panel(X, **I8_KW)
    try:
        P.set_centred(True)
        ch = Chain(P, "BayesC", y, IT, BI, 0.95, 5.0, 0.5, 13, 0)
        try:
            ch.run(IT)
            emit("BayesC centred", ch.result())
        finally:
            ch.close()
    finally:
        P.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="also write the table to this file")
    a = ap.parse_args()
    lines = []

    def emit(call, result):
        for key, v in result.items():
            lines.append("%s  %s / %s" % (digest(v), call, key))
            print(lines[-1], flush=True)

    calls(emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
