"""Line-cited numpy float64 restatement of PEGS and PEGSZ (bWGR src/RcppEigenX20251203.cpp:10-194, :576-808) for the tests.

Written from the contract in include/bwgr.h and DESIGN.md section 4.10.  Y and the real options are rounded to float once, as the reference
receives them; everything after that is float64, and the reference's float constants (1e-12f) are taken as doubles.  The marker orders come
from bwgr_amd.em_order (host-only, no GPU): in sweep s an effect of m columns is walked in em_order(m, s); `orders=` overrides them
(orders[s][e] is effect e's order in sweep s).  The designs are NOT centred.

pegsz(Y, X_list, ...) returns the reference's list as a dict (mu, b, hat, h2, GC, bend, numit, cnv; b and GC lists, bend a vector) plus
"cnv_trace" (cnv after every sweep) and, with trace=True, "trace": per sweep a list with one dict per effect -- MinDVb, maxEv (vb's smallest
and largest eigenvalue before bending), inflated, gap (0 < XFA < k: last kept minus first dropped eigenvalue of GC, else None), and the
arrays the CPU test of the tail feeds to the library's own tail (TH, vb, iG, inflate) with the sweep's ey, db2, d, ve, cnv.
pegs(Y, X, ...) is PEGS's own text (own_text=True) on one design, with b, GC and bend unwrapped.

dtype=np.longdouble runs the same recurrence with every array, accumulator, scalar option and k x k routine in long double (the yardstick
of tests/mt_tight.py): Y and the options are rounded to float as before and then widened, the k x k routines are those of
tests/ld_linalg.py, and an effect's systems of a sweep are inverted in one batched call.  dot(x_J, e) stands in for the step's dependent
dot x_J'e, or dot[f] does for effect f alone where dot is a list (None: that effect's dot as it is) -- the mutants of
tests/test_mt_tight_cpu.py.  The trace also holds near0: min |vb| / max |vb| before NNC's clamp, over the entries that
are not exactly zero (None without NNC).  mu_div_n=True is PEGSZ_sparse's text (:1010-1250), which differs in two divisors: iN is
1 / (max(n_t, 1) - 1) (:1076) and the intercept step divides the residual sums by n_t (:1202); tests/pegs_sparse_restatement.py calls it.
"""
import numpy as np

import ld_linalg


def _orders(m, s):
    import bwgr_amd
    return bwgr_amd.em_order(m, s)


def _f32(v):
    return float(np.float32(v))


def _gc(vb):
    sd = np.sqrt(np.diag(vb))
    sd = np.where(sd < 1e-12, 1e-12, sd)
    return vb / np.outer(sd, sd), sd


def tail_vb(TH, Tr, k, XFA, NNC, covbend, covMinEv, inflate, own_text, dtype=np.float64):
    """one effect's covariance after a sweep (:127-160, :717-756) -> vb, iG, inflate, record"""
    wide = np.dtype(dtype) == np.dtype(np.longdouble)
    la, num = (ld_linalg, dtype) if wide else (np.linalg, float)
    vb = np.zeros((k, k), dtype)
    for i in range(k):
        for j in range(k):
            if i == j:
                vb[i, i] = TH[i, i] / Tr[i] if (own_text or Tr[i] != 0) else 0.0
            else:
                vb[i, j] = (TH[i, j] + TH[j, i]) / (Tr[i] + Tr[j]) if (own_text or Tr[i] + Tr[j] != 0) else 0.0
    gap = None
    if XFA == 0:                                                     # :134-138
        vb = np.diag(np.diag(vb))
    elif own_text or XFA < k:                                        # :139-153 (PEGS: XFA > 0), :734-747 (PEGSZ: 0 < XFA < k)
        GC, sd = _gc(vb)
        w, V = la.eigh(GC)
        if XFA < k:
            gap = num(w[k - XFA] - w[k - XFA - 1])
        GC = (V[:, k - XFA:] * w[k - XFA:]) @ V[:, k - XFA:].T
        np.fill_diagonal(GC, 1.0)
        vb = GC * np.outer(sd, sd)
    near0 = None
    if NNC:                                                          # :156
        near0 = num(np.abs(vb[vb != 0]).min(initial=np.inf) / max(np.abs(vb).max(), 1e-300))   # (an exact zero is no decision: XFA = 0)
        vb = np.maximum(vb, 0.0)
    ev = la.eigvalsh(vb)
    MinDVb = num(ev[0])                                              # :157
    if MinDVb < covMinEv:                                            # :158: a running maximum
        inflate = max(inflate, abs(MinDVb * covbend))
    inflated = bool(k >= 5 or MinDVb < covMinEv)                     # :159
    if inflated:
        vb = vb + inflate * np.eye(k, dtype=dtype)
    iG = la.pinv(vb)                                                 # :160
    return vb, iG, inflate, dict(MinDVb=MinDVb, maxEv=num(ev[-1]), inflated=inflated, gap=gap, near0=near0)


def pegsz(Y, X_list, maxit=100, logtol=-4.0, covbend=1.1, covMinEv=10e-4, XFA=-1, NNC=True, own_text=False, orders=None, trace=False,
          dtype=np.float64, dot=None, mu_div_n=False):
    wide = np.dtype(dtype) == np.dtype(np.longdouble)
    la, num = (ld_linalg, dtype) if wide else (np.linalg, float)
    Y = np.array(Y, np.float64, copy=True)
    if Y.ndim == 1:
        Y = Y[:, None]
    Y = Y.astype(np.float32).astype(dtype)
    logtol, covbend, covMinEv = _f32(logtol), _f32(covbend), _f32(covMinEv)
    if wide:
        logtol, covbend, covMinEv = dtype(logtol), dtype(covbend), dtype(covMinEv)
    Xs = [np.asarray(X, dtype).reshape(Y.shape[0], -1) for X in X_list]
    dots = list(dot) if isinstance(dot, (list, tuple)) else [dot] * len(Xs)
    n0, k = Y.shape
    ne = len(Xs)
    Z = (~np.isnan(Y)).astype(dtype)                            # :23-29
    Y[np.isnan(Y)] = 0
    n = Z.sum(0)                                                     # :32
    mu = Y.sum(0) / n                                                # :36-37
    y = (Y - mu) * Z                                                 # :40
    XX, Tr, MSx, tilde = [], [], [], []
    for X in Xs:
        xx = (X ** 2).T @ Z                                          # :43-45
        xsx = xx / n - ((X.T @ Z) / n) ** 2                          # :48-51
        XX.append(xx); MSx.append(xsx.sum(0)); Tr.append(n * xsx.sum(0))   # :52-53
        tilde.append(X.T @ y)                                        # :66
    iN = 1 / (np.maximum(n, 1.0) - 1) if mu_div_n else 1 / (n - 1)  # :56; PEGSZ_sparse's :1076
    vy = (y ** 2).sum(0) * iN                                        # :57
    ve = vy * 0.5                                                    # :58
    vb = [np.diag(ve / m) for m in MSx]                              # :61
    iG = [np.diag(m / ve) for m in MSx]                              # :62
    b = [np.zeros((X.shape[1], k), dtype) for X in Xs]
    e = y.copy()                                                     # :73
    inflate = [num(0.0)] * ne
    if XFA < 0:                                                      # :94
        XFA = k
    assert XFA <= k
    cnv, numit, cnvs, trc = num(10.0), 0, [], []
    while numit < maxit:
        beta0 = [a.copy() for a in b]
        iVe = 1 / ve
        for f, X in enumerate(Xs):                                   # :689-708
            order = _orders(X.shape[1], numit) if orders is None else orders[numit][f]
            Linv = la.inv(iG[f] + (XX[f] * iVe)[:, :, None] * np.eye(k, dtype=dtype)) if wide else None   # every column's LHS^-1 at once
            for J in order:
                b0 = b[f][J].copy()
                LHS = iG[f] + np.diag(XX[f][J] * iVe)                # :113
                RHS = ((X[:, J] @ e if dots[f] is None else dots[f](X[:, J], e)) + XX[f][J] * b0) * iVe   # :114-115
                b1 = Linv[J] @ RHS if wide else np.linalg.solve(LHS, RHS)   # :116
                b[f][J] = b1
                e = e - np.outer(X[:, J], b1 - b0) * Z               # :119
        ey = (e * y).sum(0)
        ve = ey * iN                                                 # :123-124
        recs = []
        for f in range(ne):
            TH = b[f].T @ tilde[f]                                   # :128
            vb[f], iG[f], inflate[f], rec = tail_vb(TH, Tr[f], k, XFA, NNC, covbend, covMinEv, inflate[f], own_text, dtype)
            rec.update(TH=TH, vb=vb[f].copy(), iG=iG[f].copy(), inflate=inflate[f])
            recs.append(rec)
        se = e.sum(0)
        d = se / n if mu_div_n else se * iN                          # :163-164: 1 / (n - 1), as written; PEGSZ_sparse's :1200-1202: 1 / n_t
        mu = mu + d
        e = (e - d) * Z                                              # :165-166
        db2 = [num(((beta0[f] - b[f]) ** 2).sum()) for f in range(ne)]
        with np.errstate(divide="ignore"):
            cnv = num(np.log10(sum(db2)))                          # :169, :766-770
        numit += 1
        cnvs.append(cnv)
        if trace:
            recs[0].update(ey=ey.copy(), se=se.copy(), db2=db2, d=d.copy(), ve=ve.copy(), cnv=cnv, mu=mu.copy())
            trc.append(recs)
        if cnv < logtol:                                             # :171
            break
    h2 = 1 - ve / vy                                                 # :175
    hat = np.zeros((n0, k), dtype)
    for f, X in enumerate(Xs):                                       # :777-781
        hat = hat + X @ b[f]
    hat = hat + mu
    out = {"mu": mu, "b": b, "hat": hat, "h2": h2, "GC": [_gc(v)[0] for v in vb], "bend": np.array(inflate), "numit": numit, "cnv": cnv,
           "cnv_trace": np.array(cnvs)}
    if trace:
        out["trace"] = trc
        out["start"] = dict(nt=n, vy=vy, mu0=Y.sum(0) / n, MSx=np.array(MSx))
    return out


def pegs(Y, X, **kw):
    r = pegsz(Y, [X], own_text=True, **kw)
    r["b"], r["GC"], r["bend"] = r["b"][0], r["GC"][0], float(r["bend"][0])
    return r


def scaled_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.max(np.abs(b)) if b.size else 0.0
    return float(np.max(np.abs(a - b)) / (den if den > 0 else 1.0)) if b.size else 0.0
