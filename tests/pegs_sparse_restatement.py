"""What tests/pegs_restatement.py and tests/pegsx_restatement.py lack for the sparse effects (bWGR src/RcppEigenX20251203.cpp:811-1007,
:1010-1250): a column-compressed builder in numpy, so that the tests need no scipy, and PEGSZ_sparse's text.

The sparse functions are PEGS / PEGSZ with the designs held column-compressed: every sum runs over the stored entries and gives the numbers
of the dense copy, so PEGS_sparse is restated by pegs_restatement.pegs and a sparse effect in a PEGSZ / PEGSX list by pegsz / pegsx, each on
the dense copy (values rounded to float, as the reference casts S).  The one line of text that differs is PEGSZ_sparse's intercept step,
which divides the residual sums by n_t (iN_mu, :1202) where PEGSZ divides by n_t - 1 (:760): pegsz_sparse below is pegsz with that divisor
(its "trace" holds tail_vb's record per sweep and effect: MinDVb, maxEv, inflated, gap).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pegs_restatement as PR  # noqa: E402


def csc(A, stored=None):
    """(data, indices int32, indptr int64) of the 2-D array A, rows ascending within a column: its nonzeros, or the entries where the mask
    `stored` is set (a stored zero is an entry)"""
    A = np.asarray(A, np.float64)
    cols, rows = np.nonzero(A.T if stored is None else np.asarray(stored).T)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=A.shape[1]))]).astype(np.int64)
    return A[rows, cols].copy(), rows.astype(np.int32), indptr


def f32(A):
    return np.asarray(A, np.float64).astype(np.float32).astype(np.float64)


def row_disjoint(A):
    return bool(np.all((np.asarray(A) != 0).sum(1) <= 1))


def pegsz_sparse(Y, X_list, maxit=100, logtol=-4.0, covbend=1.1, covMinEv=10e-4, XFA=-1, NNC=True, orders=None):
    """PEGSZ_sparse (:1010-1250) on the dense copies X_list: pegs_restatement.pegsz's sweeps and tail with the intercept step of :1199-1206"""
    Y = np.array(Y, np.float64, copy=True)
    if Y.ndim == 1:
        Y = Y[:, None]
    Y = Y.astype(np.float32).astype(np.float64)
    logtol, covbend, covMinEv = PR._f32(logtol), PR._f32(covbend), PR._f32(covMinEv)
    Xs = [f32(np.asarray(X, np.float64).reshape(Y.shape[0], -1)) for X in X_list]   # :1028
    n0, k = Y.shape
    ne = len(Xs)
    Z = (~np.isnan(Y)).astype(np.float64)                            # :1033-1039
    Y[np.isnan(Y)] = 0
    n = Z.sum(0)                                                     # :1042
    mu = Y.sum(0) / n                                                # :1046-1047
    y = (Y - mu) * Z                                                 # :1050
    XX, Tr, MSx, tilde = [], [], [], []
    for X in Xs:
        xx = (X ** 2).T @ Z                                          # :1060-1063
        xsx = xx / n - ((X.T @ Z) / n) ** 2                          # :1067-1070
        XX.append(xx); MSx.append(xsx.sum(0)); Tr.append(n * xsx.sum(0))   # :1071-1072
        tilde.append(X.T @ y)                                        # :1091
    iN = 1 / (np.maximum(n, 1.0) - 1)                                # :1076
    vy = (y ** 2).sum(0) * iN                                        # :1077
    ve = vy * 0.5                                                    # :1078
    vb = [np.diag(ve / m) for m in MSx]                              # :1084
    iG = [np.diag(m / ve) for m in MSx]                              # :1085
    b = [np.zeros((X.shape[1], k)) for X in Xs]
    e = y.copy()                                                     # :1102
    inflate = [0.0] * ne
    if XFA < 0:                                                      # :1116
        XFA = k
    assert XFA <= k
    cnv, numit, cnvs, trc = 10.0, 0, [], []
    while numit < maxit:
        beta0 = [a.copy() for a in b]
        iVe = 1 / ve
        for f, X in enumerate(Xs):                                   # :1126-1150
            order = PR._orders(X.shape[1], numit) if orders is None else orders[numit][f]
            for J in order:
                b0 = b[f][J].copy()
                LHS = iG[f] + np.diag(XX[f][J] * iVe)                # :1136-1137
                RHS = (X[:, J] @ e + XX[f][J] * b0) * iVe            # :1138-1139
                b1 = np.linalg.solve(LHS, RHS)                       # :1140
                b[f][J] = b1
                e = e - np.outer(X[:, J], b1 - b0) * Z               # :1144-1148
        ve = (e * y).sum(0) * iN                                     # :1153-1154
        recs = []
        for f in range(ne):                                          # :1158-1197, PEGSZ's text (own_text = False)
            vb[f], iG[f], inflate[f], rec = PR.tail_vb(b[f].T @ tilde[f], Tr[f], k, XFA, NNC, covbend, covMinEv, inflate[f], False)
            recs.append(rec)
        trc.append(recs)
        d = e.sum(0) / n                                             # :1200-1202: iN_mu, 1 / n_t
        mu = mu + d
        e = (e - d) * Z                                              # :1203-1206
        with np.errstate(divide="ignore"):
            cnv = float(np.log10(sum(float(((beta0[f] - b[f]) ** 2).sum()) for f in range(ne))))   # :1209-1213
        numit += 1
        cnvs.append(cnv)
        if cnv < logtol:                                             # :1216
            break
    h2 = 1 - ve / vy                                                 # :1227
    hat = np.zeros((n0, k))
    for f, X in enumerate(Xs):                                       # :1220-1224
        hat = hat + X @ b[f]
    hat = hat + mu
    return {"mu": mu, "b": b, "hat": hat, "h2": h2, "GC": [PR._gc(v)[0] for v in vb], "bend": np.array(inflate), "numit": numit, "cnv": cnv,
            "cnv_trace": np.array(cnvs), "trace": trc}
