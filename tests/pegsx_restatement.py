"""Line-cited numpy float64 restatement of PEGSX (bWGR src/RcppEigenX20251203.cpp:197-573) for the tests.

Written from the contract in include/bwgr.h and DESIGN.md section 4.11.  Y, X, dense Z and the real options are rounded to float once, as the
reference receives them; everything after that is float64, and the reference's float floors (1e-8f, 1e-12f) are taken as doubles.  The marker
orders come from bwgr_amd.em_order (host-only, no GPU): in sweep s an effect of m columns is walked in em_order(m, s); `orders=` overrides them
(orders[s][r] is effect r's order in sweep s).  Nothing is centred and there is no intercept: an intercept is a column of X.

Both pseudo-inverses of M'M (:250, :304-311) are one symmetric pseudo-inverse that drops eigenvalues with |lambda| <= f 2^-23 max |lambda|
(sym_pinv), the reference's float rank decision.

pegsx(Y, X, Z_list, ...) returns the reference's list as a dict (TrZSZ, b, u, vb_list, GC_list, ve, hat, its, cnv, bend) plus "cnv_trace"
(cnv after every sweep), "mm" (per trait the kept and dropped eigenvalue ratios of M'M), "floors0" (the floors active in the start values) and,
with trace=True, "start" and "trace": per sweep a list with one dict per effect -- MinDVb, maxEv, inflated, gap (where XFA truncates: last kept
minus first dropped eigenvalue of GC, else None), near0 (min |vb| / max |vb| before NNC's clamp, over the entries that are not exactly zero;
None without NNC), floors (names of the floors active in that update) and the arrays the CPU test of the tail feeds to the library's own tail
(TH, vb, iG, inflate) with the sweep's ey, db2, ve, cnv.

dtype=np.longdouble runs the same recurrence with every array, accumulator and scalar option in long double (the yardstick of
tests/mt_tight.py): Y, X, dense Z and the options are rounded to float as before and then widened, the floors are the same doubles widened, the
k x k tail and sym_pinv (with its f 2^-23 rank rule) go through tests/ld_linalg.py, an effect's systems of a sweep are inverted in one batched
call, and traits that share a missingness pattern share one Jacobi of M'M.  The mutant hooks of tests/test_mt_tight_cpu.py: dot(z_J, e) stands
in for the sweep's dependent dot z_J'e, or dot[r] does for effect r alone where dot is a list (None: that effect's dot as it is);
fixed_dot(M_t, e_t) stands in for M_t'e_t in the fixed step (:503-509); trace_dot(M_g, Zw) stands in for M_g'z_j, all columns j at once, in
the trace (:292-323).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ld_linalg  # noqa: E402
from pegs_restatement import _f32, _gc, _orders, scaled_err  # noqa: E402, F401


def _wide(dtype):
    return np.dtype(dtype) == np.dtype(np.longdouble)


def sym_pinv(A, dtype=np.float64):
    """-> pinv, ratios |lambda| / max |lambda| (ascending lambda), kept mask"""
    f = A.shape[0]
    w, V = (ld_linalg if _wide(dtype) else np.linalg).eigh(A)
    mx = np.max(np.abs(w))
    keep = np.abs(w) > f * 2.0 ** -23 * mx
    P = (V[:, keep] / w[keep]) @ V[:, keep].T
    return P, (np.abs(w) / mx if mx > 0 else np.zeros(f, dtype)), keep


def tail_vb(TH, Tr, Sb, k, df0, NNC, XFA, NumXFA, covbend, covMinEv, inflate, dtype=np.float64):
    """one effect's covariance after a sweep (:437-498) -> vb, iG, inflate, record"""
    la, num = (ld_linalg, dtype) if _wide(dtype) else (np.linalg, float)
    F8, F12 = num(1e-8), num(1e-12)
    floors = set()
    vb = np.zeros((k, k), dtype)
    for i in range(k):
        if Tr[i] < F8:
            floors.add("tr")
        vb[i, i] = (TH[i, i] + Sb[i]) / (max(Tr[i], F8) + df0)               # :440-443
        for j in range(i + 1, k):
            if Tr[i] + Tr[j] < F8:
                floors.add("tr")
            vb[i, j] = vb[j, i] = (TH[i, j] + TH[j, i]) / max(Tr[i] + Tr[j], F8)     # :444-451
    near0 = None
    if NNC:                                                                  # :453-457
        near0 = num(np.abs(vb[vb != 0]).min(initial=np.inf) / max(np.abs(vb).max(), 1e-300))
        vb = np.maximum(vb, 0.0)
    gap = None
    if XFA and NumXFA > 0:                                                   # :459-485
        nf = min(NumXFA, k)
        sd = np.sqrt(np.diag(vb))
        if np.any(sd < F12) or np.any(np.diag(vb) < F12):
            floors.add("sd")
        sd = np.maximum(sd, F12)
        sc = np.sqrt(np.maximum(np.diag(vb), F12))
        GC = vb / np.outer(sd, sd)
        w, V = la.eigh(GC)
        if nf < k:
            gap = num(w[k - nf] - w[k - nf - 1])
        GC = (V[:, k - nf:] * w[k - nf:]) @ V[:, k - nf:].T
        np.fill_diagonal(GC, 1.0)
        vb = GC * np.outer(sc, sc)
    ev = la.eigvalsh(vb)
    MinDVb = num(ev[0])                                                      # :487-488
    if MinDVb < covMinEv:                                                    # :489-492: a running maximum
        inflate = max(inflate, abs(MinDVb * covbend))
    inflated = bool(k >= 5 or MinDVb < covMinEv)                             # :494-496
    if inflated:
        vb = vb + inflate * np.eye(k, dtype=dtype)
    iG = la.pinv(vb)                                                         # :498
    return vb, iG, inflate, dict(MinDVb=MinDVb, maxEv=num(ev[-1]), inflated=inflated, gap=gap, near0=near0, floors=floors)


def pegsx(Y, X, Z_list, maxit=500, logtol=-8.0, covbend=1.1, covMinEv=10e-4, cores=1, verbose=False, df0=1.1, NNC=False, InnerGS=False, NoInv=False,
          XFA=False, NumXFA=3, dense=None, trace=False, dtype=np.float64, orders=None, dot=None, fixed_dot=None, trace_dot=None):
    """dense: per effect whether it is a dense one (rounded to float); default: none is (integer panels are exact)"""
    assert not InnerGS and not NoInv
    wide = _wide(dtype)
    la, num = (ld_linalg, dtype) if wide else (np.linalg, float)
    F8, F20 = num(1e-8), num(1e-20)
    Y = np.array(Y, np.float64, copy=True)
    if Y.ndim == 1:
        Y = Y[:, None]
    Y = Y.astype(np.float32).astype(dtype)
    X = np.asarray(X, np.float64).reshape(Y.shape[0], -1).astype(np.float32).astype(dtype)
    logtol, covbend, covMinEv, df0 = _f32(logtol), _f32(covbend), _f32(covMinEv), _f32(df0)
    if wide:
        logtol, covbend, covMinEv, df0 = dtype(logtol), dtype(covbend), dtype(covMinEv), dtype(df0)
    dense = [False] * len(Z_list) if dense is None else dense
    Zs = [np.asarray(Z, np.float64).reshape(Y.shape[0], -1) for Z in Z_list]
    Zs = [Z.astype(np.float32).astype(dtype) if d else Z.astype(dtype, copy=False) for Z, d in zip(Zs, dense)]
    dots = list(dot) if isinstance(dot, (list, tuple)) else [dot] * len(Zs)
    n0, k = Y.shape
    f, ne = X.shape[1], len(Zs)
    Yin = Y.copy()
    W = (~np.isnan(Y)).astype(dtype)                                         # :228-238
    Y[np.isnan(Y)] = 0
    nt = W.sum(0)                                                            # :239
    b = np.zeros((f, k), dtype)
    iXX, mm, shared = [], [], {}
    for t in range(k):                                                       # :246-253
        M = X * W[:, [t]]
        pat = W[:, t].tobytes()
        if not wide or pat not in shared:
            shared[pat] = sym_pinv(M.T @ M, dtype)
        P, ratios, keep = shared[pat]
        iXX.append(P)
        mm.append(dict(kept=ratios[keep], dropped=ratios[~keep]))
        b[:, t] = P @ (M.T @ Y[:, t])
    y = np.stack([(Y[:, t] - (X * W[:, [t]]) @ b[:, t]) * W[:, t] for t in range(k)], 1)   # :257-260
    b0 = b.copy()
    ZZ = [(Z ** 2).T @ W for Z in Zs]                                        # :277-290
    Tr = []
    for Z in Zs:                                                             # :292-323
        tr = np.zeros(k, dtype)
        for t in range(k):
            M = X * W[:, [t]]
            V = M.T @ (Z * W[:, [t]]) if trace_dot is None else trace_dot(M, Z * W[:, [t]])   # f x q
            tr[t] = ((Z * W[:, [t]]) ** 2).sum() - np.einsum("cj,cd,dj->", V, iXX[t], V)
        Tr.append(tr)
    tilde = [Z.T @ y for Z in Zs]                                            # :325-330
    floors0 = set()
    ssy = (y ** 2).sum(0)                                                    # :336
    if np.any(nt - f < 1) or np.any(nt + df0 - f < 1):
        floors0.add("denom")
    iN = 1 / np.maximum(nt - f, 1.0)                                         # :337-339
    ve = 0.5 * ssy * iN                                                      # :340
    if np.any(ve < F8):
        floors0.add("ve")
    ve = np.maximum(ve, F8)                                                  # :341
    vb, iG, Sb = [], [], []
    for r in range(ne):                                                      # :345-361
        den = Tr[r] * iN
        if np.any(den < F8):
            floors0.add("tr")
        d = ve / np.maximum(den, F8)
        vb.append(np.diag(d)); iG.append(np.diag(1 / d)); Sb.append(df0 * d)
    Se = ve * df0                                                            # :362
    iNp = 1 / np.maximum(nt + df0 - f, 1.0)                                  # :363-364
    start = dict(nt=nt, ssy=ssy, Tr=np.array(Tr), ve=ve.copy(), vb=[v.copy() for v in vb], f=f)
    e = y.copy()                                                             # :367
    u = [np.zeros((Z.shape[1], k), dtype) for Z in Zs]
    inflate = [num(0.0)] * ne
    cnv, numit, cnvs, trc = num(10.0), 0, [], []
    while numit < maxit:
        u0 = [a.copy() for a in u]
        iVe = 1 / ve
        for r, Z in enumerate(Zs):                                           # :381-434
            Linv = la.inv(iG[r] + (ZZ[r] * iVe)[:, :, None] * np.eye(k, dtype=dtype)) if wide else None   # every column's LHS^-1 at once
            for J in (_orders(Z.shape[1], numit) if orders is None else orders[numit][r]):
                a0 = u[r][J].copy()
                LHS = iG[r] + np.diag(ZZ[r][J] * iVe)                        # :409-410
                RHS = ((Z[:, J] @ e if dots[r] is None else dots[r](Z[:, J], e)) + ZZ[r][J] * a0) * iVe   # :411-413
                a1 = Linv[J] @ RHS if wide else np.linalg.solve(LHS, RHS)    # :430
                u[r][J] = a1
                e = e - np.outer(Z[:, J], a1 - a0) * W                       # :433
        recs = []
        for r in range(ne):                                                  # :437-498 (an effect's vb depends on its own u alone)
            TH = u[r].T @ tilde[r]
            vb[r], iG[r], inflate[r], rec = tail_vb(TH, Tr[r], Sb[r], k, df0, NNC, XFA, NumXFA, covbend, covMinEv, inflate[r], dtype)
            rec.update(TH=TH, vb=vb[r].copy(), iG=iG[r].copy(), inflate=inflate[r])
            recs.append(rec)
        for t in range(k):                                                   # :503-509
            M = X * W[:, [t]]
            d = iXX[t] @ (M.T @ e[:, t] if fixed_dot is None else fixed_dot(M, e[:, t]))
            b[:, t] += d
            e[:, t] = (e[:, t] - M @ d) * W[:, t]
        ey = (e * y).sum(0)                                                  # :512
        ve = (ey + Se) * iNp                                                 # :513
        if np.any(ve < F8):
            recs[0]["floors"].add("ve")
        ve = np.maximum(ve, F8)                                              # :514
        db2 = [num(((u0[r] - u[r]) ** 2).sum()) for r in range(ne)]
        smax = max(db2)                                                      # :519-523: the maximum over the effects
        if smax < F20:
            recs[0]["floors"].add("cnv")
        cnv = num(np.log10(max(smax, F20)))                                  # :524
        numit += 1
        cnvs.append(cnv)
        if trace:
            recs[0].update(ey=ey.copy(), db2=db2, ve=ve.copy(), cnv=cnv)
            trc.append(recs)
        if numit >= 5 and (cnv < logtol or np.isnan(cnv)):                   # :527
            break
    hat = X @ b                                                              # :536-540
    for r, Z in enumerate(Zs):
        hat = hat + Z @ u[r]
    out = {"TrZSZ": Tr, "b": b, "u": u, "vb_list": vb, "GC_list": [_gc(v)[0] for v in vb], "ve": ve, "hat": hat, "its": numit, "cnv": cnv,
           "bend": np.array(inflate), "cnv_trace": np.array(cnvs), "mm": mm, "floors0": floors0}
    if trace:
        out["trace"] = trc
        out["start"] = start
        out["setup"] = dict(iXX=iXX, b0=b0, y=y, Y=Yin, X=X)
    return out
