"""Line-cited numpy restatement of MRR3 / MRR3F (bWGR src/RcppEigen20230423.cpp:318-700, :704-1080) for the tests.

Written from the contract in include/bwgr.h and DESIGN.md section 4.5, in float64 (dtype=np.float32 gives the MRR3F flavour: the
same steps with float arrays).  The marker orders come from bwgr_amd.em_order, the library's own std::shuffle(order,
std::mt19937(it)) made cumulatively, as the reference makes it (:869); that call is host-only and needs no GPU.

mrr(Y, X, ...) returns the reference's list as a dict (mu, b, hat, h2, GC, vb, ve, MSx, cnvB, cnvH2, cnvV, b_Weights, Its) and,
with trace=True, also "trace": one dict per iteration (e, y, Z, Xc, b, ve/vb used by the sweep, bent, and lam: the smallest eigenvalue
of GC before bending) for invariant tests.

dtype=np.longdouble runs the same recurrence with every array, accumulator, scalar option and k x k routine in long double (the yardstick
of tests/mt_tight.py): the k x k routines are those of tests/ld_linalg.py, and the markers' systems of a sweep are inverted in one batched
call, as k_mrr_linv inverts them.  dot(x_J, e) stands in for the step's dependent dot x_J'e (the mutants of tests/test_mt_tight_cpu.py).
"""
import numpy as np

import ld_linalg


def _cumulative_orders(p, upto):
    import bwgr_amd
    return bwgr_amd.em_order(p, upto)


def mrr(Y, X, maxit=500, tol=10e-9, TH=False, HCS=False, XFA=False, ACS=False, NumXFA=3, R2=0.5, gc0=0.5, df0=1.0,
        updateMu=False, weight_prior_h2=0.01, weight_prior_gc=0.01, OneVarB=False, OneVarE=False, dtype=np.float64,
        trace=False, orders=None, dot=None):
    f = dtype
    wide = np.dtype(f) == np.dtype(np.longdouble)
    la = ld_linalg if wide else np.linalg
    if wide:
        tol, R2, gc0, df0, weight_prior_h2, weight_prior_gc = f(tol), f(R2), f(gc0), f(df0), f(weight_prior_h2), f(weight_prior_gc)
    Y = np.array(Y, dtype=f, copy=True)
    if Y.ndim == 1:
        Y = Y[:, None]
    X = np.asarray(X, dtype=f)
    n0, k = Y.shape
    p = X.shape[1]
    # incidence matrix Z: NaN -> Z = 0, Y = 0 (:746-750)
    Z = (~np.isnan(Y)).astype(f)
    Y[np.isnan(Y)] = 0
    n = Z.sum(0)                                                     # observed rows per trait (:754)
    iN = 1 / n                                                       # :755
    mu = Y.sum(0) * iN                                               # :758-759
    y = (Y - mu) * Z                                                 # :761
    Xc = X - X.mean(0)                                               # centred by the all-rows column mean (:763-765)
    XX = (Xc ** 2).T @ Z                                             # p x k: sum_r z_rt x_c,rj^2 (:768-770)
    XZ = Xc.T @ Z
    XSX = XX * iN - (XZ * iN) ** 2                                   # population variances over observed rows (:772-775)
    MSx = XSX.sum(0)                                                 # :777
    TrXSX = n * MSx                                                  # :778
    iN = 1 / (n - 1)                                                 # from here on (:781); updateMu uses it (quirk)
    vy = (y ** 2).sum(0) * iN                                        # :781-782
    ve = vy * (1 - R2)                                               # :784
    vbInit = vy * R2 / MSx                                           # :787
    veInit = ve.copy()                                               # :788
    vb = np.diag(vbInit).astype(f)                                   # :789
    iG = la.inv(vb)                                                  # :790, before the covariances are set
    h2 = 1 - ve / vy                                                 # :791
    for i in range(k):                                               # :796-804
        for j in range(i):
            vb[i, j] = vb[j, i] = gc0 * np.sqrt(vb[i, i] * vb[j, j])
    tilde = Xc.T @ y                                                 # :806
    XSXn = XSX * n if TH else XSX                                    # :807-812
    Sb = vb * df0                                                    # :816
    Se = ve * df0                                                    # :817
    iNp = 1 / (n + df0 - 1)                                          # :818
    b = np.zeros((p, k), f)                                          # :823
    e = y.copy()                                                     # :825
    GC = vb.copy()
    cnv1, cnv2, cnv3 = [], [], []
    logtol = np.log10(tol) if tol > 0 else -np.inf
    numit = 0
    trc = []
    ords = orders
    while numit < maxit:
        beta0, vb0, h20 = b.copy(), vb.copy(), h2.copy()             # :863-866
        order = _cumulative_orders(p, numit) if ords is None else ords[numit]   # :869
        iVe = 1 / ve
        ve_used, iG_used = ve.copy(), iG.copy()
        Linv = la.inv(iG + (XX * iVe)[:, :, None] * np.eye(k, dtype=f)) if wide else None   # every marker's LHS^-1 at once
        for J in order:                                              # :871-902
            b0 = b[J].copy()
            LHS = iG + np.diag(XX[J] * iVe)                          # :884
            RHS = ((Xc[:, J] @ e if dot is None else dot(Xc[:, J], e)) + XX[J] * b0) * iVe   # :885-886
            b1 = Linv[J] @ RHS if wide else np.linalg.solve(LHS, RHS)   # LLT solve (:896)
            b[J] = b1
            e = e - np.outer(Xc[:, J], b1 - b0) * Z                  # :900-901
        rec = {"e": e.copy(), "y": y, "Z": Z, "Xc": Xc, "b": b.copy(), "ve_sweep": ve_used, "iG_sweep": iG_used, "mu": mu.copy()} if trace else None
        ve = ((e * y).sum(0) + Se) * iNp                             # :916-917
        h2 = 1 - ve / vy                                             # :918, before the prior
        if weight_prior_h2 > 0:                                      # :920
            ve = ve * (1 - weight_prior_h2) + weight_prior_h2 * veInit
        if OneVarE:                                                  # :922
            ve = np.full(k, ve.mean(), f)
        iVe = 1 / ve
        if TH:                                                       # :928-934
            Dinv = 1 / (XSXn / ve + np.diag(iG))
            TrD = (XSXn * Dinv).sum(0)
            TildeHat = b.T @ (Dinv * tilde)
            Tr = TrD
        else:
            TildeHat = b.T @ tilde                                   # :936
            Tr = TrXSX
        vb = np.empty((k, k), f)
        for i in range(k):                                           # :941-955
            for j in range(k):
                if i == j:
                    vb[i, i] = (TildeHat[i, i] + Sb[i, i]) / (Tr[i] + df0)
                else:
                    vb[i, j] = (TildeHat[i, j] + TildeHat[j, i] + Sb[i, j]) / (Tr[i] + Tr[j] + df0)
        if weight_prior_h2 > 0:                                      # :957-958
            for i in range(k):
                vb[i, i] = vb[i, i] * (1 - weight_prior_h2) + weight_prior_h2 * vbInit[i]
        sd = np.sqrt(np.diag(vb))
        if weight_prior_gc > 0:                                      # :959-962
            GC = (1 - weight_prior_gc) * vb / np.outer(sd, sd) + gc0 * weight_prior_gc
            np.fill_diagonal(GC, 1)
            off = ~np.eye(k, dtype=bool)
            vb[off] = (GC * np.outer(sd, sd))[off]
        else:
            GC = vb / np.outer(sd, sd)                               # :964
        if ACS:                                                      # :967-973
            gs = (GC.sum() - k) / (k * (k - 1)) / 2.0
            GC = (_udu(GC, NumXFA, la) + gs) * 0.5
            np.fill_diagonal(GC, 1)
        elif HCS:                                                    # :974-981
            gs = GC[np.tril_indices(k, -1)].sum() / ((k * (k - 1)) // 2) if k > 1 else 0.0
            GC = np.full((k, k), gs, f)
            np.fill_diagonal(GC, 1)
        elif XFA:                                                    # :982-986
            GC = _udu(GC, NumXFA, la)
            np.fill_diagonal(GC, 1)
        lam = la.eigvalsh(GC).min()                                  # bending (:1009-1022)
        bent = lam < 0
        if bent:
            inflate = abs(lam * 1.1)
            GC = (GC + inflate * np.eye(k)) / (1 + inflate)
        if OneVarB:                                                  # :1023
            vb = GC * np.diag(TildeHat).mean()
        else:                                                        # :1023-1025
            sd = np.sqrt(np.diag(vb))
            vb = GC * np.outer(sd, sd)
        iG = la.pinv(vb)                                             # :1027
        if updateMu:                                                 # :1030-1036
            d = e.sum(0) * iN
            mu = mu + d
            e = (e - d) * Z
        if trace:
            rec["bent"] = bool(bent)
            rec["lam"] = lam
            trc.append(rec)
        cnv = np.log10(((beta0 - b) ** 2).sum(0).max())              # :1041
        cnv1.append(cnv)
        if np.isnan(cnv):                                            # stops before numit is incremented
            cnv1.pop()
            break
        cnv2.append(np.log10(((h20 - h2) ** 2).sum()))               # :1042
        cnv3.append(np.log10(((vb0 - vb) ** 2).sum()))               # :1043
        numit += 1
        if cnv < logtol:
            break
    hat = Xc @ b + mu                                                # :1054-1055, every row
    out = {"mu": mu, "b": b, "hat": hat, "h2": h2, "GC": GC, "vb": vb, "ve": ve, "MSx": MSx, "cnvB": np.array(cnv1),
           "cnvH2": np.array(cnv2), "cnvV": np.array(cnv3), "b_Weights": np.ones((p, k)), "Its": numit}
    if trace:
        out["trace"] = trc
    return out


def _udu(GC, nf, la=np.linalg):
    """sum of the nf leading eigen-terms lambda v v' (:990-991)."""
    w, V = la.eigh(GC)
    k = len(w)
    U = np.zeros_like(GC)
    for i in range(nf):
        U += w[k - 1 - i] * np.outer(V[:, k - 1 - i], V[:, k - 1 - i])
    return U


def scaled_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (den if den > 0 else 1.0))
