"""Line-cited numpy restatement of mrr_svd (bWGR src/RcppEigen20230423.cpp:1083-1260) for the tests, in float64, written from the reference's
text and the contract in include/bwgr.h.

design_eigh(W): the library's design -- eigh of the exact, double-centred Gram matrix, the rank rule on the eigenvalues (bwgr_amd/svd.py).
design_svd(W):  the reference's -- numpy.linalg.svd of the centred matrix (:1094-1101), the same rank rule on the singular values; V too.
fit(Y, X):      the Gauss-Seidel (:1103-1243) on a given design; Y as it is.
mrr_svd(Y, W):  the whole entry on design_svd, Y rounded to float once: the WModel list as a dict, MarkerEffects = V b (:1235).
tail(TH, Tr):   the covariance update alone (:1203-1216), for the header's check.
xta_ld(W, A, centre): X'A in numpy.longdouble with the implicit centring's terms, and the elementwise bound of the issue.
asum(A):        s_t as bwgr_panel_xta sums it: 256 partial sums over the rows q, q + 256, ..., then the partials in ascending q.
"""
import numpy as np

WMODEL_KEYS = ("Intercepts", "MarkerEffects", "FittedValues", "Heritability", "WCorrelations", "VarBeta", "VarResiduals", "ConvergenceBeta",
               "ConvergenceH2", "ConvergenceVar", "NumOfIterations")


def rank_factor(n, p):
    """a singular value is kept above d_1 * this (numpy's matrix_rank rule at float precision)"""
    return max(n, p) * 2.0 ** -24


def design_eigh(W):
    W = np.asarray(W)
    n, p = W.shape
    Wi = W.astype(np.int64)
    G = Wi @ Wi.T
    rs = G.sum(1).astype(np.float64)
    tot = float(G.sum())
    Gc = G.astype(np.float64) - rs[:, None] / n - rs[None, :] / n + tot / (float(n) * float(n))
    w, V = np.linalg.eigh((Gc + Gc.T) * 0.5)
    w, V = w[::-1], V[:, ::-1]
    r = int(np.sum(w > w[0] * rank_factor(n, p) ** 2))
    d = np.sqrt(w[:r])
    return dict(X=V[:, :r] * d, d=d, U=V[:, :r], lam=w, r=r)


def design_svd(W):
    W = np.asarray(W, np.float64)
    n, p = W.shape
    Wc = W - W.mean(0)                                               # :1094-1096
    U, d, Vt = np.linalg.svd(Wc, full_matrices=False)                # :1098
    r = int(np.sum(d > d[0] * rank_factor(n, p)))
    return dict(X=U[:, :r] * d[:r], d=d[:r], U=U[:, :r], V=Vt[:r].T, Wc=Wc, dall=d, r=r)   # X = U D (:1100), beta = V b (:1235)


def tail(TH, Tr):
    """vb, iG, whether it bent, the smallest eigenvalue (:1203-1216)"""
    k = len(Tr)
    vb = np.empty((k, k))
    for i in range(k):
        for j in range(k):
            vb[i, j] = TH[i, i] / Tr[i] if i == j else (TH[i, j] + TH[j, i]) / (Tr[i] + Tr[j])
    lam = np.linalg.eigvalsh(vb).min()                               # :1213
    bent = bool(lam < 0.0)
    if bent:
        vb = vb + np.eye(k) * abs(lam * 1.1)                         # :1214-1215
    return vb, np.linalg.pinv(vb), bent, lam                         # :1216


def fit(Y, X, maxit=500, tol=10e-9, trace=False):
    Y = np.array(Y, np.float64, copy=True)
    if Y.ndim == 1:
        Y = Y[:, None]
    X = np.asarray(X, np.float64)
    k = Y.shape[1]
    p = X.shape[1]
    Z = (~np.isnan(Y)).astype(np.float64)                            # :1106-1111
    Y[np.isnan(Y)] = 0.0
    n = Z.sum(0)                                                     # :1114
    iN = 1.0 / n
    mu = Y.sum(0) * iN                                               # :1119-1120
    y = (Y - mu) * Z                                                 # :1121-1124
    XX = (X ** 2).T @ Z                                              # :1128-1129
    XSX = XX * iN - ((X.T @ Z) * iN) ** 2                            # :1131-1133
    MSx = XSX.sum(0)                                                 # :1134
    iN = 1.0 / (n - 1.0)                                             # :1139
    vy = (y ** 2).sum(0) * iN                                        # :1140
    ve = vy * 0.5                                                    # :1141
    iVe = 1.0 / ve
    vb = np.diag(ve / MSx)                                           # :1144
    iG = np.diag(MSx / ve)                                           # :1145
    h2 = 1.0 - ve / vy                                               # :1146
    tilde = X.T @ y                                                  # :1148
    XSXn = XSX * n                                                   # :1151
    b = np.zeros((p, k))
    e = y.copy()
    logtol = np.log10(tol) if tol > 0 else -np.inf
    c1, c2, c3, trc = [], [], [], []
    numit = 0
    while numit < maxit:
        beta0, vb0, h20 = b.copy(), vb.copy(), h2.copy()             # :1169-1172
        for J in range(p):                                           # the natural order (:1175)
            b0 = b[J].copy()
            LHS = iG + np.diag(XX[J] * iVe)                          # :1178
            RHS = (X[:, J] @ e + XX[J] * b0) * iVe                   # :1179-1180
            b1 = np.linalg.solve(LHS, RHS)                           # :1181
            b[J] = b1
            e = e - np.outer(X[:, J], b1 - b0) * Z                   # :1184
        ve = (e * y).sum(0) * iN                                     # :1188-1189
        iVe = 1.0 / ve
        h2 = 1.0 - ve / vy                                           # :1191
        Dinv = 1.0 / (XSXn / ve + np.diag(iG))                       # :1195
        Tr = (XSXn * Dinv).sum(0)                                    # :1196
        TH = b.T @ (Dinv * tilde)                                    # :1197
        vb, iG, bent, lam = tail(TH, Tr)
        if trace:
            trc.append(dict(TH=TH, Tr=Tr, vb=vb.copy(), iG=iG.copy(), bent=bent, lam=lam))
        with np.errstate(divide="ignore", invalid="ignore"):
            cnv = np.log10(((beta0 - b) ** 2).sum())                 # :1219
            c1.append(cnv)
            c2.append(np.log10(((h20 - h2) ** 2).sum()))             # :1220
            c3.append(np.log10(((vb0 - vb) ** 2).sum()))             # :1221
        numit += 1                                                   # :1224
        if cnv < logtol or np.isnan(cnv):                            # :1226-1227
            break
    hat = X @ b + mu                                                 # :1233-1234
    sd = np.sqrt(np.diag(vb))
    out = dict(mu=mu, b=b, hat=hat, h2=h2, GC=vb / np.outer(sd, sd), vb=vb, ve=ve, cnvB=np.array(c1), cnvH2=np.array(c2), cnvV=np.array(c3), Its=numit)
    if trace:
        out["trace"] = trc
    return out


def mrr_svd(Y, W, maxit=500, tol=10e-9):
    Yf = np.asarray(Y, np.float64)
    if Yf.ndim == 1:
        Yf = Yf[:, None]
    Yf = Yf.astype(np.float32).astype(np.float64)
    D = design_svd(W)
    f = fit(Yf, D["X"], maxit, tol)
    beta = D["V"] @ f["b"]                                           # :1235
    vals = (f["mu"], beta, f["hat"], f["h2"], f["GC"], f["vb"], f["ve"], f["cnvB"], f["cnvH2"], f["cnvV"], f["Its"])
    return dict(zip(WMODEL_KEYS, vals))


def asum(A, n=None):
    A = np.asarray(A, np.float64)
    if A.ndim == 1:
        A = A[:, None]
    n = A.shape[0] if n is None else n
    part = np.zeros((256, A.shape[1]))
    for i0 in range(0, n, 256):
        rows = A[i0:min(i0 + 256, n)]
        part[:rows.shape[0]] = part[:rows.shape[0]] + rows
    s = np.zeros(A.shape[1])
    for q in range(256):
        s = s + part[q]
    return s


def xta_ld(W, A, centre):
    """(X'A or X_c'A in long double, the bound (n + 8) 2^-53 (|X|'|A| + |xbar| sum|A|)) -- both p x k"""
    W = np.asarray(W)
    A = np.asarray(A, np.float64)
    if A.ndim == 1:
        A = A[:, None]
    n = W.shape[0]
    Wl, Al = W.astype(np.longdouble), A.astype(np.longdouble)
    ref = Wl.T @ Al
    xbar = Wl.sum(0) / np.longdouble(n)
    if centre:
        ref = ref - np.outer(xbar, Al.sum(0))
    bound = (n + 8) * 2.0 ** -53 * (np.abs(Wl).T @ np.abs(Al) + np.outer(np.abs(xbar), np.abs(Al).sum(0)))
    return ref, bound.astype(np.float64)


def scaled_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (den if den > 0 else 1.0))
