"""A float64 numpy restatement of MLM (src/RcppEigen20230423.cpp:1262-1405), the multivariate model with fixed effects, on the float-rounded
inputs: what tests/test_gpu_mlm.py holds bwgr_amd.mlm.MLM against.  The reference's own steps in its order, in float64 where it computes in
float; the column orders come from bwgr_amd.em_order, the library's std::shuffle(order, std::mt19937(sweep)) applied cumulatively, as the
reference applies it to its RGSvec.  Nothing here is shared with the code under test but that order."""
import numpy as np

MLM_KEYS = ("b", "u", "hat", "h2", "GC", "vb", "ve", "cnv", "its")


def f32(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def scaled_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.max(np.abs(b)) if b.size else 0.0
    return float(np.max(np.abs(a - b)) / (den if den > 0 else 1.0)) if b.size else 0.0


def project(Z, X):
    """(Zp, C): Zp = Z - X C, C = (X'X)^-1 X'Z over all rows (:1287-1288)"""
    C = np.linalg.solve(X.T @ X, X.T @ Z)
    return Z - X @ C, C


def fixed(Y, X):
    """(W, MU, y): the masks, MU_t = (M_t'M_t)^-1 M_t'Y_t on trait t's rows, y_t = (Y_t - M_t MU_t) o W_t (:1270-1286)"""
    W = (~np.isnan(Y)).astype(np.float64)
    Y0 = np.where(np.isnan(Y), 0.0, Y)
    k, f = Y.shape[1], X.shape[1]
    MU, y = np.zeros((f, k)), np.zeros_like(Y0)
    for t in range(k):
        M = X * W[:, t:t + 1]
        MU[:, t] = np.linalg.solve(M.T @ M, M.T @ Y0[:, t])
        y[:, t] = (Y0[:, t] - M @ MU[:, t]) * W[:, t]
    return W, MU, y


def bend(vb, inflate):
    """(vb with inflate on its diagonal, inflate, the smallest eigenvalue before): inflate only grows (:1366-1369)"""
    lam = float(np.linalg.eigvalsh((vb + vb.T) / 2)[0])
    if lam < 0.001 and abs(lam * 1.1) > inflate:
        inflate = abs(lam * 1.1)
    return vb + np.eye(vb.shape[0]) * inflate, inflate, lam


def fit(Y, X, Z, maxit=500, logtol=-8.0, verb=False, df0=1.1, trace=False, orders=None):
    """The reference's list as a dict in its order.  trace=True adds "trace": per sweep ey, TH, db2, ve, vb, iG, inflate and the smallest eigenvalue
    of vb before bending, and "start": Tr, ssy, nt.  orders(p, s): the column order of sweep s (default bwgr_amd.em_order)."""
    if orders is None:
        import bwgr_amd
        orders = bwgr_amd.em_order
    Y, X, Z = f32(Y), f32(X), f32(Z)
    if Y.ndim == 1:
        Y = Y[:, None]
    logtol, df0 = float(np.float32(logtol)), float(np.float32(df0))
    k, f, p = Y.shape[1], X.shape[1], Z.shape[1]
    W, MU, y = fixed(Y, X)
    nt = W.sum(0)
    iN = 1.0 / (nt - f)
    Zp, _ = project(Z, X)
    ZZ = (Zp * Zp).T @ W                                               # :1292
    Tr = ZZ.sum(0)
    b = np.zeros((p, k))
    e = y.copy()
    ssy = (y * y).sum(0)
    vy = ssy * iN
    ve = vy * 0.5
    vb = np.diag(ve / (Tr * iN))
    iG = np.diag(1.0 / np.diag(vb))
    tilde = Zp.T @ y
    inflate = 0.0
    Sb, Se = vb * df0, ve * df0
    iNp = 1.0 / (nt + df0 - f)
    cnv, numit, tr = 10.0, 0, []
    while numit < maxit:
        beta0 = b.copy()
        iVe = 1.0 / ve
        for J in orders(p, numit):
            b0 = b[J].copy()
            LHS = iG + np.diag(ZZ[J] * iVe)
            RHS = (Zp[:, J] @ e + ZZ[J] * b0) * iVe
            b1 = np.linalg.solve(LHS, RHS)
            b[J] = b1
            e -= np.outer(Zp[:, J], b1 - b0) * W
        ey = (e * y).sum(0)
        ve = (ey + Se) * iNp
        TH = b.T @ tilde
        vb = (TH + TH.T) / (Tr[:, None] + Tr[None, :])
        vb[np.diag_indices(k)] = (np.diag(TH) + np.diag(Sb)) / (Tr + df0)
        vb, inflate, lam = bend(vb, inflate)
        iG = np.linalg.pinv(vb, hermitian=True)
        numit += 1
        db2 = float(((beta0 - b) ** 2).sum())
        with np.errstate(divide="ignore"):
            cnv = float(np.log10(db2))
        if trace:
            tr.append(dict(ey=ey.copy(), TH=TH.copy(), db2=db2, ve=ve.copy(), vb=vb.copy(), iG=iG.copy(), inflate=inflate, lam=lam))
        if np.isnan(cnv):
            break
        if verb and cnv < logtol:
            break
    h2 = 1.0 - ve / vy
    hat = Zp @ b + X @ MU
    sd = np.sqrt(np.diag(vb))
    out = dict(zip(MLM_KEYS, (MU, b, hat, h2, vb / np.outer(sd, sd), vb, ve, cnv, numit)))
    if trace:
        out["trace"] = tr
        out["start"] = dict(Tr=Tr, ssy=ssy, nt=nt, vy=vy)
    return out
