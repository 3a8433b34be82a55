"""Line-cited numpy restatement of the two-design solver and its drivers (bWGR src/RcppEigen20230423.cpp) for the tests:

  solver2x :1446-1493      GetImputedY :1517-1528      LatentSpaces :1530-1539      MEGA :1542-1579      GSEM :1582-1610

Written from those lines in float64 on top of uvb_restatement (solver1x / UVBETA, the marker orders of bwgr_amd.em_order, the row subsetting
of submat_f / subvec_f) and sem_restatement.latent (Eigen's BDCSVD with thin U and V, the npc rule, flip).  These programs are double
programs: nothing is rounded.  solver2x's maxit, tol and df0 are arguments of MEGA and GSEM here, as in the library; the reference calls it
with its defaults (100, 10e-7, 20).

The library's departures (include/bwgr.h) are carried:
  1. where XX_iJ is exactly 0 the coefficient is exactly 0, in both designs;
  2. a design whose TrXSX_i is 0 on the rows given (every column constant) is skipped: its coefficients stay 0, its lambda is never formed,
     its vb_i is NaN, and the other design runs as if alone (the reference divides by zero and returns NaN);
  3. a trait without observed rows gives zero columns, its = 0, mu = h2 = 0 and NaN elsewhere (uvbeta2; MEGA refuses it);
  4. h2 = 1 - ve / vy is reported;
  5. GSEM's b uses V.leftCols(npc) (:1609 multiplies by the whole V, conformable only for npc = min(n, k), where the two agree; whole_v=True
     restates the line as written).

Every function returns the reference's list as a dict, in its order, and with it every intermediate.  flip: a sequence of +-1, one per
singular pair, applied to (U, V): b, hat, gebv, mu and BETA2 must not depend on it; LS, LS_BETA and BETA1 flip with it.
"""
import numpy as np

import sem_restatement as SR
import uvb_restatement as UR


def solver2x(Y, X1, X2, maxit=100, tol=10e-7, df0=20.0, lam=None, record=None, dtype=np.float64, dot1=None, dot2=None):
    """One trait on the rows it is given.  dict(b1, b2, mu, h2, ve, vb1, vb2, its, cnv, XX1, XX2, lam1, lam2, trace); trace[s] = cnv after
    sweep s.  lam = (lambda_1, lambda_2): fixed lambdas in place of the variance updates (the ridge pin of the CPU tests).  record: as
    uvb_restatement.solver's, with X2 as that solver's X (TrXSX, vb, lam, p, bb, tb, db2 are X2's) and X1's beside them: TrXSX1, vb1, lam1,
    q1 = p1, and per sweep the leg's three sums d1 = sum (delta b_1)^2, bb1 = b_1'b_1, tb1 = tilde1'b_1.  dtype, dot1, dot2: as
    uvb_restatement.solver's dtype and dot, one dot per leg."""
    f = dtype
    tol, df0 = f(tol), f(df0)
    Y = np.asarray(Y, f)
    X1 = np.array(X1, f, copy=True)
    X2 = np.array(X2, f, copy=True)
    n, p1, p2 = X1.shape[0], X1.shape[1], X2.shape[1]                # :1448
    mu = Y.mean()                                                    # :1449
    y = Y - mu                                                       # :1450
    tilde1 = X1.T @ y; tilde2 = X2.T @ y                             # :1451, before the designs are centred
    X1 -= X1.mean(0)                                                 # :1452
    X2 -= X2.mean(0)                                                 # :1453
    XX1 = (X1 ** 2).sum(0); XX2 = (X2 ** 2).sum(0)                   # :1454
    TrXSX1 = XX1.sum(); TrXSX2 = XX2.sum()                           # :1455
    run1, run2 = TrXSX1 != 0, TrXSX2 != 0                            # departure 2
    with np.errstate(all="ignore"):
        vy = (y @ Y) / (n - 1)                                       # :1456
        ve = vy * 0.5                                                # :1457
        vb1 = (vy * 0.5) / (TrXSX1 / (n - 1)) if run1 else np.nan
        vb2 = (vy * 0.5) / (TrXSX2 / (n - 1)) if run2 else np.nan
        lam1 = ve / vb1 if run1 else np.nan                          # :1461
        lam2 = ve / vb2 if run2 else np.nan
    vb01 = vb1 * df0; vb02 = vb2 * df0; ve0 = ve * df0               # :1462
    if lam is not None:
        lam1, lam2 = f(lam[0]), f(lam[1])
    b_1 = np.zeros(p1, f); b_2 = np.zeros(p2, f)                     # :1458-1459
    e = y.copy()                                                     # :1460
    logtol = np.log10(tol) if tol > 0 else -np.inf
    numit, cnv, trace = 0, np.nan, []
    if record is not None:
        record.update(nt=n, mu=mu, sumy=y.sum(), vy=vy, TrXSX=TrXSX2, TrXSX1=TrXSX1, ve=ve, vb=vb2, vb1=vb1, lam=lam2, lam1=lam1, logtol=logtol,
                      df0=df0, p=p2, q1=p1, sweeps=[])

    def leg(X, XX, b, lmb, order, dot):
        for J in order:
            if not XX[J] > 0:                                        # departure 1
                b[J] = 0.0
                continue
            b0 = b[J]                                                # :1471, :1475
            ex = e @ X[:, J] if dot is None else dot(e, X[:, J])
            with np.errstate(all="ignore"):
                b1 = (ex + XX[J] * b0) / (XX[J] + lmb)               # :1472, :1476
            e[:] = e - X[:, J] * (b1 - b0); b[J] = b1                # :1473, :1477

    while numit < maxit:                                             # :1466
        beta01 = b_1.copy(); beta02 = b_2.copy()                     # :1467
        if run1:
            leg(X1, XX1, b_1, lam1, UR.order(p1, numit), dot1)       # :1468, :1470-1473
        if run2:
            leg(X2, XX2, b_2, lam2, UR.order(p2, numit), dot2)       # :1469, :1474-1477
        if record is not None:
            with np.errstate(all="ignore"):
                sums = dict(se=e.sum(), ey=e @ y, ee=e @ e, bb=b_2 @ b_2, tb=tilde2 @ b_2, db2=((beta02 - b_2) ** 2).sum(),
                            d1=((beta01 - b_1) ** 2).sum(), bb1=b_1 @ b_1, tb1=tilde1 @ b_1)
        mu0 = e.mean(); mu += mu0; e -= mu0                          # :1478
        with np.errstate(all="ignore"):
            ve = (e @ e + e @ y + ve0) / (2 * n - 1 + df0)           # :1479-1481
            if run1:
                vb1 = (tilde1 @ b_1 + b_1 @ b_1 + vb01) / (TrXSX1 + p1 + df0)   # :1482, :1484
            if run2:
                vb2 = (tilde2 @ b_2 + b_2 @ b_2 + vb02) / (TrXSX2 + p2 + df0)   # :1483-1484
            if lam is None:
                if run1:
                    lam1 = ve / vb1                                  # :1485
                if run2:
                    lam2 = ve / vb2
            cnv = np.log10(((beta01 - b_1) ** 2).sum() + ((beta02 - b_2) ** 2).sum())   # :1486
        trace.append(cnv)
        numit += 1
        stop = cnv < logtol or numit == maxit or np.isnan(cnv)       # :1487
        if record is not None:
            record["sweeps"].append(dict(sums, mu=mu, ve=ve, vb=vb2, vb1=vb1, lam=lam2, lam1=lam1, cnv=cnv, its=numit, on=not stop))
        if stop:
            break
    with np.errstate(all="ignore"):
        h2 = 1 - ve / vy                                             # departure 4
    return dict(b1=b_1, b2=b_2, mu=mu, h2=h2, ve=ve, vb1=vb1, vb2=vb2, its=numit, cnv=cnv, XX1=XX1, XX2=XX2, lam1=lam1, lam2=lam2, trace=trace)


def uvbeta2(Y, Z, X, maxit=100, tol=10e-7, df0=20.0, dtype=np.float64, dot1=None, dot2=None):
    """solver2x per column of Y on the rows where it is not NaN, as MEGA and GSEM call it (:1553-1561, :1595-1603).  A column without observed
    rows: departure 3.  dict(b1 [q x k], b2 [p x k], mu, h2, ve, vb1, vb2, its, cnv, trace [per trait]).  dtype, dot1, dot2: as solver2x's."""
    f = dtype
    Y = np.asarray(Y, f)
    if Y.ndim == 1:
        Y = Y[:, None]
    Z = np.asarray(Z, f)
    if Z.ndim == 1:
        Z = Z[:, None]
    X = np.asarray(X, f)
    q, p, k = Z.shape[1], X.shape[1], Y.shape[1]
    out = dict(b1=np.zeros((q, k), f), b2=np.zeros((p, k), f), mu=np.zeros(k, f), h2=np.zeros(k, f), ve=np.full(k, np.nan, f),
               vb1=np.full(k, np.nan, f), vb2=np.full(k, np.nan, f), its=np.zeros(k, np.int32), cnv=np.full(k, np.nan, f),
               trace=[[] for _ in range(k)])
    for t in range(k):
        w = ~np.isnan(Y[:, t])                                       # :1544
        if w.sum() == 0:
            continue
        r = solver2x(Y[w, t], Z[w], X[w], maxit, tol, df0, dtype=f, dot1=dot1, dot2=dot2)   # subvec_f / submat_f, :1554-1557
        out["b1"][:, t] = r["b1"]; out["b2"][:, t] = r["b2"]; out["trace"][t] = r["trace"]
        for key in ("mu", "h2", "ve", "vb1", "vb2", "its", "cnv"):
            out[key][t] = r[key]
    return out


def imputed_y(Y, G):
    """GetImputedY (:1517-1528) with G = X BETA: the records minus their trait's mean where observed, G where missing."""
    Y = np.array(Y, np.float64, copy=True)
    w = ~np.isnan(Y)
    N = w.sum(0).astype(np.float64)                                  # :1521
    with np.errstate(all="ignore"):
        Mu = np.where(w, Y, 0.0).sum(0) / N                          # :1521-1522
    return np.where(w, Y - Mu, G)                                    # :1523-1527


def latent_spaces(Y, G, npc=0, flip=None):
    """LatentSpaces (:1530-1539): dict(Y2 (scaled), s, U, V, Z = LS, npc)."""
    n = Y.shape[0]
    Y2 = imputed_y(Y, G)                                             # :1532
    SD = np.sqrt((Y2 ** 2).sum(0) / (n - 1))                         # :1533
    Y2 = Y2 / SD                                                     # :1534
    L = SR.latent(Y2, npc, flip)                                     # :1535-1539
    L["Y2"] = Y2
    return L


def _matrix(Y):
    Y = np.asarray(Y, np.float64)
    return Y[:, None] if Y.ndim == 1 else Y


def MEGA(Y, X, npc=-1, maxit=100, tol=10e-7, df0=20.0, flip=None):
    Y, X = _matrix(Y), np.asarray(X, np.float64)
    if not (~np.isnan(Y)).any(0).all():
        raise ValueError("MEGA: a trait without records (Y2 would be NaN, :1522)")
    BETA = UR.uvbeta(Y, X, "D", maxit, tol, df0)                     # :1545
    G = X @ BETA["b"]                                                # :1527
    L = latent_spaces(Y, G, npc, flip)                               # :1546
    LS = L["Z"]
    LSB = UR.uvbeta(LS, X, "D", maxit, tol, df0)                     # :1547
    fit = uvbeta2(Y, LS, X, maxit, tol, df0)                         # :1553-1561
    mu, b1, b2 = fit["mu"], fit["b1"], fit["b2"]
    b = LSB["b"] @ b1 + b2                                           # :1563
    hat = LS @ b1 + X @ b2 + mu                                      # :1564, :1567
    gebv = X @ b + mu                                                # :1565, :1568
    out = dict(mu=mu, b=b, hat=hat, LS=LS, LS_BETA=LSB["b"], BETA1=b1, BETA2=b2, gebv=gebv)   # :1571-1578
    out.update(BETA=BETA, G=G, LSB=LSB, fit=fit, s=L["s"], U=L["U"], V=L["V"], Y2=L["Y2"], npc=L["npc"])
    return out


def GSEM(Y, X, npc=-1, maxit=100, tol=10e-7, df0=20.0, flip=None, whole_v=False):
    Y, X = _matrix(Y), np.asarray(X, np.float64)
    BETA = UR.uvbeta(Y, X, "D", maxit, tol, df0)                     # :1585
    G = X @ BETA["b"]                                                # :1586
    L = SR.latent(G, npc, flip)                                      # :1586-1589
    LS = L["Z"]
    fit = uvbeta2(Y, LS, X, maxit, tol, df0)                         # :1595-1603
    mu, b1, b2 = fit["mu"], fit["b1"], fit["b2"]
    hat = LS @ b1 + X @ b2 + mu                                      # :1605-1606
    V = L["V"] if whole_v else L["V"][:, :L["npc"]]                  # departure 5
    b = BETA["b"] @ V @ b1 + b2                                      # :1609
    out = dict(mu=mu, b=b, hat=hat)                                  # :1608-1610
    out.update(BETA=BETA, G=G, LS=LS, BETA1=b1, BETA2=b2, fit=fit, s=L["s"], U=L["U"], V=L["V"], npc=L["npc"])
    return out
