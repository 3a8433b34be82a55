"""Line-cited numpy restatement of the per-trait ridge solvers (bWGR src/RcppEigen20230423.cpp) for the tests:

  D  solver1x :1410-1443 / UVBETA :1506-1515          F  solver1xF :1613-1646 / FUVBETA :1709-1718
  X  xsolver1xF :1721-1743 / XFUVBETA :1746-1753      Z  zsolver1xF :1771-1804 / ZFUVBETA :1807-1816

Written from those lines in float64.  The reference's F, X and Z are float programs; the library runs its fp64 engine on inputs rounded to
float (include/bwgr.h), so the tests hand this restatement the rounded Y, and it rounds tol and df0 itself for those variants.  The marker
orders come from bwgr_amd.em_order, the library's own std::shuffle(order, std::mt19937(numit)) made cumulatively as the reference makes it
(:1428); that call is host-only and needs no GPU.  The per-trait row subsetting is submat_f / subvec_f (:1495-1503): the observed rows, in
order.  xsolver1xF and zsolver1xF have maxit = 100, tol = 10e-7 and df0 = 20 built in (:1722-1723, :1772); here they are arguments, as in
the library.
"""
import numpy as np

_ORDERS = {}


def order(p, sweep):
    if (p, sweep) not in _ORDERS:
        import bwgr_amd
        _ORDERS[(p, sweep)] = bwgr_amd.em_order(p, sweep)
    return _ORDERS[(p, sweep)]


def solver(Y, X, variant="D", maxit=100, tol=10e-7, df0=20.0, lam=None, record=None, dtype=np.float64, dot=None):
    """One trait on the rows it is given.  dict(b, mu, h2, ve, vb, its, cnv, XX, trace); trace[s] = cnv after sweep s.  lam: a fixed lambda
    for variant X in place of XX.mean() (the ridge pin of the CPU tests).  record: a dict that receives the start values (nt, mu, sumy, vy,
    TrXSX, ve, vb, lam, and logtol, df0, p as used) and, under "sweeps", per sweep the six sums a sweep leaves, taken before the mean is
    removed from e (se, ey, ee, bb, tb, db2), with what the tail makes of them (mu, ve, vb, lam, cnv, its, on: the trait goes on).
    dtype: np.longdouble runs the same recurrence with every array, accumulator and scalar in long double (the yardstick of
    tests/uvb_tight.py); tol, df0 and F's guard are rounded as for float64 and then widened.  dot(e, x_J): stands in for the step's dependent
    dot e'x_J (the mutants of tests/test_uvb_tight_cpu.py)."""
    assert variant in "DFXZ"
    f = dtype
    if variant != "D":
        tol = float(np.float32(tol)); df0 = float(np.float32(df0))
    tol, df0, guard = f(tol), f(df0), f(0.00001)
    Y = np.asarray(Y, f)
    X = np.array(X, f, copy=True)
    n, p = X.shape
    mu = Y.mean()                                                    # :1413
    y = Y - mu                                                       # :1414
    tilde = X.T @ y                                                  # :1415, before X is centred
    X -= X.mean(0)                                                   # :1416
    XX = (X ** 2).sum(0)                                             # :1417
    TrXSX = XX.sum()                                                 # :1418
    with np.errstate(all="ignore"):
        MSx = TrXSX / (n - 1); vy = (y @ Y) / (n - 1)                # :1419
        ve = vy * 0.5; vb = (vy * 0.5) / MSx                         # :1420
        lmb = ve / vb; vb0 = vb * df0; ve0 = ve * df0                # :1423
    if variant == "X":
        lmb = XX.mean() if lam is None else f(lam)                   # :1730
        ve = vb = np.nan
    b = np.zeros(p, f)                                               # :1421
    e = y.copy()                                                     # :1422
    logtol = np.log10(tol) if tol > 0 else -np.inf
    numit, cnv, trace = 0, np.nan, []
    if record is not None:
        record.update(nt=n, mu=mu, sumy=y.sum(), vy=vy, TrXSX=TrXSX, ve=ve, vb=vb, lam=lmb, logtol=logtol, df0=df0, p=p, sweeps=[])
    while numit < maxit:                                             # :1426
        beta0 = b.copy()                                             # :1427
        for J in order(p, numit):                                    # :1428-1429
            if variant == "F" and not XX[J] > guard:                 # :1633, :1635
                b[J] = 0.0
                continue
            b0 = b[J]                                                # :1430
            ex = e @ X[:, J] if dot is None else dot(e, X[:, J])
            with np.errstate(all="ignore"):
                b1 = (ex + XX[J] * b0) / (XX[J] + lmb)               # :1431
            e -= X[:, J] * (b1 - b0); b[J] = b1                      # :1432
        if record is not None:
            with np.errstate(all="ignore"):
                sums = dict(se=e.sum(), ey=e @ y, ee=e @ e, bb=b @ b, tb=tilde @ b, db2=((beta0 - b) ** 2).sum())
        mu0 = e.mean(); mu += mu0; e -= mu0                          # :1433
        with np.errstate(all="ignore"):
            if variant in "DF":
                ve = (e @ y + e @ e + ve0) / (2 * n - 1 + df0)       # :1434-1436
                vb = (b @ b + tilde @ b + vb0) / (TrXSX + p + df0)   # :1437-1439
                lmb = ve / vb
            elif variant == "Z":
                ve = (e @ y + ve0) / (n + df0)                       # :1795-1796
                vb = (tilde @ b + vb0) / (TrXSX + df0)               # :1797-1798
                lmb = ve / vb                                        # :1799
            cnv = np.log10(((beta0 - b) ** 2).sum())                 # :1440
        trace.append(cnv)
        numit += 1
        stop = cnv < logtol or numit == maxit or np.isnan(cnv)       # :1441
        if record is not None:
            record["sweeps"].append(dict(sums, mu=mu, ve=ve, vb=vb, lam=lmb, cnv=cnv, its=numit, on=not stop))
        if stop:
            break
    with np.errstate(all="ignore"):
        h2 = np.nan if variant == "X" else 1 - ve / vy               # :1802
    return dict(b=b, mu=mu, h2=h2, ve=ve, vb=vb, its=numit, cnv=cnv, XX=XX, lam=lmb, trace=trace)


def uvbeta(Y, X, variant="D", maxit=100, tol=10e-7, df0=20.0, dtype=np.float64, dot=None):
    """UVBETA / FUVBETA / XFUVBETA / ZFUVBETA: one solver per column of Y on the rows where it is not NaN (:1507-1514).  A column without
    observed rows is a zero column with its = 0 (:1510, :1713, :1811; XFUVBETA has no such test, the library returns zeros there too).
    dict(b [p x k], mu, h2, ve, vb, its, cnv, XX [p x k], trace [per trait]).  dtype, dot: as solver's."""
    f = dtype
    Y = np.asarray(Y, f)
    if Y.ndim == 1:
        Y = Y[:, None]
    X = np.asarray(X, f)
    p, k = X.shape[1], Y.shape[1]
    out = dict(b=np.zeros((p, k), f), mu=np.zeros(k, f), h2=np.zeros(k, f), ve=np.full(k, np.nan, f), vb=np.full(k, np.nan, f),
               its=np.zeros(k, np.int32), cnv=np.full(k, np.nan, f), XX=np.zeros((p, k), f), trace=[[] for _ in range(k)])
    for t in range(k):
        w = ~np.isnan(Y[:, t])                                       # :1508
        if w.sum() == 0:                                             # :1510
            continue
        r = solver(Y[w, t], X[w], variant, maxit, tol, df0, dtype=f, dot=dot)   # subvec_f / submat_f, :1511-1513
        out["b"][:, t] = r["b"]; out["XX"][:, t] = r["XX"]; out["trace"][t] = r["trace"]
        for key in ("mu", "h2", "ve", "vb", "its", "cnv"):
            out[key][t] = r[key]
    return out

