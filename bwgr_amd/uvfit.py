"""The per-trait ridge fits and what is built of them: uvbeta, uvbeta_dense, uvbeta2, the solver1x / UVBETA family, XSEMF / ZSEMF / YSEMF, MEGA and
GSEM (bwgr_uvbeta*, include/bwgr.h)."""
import numpy as np

from . import _lib
from ._lib import BwgrError, check
from ._marshal import _dp, _ip, _matrix, _plan
from .panel import as_panel


# ---- per-trait ridge fits: solver1x / UVBETA, solver1xF / FUVBETA, XFUVBETA, ZFUVBETA (bwgr_uvbeta, include/bwgr.h) ----
UVB_VARIANTS = {"D": 0, "F": 1, "X": 2, "Z": 3}   # BWGR_UVB_*
UVB_KEYS = ("b", "mu", "h2", "ve", "vb", "its", "cnv")


def uvb_plan(n, p, k):
    """bwgr_debug_uvb_plan (host arithmetic, no GPU): dict(W, groups, solve_traits, ngl, solve_lds, pass_lds, pass_wg, ws_bytes)."""
    return _plan("bwgr_debug_uvb_plan", ("W", "groups", "solve_traits", "ngl", "solve_lds", "pass_lds", "pass_wg", "ws_bytes"), n, p, k)


def _uvb_variant(variant, who):
    if isinstance(variant, str) and variant not in UVB_VARIANTS:
        raise BwgrError(1, "%s: unknown variant %r (one of D, F, X, Z)" % (who, variant))
    return UVB_VARIANTS[variant] if isinstance(variant, str) else int(variant)   # (an integer is passed on: the library checks it)


def _uvb_inputs(Y, nrow, v, tol, df0, who):
    """Y as an n x k float64 matrix; for the float variants Y, tol and df0 rounded to float, as the reference receives them."""
    Ym = _matrix(Y, who, nrow)
    if v != 0:
        Ym = Ym.astype(np.float32).astype(np.float64)
        tol = float(np.float32(tol)); df0 = float(np.float32(df0))
    return Ym, tol, df0


def _uvb_outputs(ncoef, k):
    kk = max(k, 1)
    return (np.zeros((ncoef, kk), order="F"), np.zeros(kk), np.zeros(kk), np.zeros(kk), np.zeros(kk), np.zeros(kk, np.int32), np.zeros(kk))


def _uvb_panel(P, Ym, v, maxit, tol, df0, xb=False):
    """bwgr_uvbeta on exactly what it is given (n x k float64 Y): no rounding."""
    k = Ym.shape[1]
    Yf = np.asfortranarray(Ym)
    b, mu, h2, ve, vb, its, cnv = _uvb_outputs(P.p, k)
    xbm = np.zeros((P.n, max(k, 1)), order="F") if xb else None
    check(_lib.lib().bwgr_uvbeta(P._h, _dp(Yf), int(k), int(v), int(maxit), float(tol), float(df0), _dp(b), _dp(mu), _dp(h2), _dp(ve), _dp(vb),
                                 _ip(its), _dp(cnv), _dp(xbm) if xb else None))
    out = dict(zip(UVB_KEYS, (b, mu, h2, ve, vb, its, cnv)))
    if xb:
        out["xb"] = xbm
    return out


def _uvb_dense(Ym, Z, v, maxit, tol, df0, device=0):
    """bwgr_uvbeta_dense on exactly what it is given (n x k float64 Y, n x q float64 Z): no rounding."""
    Zf = np.asarray(Z, np.float64)
    n, q = Zf.shape
    if q < 2 or Zf.strides[0] != 8 or Zf.strides[1] % 8 or Zf.strides[1] < 8 * n:   # (the rows of a column-major matrix are passed as they lie: ldz > n)
        Zf = np.asfortranarray(Zf)
    ldz = Zf.strides[1] // 8 if q > 1 else max(n, 1)
    k = Ym.shape[1]
    Yf = np.asfortranarray(Ym)
    b, mu, h2, ve, vb, its, cnv = _uvb_outputs(q, k)
    check(_lib.lib().bwgr_uvbeta_dense(int(device), _dp(Zf), int(n), int(q), int(ldz), _dp(Yf), int(k), int(v), int(maxit), float(tol), float(df0),
                                       _dp(b), _dp(mu), _dp(h2), _dp(ve), _dp(vb), _ip(its), _dp(cnv)))
    return dict(zip(UVB_KEYS, (b, mu, h2, ve, vb, its, cnv)))


def uvbeta(Y, X, variant="D", maxit=100, tol=10e-7, df0=20.0, xb=False, **kw):
    """One ridge fit per column of Y on one X (bwgr_uvbeta): Y is n x k (NaN = missing) or a vector; variant "D" solver1x / UVBETA,
    "F" solver1xF / FUVBETA, "X" xsolver1xF / XFUVBETA, "Z" zsolver1xF / ZFUVBETA (src/RcppEigen20230423.cpp:1410-1816).  The float
    variants receive Y, tol and df0 rounded to float, as the reference does; the engine is fp64.  Returns dict(b [p x k], mu, h2, ve, vb,
    its, cnv[, xb [n x k] = X b on the raw genotypes]).  X is an array or a Panel."""
    v = _uvb_variant(variant, "uvbeta")
    with as_panel(X, **kw) as P:
        Ym, tol, df0 = _uvb_inputs(Y, P.n, v, tol, df0, "uvbeta")
        return _uvb_panel(P, Ym, v, maxit, tol, df0, xb)


def uvbd_plan(n, q, k):
    """bwgr_debug_uvbd_plan (host arithmetic, no GPU): dict(lds_rows, e_in_lds, threads, lds_bytes, ws_bytes)."""
    return _plan("bwgr_debug_uvbd_plan", ("lds_rows", "e_in_lds", "threads", "lds_bytes", "ws_bytes"), n, q, k)


def uvbeta_dense(Y, Z, variant="D", maxit=100, tol=10e-7, df0=20.0, *, device=0):
    """uvbeta's fits on a small dense real-valued design Z (n x q float64; bwgr_uvbeta_dense): one workgroup per trait runs the trait's whole
    fit.  Same variants, rounding of Y, tol and df0, rules and return dict (b is q x k) as uvbeta."""
    v = _uvb_variant(variant, "uvbeta_dense")
    Zm = _matrix(Z, "uvbeta_dense")
    if Zm.ndim != 2:
        raise BwgrError(1, "uvbeta_dense: Z has shape %s; it must be n x q" % (Zm.shape,))
    Ym, tol, df0 = _uvb_inputs(Y, Zm.shape[0], v, tol, df0, "uvbeta_dense")
    return _uvb_dense(Ym, Zm, v, maxit, tol, df0, device)


# ---- latent-space fits: XSEMF / ZSEMF / YSEMF (src/RcppEigen20230423.cpp:1756-1769, :1819-1874; R/RcppExports.R:232, 240, 244) ----
# Y is rounded to float once, as the reference receives it; everything after runs in fp64 on unrounded intermediates (G, Z, Y - G), where the
# reference computes in float throughout.  The thin SVD of G (n x k) is numpy's, on the host.  The results do not
# depend on the sign of a singular pair: the sign flips Z's column, V's column and the fitted coefficient together.
def _sem_npc(npc, m, who):
    """The latent columns kept of m = min(n, k) (:1760-1761).  npc < 0: round(2 sqrt(m)), which never lies on a tie ((x + 1/2)^2 is no
    integer); 0: m.  More than m is refused: leftCols(npc) would leave the matrix."""
    npc = int(npc)
    if npc < 0:
        npc = int(np.floor(2.0 * np.sqrt(m) + 0.5))                  # :1760
    if npc == 0:
        npc = m                                                      # :1761
    if npc > m:
        raise BwgrError(1, "%s: npc = %d exceeds min(nrow(Y), ncol(Y)) = %d" % (who, npc, m))
    return npc


def _sem_latent(G, npc, who):
    """Z = (U diag(s)).leftCols(npc) and V.leftCols(npc) of G = U diag(s) V' (:1759-1762)."""
    U, s, Vt = np.linalg.svd(G, full_matrices=False)
    npc = _sem_npc(npc, s.shape[0], who)
    return (U * s)[:, :npc], Vt.T[:, :npc]


def _sem_gc(G):
    """(:1765-1768) the columns centred and scaled to unit population variance, and their correlations; a zero column gives NaN, as there."""
    N = G.shape[0]
    G = G - G.mean(0)
    with np.errstate(all="ignore"):
        G = G / np.sqrt((G ** 2).sum(0) / N)
        return G, (G.T @ G) / N


def _sem(which, Y, X, npc, maxit, tol, df0, panel_kw):
    v = UVB_VARIANTS["X" if which == "XSEMF" else "Z"]
    with as_panel(X, **panel_kw) as P:
        Ym, tol, df0 = _uvb_inputs(Y, P.n, v, tol, df0, which)
        npc = _sem_npc(npc, min(Ym.shape), which)                    # (refused before anything runs)
        s1 = _uvb_panel(P, Ym, v, maxit, tol, df0)                   # BETA = XFUVBETA / ZFUVBETA(Y, X)
        Z, V = _sem_latent(P.xb(s1["b"]), npc, which)                # G = X BETA and its latent design
        s2 = _uvb_dense(Ym, Z, v, maxit, tol, df0, P.device)         # ALPHA / Coef = XFUVBETA / ZFUVBETA(Y, Z)
        b = s1["b"] @ (V @ s2["b"])
        G = P.xb(b)
        if which == "XSEMF":
            hat, GC = _sem_gc(G)
            return dict(zip(("b", "GC", "hat"), (b, GC, hat)))
        if which == "ZSEMF":
            return dict(zip(("mu", "b", "hat", "h2", "GC"), (s2["mu"], b, G + s2["mu"], s2["h2"], _sem_gc(G)[1])))
        s3 = _uvb_panel(P, Ym - G, v, maxit, tol, df0)               # beta_Xd = ZFUVBETA(Y - G, X), :1859
        b = b + s3["b"]
        G = P.xb(b)
        return dict(zip(("mu", "b", "hat", "h2", "GC"), (s3["mu"], b, G + s3["mu"], s2["h2"] + s3["h2"], _sem_gc(G)[1])))


def XSEMF(Y, X, npc=0, *, maxit=100, tol=10e-7, df0=20.0, **kw):
    """XSEMF(Y, X, npc), src/RcppEigen20230423.cpp:1756-1769 (R/RcppExports.R:232): XFUVBETA on the panel, the SVD of X BETA, XFUVBETA on its
    first npc latent columns, the coefficients mapped back.  list(b, GC, hat); hat is the standardised X b.  X is an array or a Panel."""
    return _sem("XSEMF", Y, X, npc, maxit, tol, df0, kw)


def ZSEMF(Y, X, npc=0, *, maxit=100, tol=10e-7, df0=20.0, **kw):
    """ZSEMF(Y, X, npc), src/RcppEigen20230423.cpp:1819-1845 (R/RcppExports.R:240): XSEMF's steps with ZFUVBETA.  list(mu, b, hat, h2, GC)."""
    return _sem("ZSEMF", Y, X, npc, maxit, tol, df0, kw)


def YSEMF(Y, X, npc=-1, *, maxit=100, tol=10e-7, df0=20.0, **kw):
    """YSEMF(Y, X, npc), src/RcppEigen20230423.cpp:1848-1874 (R/RcppExports.R:244): ZSEMF's latent fit, then ZFUVBETA(Y - X b, X) on the
    panel for what the latent space left.  list(mu, b, hat, h2, GC); npc = -1: round(2 sqrt(min(n, k))) latent columns."""
    return _sem("YSEMF", Y, X, npc, maxit, tol, df0, kw)


# ---- two designs in one sweep: solver2x, MEGA, GSEM (src/RcppEigen20230423.cpp:1446-1493, :1542-1610; R/RcppExports.R:200, 208, 212) ----
# Double precision throughout, as the reference: nothing is rounded.  The thin SVDs are numpy's, on the host.  The results do not depend on
# the sign of a singular pair: it flips LS's column, LS_BETA's (or V's) column and BETA1's row together, exactly, so b, hat, gebv, mu and
# BETA2 are invariant and LS, LS_BETA and BETA1 are defined up to that sign.
UVB2_KEYS = ("b1", "b2", "mu", "h2", "ve", "vb1", "vb2", "its", "cnv")


def _uvb2_panel(P, Ym, Z, maxit, tol, df0):
    """bwgr_uvbeta2 on exactly what it is given (n x k float64 Y, n x q float64 Z)."""
    Zf = np.asfortranarray(_matrix(Z, "uvbeta2", P.n, what="Z"))
    q = Zf.shape[1]
    k = Ym.shape[1]
    Yf = np.asfortranarray(Ym)
    b2, mu, h2, ve, vb2, its, cnv = _uvb_outputs(P.p, k)      # (one design's outputs for the panel, and Z's effects and variance beside them)
    b1, vb1 = np.zeros((q, max(k, 1)), order="F"), np.zeros(max(k, 1))
    check(_lib.lib().bwgr_uvbeta2(P._h, _dp(Zf), int(q), int(P.n), _dp(Yf), int(k), int(maxit), float(tol), float(df0), _dp(b1), _dp(b2), _dp(mu),
                                  _dp(h2), _dp(ve), _dp(vb1), _dp(vb2), _ip(its), _dp(cnv)))
    return dict(zip(UVB2_KEYS, (b1, b2, mu, h2, ve, vb1, vb2, its, cnv)))


def uvbeta2(Y, Z, X, maxit=100, tol=10e-7, df0=20.0, **kw):
    """solver2x for every column of Y (bwgr_uvbeta2): in each sweep the q columns of the dense design Z (n x q float64), then the markers of X,
    against one residual, each design with its own lambda; each trait on its own observed rows (NaN = missing), fp64.  Returns dict(b1 [q x k],
    b2 [p x k], mu, h2, ve, vb1, vb2, its, cnv).  X is a genotype matrix or a Panel."""
    with as_panel(X, **kw) as P:
        Ym, tol, df0 = _uvb_inputs(Y, P.n, 0, tol, df0, "uvbeta2")
        return _uvb2_panel(P, Ym, Z, maxit, tol, df0)


def solver2x(Y, X1, X2, maxit=100, tol=10e-7, df0=20.0, **kw):
    """solver2x(Y, X1, X2, maxit, tol, df0), src/RcppEigen20230423.cpp:1446-1493 (R/RcppExports.R:200): the vector (mu, b_1, b_2) of length
    1 + p1 + p2 of one trait.  X1 is the dense design (n x p1 float64) and X2 the genotypes or a Panel, which is how MEGA and GSEM call it; a
    dense X2 is not taken.  NaN rows of Y are treated as unobserved."""
    r = uvbeta2(np.asarray(Y, np.float64).reshape(-1), X1, X2, maxit, tol, df0, **kw)
    return np.concatenate([r["mu"][:1], r["b1"][:, 0], r["b2"][:, 0]])


def _mega_latent(Ym, G, npc, who):
    """LatentSpaces (:1530-1539) on G = X BETA: the centred records where observed and G where missing (GetImputedY, :1517-1528), each column
    divided by sqrt(sum Y2^2 / (n - 1)), then LS = (U diag(s)).leftCols(npc)."""
    w = ~np.isnan(Ym)
    Y2 = np.where(w, Ym - np.nanmean(Ym, 0), G)                      # :1519-1527
    Y2 = Y2 / np.sqrt((Y2 ** 2).sum(0) / (Ym.shape[0] - 1))          # :1533-1534
    return _sem_latent(Y2, npc, who)[0]


def _sem2(which, Y, X, npc, maxit, tol, df0, panel_kw):
    with as_panel(X, **panel_kw) as P:
        Ym, tol, df0 = _uvb_inputs(Y, P.n, 0, tol, df0, which)
        npc = _sem_npc(npc, min(Ym.shape), which)                    # (refused before anything runs)
        if which == "MEGA":
            empty = np.flatnonzero(~(~np.isnan(Ym)).any(0))
            if empty.size:
                raise BwgrError(1, "MEGA: trait %d has no record (its imputed column would be NaN)" % empty[0])
        BETA = _uvb_panel(P, Ym, 0, maxit, tol, df0)["b"]            # UVBETA(Y, X), :1545, :1585
        G = P.xb(BETA)
        if which == "MEGA":
            LS = _mega_latent(Ym, G, npc, which)                     # :1546
            LS_BETA = _uvb_panel(P, LS, 0, maxit, tol, df0)["b"]     # UVBETA(LS, X), :1547
        else:
            LS, V = _sem_latent(G, npc, which)                       # :1586-1589
        s = _uvb2_panel(P, Ym, LS, maxit, tol, df0)                  # solver2x per trait, :1553-1561, :1595-1603
        mu, b1, b2 = s["mu"], s["b1"], s["b2"]
        if which == "MEGA":
            b = LS_BETA @ b1 + b2                                    # :1563
            XB = P.xb(np.hstack([b2, b]))                            # X b2 and X b in one pass over the panel
            k = Ym.shape[1]
            hat = LS @ b1 + XB[:, :k] + mu                           # :1564, :1567
            gebv = XB[:, k:] + mu                                    # :1565, :1568
            return dict(zip(("mu", "b", "hat", "LS", "LS_BETA", "BETA1", "BETA2", "gebv"), (mu, b, hat, LS, LS_BETA, b1, b2, gebv)))
        b = BETA @ (V @ b1) + b2                                     # :1609 with V.leftCols(npc)
        hat = LS @ b1 + P.xb(b2) + mu                                # :1605-1606
        return dict(zip(("mu", "b", "hat"), (mu, b, hat)))


def MEGA(Y, X, npc=-1, *, maxit=100, tol=10e-7, df0=20.0, **kw):
    """MEGA(Y, X, npc), src/RcppEigen20230423.cpp:1542-1579 (R/RcppExports.R:208): UVBETA on the panel, the latent spaces LS of the records
    imputed with X BETA, UVBETA(LS, X), then solver2x(y, LS, X) per trait on its observed rows.  list(mu, b, hat, LS, LS_BETA, BETA1, BETA2,
    gebv) with b = LS_BETA BETA1 + BETA2.  maxit, tol, df0 are the solvers' (the reference has their defaults built in).  A trait without
    records is refused (the reference's imputed column is NaN there).  X is an array or a Panel."""
    return _sem2("MEGA", Y, X, npc, maxit, tol, df0, kw)


def GSEM(Y, X, npc=-1, *, maxit=100, tol=10e-7, df0=20.0, **kw):
    """GSEM(Y, X, npc), src/RcppEigen20230423.cpp:1582-1610 (R/RcppExports.R:212): UVBETA on the panel, LS = the first npc latent columns of
    X BETA, then solver2x(y, LS, X) per trait.  list(mu, b, hat) with b = BETA V.leftCols(npc) BETA1 + BETA2: the reference multiplies by the
    whole V (:1609), which is conformable only for npc = min(n, k), where the two agree.  A trait without records gives zero columns.  LS lies in X's span, so the reference's variance update can turn vb2 and
    lambda_2 negative and a trait's sweep can diverge; such a trait stops on its NaN convergence value with non-finite columns, as in the
    reference, and the others are not affected."""
    return _sem2("GSEM", Y, X, npc, maxit, tol, df0, kw)


def solver1x(Y, X, maxit=100, tol=10e-7, df0=20.0, **kw):
    """solver1x(Y, X, maxit, tol, df0), src/RcppEigen20230423.cpp:1410-1443 (R/RcppExports.R:196): the p effects of one ridge fit.  NaN rows
    of Y are treated as unobserved."""
    return uvbeta(np.asarray(Y, np.float64).reshape(-1), X, "D", maxit, tol, df0, **kw)["b"][:, 0]


def solver1xF(Y, X, maxit=100, tol=10e-7, df0=20.0, **kw):
    """solver1xF(Y, X, maxit, tol, df0), src/RcppEigen20230423.cpp:1613-1646 (R/RcppExports.R:216): solver1x on float inputs, with its test
    XX_j > 1e-5."""
    return uvbeta(np.asarray(Y, np.float64).reshape(-1), X, "F", maxit, tol, df0, **kw)["b"][:, 0]


def UVBETA(Y, X, **kw):
    """UVBETA(Y, X), src/RcppEigen20230423.cpp:1506-1515 (R/RcppExports.R:204): p x k, solver1x per trait on the trait's observed rows."""
    return uvbeta(Y, X, "D", **kw)["b"]


def FUVBETA(Y, X, **kw):
    """FUVBETA(Y, X), src/RcppEigen20230423.cpp:1709-1718 (R/RcppExports.R:224): p x k, solver1xF per trait."""
    return uvbeta(Y, X, "F", **kw)["b"]


def XFUVBETA(Y, X, **kw):
    """XFUVBETA(Y, X), src/RcppEigen20230423.cpp:1746-1753 (R/RcppExports.R:228): p x k, xsolver1xF per trait (lambda = mean XX_j).  A trait
    with no observed row gives a zero column (the reference has no such test there and returns NaN)."""
    return uvbeta(Y, X, "X", **kw)["b"]


def ZFUVBETA(Y, X, **kw):
    """ZFUVBETA(Y, X), src/RcppEigen20230423.cpp:1807-1816 (R/RcppExports.R:236): (p + 2) x k; row 0 is 1 - ve / vy, row 1 mu, then b."""
    r = uvbeta(Y, X, "Z", **kw)
    return np.vstack([r["h2"][None, :], r["mu"][None, :], r["b"]])
