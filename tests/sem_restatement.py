"""Line-cited numpy restatement of the latent-space fits (bWGR src/RcppEigen20230423.cpp) for the tests:

  XSEMF :1756-1769      ZSEMF :1819-1845      YSEMF :1848-1874

Written from those lines in float64 on top of uvb_restatement.uvbeta (XFUVBETA :1746-1753, ZFUVBETA :1807-1816), which takes a dense float64
design as well as genotypes, and numpy.linalg.svd for Eigen's BDCSVD with thin U and V (:1759).  The reference's programs are float
throughout; the library rounds Y (and tol, df0) to float once and runs every later stage in fp64 on unrounded intermediates, so the tests hand
this restatement the rounded Y and it rounds nothing else (uvb_restatement rounds tol and df0 itself for the float variants).  xsolver1xF and
zsolver1xF have maxit = 100, tol = 10e-7 and df0 = 20 built in (:1722-1723, :1772); here they are arguments, as in the library.

Every function returns the reference's list as a dict, in its order, and with it every intermediate: BETA (the first stage's dict), G, s, U,
V, Z, second (the second stage's dict) and, for YSEMF, third.  flip: a sequence of +-1, one per singular pair, applied to (U, V) -- the
outputs must not depend on it (tests/test_sem_cpu.py).
"""
import numpy as np

import uvb_restatement as UR


def n_components(npc, m):
    """:1760-1761 with m = svd.matrixU().cols() = min(n, k).  C's round() is half away from zero; (x + 1/2)^2 is never an integer, so 2 sqrt(m)
    never lies on a tie."""
    npc = int(npc)
    if npc < 0:
        npc = int(np.floor(2.0 * np.sqrt(m) + 0.5))                  # :1760
    if npc == 0:
        npc += m                                                     # :1761
    if npc > m:
        raise ValueError("npc = %d exceeds min(n, k) = %d (leftCols would leave the matrix)" % (npc, m))
    return npc


def latent(G, npc, flip=None):
    """:1759-1762 -> dict(s, U, V, Z, npc); U, V thin, Z = (U diag(s)).leftCols(npc)."""
    U, s, Vt = np.linalg.svd(np.asarray(G, np.float64), full_matrices=False)   # :1759
    V = Vt.T
    if flip is not None:
        f = np.asarray(flip, np.float64)
        U, V = U * f, V * f
    npc = n_components(npc, s.shape[0])
    return dict(s=s, U=U, V=V, Z=(U * s)[:, :npc], npc=npc)                     # :1762


def gc(G):
    """:1765-1768: dict(hat = the columns centred and divided by their population sd, GC).  A zero column gives 0 / 0 = NaN, as there."""
    G = np.array(G, np.float64, copy=True)
    N = G.shape[0]
    G -= G.mean(0)                                                   # :1765
    with np.errstate(all="ignore"):
        vg = np.sqrt((G ** 2).sum(0) / N)                            # :1766
        G = G / vg                                                   # :1767
        return dict(hat=G, GC=(G.T @ G) / N)                         # :1768


def _matrix(Y):
    Y = np.asarray(Y, np.float64)
    return Y[:, None] if Y.ndim == 1 else Y


def XSEMF(Y, X, npc=0, maxit=100, tol=10e-7, df0=20.0, flip=None):
    Y, X = _matrix(Y), np.asarray(X, np.float64)
    BETA = UR.uvbeta(Y, X, "X", maxit, tol, df0)                     # :1757
    G = X @ BETA["b"]                                                # :1758
    L = latent(G, npc, flip)
    second = UR.uvbeta(Y, L["Z"], "X", maxit, tol, df0)              # :1763 ALPHA
    b = BETA["b"] @ L["V"][:, :L["npc"]] @ second["b"]               # :1764
    g = gc(X @ b)
    out = dict(b=b, GC=g["GC"], hat=g["hat"])                        # :1769
    out.update(BETA=BETA, G=G, second=second, **L)
    return out


def _zfit(Y, X, npc, maxit, tol, df0, flip):
    BETA = UR.uvbeta(Y, X, "Z", maxit, tol, df0)                     # :1821, :1850
    G = X @ BETA["b"]                                                # :1822, :1851
    L = latent(G, npc, flip)
    second = UR.uvbeta(Y, L["Z"], "Z", maxit, tol, df0)              # :1828 Coef, :1856 ALPHA
    b = BETA["b"] @ L["V"][:, :L["npc"]] @ second["b"]               # :1830, :1857
    return BETA, G, L, second, b


def ZSEMF(Y, X, npc=0, maxit=100, tol=10e-7, df0=20.0, flip=None):
    Y, X = _matrix(Y), np.asarray(X, np.float64)
    BETA, G, L, second, b = _zfit(Y, X, npc, maxit, tol, df0, flip)
    G2 = X @ b                                                       # :1831
    out = dict(mu=second["mu"], b=b, hat=G2 + second["mu"], h2=second["h2"], GC=gc(G2)["GC"])   # :1832-1845
    out.update(BETA=BETA, G=G, second=second, **L)
    return out


def YSEMF(Y, X, npc=-1, maxit=100, tol=10e-7, df0=20.0, flip=None):
    Y, X = _matrix(Y), np.asarray(X, np.float64)
    BETA, G, L, second, b_fa = _zfit(Y, X, npc, maxit, tol, df0, flip)
    G_fa = X @ b_fa                                                  # :1858
    third = UR.uvbeta(Y - G_fa, X, "Z", maxit, tol, df0)             # :1859 beta_Xd
    b = b_fa + third["b"]                                            # :1860
    G2 = X @ b                                                       # :1861
    out = dict(mu=third["mu"], b=b, hat=G2 + third["mu"], h2=second["h2"] + third["h2"], GC=gc(G2)["GC"])   # :1862-1874
    out.update(BETA=BETA, G=G, second=second, third=third, b_fa=b_fa, G_fa=G_fa, **L)
    return out
