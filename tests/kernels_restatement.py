"""float64 restatement (numpy) of the reference's relationship kernels: GAU / GRM (src/Rcpp20260726ai.cpp:1338-1383) and EigenARC / EigenGAU /
EigenGRM (src/RcppEigen20230423.cpp:8-51).  The reference computes in float; as for mrr, the library returns the fp64 value of the
reference's formulas and parity is against this file.  Reference quirks are kept: GRM's Code012 divides by sum_j mean_j^2 / 2 (not sum 2pq),
EigenARC uses the literals 3.1416 and 1.001, EigenGRM adds 1 to the diagonal before it normalises.

G = X X' is an int64 matmul; the centred product comes either from the centring identity (what the library uses) or directly."""
import numpy as np


def int_matmul(A, B):
    """A B' of integer matrices as int64, through the float64 product: every partial sum is an integer below 2^53 (asserted), so each is
    exact in any order of summation and the result is the int64 product's, at BLAS speed"""
    A, B = np.asarray(A), np.asarray(B)
    assert float(np.abs(A).max(initial=0)) * float(np.abs(B).max(initial=0)) * A.shape[1] < 2.0 ** 53
    return np.rint(A.astype(np.float64) @ B.astype(np.float64).T).astype(np.int64)


def crossprod(X):
    return int_matmul(X, X)


def zz_identity(X):
    """ZZ' with Z = X - 1 m' from G, s and X s:  G_ii' - r_i - r_i' + c,  r = X s / n,  c = s.s / n^2."""
    Xi = np.asarray(X).astype(np.int64)
    n = Xi.shape[0]
    G = crossprod(X)
    s = Xi.sum(0)
    r = (Xi @ s).astype(np.float64) / n
    c = float(np.sum((s.astype(np.float64) / n) ** 2))
    return G.astype(np.float64) - (r[:, None] + r[None, :]) + c


def zz_direct(X):
    Xf = np.asarray(X).astype(np.float64)
    Z = Xf - Xf.mean(0)
    return Z @ Z.T


def _d2(G):
    d = np.diag(G)
    return (d[:, None] + d[None, :] - 2 * G).astype(np.float64)     # exact: integers


def GRM(X, Code012=False):
    Xi = np.asarray(X).astype(np.int64)
    n = Xi.shape[0]
    s = Xi.sum(0).astype(np.float64)
    q = (Xi * Xi).sum(0).astype(np.float64)
    m = s / n
    if Code012:
        D = float(np.sum(m * m / 2.0))
    else:
        D = float(np.sum((q - s * s / n) / (n - 1.0)))
    return zz_identity(X) / D


def GAU(X):
    G = crossprod(X)
    n = G.shape[0]
    d2 = _d2(G)
    md = float(d2.sum()) / (n * (n - 1.0))          # the diagonal of d2 is zero: the off-diagonal mean
    return np.exp(-d2 / md)


def EigenGRM(X, centralizeZ=True):
    A = zz_identity(X) if centralizeZ else crossprod(X).astype(np.float64)
    A = A.copy()
    A[np.diag_indices_from(A)] += 1.0
    return A * (1.0 / np.mean(np.diag(A)))


def EigenGAU(X, phi=1.0):
    G = crossprod(X)
    n = G.shape[0]
    d = np.sqrt(_d2(G))
    np.fill_diagonal(d, 0.0)
    t = phi * (-(n * (n - 1.0))) / d.sum()
    return np.exp(t * d)


def EigenARC(X, centralizeX=True):
    A = zz_identity(X) if centralizeX else crossprod(X).astype(np.float64)
    A = A * (1.0 / np.mean(np.diag(A)))
    dg = np.diag(A)
    N = np.sqrt(dg[:, None] * dg[None, :] * 1.001)
    th = np.arccos(A / N)
    return N / 3.1416 * (np.sin(th) + (3.1416 - th) * np.cos(th))


def scaled_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (den if den > 0 else 1.0))


KINDS = [("GRM", {"Code012": False}), ("GRM", {"Code012": True}), ("GAU", {}), ("EigenGRM", {"centralizeZ": True}), ("EigenGRM", {"centralizeZ": False}),
         ("EigenGAU", {"phi": 1.0}), ("EigenGAU", {"phi": 0.5}), ("EigenARC", {"centralizeX": True}), ("EigenARC", {"centralizeX": False})]


def restate(name, X, **kw):
    return {"GRM": GRM, "GAU": GAU, "EigenGRM": EigenGRM, "EigenGAU": EigenGAU, "EigenARC": EigenARC}[name](X, **kw)
