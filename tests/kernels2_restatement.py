"""float64 restatement (numpy) of the reference's founder-by-sample kernels EigenArcZ / EigenGauZ (src/RcppEigen20230423.cpp:1877-1939).  The
reference computes in float; the library returns the fp64 value of the reference's formulas and parity is against this file.  Reference
quirks are kept: the literals 3.14159 (not EigenARC's 3.1416) and 1.001, the founders' column means centre BOTH matrices under ARC, and
Kscalar is taken from the finished diagonal of K_ff.

G_ff = X_f X_f' and G_fs = X_f X_s' are int64 matmuls; the centred products come either from the centring identity (what the library uses)
or directly."""
import numpy as np

from kernels_restatement import int_matmul

NPI = 3.14159


def crossprod2(Xf, Xs):
    return int_matmul(Xf, Xs)


def arc_centred_direct(Xf, Xs):
    """(A_ff, A_fs, d_s): both matrices centred by the founders' column means, then multiplied."""
    F, S = np.asarray(Xf).astype(np.float64), np.asarray(Xs).astype(np.float64)
    m = F.mean(0)
    Zf, Zs = F - m, S - m
    return Zf @ Zf.T, Zf @ Zs.T, (Zs * Zs).sum(1)


def arc_centred_identity(Xf, Xs):
    """The same from the exact integers: s = X_f' 1, m = s / n_f, r_f = X_f s / n_f, r_s = X_s s / n_f, c = sum m^2, q_s = rowsums(X_s^2):
    A_ff = G_ff - (r_f,i + r_f,i') + c,  A_fs = G_fs - r_f,i - r_s,j + c,  d_s,j = q_s,j - 2 r_s,j + c."""
    Fi, Si = np.asarray(Xf).astype(np.int64), np.asarray(Xs).astype(np.int64)
    nf = Fi.shape[0]
    s = Fi.sum(0)
    rf = (Fi @ s).astype(np.float64) / nf
    rs = (Si @ s).astype(np.float64) / nf
    c = float(np.sum((s.astype(np.float64) / nf) ** 2))
    qs = (Si * Si).sum(1).astype(np.float64)
    Aff = int_matmul(Fi, Fi).astype(np.float64) - (rf[:, None] + rf[None, :]) + c
    Afs = int_matmul(Fi, Si).astype(np.float64) - rf[:, None] - rs[None, :] + c
    return Aff, Afs, qs - 2.0 * rs + c


def _arc(A, da, db):
    N = np.sqrt(da[:, None] * db[None, :] * 1.001)
    th = np.arccos(A / N)
    return N * (np.sin(th) + (NPI - th) * np.cos(th)) / NPI


def arc_kernels(Xf, Xs, direct=False):
    """(K_ff, K_fs) of EigenArcZ, :1881-1902"""
    Aff, Afs, ds = (arc_centred_direct if direct else arc_centred_identity)(Xf, Xs)
    df = np.diag(Aff).copy()
    Kff = _arc(Aff, df, df)
    Kfs = _arc(Afs, df, ds)
    kscalar = 1.0 / np.mean(np.diag(Kff))
    return Kff * kscalar, Kfs * kscalar


def gau_kernels(Xf, Xs, phi=1.0):
    """(K_ff, K_fs) of EigenGauZ, :1914-1934; n_f (n_f - 1) in double"""
    Fi, Si = np.asarray(Xf).astype(np.int64), np.asarray(Xs).astype(np.int64)
    nf = Fi.shape[0]
    Gff, Gfs = int_matmul(Fi, Fi), int_matmul(Fi, Si)
    dff = np.diag(Gff)
    qs = (Si * Si).sum(1)
    Dfs = np.sqrt((dff[:, None] + qs[None, :] - 2 * Gfs).astype(np.float64))     # exact integers under the root
    Dff = np.sqrt((dff[:, None] + dff[None, :] - 2 * Gff).astype(np.float64))
    np.fill_diagonal(Dff, 0.0)
    t = phi * (-(nf * (nf - 1.0))) / Dff.sum()
    return np.exp(Dff * t), np.exp(Dfs * t)


def kernels(kind, Xf, Xs, phi=1.0):
    return arc_kernels(Xf, Xs) if kind == "ARC" else gau_kernels(Xf, Xs, phi)


def coordinates(Kff, Kfs):
    """Z = K_fs' V L^(-1/2), eigenvalues ascending (:1904-1906)"""
    w, V = np.linalg.eigh(Kff)
    return Kfs.T @ (V / np.sqrt(w))


def EigenArcZ(Zfndr, Zsamp):
    return coordinates(*arc_kernels(Zfndr, Zsamp))


def EigenGauZ(Zfndr, Zsamp, phi=1.0):
    return coordinates(*gau_kernels(Zfndr, Zsamp, phi))
