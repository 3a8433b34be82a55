"""The relationship kernels: GRM, GAU, EigenGRM / EigenGAU / EigenARC, the exact integer products, and the founder-by-sample kernels EigenArcZ /
EigenGauZ (bwgr_panel_kernel*, bwgr_panel_crossprod*)."""
import contextlib
import numpy as np

from .panel import Panel, as_panel, KERNELS, KERNELS2  # noqa: F401  (the kinds of Panel.kernel and Panel.kernel2 are this family's)


# ---- relationship kernels: GRM / GAU (R/RcppExports.R:100-106), EigenARC / EigenGAU / EigenGRM (:140-150) ----
def _kernel_input(X):
    """(X as what Panel() takes for an int8 panel, its number of columns), without touching the library: a Panel, an int8 device tensor, or an
    int8 numpy matrix.  A float matrix must hold integers in -128..127; float panels are out of scope."""
    if isinstance(X, Panel):
        return X, X.p
    if hasattr(X, "data_ptr"):
        if "int8" not in str(X.dtype):
            raise ValueError("relationship kernels take int8 genotypes; got a %s tensor" % (X.dtype,))
        return X, int(X.shape[0])      # (p, ldx): row j = marker j
    X = np.asarray(X)
    if X.dtype != np.int8:
        if not (X.size and np.all(np.isfinite(X)) and np.all(X == np.rint(X)) and X.min() >= -128 and X.max() <= 127):
            raise ValueError("relationship kernels take integer genotypes in -128..127 (the int8 panel); float panels are not supported")
        X = X.astype(np.int8)
    return X, (int(X.shape[1]) if X.ndim == 2 else -1)


def _kernel_panel(X, panel_kw):
    """X as an int8 panel.  The int8 product is the feature: the input is checked (_kernel_input) before the library is touched."""
    return as_panel(_kernel_input(X)[0], **panel_kw)


def _kernel(kind, X, par, flag, device_out, panel_kw):
    with _kernel_panel(X, panel_kw) as P:
        return P.kernel(kind, par, flag, device_out=device_out)


def GRM(X, Code012=False, *, device_out=False, **kw):
    """GRM(X, Code012), src/Rcpp20260726ai.cpp:1363-1383: ZZ' / sum_j var(x_j) (Code012: / sum_j mean_j^2 / 2, as written there)."""
    return _kernel("GRM", X, 1.0, Code012, device_out, kw)


def GAU(X, *, device_out=False, **kw):
    """GAU(X), src/Rcpp20260726ai.cpp:1338-1360: exp(-d2 / mean off-diagonal d2)."""
    return _kernel("GAU", X, 1.0, False, device_out, kw)


def EigenGRM(X, centralizeZ=True, cores=1, *, device_out=False, **kw):
    """EigenGRM(X, centralizeZ, cores), src/RcppEigen20230423.cpp:41-51 (cores is accepted and ignored)."""
    return _kernel("EigenGRM", X, 1.0, centralizeZ, device_out, kw)


def EigenGAU(X, phi=1.0, cores=1, *, device_out=False, **kw):
    """EigenGAU(X, phi, cores), src/RcppEigen20230423.cpp:29-38 (cores is accepted and ignored)."""
    return _kernel("EigenGAU", X, phi, False, device_out, kw)


def EigenARC(X, centralizeX=True, cores=1, *, device_out=False, **kw):
    """EigenARC(X, centralizeX, cores), src/RcppEigen20230423.cpp:8-26 (cores is accepted and ignored)."""
    return _kernel("EigenARC", X, 1.0, centralizeX, device_out, kw)


def crossprod(X, *, device_out=False, **kw):
    """The exact X X' of integer genotypes, n x n int64 (no reference counterpart of its own: the product inside the five kernels)."""
    with _kernel_panel(X, kw) as P:
        return P.crossprod(device_out=device_out)


# ---- founder-by-sample kernels: EigenArcZ / EigenGauZ (R/RcppExports.R:248-254) ----
@contextlib.contextmanager
def _panels2(Xf, Xs, who, panel_kw):
    """The founders' and the samples' int8 panels of one call, from Panels or matrices under _kernel_panel's rules.  Both inputs are checked,
    their column counts compared, before the library is touched; the same matrix on both sides makes one panel."""
    same = Xs is Xf
    Xf, pf = _kernel_input(Xf)
    Xs, ps = (Xf, pf) if same else _kernel_input(Xs)
    if pf != ps:
        raise ValueError("%s: the founders have %d columns (markers), the samples %d" % (who, pf, ps))
    made = []

    def panel(X):
        if not isinstance(X, Panel):
            X = Panel(X, **panel_kw)
            made.append(X)
        return X
    try:
        Pf = panel(Xf)
        yield Pf, (Pf if same else panel(Xs))
    finally:
        for P in made:      # (in the order they were made)
            P.close()


def crossprod2(Xf, Xs, *, device_out=False, **kw):
    """The exact X_f X_s' of integer genotypes over the same markers, n_f x n_s int64 (the product inside EigenArcZ / EigenGauZ)."""
    with _panels2(Xf, Xs, "crossprod2", kw) as (Pf, Ps):
        return Pf.crossprod2(Ps, device_out=device_out)


def _kernel2z(kind, Zfndr, Zsamp, par, parts, who, panel_kw):
    with _panels2(Zfndr, Zsamp, who, panel_kw) as (Pf, Ps):
        Kff, Kfs = Pf.kernel2(Ps, kind, par)
    w, V = np.linalg.eigh(Kff)          # ascending, the order of Eigen's SelfAdjointEigenSolver
    Z = Kfs.T @ (V / np.sqrt(w))
    if parts:
        return {"Z": Z, "Kff": Kff, "Kfs": Kfs, "values": w, "vectors": V}
    return Z


def EigenArcZ(Zfndr, Zsamp, cores=1, *, parts=False, **kw):
    """EigenArcZ(Zfndr, Zsamp, cores), src/RcppEigen20230423.cpp:1877-1907 (cores is accepted and ignored): the samples' coordinates
    Kfs' V L^(-1/2) in the founders' arc-cosine kernel, n_s x n_f float64.  The library makes Kff and Kfs (Panel.kernel2); the
    eigendecomposition Kff = V L V' is numpy's, on the host in fp64, eigenvalues ascending.  The columns of Z are defined up to sign, and up
    to rotation inside close eigenvalues; Z Z' is not affected.  parts=True returns dict(Z, Kff, Kfs, values, vectors)."""
    return _kernel2z("ARC", Zfndr, Zsamp, 1.0, parts, "EigenArcZ", kw)


def EigenGauZ(Zfndr, Zsamp, phi=1.0, cores=1, *, parts=False, **kw):
    """EigenGauZ(Zfndr, Zsamp, phi, cores), src/RcppEigen20230423.cpp:1910-1939 (cores is accepted and ignored): the samples' coordinates
    Kfs' V L^(-1/2) in the founders' Gaussian kernel exp(D t), n_s x n_f float64.  The library makes Kff and Kfs (Panel.kernel2); the
    eigendecomposition Kff = V L V' is numpy's, on the host in fp64, eigenvalues ascending.  The columns of Z are defined up to sign, and up
    to rotation inside close eigenvalues; Z Z' is not affected.  parts=True returns dict(Z, Kff, Kfs, values, vectors)."""
    return _kernel2z("GAU", Zfndr, Zsamp, phi, parts, "EigenGauZ", kw)
