"""mrr_svd: the multi-trait fit in the principal components of the marker panel, and the transpose product X'A it maps back with
(bwgr_mrr_svd_fit, bwgr_panel_xta, bwgr_debug_xta_plan; include/bwgr.h).  Reached as bwgr_amd.svd.NAME."""
import ctypes as C
import sys

import numpy as np

from . import _lib
from ._lib import BwgrError, check
from ._marshal import HOST, DEVICE, _dp, _vp, _is_device_tensor, _matrix, _plan
from .kernels import _kernel_input
from .panel import Panel, as_panel

WMODEL_KEYS = ("Intercepts", "MarkerEffects", "FittedValues", "Heritability", "WCorrelations", "VarBeta", "VarResiduals", "ConvergenceBeta",
               "ConvergenceH2", "ConvergenceVar", "NumOfIterations")
XTA_PLAN_FIELDS = ("groups", "cols_wg", "cols_wave", "grid", "trips", "lds_bytes", "row_tile", "tiles", "ws_bytes")


def xta_plan(n, p, k, slab_rows):
    """bwgr_debug_xta_plan (host arithmetic, no GPU) of panel_xta for n rows, p columns, k columns of A and slabs of slab_rows rows: the trait
    groups, the columns a workgroup and a wave own, the grid, the column blocks a workgroup takes at most, the LDS bytes, the rows of a tile,
    the tiles and the device workspace."""
    return _plan("bwgr_debug_xta_plan", XTA_PLAN_FIELDS, n, p, k, slab_rows)


def _int8_input(X, who):
    """X under the relationship kernels' rules (kernels._kernel_input): a Panel, an int8 device tensor or an integer matrix within -128..127.
    dense(X) and fp32 panels are refused in `who`'s name before the library is touched."""
    from .mtfit import dense
    if isinstance(X, dense):
        raise BwgrError(1, "%s: dense(W) designs are not supported; W must be an int8 panel (integer genotypes in -128..127)" % who)
    try:
        X, p = _kernel_input(X)
    except ValueError as e:
        raise BwgrError(1, "%s: %s" % (who, e)) from None
    if isinstance(X, np.ndarray) and X.ndim != 2:
        raise BwgrError(1, "%s: W has shape %s; it must be n x p" % (who, X.shape))
    return X


def panel_xta(X, A, centre=True, *, device_out=False, **panel_kw):
    """X'A (centre=False) or X_c'A with X_c = X - 1 xbar' (centre=True) on the int8 genotypes, p x k float64 (bwgr_panel_xta): marker effects
    from row coefficients.  X is a Panel or what makes an int8 one; A is n x k or a vector of n.  A numpy A is passed from the host and the
    result is a numpy array; a CUDA tensor stays on the device, and so does its result (device_out=True asks for a tensor from a numpy A too)."""
    X = _int8_input(X, "panel_xta")
    if not _is_device_tensor(A) and not hasattr(X, "data_ptr"):      # (a shape that cannot fit is refused before the library is touched)
        _matrix(A, "panel_xta", X.n if isinstance(X, Panel) else X.shape[0], what="A")
    with as_panel(X, **panel_kw) as P:
        L = _lib.lib()
        if _is_device_tensor(A):
            import torch
            At = A.to(torch.float64)
            if At.dim() == 1:
                At = At[:, None]
            if At.dim() != 2 or At.shape[0] != P.n:
                raise BwgrError(1, "panel_xta: A has shape %s; nrow(A) must equal nrow(X) = %d" % (tuple(At.shape), P.n))
            if (At.device.index or 0) != P.device:
                raise BwgrError(1, "panel_xta: A is on device %d, the panel on device %d" % (At.device.index or 0, P.device))
            k = int(At.shape[1])
            if k < 1:
                raise BwgrError(1, "panel_xta: A has no columns")
            if At.stride(0) != 1 or (k > 1 and At.stride(1) < P.n):
                At = At.t().contiguous().t()
            lda = int(At.stride(1)) if k > 1 else P.n
            out = torch.empty((k, P.p), dtype=torch.float64, device=At.device).t()          # p x k, column-major
            torch.cuda.synchronize(At.device)
            check(L.bwgr_panel_xta(P._h, C.c_void_p(At.data_ptr()), lda, k, int(bool(centre)), DEVICE, C.c_void_p(out.data_ptr()), P.p))
            torch.cuda.synchronize(At.device)
            return out
        Am = _matrix(A, "panel_xta", P.n, what="A")
        if Am.shape[1] < 1:
            raise BwgrError(1, "panel_xta: A has no columns")
        Af = np.asfortranarray(Am)
        out = np.zeros((P.p, Af.shape[1]), order="F")
        check(L.bwgr_panel_xta(P._h, _vp(Af), P.n, Af.shape[1], int(bool(centre)), HOST, _vp(out), P.p))
        if device_out:
            torch = sys.modules.get("torch")
            if torch is None:
                raise RuntimeError("device_out=True: import torch before calling (the result is a torch tensor)")
            return torch.from_numpy(out.T.copy()).to("cuda:%d" % P.device).t()
        return out


def rank_threshold(n, p):
    """The rank rule's factor: a direction is kept when lambda_i > lambda_1 (max(n, p) 2^-24)^2 -- numpy's matrix_rank rule at the precision of
    the reference's float SVD, written for the eigenvalues of W_c W_c'."""
    return (max(int(n), int(p)) * 2.0 ** -24) ** 2


def svd_design(W, **panel_kw):
    """The design of mrr_svd: dict(X, d, U, xbar_free=True) with X = U diag(d) (n x r float64, column-major), d the r singular values of the centred
    marker matrix W_c = W - 1 xbar' in decreasing order and U its left singular vectors.  G = W W' is formed exactly on the int8 matrix cores
    (Panel.crossprod), double-centred in fp64 from the exact integers (G_ij - rs_i / n - rs_j / n + tot / n^2 = W_c W_c'), and decomposed by
    eigh; d = sqrt(lambda).  r counts the lambda_i > lambda_1 (max(n, p) 2^-24)^2 (rank_threshold).  When torch is imported, everything runs on
    the panel's device (torch.linalg.eigh) and X, d, U are tensors there; else numpy.linalg.eigh on the host.  xbar_free: the columns of X sum
    to zero up to rounding, so the fit's explicit centring changes nothing."""
    W = _int8_input(W, "svd_design")
    torch = sys.modules.get("torch")
    with as_panel(W, **panel_kw) as P:
        n, p = P.n, P.p
        G = P.crossprod(device_out=torch is not None)
    thr = rank_threshold(n, p)
    if torch is not None:
        Gf = G.to(torch.float64)                       # exact: |G_ij| <= 2^14 p < 2^53 for every panel
        rs = G.sum(1).to(torch.float64)
        tot = float(G.sum())
        Gc = Gf - rs[:, None] / n - rs[None, :] / n + tot / (float(n) * float(n))
        w, V = torch.linalg.eigh((Gc + Gc.t()) * 0.5)
        w, V = torch.flip(w, (0,)), torch.flip(V, (1,))
        r = int((w > w[0] * thr).sum()) if float(w[0]) > 0 else 0
        d = torch.sqrt(w[:r])
        U = V[:, :r].t().contiguous().t()
        X = (U * d).t().contiguous().t()
    else:
        Gf = G.astype(np.float64)
        rs = G.sum(1).astype(np.float64)
        tot = float(G.sum())
        Gc = Gf - rs[:, None] / n - rs[None, :] / n + tot / (float(n) * float(n))
        w, V = np.linalg.eigh((Gc + Gc.T) * 0.5)
        w, V = w[::-1], V[:, ::-1]
        r = int(np.sum(w > w[0] * thr)) if w[0] > 0 else 0
        d = np.sqrt(w[:r])
        U = np.asfortranarray(V[:, :r])
        X = np.asfortranarray(U * d)
    if r < 1:
        raise BwgrError(1, "svd_design: the centred marker matrix has rank 0 (every column of W is constant)")
    return dict(X=X, d=d, U=U, xbar_free=True)


def mrr_svd_fit(Y, X, *, maxit=500, tol=10e-9, verbose=False, device=0):
    """bwgr_mrr_svd_fit: mrr_svd's Gauss-Seidel (src/RcppEigen20230423.cpp:1103-1243) on a given n x r design -- a numpy matrix, or a CUDA tensor,
    which stays on the device.  Y is n x k (NaN = missing) or a vector, taken as it is.  dict(mu, b, hat, h2, GC, vb, ve, cnvB, cnvH2, cnvV,
    Its); b holds the effects of X's columns."""
    if _is_device_tensor(X):
        import torch
        Xd = X.to(torch.float64)
        if Xd.dim() != 2:
            raise BwgrError(1, "mrr_svd_fit: X has shape %s; it must be n x r" % (tuple(Xd.shape),))
        if Xd.stride(0) != 1 or (Xd.shape[1] > 1 and Xd.stride(1) < Xd.shape[0]):
            Xd = Xd.t().contiguous().t()
        n, r = int(Xd.shape[0]), int(Xd.shape[1])
        ldx = int(Xd.stride(1)) if r > 1 else n
        device = Xd.device.index or 0
        torch.cuda.synchronize(Xd.device)
        xptr, loc = C.c_void_p(Xd.data_ptr()), DEVICE
    else:
        Xh = np.asfortranarray(np.asarray(X, np.float64))
        if Xh.ndim != 2:
            raise BwgrError(1, "mrr_svd_fit: X has shape %s; it must be n x r" % (Xh.shape,))
        n, r = Xh.shape
        ldx, xptr, loc = n, _vp(Xh), HOST
    Yf = np.asfortranarray(_matrix(Y, "mrr_svd_fit", n))
    k = Yf.shape[1]
    kk, sweeps = max(k, 1), max(int(maxit), 1)
    outs = (np.zeros(kk), np.zeros((max(r, 1), kk), order="F"), np.zeros((max(n, 1), kk), order="F"), np.zeros(kk), np.zeros((kk, kk), order="F"),
            np.zeros((kk, kk), order="F"), np.zeros(kk), np.zeros(sweeps), np.zeros(sweeps), np.zeros(sweeps))
    its = C.c_int()
    check(_lib.lib().bwgr_mrr_svd_fit(int(device), xptr, loc, int(n), int(r), int(ldx), _dp(Yf), k, int(maxit), float(tol), int(bool(verbose)),
                                      *[_dp(a) for a in outs], C.byref(its)))
    n_it = int(its.value)
    names = ("mu", "b", "hat", "h2", "GC", "vb", "ve", "cnvB", "cnvH2", "cnvV")
    return dict(zip(names + ("Its",), outs[:7] + tuple(c[:n_it].copy() for c in outs[7:]) + (n_it,)))


def mrr_svd(Y, W, *, maxit=500, tol=10e-9, verbose=False, device_out=False, **panel_kw):
    """mrr_svd(Y, W), src/RcppEigen20230423.cpp:1083-1260 (R/RcppExports.R:188): the multi-trait ridge fit by Gauss-Seidel on the principal
    components of the centred marker matrix, mapped back to marker effects.  Y is n x k (NaN = missing), rounded to float once as the reference
    receives it; W is a Panel or what makes an int8 one.  Returns the reference's list as a dict in its order (WMODEL_KEYS): Intercepts,
    MarkerEffects (p x k), FittedValues (n x k), Heritability, WCorrelations, VarBeta, VarResiduals, the three convergence traces and
    NumOfIterations.  The flow: svd_design(W); bwgr_mrr_svd_fit on X = U diag(d), device-resident where it was made there; MarkerEffects =
    W_c'(U (b / d)) by panel_xta, since V = W_c'U diag(1/d) is never formed (device_out=True leaves them on the device).
    Departures: the decomposition is an fp64 eigh of the exact Gram matrix, not a float SVD, and everything after Y's rounding is fp64; the
    directions below the rank rule (svd_design) are dropped, where the reference keeps them at noise scale (K2X's departure); no output depends
    on the eigensolver's signs.  dense(W) and fp32 panels are refused; a non-integer W is out of scope."""
    W = _int8_input(W, "mrr_svd")
    n = W.n if isinstance(W, Panel) else int(W.shape[1] if hasattr(W, "data_ptr") else W.shape[0])
    Yf = _matrix(Y, "mrr_svd", None, True)
    if Yf.ndim != 2 or (not hasattr(W, "data_ptr") and Yf.shape[0] != n):
        raise BwgrError(1, "mrr_svd: Y has shape %s; nrow(Y) must equal nrow(W) = %d" % (Yf.shape, n))
    with as_panel(W, **panel_kw) as P:
        if Yf.shape[0] != P.n:
            raise BwgrError(1, "mrr_svd: Y has shape %s; nrow(Y) must equal nrow(W) = %d" % (Yf.shape, P.n))
        D = svd_design(P)
        f = mrr_svd_fit(Yf, D["X"], maxit=maxit, tol=tol, verbose=verbose, device=P.device)
        if _is_device_tensor(D["U"]):
            import torch
            coef = D["U"] @ (torch.from_numpy(f["b"]).to(D["U"].device) / D["d"][:, None])
            beta = panel_xta(P, coef, centre=True)
            if not device_out:
                beta = beta.cpu().numpy()
        else:
            beta = panel_xta(P, D["U"] @ (f["b"] / D["d"][:, None]), centre=True, device_out=device_out)
    vals = (f["mu"], beta, f["hat"], f["h2"], f["GC"], f["vb"], f["ve"], f["cnvB"], f["cnvH2"], f["cnvV"], f["Its"])
    return dict(zip(WMODEL_KEYS, vals))
