"""MLM: the multi-trait fit with fixed effects, Z projected off X, and the projection on its own (bwgr_mlm, bwgr_project, bwgr_debug_mlm_plan;
include/bwgr.h).  Reached as bwgr_amd.mlm.NAME."""
import ctypes as C
import sys

import numpy as np

from . import _lib
from ._lib import BwgrError, check
from ._marshal import HOST, DEVICE, _dp, _vp, _is_device_tensor, _matrix, _plan
from .kernels import _kernel_input
from .mtfit import dense
from .panel import Panel, as_panel

MLM_KEYS = ("b", "u", "hat", "h2", "GC", "vb", "ve", "cnv", "its")
MLM_PLAN_FIELDS = ("ld", "nblk", "edge", "tiles", "pass_wg", "trips", "cols_wg", "hat_wg", "linv_lds", "ngl", "lds_gram", "lds_pass", "lds_solve", "lds_linv",
                   "train_bytes", "proj_blocks", "proj_row_wg", "proj_trips", "f_pieces", "f_piece", "proj_lds", "ztx_groups", "proj_bytes", "ws_bytes")
F_MAX = 256


def mlm_plan(n, p, f, k, npat):
    """bwgr_debug_mlm_plan (host arithmetic, no GPU) of MLM for n rows, p columns of Z, f covariates, k traits and npat missingness patterns:
    the dense train's plan on the projected Z (mrr_dense_plan's fields, its workspace as train_bytes), the projection's grid (64-column
    blocks x row-tile workgroups) and the row tiles one workgroup takes at most, the f-pieces and their length, the LDS bytes of the
    projection, the trait groups of Z'X, the bytes the projection adds, and the whole device workspace -- the n p 8-byte fp64 copy of the
    projected Z included: 2 GB at 5 000 x 50 000, 80 GB at 10 000 x 1 000 000."""
    return _plan("bwgr_debug_mlm_plan", MLM_PLAN_FIELDS, n, p, f, k, npat)


def _source(Z, who):
    """Z as the entries take it: ("dense", dense(Z)) or ("panel", what makes an int8 panel), decided without touching the library.  A float
    matrix with a non-integer value is refused: mark it dense(Z)."""
    if isinstance(Z, dense):
        return "dense", Z
    if isinstance(Z, Panel):
        return "panel", Z
    try:
        Zi, _ = _kernel_input(Z)
    except ValueError:
        raise BwgrError(1, "%s: Z is a Panel, an integer matrix within -128..127 (the int8 panel) or dense(Z); a real-valued Z must be marked dense(Z)" % who) from None
    if isinstance(Zi, np.ndarray) and Zi.ndim != 2:
        raise BwgrError(1, "%s: Z has shape %s; it must be n x p" % (who, Zi.shape))
    return "panel", Zi


def _rows(kind, Z):
    """the rows of Z where they are known before a panel is made (else None)"""
    if kind == "dense":
        Zd = Z.device_tensor()
        return int(Zd.shape[0]) if Zd is not None else Z.Z.shape[0]
    if isinstance(Z, Panel):
        return Z.n
    return None if hasattr(Z, "data_ptr") else Z.shape[0]


def _covariates(X, who, n, single):
    """X as an n x f float64 column-major matrix (a vector is one column); 1 <= f <= 256"""
    Xm = _matrix(X, who, None, single, what="X")
    if Xm.ndim != 2:
        raise BwgrError(1, "%s: X has shape %s; it must be n x f" % (who, Xm.shape))
    if n is not None and Xm.shape[0] != n:
        raise BwgrError(1, "%s: X has shape %s; nrow(X) must equal nrow(Z) = %d" % (who, Xm.shape, n))
    if not 1 <= Xm.shape[1] <= F_MAX:
        raise BwgrError(1, "%s: f = %d covariates; this entry takes 1 <= f <= %d" % (who, Xm.shape[1], F_MAX))
    return np.asfortranarray(Xm)


def _dense_args(D, single, device):
    """(pointer, memloc, n, p, ldz, device, what keeps the memory alive) of a dense design; `single`: rounded through float"""
    Zd = D.device_tensor()
    if Zd is not None:
        import torch
        if single:
            Zd = Zd.to(torch.float32).to(torch.float64)
        if Zd.stride(0) != 1 or (Zd.shape[1] > 1 and Zd.stride(1) < Zd.shape[0]):
            Zd = Zd.t().contiguous().t()
        n, p = int(Zd.shape[0]), int(Zd.shape[1])
        torch.cuda.synchronize(Zd.device)
        return C.c_void_p(Zd.data_ptr()), DEVICE, n, p, (int(Zd.stride(1)) if p > 1 else n), Zd.device.index or 0, Zd
    Zh = D.Z
    if single:
        with np.errstate(over="ignore"):
            Zh = np.asfortranarray(Zh.astype(np.float32).astype(np.float64))
    return _vp(Zh), HOST, Zh.shape[0], Zh.shape[1], Zh.shape[0], int(device), Zh


def project(Z, X, *, device_out=False, **panel_kw):
    """Zp = Z - X (X'X)^-1 X'Z over all rows (bwgr_project): the residual of every column of Z on the covariates X -- genotypes cleared of
    population-structure components, of year or location means.  Z is a Panel or what makes an int8 one, or dense(Z) (a numpy matrix or a CUDA
    tensor); X is n x f float64 on the host, 1 <= f <= 256, taken as it is.  Returns the n x p float64 matrix: a numpy array, or a tensor on
    the device where a dense Z lives there or device_out=True (import torch first).  Every element is the chain z - x_1 c_1 - ... - x_f c_f in
    that order, one fused multiply-add per covariate: the bits do not depend on the kind of Z, on the slab height, or on the other columns."""
    kind, Z = _source(Z, "project")
    Xf = _covariates(X, "project", _rows(kind, Z), False)
    device = int(panel_kw.pop("device", 0)) if kind == "dense" else 0
    if kind == "dense" and panel_kw:
        raise BwgrError(1, "project: %s do(es) not apply to a dense Z (only device=)" % sorted(panel_kw))
    torch = sys.modules.get("torch")
    L = _lib.lib()

    def run(h, zptr, zloc, n, p, ldz, dev, on_device):
        if Xf.shape[0] != n:
            raise BwgrError(1, "project: X has shape %s; nrow(X) must equal nrow(Z) = %d" % (Xf.shape, n))
        if on_device:
            if torch is None:
                raise RuntimeError("device_out=True: import torch before calling (the result is a torch tensor)")
            out = torch.empty((p, n), dtype=torch.float64, device="cuda:%d" % dev).t()     # n x p, column-major
            torch.cuda.synchronize(out.device)
            check(L.bwgr_project(dev, h, zptr, zloc, n, p, ldz, _dp(Xf), Xf.shape[1], n, C.c_void_p(out.data_ptr()), DEVICE, n))
            torch.cuda.synchronize(out.device)
            return out
        out = np.zeros((n, p), order="F")
        check(L.bwgr_project(dev, h, zptr, zloc, n, p, ldz, _dp(Xf), Xf.shape[1], n, _vp(out), HOST, n))
        return out

    if kind == "dense":
        zptr, zloc, n, p, ldz, dev, keep = _dense_args(Z, False, device)
        return run(None, zptr, zloc, n, p, ldz, dev, device_out or zloc == DEVICE)
    with as_panel(Z, **panel_kw) as P:
        return run(P._h, None, HOST, P.n, P.p, P.n, P.device, device_out)


def MLM(Y, X, Z, maxit=500, logtol=-8, cores=1, verb=False, df0=1.1, **panel_kw):
    """MLM(Y, X, Z, ...), src/RcppEigen20230423.cpp:1260-1407 (R/RcppExports.R:192): the multivariate model with fixed effects.  Y is n x k
    (NaN = missing), X the n x f fixed-effects design (1 <= f <= 256), Z a Panel, an integer matrix (staged as an int8 panel) or dense(Z).
    Per trait the fixed effects b_t = (M_t'M_t)^-1 M_t'Y_t are fitted on its records and taken off; Z is projected off X over all rows
    (project); the random effects u are fitted by randomized Gauss-Seidel on the projected Z, with the variances' priors weighted by df0.
    Returns the reference's list as a dict in its order: b (f x k), u (p x k), hat (n x k, every row), h2, GC, vb, ve, cnv, its.
    The stopping rule is the reference's: with verb=False the loop stops only on a NaN, so it runs all maxit sweeps whatever logtol is; with
    verb=True it stops at cnv < logtol, and prints.  maxit=0 returns the start (u = 0, cnv = 10, its = 0).  `cores` is ignored.
    Y, X, a dense Z, logtol and df0 are rounded to float once, as the reference receives them; the arithmetic is fp64.  Departures: the two
    kinds of (X'X)^-1 are fp64 symmetric solves, and a design whose smallest eigenvalue is below f 2^-23 of its largest is refused, naming the
    trait, where the reference returns Inf.  The projected Z is an n x p fp64 matrix on the device whatever Z was (mlm_plan shows the bytes
    before a call).  With dense(Z), device= chooses the GPU; other keywords go to the panel that is made of an integer Z."""
    kind, Z = _source(Z, "MLM")
    n = _rows(kind, Z)
    Xf = _covariates(X, "MLM", n, True)
    n = Xf.shape[0]
    Yf = _matrix(Y, "MLM", None, True)
    if Yf.ndim != 2 or Yf.shape[0] != n:
        raise BwgrError(1, "MLM: Y has shape %s; nrow(Y) must equal nrow(X) = %d" % (Yf.shape, n))
    Yf = np.asfortranarray(Yf)
    k, f = Yf.shape[1], Xf.shape[1]
    if not 1 <= k <= 16:
        raise BwgrError(1, "MLM: k = %d traits; this engine takes 1 <= k <= 16" % k)
    if int(maxit) < 0:
        raise BwgrError(1, "MLM: maxit = %d" % int(maxit))
    logtol, df0 = float(np.float32(logtol)), float(np.float32(df0))
    device = int(panel_kw.pop("device", 0)) if kind == "dense" else 0
    if kind == "dense" and panel_kw:
        raise BwgrError(1, "MLM: %s do(es) not apply to a dense Z (only device=)" % sorted(panel_kw))

    def run(h, zptr, zloc, nz, p, ldz, dev):
        if nz != n:
            raise BwgrError(1, "MLM: Z has %d rows; nrow(Z) must equal nrow(X) = %d" % (nz, n))
        outs = (np.zeros((f, k), order="F"), np.zeros((p, k), order="F"), np.zeros((n, k), order="F"), np.zeros(k), np.zeros((k, k), order="F"),
                np.zeros((k, k), order="F"), np.zeros(k), np.zeros(1))
        its = C.c_int()
        check(_lib.lib().bwgr_mlm(dev, h, zptr, zloc, n, p, ldz, _dp(Xf), f, n, _dp(Yf), k, int(maxit), logtol, df0, int(bool(verb)),
                                  *[_dp(a) for a in outs], C.byref(its)))
        return dict(zip(MLM_KEYS, outs[:7] + (float(outs[7][0]), int(its.value))))

    if kind == "dense":
        zptr, zloc, nz, p, ldz, dev, keep = _dense_args(Z, True, device)
        return run(None, zptr, zloc, nz, p, ldz, dev)
    with as_panel(Z, **panel_kw) as P:
        return run(P._h, None, HOST, P.n, P.p, P.n, P.device)
