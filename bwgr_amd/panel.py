"""Panel: the genotype matrix staged once on the device (bwgr_panel_*, include/bwgr.h), and what is computed on a panel alone."""
import contextlib
import ctypes as C
import numpy as np

from . import _lib
from ._lib import BwgrError, check
from ._marshal import X_I8, X_F32, X_F64, HOST, DEVICE, _fp, _dp, _vp, _plan


KERNELS = {"GRM": 0, "GAU": 1, "EigenGRM": 2, "EigenGAU": 3, "EigenARC": 4}
KERNELS2 = {"ARC": 0, "GAU": 1}     # the founder-by-sample kinds (BWGR_KZ_*)
_INFO = ("n", "p", "ld", "block", "nwg", "slab_rows", "x_bytes", "gram_bytes")     # bwgr_panel_info's fields, a panel's attributes


class Panel:
    """Genotype matrix X staged once in HBM (column-major, rows zero-padded to the slab grid), together with
    xx, vx, MSx (src/Rcpp20260726ai.cpp:593-598) and the block-diagonal Gram used by the blocked sweep.

    X may be a numpy array (n x p; int8, float32 or float64 -- an all-integer float matrix within int8 range is
    stored as int8 unless as_int8=False) or a torch CUDA tensor holding the column-major matrix as shape
    (p, ldx) int8/float32 (row j of the tensor = column j of X)."""

    def __init__(self, X, n=None, device=0, block=0, nwg=0, as_int8=None):
        L = _lib.lib()
        self._h = C.c_void_p()
        self._keep = None
        if hasattr(X, "data_ptr"):  # torch tensor on the GPU, (p, ldx)
            import torch
            assert X.is_cuda and X.dim() == 2 and X.is_contiguous(), "device X must be a contiguous (p, ldx) CUDA tensor"
            p, ldx = X.shape
            n = ldx if n is None else int(n)
            xtype = {torch.int8: X_I8, torch.float32: X_F32, torch.float64: X_F64}[X.dtype]
            device = X.device.index or 0
            torch.cuda.synchronize(X.device)
            check(L.bwgr_panel_create(C.byref(self._h), C.c_void_p(X.data_ptr()), xtype, DEVICE, n, p, ldx, device, block, nwg))
        else:
            X = np.asarray(X)
            assert X.ndim == 2, "X must be n x p"
            n, p = X.shape
            if X.dtype != np.int8:
                fits = bool(X.size == 0 or (X.min() >= -128 and X.max() <= 127))   # a wider integer must not wrap
                if as_int8 is None:
                    as_int8 = fits and bool(np.issubdtype(X.dtype, np.integer) or (X.size and np.all(X == np.rint(X))))
                if as_int8:
                    if not fits or not (np.issubdtype(X.dtype, np.integer) or np.all(X == np.rint(X))):
                        raise ValueError("Panel(as_int8=True): X holds values outside -128..127 or non-integers")
                    X = X.astype(np.int8)
                elif X.dtype not in (np.float32, np.float64):
                    X = X.astype(np.float64)
            Xc = np.asfortranarray(X)
            xtype = {np.dtype(np.int8): X_I8, np.dtype(np.float32): X_F32, np.dtype(np.float64): X_F64}[Xc.dtype]
            check(L.bwgr_panel_create(C.byref(self._h), _vp(Xc), xtype, HOST, n, p, n, device, block, nwg))
        vars(self).update(_plan("bwgr_panel_info", _INFO, self._h), device=device)

    def set_stream(self, stream_ptr):
        check(_lib.lib().bwgr_panel_set_stream(self._h, C.c_void_p(stream_ptr)))

    def clone(self):
        """A second handle on the same resident genotypes with its own sweep scratch and stream (bwgr_panel_clone):
        chains on a panel and on its clones run side by side on the GPU.  Closed with (or before) the parent."""
        import weakref
        q = Panel.__new__(Panel)
        q._h = C.c_void_p(); q._keep = None
        root = getattr(self, "_parent", None) or self
        check(_lib.lib().bwgr_panel_clone(C.byref(q._h), root._h))
        q._parent = root
        for k in _INFO + ("device",):
            setattr(q, k, getattr(root, k))
        if not hasattr(root, "_clones"):
            root._clones = weakref.WeakSet()
        root._clones.add(q)
        return q

    def max_pairs(self):
        """How many pairs of chains (Chain.run_pair) fit the chip at once (bwgr_panel_max_pairs); 0 without k_sweep3."""
        c = C.c_int(0)
        check(_lib.lib().bwgr_panel_max_pairs(self._h, C.byref(c)))
        return c.value

    def max_concurrent(self, selection):
        """How many sweeps of this geometry fit the chip at once (bwgr_panel_max_concurrent)."""
        c = C.c_int()
        check(_lib.lib().bwgr_panel_max_concurrent(self._h, int(bool(selection)), C.byref(c)))
        return int(c.value)

    def centred(self):
        """True when every column's |mean| <= 1e-3 sd (from the panel's own statistics): what the marker-sharded sampler needs to be sound."""
        k = C.c_int()
        check(_lib.lib().bwgr_panel_centred(self._h, C.byref(k)))
        return bool(k.value)

    def set_centred(self, on=True):
        """Sweep the implicitly centred columns x_j - mean(x_j) of this int8 panel from now on (bwgr_panel_set_centred): the genotypes stay
        int8 in HBM and the kernels those of the raw columns; the fused chains (Chain, BayesB / C / Cpi / Dpi) then run the reference's sweep on
        the centred columns, stats() returns their squared norms and centred() is True -- what the marker-sharded sampler needs."""
        check(_lib.lib().bwgr_panel_set_centred(self._h, int(bool(on))))
        return self

    def pipeline(self, selection):
        """How a sweep over this panel is pipelined: dict(generation, lag, feeders, gram_bits) (bwgr_panel_pipeline)."""
        return _plan("bwgr_panel_pipeline", ("generation", "lag", "feeders", "gram_bits"), self._h, bool(selection), ctype=C.c_int)

    def stats(self):
        xx = np.empty(self.p, np.float32); vx = np.empty(self.p, np.float32); msx = C.c_float()
        check(_lib.lib().bwgr_panel_stats(self._h, _fp(xx), _fp(vx), C.byref(msx)))
        return xx, vx, float(msx.value)

    def crossprod(self, *, device_out=False):
        """The exact X X' over the panel's rows as n x n int64 (bwgr_panel_crossprod)."""
        L = _lib.lib()
        return self._out2d([(self.n, self.n)], np.int64, device_out, lambda ptr, ld, loc: L.bwgr_panel_crossprod(self._h, ptr[0], ld[0], loc))[0]

    def kernel(self, kind, par=1.0, flag=None, *, device_out=False):
        """A relationship kernel of the panel's genotypes, n x n float64 (bwgr_panel_kernel).  kind: "GRM" (flag = Code012, default False),
        "GAU", "EigenGRM" (flag = centralizeZ, default True), "EigenGAU" (par = phi), "EigenARC" (flag = centralizeX, default True)."""
        k = KERNELS[kind] if isinstance(kind, str) else int(kind)
        if flag is None:
            flag = k in (KERNELS["EigenGRM"], KERNELS["EigenARC"])
        L = _lib.lib()
        return self._out2d([(self.n, self.n)], np.float64, device_out,
                           lambda ptr, ld, loc: L.bwgr_panel_kernel(self._h, k, float(par), int(bool(flag)), ptr[0], ld[0], loc))[0]

    def _out2d(self, shapes, dtype, device_out, call):
        """Results of the relationship kernels, one array per shape: numpy arrays, or (device_out) torch tensors on the panel's device.
        call(pointers, leading dimensions, memloc)."""
        if device_out:
            import sys
            torch = sys.modules.get("torch")
            if torch is None:
                raise RuntimeError("device_out=True: import torch before calling (the result is a torch tensor)")
            outs = [torch.empty(sh, dtype=torch.int64 if dtype == np.int64 else torch.float64, device="cuda:%d" % self.device) for sh in shapes]
            torch.cuda.synchronize(outs[0].device)
            check(call([C.c_void_p(o.data_ptr()) for o in outs], [sh[1] for sh in shapes], DEVICE))
            return outs
        outs = [np.empty(sh, dtype) for sh in shapes]
        check(call([_vp(o) for o in outs], [sh[1] for sh in shapes], HOST))
        return outs

    def _check_other(self, other, who):
        if not isinstance(other, Panel):
            raise TypeError("%s: the samples must be a Panel" % who)
        if other.p != self.p:
            raise ValueError("%s: the founders have %d columns (markers), the samples %d" % (who, self.p, other.p))

    def crossprod2(self, other, *, device_out=False):
        """The exact X_f X_s' between this panel's rows (the founders) and another panel's (the samples) over the same markers, n_f x n_s
        int64 (bwgr_panel_crossprod2)."""
        self._check_other(other, "crossprod2")
        L = _lib.lib()
        return self._out2d([(self.n, other.n)], np.int64, device_out,
                           lambda ptr, ld, loc: L.bwgr_panel_crossprod2(self._h, other._h, ptr[0], ld[0], loc))[0]

    def kernel2(self, other, kind, par=1.0, *, device_out=False):
        """The founder-by-sample kernels (Kff, Kfs) of EigenArcZ / EigenGauZ, n_f x n_f and n_f x n_s float64 (bwgr_panel_kernel2): this
        panel holds the founders, `other` the samples.  kind: "ARC", or "GAU" (par = phi)."""
        self._check_other(other, "kernel2")
        k = KERNELS2[kind] if isinstance(kind, str) else int(kind)
        L = _lib.lib()
        Kff, Kfs = self._out2d([(self.n, self.n), (self.n, other.n)], np.float64, device_out,
                               lambda ptr, ld, loc: L.bwgr_panel_kernel2(self._h, other._h, k, float(par), ptr[0], ld[0], ptr[1], ld[1], loc))
        return Kff, Kfs

    def xb(self, B):
        """X B on the raw int8 genotypes for every row, n x k float64 (bwgr_panel_xb); B is p x k or a vector of p."""
        Bm = np.asarray(B, np.float64)
        if Bm.ndim == 1:
            Bm = Bm[:, None]
        if Bm.ndim != 2 or Bm.shape[0] != self.p:
            raise BwgrError(1, "panel_xb: B has shape %s; nrow(B) must equal ncol(X) = %d" % (Bm.shape, self.p))
        Bf = np.asfortranarray(Bm)
        k = Bf.shape[1]
        out = np.zeros((self.n, max(k, 1)), order="F")
        check(_lib.lib().bwgr_panel_xb(self._h, _dp(Bf), int(k), _dp(out)))
        return out

    def close(self):
        if self._h:
            for q in list(getattr(self, "_clones", ())):
                q.close()
            check(_lib.lib().bwgr_panel_destroy(self._h))   # refuses while chains or clones are alive: the handle stays valid
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@contextlib.contextmanager
def as_panel(X, **kw):
    """X itself where it is a Panel, else a panel made of it with **kw and closed when the block ends: a caller's panel is never closed."""
    P = X if isinstance(X, Panel) else Panel(X, **kw)
    try:
        yield P
    finally:
        if P is not X:
            P.close()


def panel_xb(X, B, **kw):
    """X B on the raw int8 genotypes, n x k float64 (bwgr_panel_xb); X is an array or a Panel."""
    with as_panel(X, **kw) as P:
        return P.xb(B)
