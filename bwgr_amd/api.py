"""Host-side mirror of the reference's R interface for the Gibbs hot path.

Same names, argument order, defaults and return-list element names/order as
  KMUP(X,b,d,xx,e,L,Ve,pi)                          R/RcppExports.R:4-6
  BayesA/BayesL/BayesRR/BayesCpi/BayesDpi(y,X,it=1500,bi=500,df=5,R2=0.5)   R/RcppExports.R:48-74
  BayesB/BayesC(y,X,it=1500,bi=500,pi=0.95,df=5,R2=0.5)
  wgr(y,X,it=1500,bi=500,th=1,bag=1,rp=FALSE,iv=FALSE,de=FALSE,pi=0,df=5,R2=0.5,eigK=NULL,VarK=0.95,verb=FALSE)
                                                    R/wgr.R:2-8
R is not available in the build image, so the host layer above the C ABI is Python (see
INTEGRATION.md for the R .Call shim that binds the same entry points).  Everything numerical happens in
libbwgr_hip.so on the GPU; this module only marshals arrays.  `seed=None` draws the seed from numpy's
global stream, so numpy.random.seed() plays the role of R's set.seed().
"""
import contextlib
import ctypes as C
import numpy as np

from . import _lib
from ._lib import BwgrError, c_f, c_d, check

MODELS = {"BayesA": 0, "BayesB": 1, "BayesC": 2, "BayesL": 3, "BayesRR": 4, "BayesCpi": 5, "BayesDpi": 6}
_PER_MARKER_VB = {"BayesA", "BayesB", "BayesL", "BayesDpi"}
KERNELS = {"GRM": 0, "GAU": 1, "EigenGRM": 2, "EigenGAU": 3, "EigenARC": 4}
KERNELS2 = {"ARC": 0, "GAU": 1}     # the founder-by-sample kinds (BWGR_KZ_*)
X_I8, X_F32, X_F64 = 0, 1, 2
HOST, DEVICE = 0, 1


def _seed(seed):
    if seed is None:
        return int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _fp(a):
    return a.ctypes.data_as(c_f)


def _dp(a):
    return a.ctypes.data_as(c_d)


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
            check(L.bwgr_panel_create(C.byref(self._h), Xc.ctypes.data_as(C.c_void_p), xtype, HOST, n, p, n, device, block, nwg))
        info = (C.c_int64 * 8)()
        check(L.bwgr_panel_info(self._h, info))
        self.n, self.p, self.ld, self.block, self.nwg, self.slab_rows, self.x_bytes, self.gram_bytes = [int(v) for v in info]
        self.device = device

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
        for k in ("n", "p", "ld", "block", "nwg", "slab_rows", "x_bytes", "gram_bytes", "device"):
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
        info = (C.c_int * 4)()
        check(_lib.lib().bwgr_panel_pipeline(self._h, int(bool(selection)), info))
        return dict(zip(("generation", "lag", "feeders", "gram_bits"), (int(v) for v in info)))

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
        check(call([o.ctypes.data_as(C.c_void_p) for o in outs], [sh[1] for sh in shapes], HOST))
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


def _as_panel(X, **kw):
    return (X, False) if isinstance(X, Panel) else (Panel(X, **kw), True)


class Chain:
    """One MCMC chain of a fused sampler, stepping interface over bwgr_chain_* (state stays on the GPU)."""

    def __init__(self, panel, model, y, it=1500, bi=500, pi=0.95, df=5.0, R2=0.5, seed=None, rng_mode=0, shard=None,
                 e_ext=None, wait_for_y=True):
        """shard = (marker0, p_total, MSx_total) makes this the chain of one marker shard (bwgr_chain_create_sharded);
        e_ext = a torch float64 CUDA tensor of panel.ld entries that will hold the (replicated) residual.  A device y is waited for
        (the whole device) before the library copies it; wait_for_y=False leaves that out for a caller who wrote y on the panel's
        own stream (Panel.set_stream), where the library's copy is ordered behind it."""
        self.panel, self.model = panel, model
        self._h = C.c_void_p()
        self.it, self.bi = int(it), int(bi)
        if hasattr(y, "data_ptr"):
            import torch
            assert y.is_cuda and y.dtype == torch.float32 and y.is_contiguous() and y.numel() == panel.n
            if wait_for_y:
                torch.cuda.synchronize(y.device)
            yptr, loc = C.c_void_p(y.data_ptr()), DEVICE
        else:
            self._y = np.ascontiguousarray(y, np.float32)
            assert self._y.size == panel.n, "length(y) must equal nrow(X)"
            yptr, loc = self._y.ctypes.data_as(C.c_void_p), HOST
        if shard is None and e_ext is None:
            check(_lib.lib().bwgr_chain_create(C.byref(self._h), panel._h, MODELS[model], yptr, loc, float(it), float(bi),
                                                float(pi), float(df), float(R2), C.c_uint64(_seed(seed)), int(rng_mode)))
        else:
            marker0, p_total, msx_total = shard if shard is not None else (0, panel.p, panel.stats()[2])
            eptr = None
            if e_ext is not None:
                import torch
                assert e_ext.is_cuda and e_ext.dtype == torch.float64 and e_ext.is_contiguous() and e_ext.numel() == panel.ld
                self._e_ext = e_ext
                eptr = C.c_void_p(e_ext.data_ptr())
            check(_lib.lib().bwgr_chain_create_sharded(C.byref(self._h), panel._h, MODELS[model], yptr, loc, float(it), float(bi),
                                                        float(pi), float(df), float(R2), C.c_uint64(_seed(seed)), int(rng_mode),
                                                        int(marker0), int(p_total), float(msx_total), eptr))
        self.nblocks = (panel.p + panel.block - 1) // panel.block

    def run(self, iters):
        check(_lib.lib().bwgr_chain_run(self._h, int(iters)))

    def run_pair(self, other, iters):
        """Advance this chain and `other` (a chain on a clone of the same resident panel) `iters` iterations in lockstep on one set
        of streamer workgroups -- one pass over the genotypes for both (bwgr_chain_run_pair).  Each chain's results are the ones it
        would have alone."""
        check(_lib.lib().bwgr_chain_run_pair(self._h, other._h, int(iters)))

    def sync(self):
        check(_lib.lib().bwgr_chain_sync(self._h))

    def sweep_blocks(self, lo, hi):
        check(_lib.lib().bwgr_chain_sweep_blocks(self._h, int(lo), int(hi)))

    def round_sweep(self, lo, hi, delta):
        """Exchange round, first half (bwgr_chain_round_sweep): delta (torch float64 CUDA tensor of panel.ld entries) receives
        e - e_before after sweeping blocks [lo, hi)."""
        check(_lib.lib().bwgr_chain_round_sweep(self._h, int(lo), int(hi), C.c_void_p(delta.data_ptr())))

    def round_apply(self, delta):
        check(_lib.lib().bwgr_chain_round_apply(self._h, C.c_void_p(delta.data_ptr())))

    def get_sums_dev(self, t):
        """{sum d, sum b^2} of the blocks swept so far into t (torch float64 CUDA tensor, 2 entries): no host round trip."""
        check(_lib.lib().bwgr_chain_get_sums_dev(self._h, C.c_void_p(t.data_ptr())))

    def end_iteration_dev(self, t):
        check(_lib.lib().bwgr_chain_end_iteration_dev(self._h, C.c_void_p(t.data_ptr())))

    def get_sums(self):
        s = np.zeros(2, np.float64)
        check(_lib.lib().bwgr_chain_get_sums(self._h, _dp(s)))
        return s

    def end_iteration(self, sums_total=None):
        if sums_total is None:
            check(_lib.lib().bwgr_chain_end_iteration(self._h, None))
        else:
            s = np.ascontiguousarray(sums_total, np.float64)
            check(_lib.lib().bwgr_chain_end_iteration(self._h, _dp(s)))

    def sweep_ms(self):
        ms = C.c_float(); nl = C.c_int()
        check(_lib.lib().bwgr_chain_sweep_ms(self._h, C.byref(ms), C.byref(nl)))
        return float(ms.value), int(nl.value)

    def redo_count(self):
        """Sweeps that left the fixed-point range of their engine and were redone on the fp64 residual."""
        k = C.c_int()
        check(_lib.lib().bwgr_chain_redo_count(self._h, C.byref(k)))
        return int(k.value)

    def state(self):
        p, n = self.panel.p, self.panel.n
        b = np.empty(p, np.float32); d = np.empty(p, np.float32); e = np.empty(n, np.float32)
        vb = np.empty(p, np.float32); s = np.empty(4, np.float32)
        check(_lib.lib().bwgr_chain_state(self._h, _fp(b), _fp(d), _fp(e), _fp(vb), _fp(s)))
        return {"b": b, "d": d, "e": e, "vb": vb, "mu": float(s[0]), "ve": float(s[1]), "vb_common": float(s[2]), "pi": float(s[3])}

    def result(self):
        """The reference's return list (names and order), src/Rcpp20260726ai.cpp:631-634, 694-698, 916-920."""
        p, n, model = self.panel.p, self.panel.n, self.model
        per = model in _PER_MARKER_VB
        B = np.empty(p, np.float32); D = np.empty(p, np.float32); hat = np.empty(n, np.float32)
        VB = np.empty(p if per else 1, np.float32); PV = np.empty(p, np.float32)
        mu = C.c_float(); ve = C.c_float(); h2 = C.c_float(); msx = C.c_float(); Pi = C.c_float()
        check(_lib.lib().bwgr_chain_result(self._h, C.byref(mu), _fp(B), _fp(D), _fp(hat), _fp(VB), C.byref(ve), C.byref(h2),
                                            C.byref(msx), C.byref(Pi), _fp(PV)))
        vb = VB if per else float(VB[0])
        if model in ("BayesA", "BayesL", "BayesRR"):
            return {"mu": mu.value, "b": B, "hat": hat, "vb": vb, "ve": ve.value, "h2": h2.value, "MSx": msx.value}
        if model in ("BayesB", "BayesC"):
            return {"mu": mu.value, "b": B, "d": D, "hat": hat, "vb": vb, "ve": ve.value, "h2": h2.value, "MSx": msx.value}
        return {"mu": mu.value, "b": B, "d": D, "pi": Pi.value, "hat": hat, "h2": h2.value, "vb": vb, "ve": ve.value, "PVAL": PV}

    def close(self):
        if self._h:
            _lib.lib().bwgr_chain_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fused(model, y, X, it, bi, pi, df, R2, seed, rng_mode, return_state=False, **panel_kw):
    P, own = _as_panel(X, **panel_kw)
    ch = Chain(P, model, y, it, bi, pi, df, R2, seed, rng_mode)
    try:
        ch.run(int(it))
        out = ch.result()
        if return_state:
            out["last"] = ch.state()
        return out
    finally:
        ch.close()
        if own:
            P.close()


def BayesA(y, X, it=1500, bi=500, df=5, R2=0.5, *, seed=None, rng_mode=0, **kw):
    return _fused("BayesA", y, X, it, bi, 0.0, df, R2, seed, rng_mode, **kw)


def BayesB(y, X, it=1500, bi=500, pi=0.95, df=5, R2=0.5, *, seed=None, rng_mode=0, **kw):
    return _fused("BayesB", y, X, it, bi, pi, df, R2, seed, rng_mode, **kw)


def BayesC(y, X, it=1500, bi=500, pi=0.95, df=5, R2=0.5, *, seed=None, rng_mode=0, **kw):
    return _fused("BayesC", y, X, it, bi, pi, df, R2, seed, rng_mode, **kw)


def BayesL(y, X, it=1500, bi=500, df=5, R2=0.5, *, seed=None, rng_mode=0, **kw):
    return _fused("BayesL", y, X, it, bi, 0.0, df, R2, seed, rng_mode, **kw)


def BayesRR(y, X, it=1500, bi=500, df=5, R2=0.5, *, seed=None, rng_mode=0, **kw):
    return _fused("BayesRR", y, X, it, bi, 0.0, df, R2, seed, rng_mode, **kw)


def BayesCpi(y, X, it=1500, bi=500, df=5, R2=0.5, *, seed=None, rng_mode=0, **kw):
    return _fused("BayesCpi", y, X, it, bi, 0.0, df, R2, seed, rng_mode, **kw)


def BayesDpi(y, X, it=1500, bi=500, df=5, R2=0.5, *, seed=None, rng_mode=0, **kw):
    return _fused("BayesDpi", y, X, it, bi, 0.0, df, R2, seed, rng_mode, **kw)


class Group:
    """One fused-sampler chain over several GPUs of this process (bwgr_group_*, include/bwgr.h): device g takes the g-th
    block-aligned marker shard of the host matrix X, the residual is replicated and re-united by RCCL all-reduces at the
    exchange rounds, one host thread drives everything.  devices=[d] is the plain exact chain on one GPU; more devices
    run the partitioned sampler (sound on centred columns only: centre=True).  This is the path an R .Call takes to more than one GPU; the
    benchmark's one-process-per-GPU driver is bwgr_amd/dist.py."""

    def __init__(self, model, y, X, devices=(0,), it=1500, bi=500, pi=0.95, df=5.0, R2=0.5, seed=None, rng_mode=0, block=0,
                 markers_per_sync=0, centre=False, n=None):
        """centre=True sweeps x_j - mean(x_j): what makes more than one shard statistically sound (on uncentred columns the library refuses
        len(devices) > 1 unless BWGR_GROUP_ALLOW_UNCENTRED=1).  Integer genotypes under the selection models (BayesB / C / Cpi / Dpi) are centred
        IMPLICITLY (the panel stays int8 in HBM: bwgr_group_create_centred; centre="explicit" asks for the float copy); float columns and the affine
        models get an explicitly centred float panel.  Centring is a reparametrisation under the flat intercept
        prior (an exact Gibbs sampler would not notice; bWGR's own chain does a little: DESIGN.md section 8); result() gives mu back in the uncentred
        parametrisation, mu - sum_j mean_j b_j.
        devices may name ONE device several times: the shards then run side by side on that GPU (streams of their own, a sum kernel per exchange
        round, no RCCL).  X may then also be a torch int8 CUDA tensor of shape (p, ldx) on that device (row j = column j of X; n rows of it used)."""
        self._xbar = None
        self._keep = None
        implicit = False
        memloc = HOST
        if hasattr(X, "data_ptr"):     # device-resident int8 genotypes, shards of that one device, implicit centring
            import torch
            assert X.is_cuda and X.dim() == 2 and X.is_contiguous() and X.dtype == torch.int8, "device X: a contiguous (p, ldx) int8 CUDA tensor"
            assert centre and centre != "explicit", "device X: implicitly centred shards (centre=True)"
            assert all(int(d) == (X.device.index or 0) for d in devices), "device X serves shards of its own device only"
            p_, ldx = X.shape
            self.n, self.p = int(ldx if n is None else n), int(p_)
            xb = torch.empty(p_, dtype=torch.float64, device=X.device)
            for c0 in range(0, p_, 65536):
                xb[c0:c0 + 65536] = X[c0:c0 + 65536, :self.n].sum(dim=1, dtype=torch.int64).to(torch.float64) / self.n
            self._xbar = xb.cpu().numpy()
            torch.cuda.synchronize(X.device)
            self._keep = X
            implicit, memloc, xtype, xptr = True, DEVICE, X_I8, C.c_void_p(X.data_ptr())
        else:
            X = np.asarray(X)
            assert X.ndim == 2
            if centre:
                Xd = X.astype(np.float64)
                self._xbar = Xd.mean(0)
                implicit = (centre != "explicit" and model in ("BayesB", "BayesC", "BayesCpi", "BayesDpi") and X.size > 0
                            and bool(np.all(X == np.rint(X))) and X.min() >= -128 and X.max() <= 127)
                if not implicit:
                    X = (Xd - self._xbar).astype(np.float32)
            if X.dtype != np.int8:
                fits = bool(X.size == 0 or (X.min() >= -128 and X.max() <= 127))
                if fits and (np.issubdtype(X.dtype, np.integer) or np.all(X == np.rint(X))):
                    X = X.astype(np.int8)
                elif X.dtype not in (np.float32, np.float64):
                    X = X.astype(np.float64)
            self._X = np.asfortranarray(X)
            self.n, self.p = self._X.shape
            ldx = self.n
            xtype = {np.dtype(np.int8): X_I8, np.dtype(np.float32): X_F32, np.dtype(np.float64): X_F64}[self._X.dtype]
            xptr = self._X.ctypes.data_as(C.c_void_p)
        self.model = model
        if hasattr(y, "data_ptr"):
            y = y.detach().cpu().numpy()
        self._y = np.ascontiguousarray(y, np.float32)
        assert self._y.size == self.n
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        self._h = C.c_void_p()
        self.implicit_centring = implicit
        args = [C.byref(self._h), len(devices), devs, xptr, xtype, self.n, self.p, int(ldx), int(block), _fp(self._y), MODELS[model], float(it), float(bi),
                float(pi), float(df), float(R2), C.c_uint64(_seed(seed)), int(rng_mode), int(markers_per_sync)]
        if implicit:
            check(_lib.lib().bwgr_group_create_centred(*(args + [memloc])))
        else:
            check(_lib.lib().bwgr_group_create(*args))

    def info(self):
        v = (C.c_int64 * 4)()
        check(_lib.lib().bwgr_group_info(self._h, v))
        out = dict(zip(("devices", "rounds_per_sweep", "markers_per_round", "rccl"), (int(x) for x in v)))
        out["statistically_sound"] = self.sound()
        return out

    def sound(self):
        """True for one device (the exact chain) or centred columns; False for several devices on uncentred columns."""
        k = C.c_int()
        check(_lib.lib().bwgr_group_sound(self._h, C.byref(k)))
        return bool(k.value)

    def run(self, iters):
        check(_lib.lib().bwgr_group_run(self._h, int(iters)))

    def sync(self):
        check(_lib.lib().bwgr_group_sync(self._h))

    def result(self):
        p, n, model = self.p, self.n, self.model
        per = model in _PER_MARKER_VB
        B = np.empty(p, np.float32); D = np.empty(p, np.float32); hat = np.empty(n, np.float32)
        VB = np.empty(p if per else 1, np.float32); PV = np.empty(p, np.float32)
        mu = C.c_float(); ve = C.c_float(); h2 = C.c_float(); msx = C.c_float(); Pi = C.c_float()
        check(_lib.lib().bwgr_group_result(self._h, C.byref(mu), _fp(B), _fp(D), _fp(hat), _fp(VB), C.byref(ve), C.byref(h2),
                                            C.byref(msx), C.byref(Pi), _fp(PV)))
        vb = VB if per else float(VB[0])
        muv = mu.value
        if self._xbar is not None:      # centred columns: the intercept of the uncentred parametrisation (posterior means are linear in it)
            muv = float(muv - float(np.dot(self._xbar, B.astype(np.float64))))
        if model in ("BayesA", "BayesL", "BayesRR"):
            out = {"mu": muv, "b": B, "hat": hat, "vb": vb, "ve": ve.value, "h2": h2.value, "MSx": msx.value}
        elif model in ("BayesB", "BayesC"):
            out = {"mu": muv, "b": B, "d": D, "hat": hat, "vb": vb, "ve": ve.value, "h2": h2.value, "MSx": msx.value}
        else:
            out = {"mu": muv, "b": B, "d": D, "pi": Pi.value, "hat": hat, "h2": h2.value, "vb": vb, "ve": ve.value, "PVAL": PV}
        out["statistically_sound"] = self.sound()     # (beyond the reference's list: False for several devices on uncentred columns)
        return out

    def close(self):
        if self._h:
            _lib.lib().bwgr_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_SELECTION = ("BayesB", "BayesC", "BayesCpi", "BayesDpi")
_DEFAULT_PI = {"BayesB": 0.95, "BayesC": 0.95}


def fit_many(X, jobs, concurrent=None, chunk=4, pair=None, **panel_kw):
    """Several fused-sampler fits on ONE resident X, run side by side: jobs = [dict(model=, y=, it=, bi=, pi=, df=,
    R2=, seed=, rng_mode=), ...] (same defaults as the BayesX functions); returns the BayesX return lists in job order.
    Every job's chain is the one BayesX(y, X, ...) alone would run -- bit for bit -- because a chain's arithmetic does
    not depend on what else is on the chip: the panel is cloned (bwgr_panel_clone: shared genotypes and Gram, private
    sweep scratch and stream) once per slot, a sweep occupies nwg + 1 + feeders compute units, and up to
    Panel.max_concurrent() of them fit.  This is the shape of the reference's multi-fit callers (mcmcCV runs seven
    samplers per fold on the same training matrix, R/cv.R:124-130), which it runs one after the other.

    pair: sparse selection jobs (BayesB / BayesC with pi >= 0.95 on a panel that has k_sweep3: up to about 6 % of the markers in the model a pair does more per compute unit than two chains apart) run TWO to a set of streamer
    workgroups (Chain.run_pair: one pass over the genotypes serves both).  A paired chain is bit for bit the chain it is alone on
    k_sweep3; a single chain whose inclusion rate passes 3 % takes some sweeps on k_sweep2 instead (the device chooses), which
    agrees to ~1e-9, not bit for bit.  None = whenever at least two jobs qualify, False = never, True = every selection job
    (dense chains are slow on k_sweep3)."""
    P, own = _as_panel(X, **panel_kw)
    handles, results = [], [None] * len(jobs)
    live = []   # every chain still open (closed on the way out, whatever happens)
    try:
        norm = []
        for j in jobs:
            j = dict(j)
            model = j.pop("model"); y = j.pop("y")
            norm.append((model, y, int(j.pop("it", 1500)), int(j.pop("bi", 500)), float(j.pop("pi", _DEFAULT_PI.get(model, 0.0))),
                         float(j.pop("df", 5)), float(j.pop("R2", 0.5)), j.pop("seed", None), int(j.pop("rng_mode", 0))))
            if j:
                raise TypeError("fit_many: unknown job keys %s" % sorted(j))
        gen3 = P.pipeline(True)["generation"] == 3   # (int8 panels with k_sweep3)
        if pair is True:
            paired = [i for i, r in enumerate(norm) if r[0] in _SELECTION] if gen3 else []
        elif pair is None:
            paired = [i for i, r in enumerate(norm) if r[0] in ("BayesB", "BayesC") and r[4] >= 0.95] if gen3 else []
        else:
            paired = []
        if len(paired) < 2:
            paired = []
        single = [i for i in range(len(norm)) if i not in set(paired)]

        def make(i, handle):
            model, y, it, bi, pi, df, R2, seed, rng_mode = norm[i]
            ch = Chain(handle, model, y, it, bi, pi, df, R2, seed, rng_mode)
            live.append(ch)
            return [i, ch, it]

        def finish(rec):
            i, ch, _ = rec
            try:
                results[i] = ch.result()
            finally:
                ch.close(); live.remove(ch)

        def need(n):   # handles 0 .. n-1 exist
            while len(handles) < n:
                handles.append(P if not handles else P.clone())

        # ---- pairs: slot s owns handles 2s and 2s+1; a pair holds (streamers + 2) compute units ----
        if paired:
            cap = max(1, P.max_pairs())
            nslot = max(1, min((len(paired) + 1) // 2, cap if concurrent is None else min(int(concurrent), cap)))
            need(2 * nslot)
            queue, active = list(paired), {}

            def unpair(rec):   # BWGR_ERANGE: a pair sweep left the fixed-point range (no redo on that path, include/bwgr.h): the job again, alone
                i, ch, _ = rec
                ch.close(); live.remove(ch)
                single.append(i)

            while queue or active:
                for s_ in range(nslot):
                    rec = active.setdefault(s_, [None, None])
                    for h in (0, 1):
                        if rec[h] is None and queue:
                            rec[h] = make(queue.pop(0), handles[2 * s_ + h])
                for s_, rec in list(active.items()):
                    a_, b_ = rec
                    if a_ is not None and b_ is not None:
                        step = min(int(chunk), a_[2], b_[2])
                        try:
                            a_[1].run_pair(b_[1], step)
                            a_[2] -= step; b_[2] -= step
                        except BwgrError as ex:   # (surfaces when an earlier pair sweep's status is read: either chain may be the one)
                            if ex.code != 6:
                                raise
                            unpair(a_); unpair(b_); rec[0] = rec[1] = None
                    else:
                        for r in (a_, b_):
                            if r is not None:
                                step = min(int(chunk), r[2]); r[1].run(step); r[2] -= step
                for s_, rec in list(active.items()):
                    for h in (0, 1):
                        if rec[h] is not None and rec[h][2] == 0:
                            try:
                                finish(rec[h])
                            except BwgrError as ex:
                                if ex.code != 6:
                                    raise
                                single.append(rec[h][0])   # (finish closed the chain)
                            rec[h] = None
                    if rec[0] is None and rec[1] is None and not queue:
                        del active[s_]
        # ---- the rest, one chain per handle ----
        if single:
            cap = P.max_concurrent(any(norm[i][0] in _SELECTION for i in single))
            nslot = max(1, min(len(single), cap if concurrent is None else min(int(concurrent), cap)))
            need(nslot)
            queue, active = list(single), {}
            while queue or active:
                for slot in range(nslot):
                    if slot not in active and queue:
                        active[slot] = make(queue.pop(0), handles[slot])
                # a few iterations per chain per turn keeps every stream's launch queue fed without one chain hogging the host
                for slot in list(active):
                    rec = active[slot]
                    step = min(int(chunk), rec[2])
                    rec[1].run(step)
                    rec[2] -= step
                for slot in list(active):
                    if active[slot][2] == 0:
                        finish(active[slot])
                        del active[slot]
        return results
    finally:
        for ch in list(live):
            ch.close()
        for h in handles[1:]:
            h.close()
        if own:
            P.close()


_EM = {"emRR": 0, "emBA": 1, "emDE": 2, "emML": 3, "emBB": 4, "emBC": 5, "emBCpi": 6, "emBL": 7, "emEN": 8, "lasso": 9}


def _em(model, y, gen, df=10.0, R2=0.5, par=0.0, D=None, maxit=0, **panel_kw):
    """The EM / Gauss-Seidel family over bwgr_em (include/bwgr.h); returns dict(mu, b, d, hat, vbvec, scal, iters)."""
    P, own = _as_panel(gen, **panel_kw)
    try:
        yv = np.ascontiguousarray(y, np.float32)
        assert yv.size == P.n, "length(y) must equal nrow(gen)"
        b = np.empty(P.p, np.float32); d = np.zeros(P.p, np.float32); hat = np.empty(P.n, np.float32); vbv = np.empty(P.p, np.float32)
        scal = np.zeros(6, np.float32); mu = C.c_float(); iters = C.c_int()
        Dv = None if D is None else np.ascontiguousarray(D, np.float32)
        if Dv is not None:
            assert Dv.size == P.p, "length(D) must equal ncol(gen)"
        check(_lib.lib().bwgr_em(P._h, _EM[model], _fp(yv), float(df), float(R2), float(par), None if Dv is None else _fp(Dv),
                                 int(maxit), C.byref(mu), _fp(b), _fp(d), _fp(hat), _fp(vbv), _fp(scal), C.byref(iters)))
        return {"mu": float(mu.value), "b": b, "d": d, "hat": hat, "vbvec": vbv, "scal": [float(v) for v in scal], "iters": int(iters.value)}
    finally:
        if own:
            P.close()


def emRR(y, gen, df=10, R2=0.5, **kw):
    """emRR(y, gen, df = 10, R2 = 0.5), src/Rcpp20260726ai.cpp:308-354: list(mu, b, hat, Va, Ve, h2)."""
    r = _em("emRR", y, gen, df, R2, **kw); s = r["scal"]
    return {"mu": r["mu"], "b": r["b"], "hat": r["hat"], "Va": s[0], "Ve": s[1], "h2": s[2]}


def emBA(y, gen, df=10, R2=0.5, **kw):
    """emBA(y, gen, df = 10, R2 = 0.5), src/Rcpp20260726ai.cpp:80-128: list(mu, b, hat, Vb, Ve, h2)."""
    r = _em("emBA", y, gen, df, R2, **kw); s = r["scal"]
    return {"mu": r["mu"], "b": r["b"], "hat": r["hat"], "Vb": r["vbvec"], "Ve": s[1], "h2": s[2]}


def emBB(y, gen, df=10, R2=0.5, Pi=0.75, **kw):
    """emBB(y, gen, df = 10, R2 = 0.5, Pi = 0.75), src/Rcpp20260726ai.cpp:131-187: list(mu, b, d, hat, Vb, Ve, h2)."""
    r = _em("emBB", y, gen, df, R2, Pi, **kw); s = r["scal"]
    return {"mu": r["mu"], "b": r["b"], "d": r["d"], "hat": r["hat"], "Vb": r["vbvec"], "Ve": s[1], "h2": s[2]}


def emBC(y, gen, df=10, R2=0.5, Pi=0.75, **kw):
    """emBC(y, gen, df = 10, R2 = 0.5, Pi = 0.75), src/Rcpp20260726ai.cpp:190-247: list(mu, b, d, hat, Vg, Va, Ve, h2)."""
    r = _em("emBC", y, gen, df, R2, Pi, **kw); s = r["scal"]
    return {"mu": r["mu"], "b": r["b"], "d": r["d"], "hat": r["hat"], "Vg": s[3], "Va": s[0], "Ve": s[1], "h2": s[2]}


def emBCpi(y, gen, df=10, R2=0.5, Pi=0.75, **kw):
    """emBCpi(y, gen, df = 10, R2 = 0.5, Pi = 0.75), src/Rcpp20260726ai.cpp:1502-1550 (natural marker order):
    list(mu, b, d, pi, hat, Vg, Va, Ve, h2)."""
    r = _em("emBCpi", y, gen, df, R2, Pi, **kw); s = r["scal"]
    return {"mu": r["mu"], "b": r["b"], "d": r["d"], "pi": s[4], "hat": r["hat"], "Vg": s[3], "Va": s[0], "Ve": s[1], "h2": s[2]}


def emDE(y, gen, R2=0.5, **kw):
    """emDE(y, gen, R2 = 0.5), src/Rcpp20260726ai.cpp:250-305: list(mu, b, hat, Vb, Ve, h2)."""
    r = _em("emDE", y, gen, 0.0, R2, **kw); s = r["scal"]
    return {"mu": r["mu"], "b": r["b"], "hat": r["hat"], "Vb": r["vbvec"], "Ve": s[1], "h2": s[2]}


def emBL(y, gen, R2=0.5, alpha=0.02, **kw):
    """emBL(y, gen, R2 = 0.5, alpha = 0.02), src/Rcpp20260726ai.cpp:357-397: list(mu, b, hat, h2)."""
    r = _em("emBL", y, gen, 0.0, R2, alpha, **kw)
    return {"mu": r["mu"], "b": r["b"], "hat": r["hat"], "h2": r["scal"][2]}


def emEN(y, gen, R2=0.5, alpha=0.02, **kw):
    """emEN(y, gen, R2 = 0.5, alpha = 0.02), src/Rcpp20260726ai.cpp:400-460: list(mu, b, hat, Va, Ve, h2)."""
    r = _em("emEN", y, gen, 0.0, R2, alpha, **kw); s = r["scal"]
    return {"mu": r["mu"], "b": r["b"], "hat": r["hat"], "Va": s[0], "Ve": s[1], "h2": s[2]}


def lasso(y, gen, **kw):
    """lasso(y, gen), src/Rcpp20260726ai.cpp:1463-1500 (natural marker order): list(mu, b, h2, hat, Lmb)."""
    r = _em("lasso", y, gen, 0.0, 0.5, 0.0, **kw); s = r["scal"]
    return {"mu": r["mu"], "b": r["b"], "h2": s[2], "hat": r["hat"], "Lmb": s[0]}


def emML(y, gen, D=None, **kw):
    """emML(y, gen, D = NULL), src/Rcpp20260726ai.cpp:463-521: list(mu, b, hat, h2, Vb, Va, Ve)."""
    r = _em("emML", y, gen, 0.0, 0.5, 0.0, D=D, **kw); s = r["scal"]
    return {"mu": r["mu"], "b": r["b"], "hat": r["hat"], "h2": s[2], "Vb": s[0], "Va": s[3], "Ve": s[1]}


def em_order(p, upto):
    """Marker order of sweep `upto` (0-based) of the EM family: std::shuffle with std::mt19937(0..upto) (host only)."""
    out = np.zeros(int(p), np.int32)
    check(_lib.lib().bwgr_em_order(int(p), int(upto), out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


def _fused2(base, y, X1, X2, it, bi, pi, df, R2, seed, rng_mode, **panel_kw):
    """BayesA2 / BayesB2 / BayesRR2(y, X1, X2, ...), src/Rcpp20260726ai.cpp:990-1218: two panels, one residual."""
    P1, own1 = _as_panel(X1, **panel_kw)
    own2 = not isinstance(X2, Panel)
    if not own2:
        P2 = X2
    else:
        # the two panels share the residual, hence the slab geometry: try X1's workgroup count for X2, else X2's for X1
        # (an fp32 panel takes fewer rows per slab than an int8 one)
        kw2 = dict(panel_kw); kw2.setdefault("nwg", P1.nwg)
        try:
            P2 = Panel(X2, **kw2)
        except BwgrError:
            if not own1:
                raise
            P2 = Panel(X2, **panel_kw)
            P1.close()
            kw1 = dict(panel_kw); kw1["nwg"] = P2.nwg
            P1 = Panel(X1, **kw1)
    try:
        assert P1.n == P2.n, "X1 and X2 must have the same rows"
        y = np.ascontiguousarray(y, np.float32)
        assert y.size == P1.n
        per = base != "BayesRR"
        b1 = np.zeros(P1.p, np.float32); d1 = np.zeros(P1.p, np.float32); vb1 = np.zeros(P1.p if per else 1, np.float32)
        b2 = np.zeros(P2.p, np.float32); d2 = np.zeros(P2.p, np.float32); vb2 = np.zeros(P2.p if per else 1, np.float32)
        hat = np.zeros(P1.n, np.float32)
        mu = np.zeros(1, np.float32); ve = np.zeros(1, np.float32); h2 = np.zeros(1, np.float32)
        check(_lib.lib().bwgr_bayes2(P1._h, P2._h, MODELS[base], _fp(y), float(it), float(bi), float(pi), float(df), float(R2),
                                      C.c_uint64(_seed(seed)), int(rng_mode), _fp(mu), _fp(b1), _fp(d1), _fp(vb1), _fp(b2), _fp(d2),
                                      _fp(vb2), _fp(ve), _fp(hat), _fp(h2)))
        out = {"hat": hat, "mu": float(mu[0]), "b1": b1, "b2": b2, "vb1": vb1 if per else float(vb1[0]),
               "vb2": vb2 if per else float(vb2[0]), "ve": float(ve[0]), "h2": float(h2[0])}
        if base == "BayesB":   # list order of :1146-1149
            out = {"mu": out["mu"], "b1": b1, "d1": d1, "vb1": vb1, "b2": b2, "d2": d2, "vb2": vb2, "ve": out["ve"], "hat": hat, "h2": out["h2"]}
        return out
    finally:
        if own2:
            P2.close()
        if own1:
            P1.close()


def BayesA2(y, X1, X2, it=1500, bi=500, df=5, R2=0.5, *, seed=None, rng_mode=0, **kw):
    return _fused2("BayesA", y, X1, X2, it, bi, 0.0, df, R2, seed, rng_mode, **kw)


def BayesB2(y, X1, X2, it=1500, bi=500, pi=0.95, df=5, R2=0.5, *, seed=None, rng_mode=0, **kw):
    return _fused2("BayesB", y, X1, X2, it, bi, pi, df, R2, seed, rng_mode, **kw)


def BayesRR2(y, X1, X2, it=1500, bi=500, df=5, R2=0.5, *, seed=None, rng_mode=0, **kw):
    return _fused2("BayesRR", y, X1, X2, it, bi, 0.0, df, R2, seed, rng_mode, **kw)


def sample_rows(seed, it, n, k, rp=False):
    """sort(sample(n, k, rp)) - 1 under the RNG contract (host only)."""
    out = np.zeros(int(k), np.int32)
    check(_lib.lib().bwgr_sample_rows(C.c_uint64(_seed(seed)), C.c_uint32(int(it)), int(n), int(k), int(bool(rp)),
                                       out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


def _cor_last(dta):
    """cor(dta, use = 'p')[-m, m]: Pearson correlation of every column with the last one over pairwise complete rows."""
    m = dta.shape[1]
    out = np.full(m - 1, np.nan)
    for i in range(m - 1):
        ok = np.isfinite(dta[:, i]) & np.isfinite(dta[:, m - 1])
        if ok.sum() > 1:
            out[i] = np.corrcoef(dta[ok, i], dta[ok, m - 1])[0, 1]
    return out


_CV_FITS = ("BayesA", "BayesB", "BayesC", "BayesL", "BayesRR", "BayesCpi", "BayesDpi")          # f1 .. f7, R/cv.R:124-130
_CV_NAMES = ("BayesA", "BayesB", "BayesC", "BayesL", "BayesCpi", "BayesDpi", "BayesRR")         # column labels, R/cv.R:132-133


def mcmcCV(y, gen, k=5, n=5, it=1500, bi=500, pi=0.95, df=5, R2=0.5, avg=True, llo=None, tbv=None, ReturnGebv=False, *,
           seed=None, **panel_kw):
    """mcmcCV(), R/cv.R:113-216: n random k-fold (or leave-level-out) cross-validation cycles of the seven fused samplers;
    every cycle stages its training rows once and runs the seven chains on that panel, side by side (fit_many).  Returns the predictive
    correlations like the reference (`avg`: one vector sorted decreasingly, else one row per cycle), rounded to 4
    digits, or list(cv, hat, beta) with ReturnGebv.  As in the reference, column i holds the predictions of fit f_i =
    (A, B, C, L, RR, Cpi, Dpi) but is *labelled* (A, B, C, L, Cpi, Dpi, RR) (R/cv.R:124-133).  Fold rows come from the
    RNG contract (iteration word = cycle number) instead of set.seed(cycle); sample()."""
    y = np.asarray(y, np.float64); gen = np.asarray(gen)
    N, p = gen.shape
    base = _seed(seed)
    if llo is None:
        Nk = int(round(N / k))
        cycles = [sample_rows(base, c + 1, N, Nk) for c in range(int(n))]
    else:
        llo = np.asarray(llo).astype(str)
        cycles = [np.nonzero(llo == lev)[0] for lev in dict.fromkeys(llo.tolist())]
    obs = y if tbv is None else np.asarray(tbv, np.float64)
    Ms, Bs = [], []
    for c, w in enumerate(cycles):
        keep = np.ones(N, bool); keep[w] = False
        P = Panel(np.ascontiguousarray(gen[keep]), **panel_kw)
        try:
            B = np.zeros((p, 7))
            ytr = y[keep].astype(np.float32)
            jobs = [dict(model=model, y=ytr, it=it, bi=bi, df=df, R2=R2, seed=(base + 1000003 * (c + 1) + i) & 0x7FFFFFFFFFFFFFFF,
                         **({"pi": pi} if model in ("BayesB", "BayesC") else {})) for i, model in enumerate(_CV_FITS)]
            for i, fit in enumerate(fit_many(P, jobs)):   # the seven chains side by side on the fold's training panel
                B[:, i] = fit["b"]
        finally:
            P.close()
        M = np.empty((len(w), 8))
        M[:, :7] = np.asarray(gen[w], np.float64) @ B
        M[:, 7] = obs[w]
        Ms.append(M); Bs.append(B)
    if avg:
        pa = _cor_last(np.vstack(Ms))
        order = np.argsort(-pa, kind="stable")
        cv = {_CV_NAMES[i]: round(float(pa[i]), 4) for i in order}
    else:
        cv = {"CV_%d" % (c + 1): {_CV_NAMES[i]: round(float(v), 4) for i, v in enumerate(_cor_last(M))} for c, M in enumerate(Ms)}
    if not ReturnGebv:
        return cv
    beta = sum(Bs) / len(Bs)
    hat = np.asarray(gen, np.float64) @ beta + np.nanmean(y)
    return {"cv": cv, "hat": hat, "beta": beta}


def KMUP(X, b, d, xx, e, L, Ve, pi, *, seed=None, it=0, rng_mode=0, **panel_kw):
    """One Gibbs sweep; returns list(b=, d=, e=) like src/Rcpp20260726ai.cpp:37.  Inputs are not modified."""
    P, own = _as_panel(X, **panel_kw)
    try:
        b = np.array(b, np.float32); d = np.array(d, np.float32); e = np.array(e, np.float32)
        xx = np.ascontiguousarray(xx, np.float32); L = np.ascontiguousarray(L, np.float32)
        assert b.size == P.p and d.size == P.p and xx.size == P.p and L.size == P.p and e.size == P.n
        check(_lib.lib().bwgr_kmup(P._h, _fp(b), _fp(d), _fp(xx), _fp(e), _fp(L), float(Ve), float(pi),
                                    C.c_uint64(_seed(seed)), C.c_uint32(int(it)), int(rng_mode)))
        return {"b": b, "d": d, "e": e}
    finally:
        if own:
            P.close()


def KMUP2(X, Use, b, d, xx, E, L, Ve, pi, *, seed=None, it=0, rng_mode=0, **panel_kw):
    """One Gibbs sweep on the row subsample Use (0-based, as wgr passes it: sort(sample(n, n*bag, rp)) - 1, R/wgr.R:68);
    returns list(b=, d=, e=) like src/Rcpp20260726ai.cpp:76 (e: the subsample's residuals).  Inputs are not modified."""
    P, own = _as_panel(X, **panel_kw)
    try:
        use = np.ascontiguousarray(np.asarray(Use), np.int32)
        b = np.array(b, np.float32); d = np.array(d, np.float32); E = np.ascontiguousarray(E, np.float32)
        xx = np.ascontiguousarray(xx, np.float32); L = np.ascontiguousarray(L, np.float32)
        assert b.size == P.p and d.size == P.p and xx.size == P.p and L.size == P.p and E.size == P.n
        e = np.zeros(use.size, np.float32)
        check(_lib.lib().bwgr_kmup2(P._h, use.ctypes.data_as(C.POINTER(C.c_int)), int(use.size), _fp(b), _fp(d), _fp(xx), _fp(E),
                                     _fp(e), _fp(L), float(Ve), float(pi), C.c_uint64(_seed(seed)), C.c_uint32(int(it)), int(rng_mode)))
        return {"b": b, "d": d, "e": e}
    finally:
        if own:
            P.close()


def wgr(y, X, it=1500, bi=500, th=1, bag=1, rp=False, iv=False, de=False, pi=0, df=5, R2=0.5, eigK=None, VarK=0.95,
        verb=False, *, seed=None, rng_mode=0, **panel_kw):
    """wgr(), R/wgr.R:2-169, device-resident.  eigK = {"values": ..., "vectors": ...} (R's eigen(K)) adds the
    polygenic kernel term; bag != 1 sweeps KMUP2 on sort(sample(n, n*bag, rp)) rows each iteration.  The two together
    are refused: the reference itself indexes out of bounds there (R/wgr.R:73-79).
    Returns wgr's list: mu, b, Vb, d, Ve, hat[, u, Vk], cxx (R/wgr.R:155-167)."""
    if bag != 1 and eigK is not None:
        raise NotImplementedError("wgr(bag != 1, eigK=...): undefined in the reference (a subsampled residual is indexed with "
                                  "full-length row ids, R/wgr.R:73-79)")
    y = np.asarray(y, np.float64)
    U0 = V = None
    if eigK is not None:                       # R/wgr.R:23-27
        Vall = np.asarray(eigK["values"], np.float64)
        pk = int(np.argmax((np.cumsum(Vall) / Vall.size) > VarK)) + 1
        U0 = np.asfortranarray(np.asarray(eigK["vectors"], np.float64)[:, :pk])
        V = np.ascontiguousarray(Vall[:pk])
    gen0 = None
    keep = None
    if np.isnan(y).any():   # R/wgr.R:34-39: drop rows with missing y (hat is still returned for every row of gen0)
        if isinstance(X, Panel) or hasattr(X, "data_ptr"):
            raise ValueError("missing y with a pre-staged X: drop the rows before staging X")
        keep = ~np.isnan(y)
        gen0 = np.asarray(X)
        y = y[keep]
    if not isinstance(X, Panel) and not hasattr(X, "data_ptr"):
        X = np.asarray(X)
        if np.issubdtype(X.dtype, np.floating) and np.isnan(X).any():   # R/wgr.R:12-18 mean imputation
            X = X.astype(np.float64, copy=True)
            cm = np.nanmean(X, axis=0); cm[np.isnan(cm)] = 0.0
            idx = np.where(np.isnan(X)); X[idx] = cm[idx[1]]
            if gen0 is not None:
                gen0 = X
        if keep is not None:
            X = X[keep]
    U = None
    if U0 is not None:
        U = np.asfortranarray(U0[keep] if keep is not None else U0)
    P, own = _as_panel(X, **panel_kw)
    try:
        n, p = P.n, P.p
        assert y.size == n, "length(y) must equal nrow(X)"
        per = bool(iv or de)
        b = np.zeros(p); d = np.zeros(p); Vb = np.zeros(p if per else 1); hat = np.zeros(n); u = np.zeros(n)
        mu = C.c_double(); Ve = C.c_double(); cxx = C.c_double(); Vk = C.c_double()
        yc = np.ascontiguousarray(y, np.float64)
        if U is None and bag == 1:
            check(_lib.lib().bwgr_wgr(P._h, _dp(yc), int(it), int(bi), int(th), int(bool(iv)), int(bool(de)), float(pi),
                                       float(df), float(R2), C.c_uint64(_seed(seed)), int(rng_mode), C.byref(mu), _dp(b), _dp(Vb),
                                       _dp(d), C.byref(Ve), _dp(hat), C.byref(cxx)))
        else:
            assert U is None or U.shape[0] == n
            check(_lib.lib().bwgr_wgr_ex(P._h, _dp(yc), int(it), int(bi), int(th), int(bool(iv)), int(bool(de)), float(pi),
                                          float(df), float(R2), C.c_uint64(_seed(seed)), int(rng_mode),
                                          _dp(U) if U is not None else None, _dp(V) if U is not None else None,
                                          C.c_int64(U.shape[1] if U is not None else 0), float(bag), int(bool(rp)), C.byref(mu),
                                          _dp(b), _dp(Vb), _dp(d), C.byref(Ve), _dp(hat), C.byref(cxx), _dp(u), C.byref(Vk)))
        if keep is not None:
            # HAT = B0 + gen0 %*% B (+ U0 %*% H) over ALL rows of gen0 (R/wgr.R:146-152): rows with missing y are predicted.
            # R-level post-processing in the reference too; the rows that were swept keep the device's values.
            full = np.empty(keep.size); full[keep] = hat
            miss = ~keep
            full[miss] = mu.value + np.asarray(gen0, np.float64)[miss] @ b
            if U is not None:
                Hk = np.linalg.lstsq(U, u, rcond=None)[0]      # u = U %*% H on the kept rows; recover H for the others
                ufull = U0 @ Hk
                full[miss] += ufull[miss]
                u = ufull
            hat = full
        out = {"mu": mu.value, "b": b, "Vb": Vb if per else float(Vb[0]), "d": d, "Ve": Ve.value, "hat": hat}
        if U is not None:
            out["u"] = u; out["Vk"] = Vk.value
        out["cxx"] = cxx.value
        return out
    finally:
        if own:
            P.close()


def debug_variates(seed, kind, marker0, count, it=0, purpose=0, nu=0.0, device=0):
    out = np.empty(count, np.float64)
    kinds = {"normal": 0, "uniform": 1, "chisq": 2}
    check(_lib.lib().bwgr_debug_variates(device, C.c_uint64(seed), kinds[kind], float(nu), C.c_uint32(marker0), C.c_uint32(it),
                                          C.c_uint32(purpose), int(count), _dp(out)))
    return out


def debug_live():
    """bwgr_debug_live: the (device arrays, streams, events) that the library's handles and running calls own in this process."""
    out = (C.c_int64 * 3)()
    check(_lib.lib().bwgr_debug_live(out))
    return tuple(out)


# ---- multi-trait ridge regression: MRR3 / MRR3F, mrr / mrr_float (bwgr_mrr, include/bwgr.h) ----
_MRR_OPTS = ["maxit", "tol", "TH", "NLfactor", "InnerGS", "NoInv", "HCS", "XFA", "ACS", "NumXFA", "R2", "gc0", "df0", "updateMu",
             "weight_prior_h2", "weight_prior_gc", "PenCor", "MinCor", "uncorH2below", "roundGCupFrom", "roundGCupTo", "roundGCdownFrom",
             "roundGCdownTo", "bucketGCfrom", "bucketGCto", "DeflateMax", "DeflateBy", "OneVarB", "OneVarE", "verbose"]   # BWGR_MRR_* order
MRR_KEYS = ("mu", "b", "hat", "h2", "GC", "vb", "ve", "MSx", "cnvB", "cnvH2", "cnvV", "b_Weights", "Its")


def _is_device_tensor(X):
    return type(X).__module__.split(".")[0] == "torch" and bool(getattr(X, "is_cuda", False))


def _mrr_traits(Y, single, nrow, who):
    Ym = np.asarray(Y, np.float64)
    if Ym.ndim == 1:
        Ym = Ym[:, None]
    if single:   # MRR3F receives float matrices (src/RcppEigen20230423.cpp:704)
        Ym = Ym.astype(np.float32).astype(np.float64)
    if Ym.ndim != 2 or Ym.shape[0] != nrow:
        raise BwgrError(1, "%s: Y has shape %s; nrow(Y) must equal nrow(X) = %d" % (who, Ym.shape, nrow))
    return np.asfortranarray(Ym)


def _mrr_opts(single, opts):
    o = np.array([float(opts[name]) for name in _MRR_OPTS], np.float64)
    if single:
        o = o.astype(np.float32).astype(np.float64)
        o[_MRR_OPTS.index("maxit")] = int(opts["maxit"])
    return o


def _mrr_dense(Y, D, single, opts, kw):
    """bwgr_mrr_dense: the design is dense(X) -- n x r float64 values on the host, or a torch tensor on the device, which stays there."""
    device = int(kw.pop("device", 0))
    if kw:
        raise BwgrError(1, "mrr: %s do(es) not apply to a dense design (only device=)" % sorted(kw))
    Xd = D.device_tensor()
    if Xd is not None:
        import torch
        device = Xd.device.index or 0
        if single:
            Xd = Xd.to(torch.float32).to(torch.float64)
        if Xd.stride(0) != 1 or (Xd.shape[1] > 1 and Xd.stride(1) < Xd.shape[0]):
            Xd = Xd.t().contiguous().t()
        n, r = int(Xd.shape[0]), int(Xd.shape[1])
        ldx = int(Xd.stride(1)) if r > 1 else n
        torch.cuda.synchronize(Xd.device)
        xptr, loc = C.c_void_p(Xd.data_ptr()), DEVICE
    else:
        Xh = D.Z
        if single:
            with np.errstate(over="ignore"):
                Xh = np.asfortranarray(Xh.astype(np.float32).astype(np.float64))
        n, r = Xh.shape
        ldx, xptr, loc = n, Xh.ctypes.data_as(C.c_void_p), HOST
    Yf = _mrr_traits(Y, single, n, "mrr")
    k = Yf.shape[1]
    o = _mrr_opts(single, opts)
    maxit = max(int(opts["maxit"]), 0)
    kk, rr = max(k, 1), max(r, 1)
    mu = np.zeros(kk); b = np.zeros((rr, kk), order="F"); hat = np.zeros((max(n, 1), kk), order="F")
    h2 = np.zeros(kk); GC = np.zeros((kk, kk), order="F"); vb = np.zeros((kk, kk), order="F"); ve = np.zeros(kk); MSx = np.zeros(kk)
    c1 = np.zeros(max(maxit, 1)); c2 = np.zeros(max(maxit, 1)); c3 = np.zeros(max(maxit, 1)); its = C.c_int()
    check(_lib.lib().bwgr_mrr_dense(device, xptr, loc, int(n), int(r), int(ldx), _dp(Yf), int(k), _dp(o), len(o), _dp(mu), _dp(b), _dp(hat), _dp(h2),
                                    _dp(GC), _dp(vb), _dp(ve), _dp(MSx), _dp(c1), _dp(c2), _dp(c3), C.byref(its)))
    n_it = int(its.value)
    vals = (mu, b, hat, h2, GC, vb, ve, MSx, c1[:n_it].copy(), c2[:n_it].copy(), c3[:n_it].copy(), np.ones((r, k)), n_it)
    return dict(zip(MRR_KEYS, vals))


def _mrr(Y, X, single, opts, panel_kw):
    """bwgr_mrr: Y is n x k (NaN = missing) or a vector (k = 1); returns the reference's list as a dict, in its order.  A design marked
    dense(X) goes to bwgr_mrr_dense; nothing else does."""
    if isinstance(X, dense):
        return _mrr_dense(Y, X, single, opts, dict(panel_kw))
    P, own = _as_panel(X, **panel_kw)
    try:
        Ym = np.asarray(Y, np.float64)
        if Ym.ndim == 1:
            Ym = Ym[:, None]
        if single:   # MRR3F receives float matrices (src/RcppEigen20230423.cpp:704)
            Ym = Ym.astype(np.float32).astype(np.float64)
        assert Ym.ndim == 2 and Ym.shape[0] == P.n, "nrow(Y) must equal nrow(X)"
        k = Ym.shape[1]
        Yf = np.asfortranarray(Ym)
        o = np.array([float(opts[name]) for name in _MRR_OPTS], np.float64)
        if single:
            o = o.astype(np.float32).astype(np.float64)
            o[_MRR_OPTS.index("maxit")] = int(opts["maxit"])
        maxit = max(int(opts["maxit"]), 0)
        kk = max(k, 1)
        mu = np.zeros(kk); b = np.zeros((P.p, kk), order="F"); hat = np.zeros((P.n, kk), order="F")
        h2 = np.zeros(kk); GC = np.zeros((kk, kk), order="F"); vb = np.zeros((kk, kk), order="F"); ve = np.zeros(kk); MSx = np.zeros(kk)
        c1 = np.zeros(max(maxit, 1)); c2 = np.zeros(max(maxit, 1)); c3 = np.zeros(max(maxit, 1)); its = C.c_int()
        check(_lib.lib().bwgr_mrr(P._h, _dp(Yf), int(k), _dp(o), len(o), _dp(mu), _dp(b), _dp(hat), _dp(h2), _dp(GC), _dp(vb), _dp(ve),
                                  _dp(MSx), _dp(c1), _dp(c2), _dp(c3), C.byref(its)))
        n_it = int(its.value)
        vals = (mu, b, hat, h2, GC, vb, ve, MSx, c1[:n_it].copy(), c2[:n_it].copy(), c3[:n_it].copy(), np.ones((P.p, k)), n_it)
        return dict(zip(MRR_KEYS, vals))
    finally:
        if own:
            P.close()


def MRR3(Y, X, maxit=500, tol=10e-9, cores=1, TH=False, NLfactor=0.0, InnerGS=False, NoInv=False, HCS=False, XFA=False, ACS=False,
         NumXFA=3, R2=0.5, gc0=0.5, df0=1.0, updateMu=False, weight_prior_h2=0.01, weight_prior_gc=0.01, PenCor=0.0, MinCor=1.0,
         uncorH2below=0.0, roundGCupFrom=1.0, roundGCupTo=1.0, roundGCdownFrom=1.0, roundGCdownTo=0.0, bucketGCfrom=1.0, bucketGCto=1.0,
         DeflateMax=0.9, DeflateBy=0.0, OneVarB=False, OneVarE=False, verbose=False, **kw):
    """MRR3(Y, X, ...), src/RcppEigen20230423.cpp:318-700 (R/RcppExports.R:180): multi-trait ridge regression by randomized
    Gauss-Seidel; NaN in Y = missing.  list(mu, b, hat, h2, GC, vb, ve, MSx, cnvB, cnvH2, cnvV, b_Weights, Its).  `cores` is
    ignored; InnerGS, NoInv, NLfactor, PenCor, MinCor, uncorH2below, round*, bucket* and DeflateBy are refused (BWGR_EINVAL) away
    from their defaults.  X is centred by its column means, as in the reference.  X is a Panel or what makes one (int8 genotypes), or
    dense(X): any real-valued n x r design (dosages, K2X's eigenvector design), swept in fp64 by the same launch train; a plain float
    matrix is never taken for one."""
    opts = dict(locals()); opts.pop("Y"); opts.pop("X"); opts.pop("kw"); opts.pop("cores")
    return _mrr(Y, X, False, opts, kw)


def MRR3F(Y, X, maxit=500, tol=10e-9, cores=1, TH=False, NonLinearFactor=0.0, InnerGS=False, NoInv=False, HCS=False, XFA=False, ACS=False,
          NumXFA=3, R2=0.5, gc0=0.5, df0=1.0, updateMu=False, weight_prior_h2=0.01, weight_prior_gc=0.01, PenCor=0.0, MinCor=1.0,
          uncorH2below=0.0, roundGCupFrom=1.0, roundGCupTo=1.0, roundGCdownFrom=1.0, roundGCdownTo=0.0, bucketGCfrom=1.0, bucketGCto=1.0,
          DeflateMax=0.9, DeflateBy=0.0, OneVarB=False, OneVarE=False, verbose=False, **kw):
    """MRR3F(Y, X, ...), src/RcppEigen20230423.cpp:704-1080 (R/RcppExports.R:184): MRR3's algorithm on float inputs.  Y and the
    real options are rounded to float as the reference receives them; the engine itself is fp64."""
    opts = dict(locals()); opts.pop("Y"); opts.pop("X"); opts.pop("kw"); opts.pop("cores")
    opts["NLfactor"] = opts.pop("NonLinearFactor")
    return _mrr(Y, X, True, opts, kw)


def mrr(Y, X, **kw):
    """mrr(Y, X, ...) = MRR3(Y, X, ...), R/mix.R:1271."""
    return MRR3(Y, X, **kw)


def mrr_float(Y, X, **kw):
    """mrr_float(Y, X, ...) = MRR3F(Y, X, ...), R/mix.R:1273."""
    return MRR3F(Y, X, **kw)


def K2X(K, MinEV=1e-8, cores=1):
    """K2X(K, MinEV = 1e-8, cores = 1), src/RcppEigen20230423.cpp:1942-1948 (R/RcppExports.R:256): the design of a relationship matrix,
    U[:, :NPC] diag(D[:NPC]) with U the left singular vectors and D the singular values of K in decreasing order, NPC the number of
    D > MinEV.  For a symmetric K these are its eigenvectors and |eigenvalues|, which is how they are computed here (numpy.linalg.eigh in
    fp64; torch.linalg.eigh when K is a torch tensor on the device, and the result stays there).  Note the reference's scaling: U times D,
    not U times sqrt(D), so X X' = K K (not K) -- mkr therefore fits the kernel K^2.  The values are rounded to float once (the reference
    returns a float matrix) and returned as float64, n x NPC, column-major.
    Departure: the reference counts NPC on a float SVD, whose noise (about 1e-7 of the largest singular value) lies above MinEV, so it keeps
    the null directions of a rank-deficient K with a negligible scale; here the count is made on the fp64 spectrum.  A K that is not
    square, or not symmetric to 1e-6 of its largest entry, is refused.  `cores` is ignored."""
    if _is_device_tensor(K):
        import torch
        Kt = K.to(torch.float64)
        if Kt.dim() != 2 or Kt.shape[0] != Kt.shape[1]:
            raise BwgrError(1, "K2X: K has shape %s; it must be square" % (tuple(Kt.shape),))
        scale = float(Kt.abs().max()) if Kt.numel() else 0.0
        if float((Kt - Kt.t()).abs().max()) > 1e-6 * scale:
            raise BwgrError(1, "K2X: K is not symmetric (to 1e-6 of its largest entry)")
        w, V = torch.linalg.eigh((Kt + Kt.t()) * 0.5)
        idx = torch.argsort(w.abs(), descending=True, stable=True)
        npc = int((w.abs() > float(MinEV)).sum())
        idx = idx[:npc]
        X = (V[:, idx] * w.abs()[idx]).to(torch.float32).to(torch.float64)
        return X.t().contiguous().t()          # column-major
    Km = np.asarray(K, np.float64)
    if Km.ndim != 2 or Km.shape[0] != Km.shape[1]:
        raise BwgrError(1, "K2X: K has shape %s; it must be square" % (Km.shape,))
    if not np.all(np.isfinite(Km)):
        raise BwgrError(1, "K2X: K has an entry that is not finite")
    scale = float(np.abs(Km).max()) if Km.size else 0.0
    if Km.size and float(np.abs(Km - Km.T).max()) > 1e-6 * scale:
        raise BwgrError(1, "K2X: K is not symmetric (to 1e-6 of its largest entry)")
    w, V = np.linalg.eigh((Km + Km.T) * 0.5)
    aw = np.abs(w)
    idx = np.argsort(-aw, kind="stable")
    idx = idx[:int(np.sum(aw > float(MinEV)))]
    with np.errstate(over="ignore"):
        return np.asfortranarray((V[:, idx] * aw[idx]).astype(np.float32).astype(np.float64))


def mkr(Y, K, **kw):
    """mkr(Y, K, ...) = MRR3(Y, K2X(K), ...), R/mix.R:1275: multi-trait kernel regression.  The list is MRR3's, so `b` holds the effects of
    K2X's eigenvector columns (their signs are the eigensolver's; mu, hat, h2, GC, vb and ve do not depend on them).  K may be a torch
    tensor on the device (GRM(..., device_out=True)): the decomposition and the design then stay there.  device= as for mrr(Y, dense(X))."""
    return MRR3(Y, dense(K2X(K)), **kw)


def mrr_dense_plan(n, r, k, npat):
    """bwgr_debug_mrr_dense_plan (host arithmetic, no GPU) of mrr(Y, dense(X)) / mkr for n rows, r columns, k traits, npat missingness
    patterns: the padded rows, the blocks of a sweep and the last one's width, the row tiles, the grids, the solve's linv_lds and ngl, the
    LDS bytes of the kernels and the device workspace."""
    out = (C.c_int64 * 15)()
    check(_lib.lib().bwgr_debug_mrr_dense_plan(int(n), int(r), int(k), int(npat), out))
    names = ("ld", "nblk", "edge", "tiles", "pass_wg", "trips", "cols_wg", "hat_wg", "linv_lds", "ngl", "lds_gram", "lds_pass", "lds_solve", "lds_linv", "ws_bytes")
    return dict(zip(names, [int(v) for v in out]))


SWEEP_PLAN_FIELDS = (("engine", "gate", "gate3_bits", "lag", "nfeed", "g16", "R3", "K3", "sub", "pf", "pf2", "dbg3", "qsplit", "skip_vb", "fixed3", "fx", "nd",
                      "npf", "ahead", "nq", "wsub", "wK3", "guarded", "draws", "nspins")
                     + tuple("spin%d_%s" % (i, f) for i in range(3) for f in ("kernel", "grid", "resident", "threads", "lds"))
                     + tuple("redo_" + f for f in ("engine", "lag", "nfeed", "g16", "fx", "nd", "npf", "ahead", "nq", "wsub", "wK3"))
                     + ("spin_run", "spin_redo", "escale_reset", "pre3", "cen3", "escale_w", "affine_inv", "cen_pre", "spec", "spec_sel", "cen_run", "cen_redo",
                        "redo_spec", "redo_cen", "vb_fill", "withhold"))


def sweep_plan(is_f32, n, p, block=0, nwg=0, kind=0, xmax=2, gram16=True, flags=0, blk_begin=0, blk_end=0, mode=0, state=0):
    """bwgr_debug_sweep_plan (host arithmetic, no GPU): every field of the plan of one sweep -- engine, gate, depth, launch shapes, the redo,
    the helper kernels -- over a panel planned as bwgr_debug_panel_plan plans it under the BWGR_* switches of the environment.  flags: the
    sweep's SWF_* bits; mode 0 a sweep alone, 1 its redo, 2 a pair; state: bit 0 clones alive, 1 a clone, 2 crowded, 3 withheld.  The fields are
    described in include/bwgr.h; a combination the library never plans raises BwgrError."""
    out = (C.c_int64 * len(SWEEP_PLAN_FIELDS))()
    check(_lib.lib().bwgr_debug_sweep_plan(int(bool(is_f32)), int(n), int(p), int(block), int(nwg), int(kind), int(xmax), int(bool(gram16)), int(flags),
                                           int(blk_begin), int(blk_end), int(mode), int(state), out))
    return dict(zip(SWEEP_PLAN_FIELDS, [int(v) for v in out]))


# ---- PEGS / PEGSZ: multi-trait fits over several designs (bwgr_pegs, include/bwgr.h) ----
PEGS_KEYS = ("mu", "b", "hat", "h2", "GC", "bend", "numit", "cnv")


class dense:
    """Marks a matrix as a dense effect of PEGS / PEGSZ: dense(Z) is swept as n x q float64 values by the dense leg, whatever it holds.
    Without the marker a Panel, an int8 or integer matrix and an integer-valued float matrix within int8 range are panel effects (staged as
    int8, as mrr stages its X), and a float matrix with a non-integer value is a dense effect."""

    def __init__(self, Z):
        self._dev = None
        if _is_device_tensor(Z):     # stays on the device (mrr / mkr read it there); a host copy is made only where .Z is asked for
            import torch
            Zt = Z.to(torch.float64)
            if Zt.dim() == 1:
                Zt = Zt[:, None]
            if Zt.dim() != 2:
                raise BwgrError(1, "dense: Z has shape %s; it must be n x q" % (tuple(Zt.shape),))
            self._dev, self._Z = Zt, None
            return
        Zm = np.asarray(Z, np.float64)
        if Zm.ndim == 1:
            Zm = Zm[:, None]
        if Zm.ndim != 2:
            raise BwgrError(1, "dense: Z has shape %s; it must be n x q" % (Zm.shape,))
        self._Z = np.asfortranarray(Zm)

    @property
    def Z(self):
        if self._Z is None:
            self._Z = np.asfortranarray(self._dev.cpu().numpy())
        return self._Z

    def device_tensor(self):
        """the torch tensor this design was made of, where it lives on the device; else None"""
        return self._dev


def _is_scipy_sparse(S):
    return type(S).__module__.split(".")[0] == "scipy" and hasattr(S, "tocsc")


class sparse:
    """Marks a design as a sparse effect of PEGS / PEGSZ / PEGSX (and is what PEGS_sparse / PEGSZ_sparse sweep): an n x q column-compressed
    matrix -- the incidence matrix of environments, locations, blocks or genotype-by-environment cells -- that takes nnz + q k^2 values on the
    device, never n q.  sparse(S) accepts
      (data, indices, indptr) with shape=(n, q): the CSC arrays as they are (row indices strictly increasing within a column);
      any scipy.sparse matrix: through .tocsc() with duplicates summed and indices sorted (scipy is imported only when given one);
      a 2-D array: its nonzeros are taken.
    The values are rounded to float once, as the reference casts S to float (src/RcppEigenX20251203.cpp:821, :1028); the engine is fp64.
    Where no row occurs in two columns the engine updates all columns at once; serial=True forces the one-wave leg that walks the columns in
    the sweep's order (for tests and tools/pegs_sparse_probe.py) -- on such a matrix both give the same bits."""

    def __init__(self, S, shape=None, serial=False):
        if isinstance(S, sparse):
            data, indices, indptr, shape = S.data, S.indices, S.indptr, S.shape
        elif _is_scipy_sparse(S):
            import scipy.sparse  # noqa: F401  (only here)
            M = S.tocsc(copy=True)
            M.sum_duplicates()
            M.sort_indices()
            data, indices, indptr, shape = M.data, M.indices, M.indptr, M.shape
        elif isinstance(S, tuple) and len(S) == 3:
            if shape is None or len(shape) != 2:
                raise BwgrError(1, "sparse: (data, indices, indptr) needs shape=(n, q)")
            data, indices, indptr = S
        else:
            A = np.asarray(S)
            if A.ndim == 1:
                A = A[:, None]
            if A.ndim != 2:
                raise BwgrError(1, "sparse: S has shape %s; it must be n x q" % (A.shape,))
            cols, rows = np.nonzero(A.T)        # (by column, rows ascending within one)
            data, indices, shape = A[rows, cols], rows, A.shape
            indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=A.shape[1]))])
        with np.errstate(over="ignore"):
            self.data = np.ascontiguousarray(np.asarray(data, np.float64).ravel().astype(np.float32).astype(np.float64))
        ind, ptr = np.asarray(indices).ravel(), np.asarray(indptr).ravel()
        if ind.size and (ind.min() < -2 ** 31 or ind.max() >= 2 ** 31):
            raise BwgrError(1, "sparse: a row index does not fit 32 bits")
        self.indices = np.ascontiguousarray(ind.astype(np.int32))
        self.indptr = np.ascontiguousarray(ptr.astype(np.int64))
        self.shape = (int(shape[0]), int(shape[1]))
        self.serial = bool(serial)
        if self.indptr.size != self.shape[1] + 1 or self.data.size != self.indices.size or (self.indptr.size and self.indptr[-1] > self.data.size):
            raise BwgrError(1, "sparse: %d values, %d indices and %d column pointers do not describe %d columns" %
                            (self.data.size, self.indices.size, self.indptr.size, self.shape[1]))

    def toarray(self):
        """the dense n x q copy (float64, column-major); entries stored twice are summed"""
        A = np.zeros(self.shape, order="F")
        cols = np.repeat(np.arange(self.shape[1]), np.diff(self.indptr))
        np.add.at(A, (self.indices[:len(cols)], cols), self.data[:len(cols)])
        return A


def pegs_sparse_plan(n, q, nnz, max_col_nnz, k, disjoint):
    """bwgr_debug_pegs_sparse_plan (host arithmetic, no GPU) for a sparse effect of n rows, q columns and nnz stored entries (at most
    max_col_nnz in a column), k traits: the threads per workgroup and the workgroups of the set-up kernel and of the two legs, the columns one
    trip of the disjoint grid covers, the leg a sweep takes ("disjoint" exactly when the matrix is row-disjoint) and the device workspace."""
    out = (C.c_int64 * 9)()
    check(_lib.lib().bwgr_debug_pegs_sparse_plan(int(n), int(q), int(nnz), int(max_col_nnz), int(k), int(bool(disjoint)), out))
    r = dict(zip(("setup_threads", "setup_wg", "serial_threads", "serial_wg", "disjoint_threads", "disjoint_wg", "trip_cols", "leg", "ws_bytes"), [int(v) for v in out]))
    r["leg"] = "disjoint" if r["leg"] else "serial"
    return r


def pegs_plan(n, q, k):
    """bwgr_debug_pegs_plan (host arithmetic, no GPU): dict(threads, lds_bytes, ws_bytes) of the dense leg."""
    out = (C.c_int64 * 3)()
    check(_lib.lib().bwgr_debug_pegs_plan(int(n), int(q), int(k), out))
    return dict(zip(("threads", "lds_bytes", "ws_bytes"), [int(v) for v in out]))


def _pegs_effect(X, panel_kw):
    """(Panel, made here), (dense, False) or (sparse, False): the rule of `dense`'s docstring; a `sparse` passes through and a scipy.sparse
    matrix is one."""
    if isinstance(X, Panel):
        return X, False
    if isinstance(X, (dense, sparse)):
        return X, False
    if _is_scipy_sparse(X):
        return sparse(X), False
    if hasattr(X, "data_ptr"):
        return Panel(X, **panel_kw), True
    Xm = np.asarray(X)
    if Xm.ndim == 1:
        Xm = Xm[:, None]
    if Xm.ndim != 2:
        raise BwgrError(1, "pegs: an effect has shape %s; it must be n x p" % (Xm.shape,))
    if np.issubdtype(Xm.dtype, np.integer) or Xm.dtype == np.bool_:
        return Panel(Xm, **panel_kw), True
    Xm = Xm.astype(np.float64, copy=False)
    if Xm.size and np.all(np.isfinite(Xm)) and np.all(Xm == np.rint(Xm)) and Xm.min() >= -128 and Xm.max() <= 127:
        return Panel(Xm, as_int8=True, **panel_kw), True
    return dense(Xm), False


class _Eff(C.Structure):
    """bwgr_pegs_effect_ex"""
    _fields_ = [("panel", C.c_void_p), ("Z", C.c_void_p), ("q", C.c_int64), ("ldz", C.c_int64),
                ("colptr", C.c_void_p), ("rowidx", C.c_void_p), ("val", C.c_void_p), ("flags", C.c_int64)]


def _eff_rows(E):
    return E.n if isinstance(E, Panel) else E.shape[0] if isinstance(E, sparse) else E.Z.shape[0]


@contextlib.contextmanager
def _pegs_effects(X_list, panel_kw, round_dense):
    """Opens an effect list through _pegs_effect: (effs, the bwgr_pegs_effect_ex array, every effect's column count), and closes the panels made
    here when the block ends.  round_dense: a dense Z is rounded to float (the copies live as long as the block)."""
    effs, made, keep, ps = [], [], [], []
    try:
        for X in X_list:
            E, own = _pegs_effect(X, panel_kw)
            effs.append(E)
            if own:
                made.append(E)
        ce = (_Eff * max(len(effs), 1))()   # (zeros)
        for i, E in enumerate(effs):
            if isinstance(E, Panel):
                ce[i].panel = E._h.value
                ps.append(E.p)
            elif isinstance(E, sparse):
                ce[i].colptr = E.indptr.ctypes.data; ce[i].rowidx = E.indices.ctypes.data; ce[i].val = E.data.ctypes.data
                ce[i].q = E.shape[1]; ce[i].flags = 1 if E.serial else 0
                ps.append(E.shape[1])
            else:
                keep.append(np.asfortranarray(E.Z.astype(np.float32).astype(np.float64)) if round_dense else E.Z)
                ce[i].Z = keep[-1].ctypes.data; ce[i].q = keep[-1].shape[1]; ce[i].ldz = max(keep[-1].shape[0], 1)
                ps.append(keep[-1].shape[1])
        yield effs, ce, ps
    finally:
        for P in made:
            P.close()


def _pegs(Y, X_list, maxit, logtol, covbend, covMinEv, XFA, NNC, text, device, cnv_trace, panel_kw):
    with _pegs_effects(X_list, dict(panel_kw, device=device), False) as (effs, ce, ps):
        if not effs:
            raise BwgrError(1, "pegs: X_list holds no effects")
        Ym = np.asarray(Y, np.float64)
        if Ym.ndim == 1:
            Ym = Ym[:, None]
        Ym = Ym.astype(np.float32).astype(np.float64)   # PEGS receives float matrices (src/RcppEigenX20251203.cpp:10)
        rows = [_eff_rows(E) for E in effs]
        n = rows[0]
        if any(r != n for r in rows):
            raise BwgrError(1, "pegs: the effects have %s rows; all must have the same" % (rows,))
        if Ym.ndim != 2 or Ym.shape[0] != n:
            raise BwgrError(1, "pegs: Y has shape %s; nrow(Y) must equal nrow(X) = %d" % (Ym.shape, n))
        k = Ym.shape[1]
        Yf = np.asfortranarray(Ym)
        neff, kk = len(effs), max(k, 1)
        f32 = lambda v: float(np.float32(v))   # the real options are floats there
        mu = np.zeros(kk); hat = np.zeros((n, kk), order="F"); h2 = np.zeros(kk); bend = np.zeros(neff)
        b = [np.zeros((p_, kk), order="F") for p_ in ps]; GC = [np.zeros((kk, kk), order="F") for _ in ps]
        bp = (C.c_void_p * neff)(*[a.ctypes.data for a in b]); gp = (C.c_void_p * neff)(*[a.ctypes.data for a in GC])
        cnv = np.zeros(max(int(maxit), 1)); its = C.c_int()
        check(_lib.lib().bwgr_pegs_ex(int(device), C.cast(ce, C.c_void_p), neff, _dp(Yf), int(n), int(k), int(maxit), f32(logtol), f32(covbend), f32(covMinEv),
                                   int(XFA), int(bool(NNC)), int(text), _dp(mu), C.cast(bp, C.c_void_p), _dp(hat), _dp(h2), C.cast(gp, C.c_void_p),
                                   _dp(bend), C.byref(its), _dp(cnv)))
        nit = int(its.value)
        out = dict(zip(PEGS_KEYS, (mu, b, hat, h2, GC, bend, nit, float(cnv[max(nit, 1) - 1]))))
        if cnv_trace:
            out["cnv_trace"] = cnv[:nit].copy()
        return out


def PEGS(Y, X, maxit=100, logtol=-4.0, covbend=1.1, covMinEv=10e-4, XFA=-1, NNC=True, *, device=0, cnv_trace=False, **kw):
    """PEGS(Y, X, ...), src/RcppEigenX20251203.cpp:10-194 (R/RcppExports.R:280): the pseudo-expectation Gauss-Seidel fit of k correlated
    traits (NaN in Y = missing) on one design, which is NOT centred.  list(mu, b, hat, h2, GC, bend, numit, cnv) as a dict; b is p x k, GC k x k
    and bend a number.  X is an effect as `dense` describes.  Y and the real options are rounded to float as the reference receives them;
    the engine is fp64.  The marker order of sweep s is em_order(p, s) (the reference's order is seeded from the machine and cannot be
    reproduced).  cnv_trace=True adds "cnv_trace", cnv after every sweep."""
    r = _pegs(Y, [X], maxit, logtol, covbend, covMinEv, XFA, NNC, 1, device, cnv_trace, kw)
    r["b"], r["GC"], r["bend"] = r["b"][0], r["GC"][0], float(r["bend"][0])
    return r


def PEGSZ(Y, X_list, maxit=100, logtol=-4.0, covbend=1.1, covMinEv=10e-4, XFA=-1, NNC=True, *, device=0, cnv_trace=False, **kw):
    """PEGSZ(Y, X_list, ...), src/RcppEigenX20251203.cpp:576-808 (R/RcppExports.R:288): PEGS over a list of designs, swept one after another
    in list order against one residual, each with its own k x k covariance.  Every element of X_list is an effect as `dense` describes: a
    Panel / integer matrix (int8 genotypes on the device), a dense float matrix / dense(Z) or a sparse one (sparse(S) or a scipy.sparse
    matrix: an incidence matrix held column-compressed); all have the same n, all panels live on one
    device and are made with the same block / nwg.  device= matters only when no effect is a panel.  Returns PEGS's dict with b and GC as
    lists (one entry per effect) and bend as a vector."""
    return _pegs(Y, list(X_list), maxit, logtol, covbend, covMinEv, XFA, NNC, 0, device, cnv_trace, kw)


def PEGS_sparse(Y, S, maxit=100, logtol=-4.0, covbend=1.1, covMinEv=10e-4, XFA=-1, NNC=True, *, device=0, cnv_trace=False, **kw):
    """PEGS_sparse(Y, S, ...), src/RcppEigenX20251203.cpp:811-1007 (R/RcppExports.R:292): PEGS on one sparse design.  S is whatever `sparse`
    accepts (a `sparse`, a scipy.sparse matrix, a 2-D array whose nonzeros are taken); its values are rounded to float as the reference casts
    them.  Returns PEGS's dict.  The text is PEGS's own (the intercept step divides by n_t - 1, :977)."""
    r = _pegs(Y, [S if isinstance(S, sparse) else sparse(S)], maxit, logtol, covbend, covMinEv, XFA, NNC, 1, device, cnv_trace, kw)
    r["b"], r["GC"], r["bend"] = r["b"][0], r["GC"][0], float(r["bend"][0])
    return r


def PEGSZ_sparse(Y, X_list, maxit=100, logtol=-4.0, covbend=1.1, covMinEv=10e-4, XFA=-1, NNC=True, *, device=0, cnv_trace=False, **kw):
    """PEGSZ_sparse(Y, X_list, ...), src/RcppEigenX20251203.cpp:1010-1250 (R/RcppExports.R:296): PEGSZ over a list of sparse designs, under
    that function's own text -- its intercept step divides the residual sums by n_t (:1202) where PEGSZ divides by n_t - 1.  Every element
    of X_list that is not already an effect (`sparse`, `dense`, Panel) is made a `sparse`; the reference takes sparse designs only, here any
    mix of effect kinds runs under this text.  Returns PEGSZ's dict."""
    effs = [X if isinstance(X, (sparse, dense, Panel)) else sparse(X) for X in X_list]
    return _pegs(Y, effs, maxit, logtol, covbend, covMinEv, XFA, NNC, 2, device, cnv_trace, kw)


# ---- PEGSX: fixed effects beside the random effects of the multi-trait fit (bwgr_pegsx, include/bwgr.h) ----
PEGSX_KEYS = ("TrZSZ", "b", "u", "vb_list", "GC_list", "ve", "hat", "its", "cnv", "bend")


def pegsx_plan(n, f, k):
    """bwgr_debug_pegsx_plan (host arithmetic, no GPU): dict(threads, lds_bytes, ws_bytes) of the fixed step and (jc, fc, trace_lds_bytes),
    the trace kernels' tiling."""
    out = (C.c_int64 * 6)()
    check(_lib.lib().bwgr_debug_pegsx_plan(int(n), int(f), int(k), out))
    return dict(zip(("threads", "lds_bytes", "ws_bytes", "jc", "fc", "trace_lds_bytes"), [int(v) for v in out]))


def pegs_launch_plan(n, m):
    """bwgr_debug_pegs_launch_plan (host arithmetic, no GPU) for n rows and an effect of m columns: dict(trace_wg, trace_cols, setup_wg,
    setup_cols, leg_threads, fixed_threads) -- the trace kernels' workgroups and the columns one trip of them covers, the same of
    k_pegs_dense_setup, the threads of k_pegs_dense_leg and of k_pegsx_fixed."""
    out = (C.c_int64 * 6)()
    check(_lib.lib().bwgr_debug_pegs_launch_plan(int(n), int(m), out))
    return dict(zip(("trace_wg", "trace_cols", "setup_wg", "setup_cols", "leg_threads", "fixed_threads"), [int(v) for v in out]))


def pegsx_timing(mode):
    """bwgr_debug_pegsx_timing: sets the timing mode of the PEGSX calls that follow (0 off, 1 set-up and sweeps, 2 and the fixed step) and
    returns what the last timed call left, in ms."""
    out = (C.c_double * 9)()
    check(_lib.lib().bwgr_debug_pegsx_timing(int(mode), out))
    v = [float(x) for x in out]
    return dict(trace_ms=v[0], setup_cols_ms=v[1], sweeps=int(v[2]), sweep_ms=dict(mean=v[3], min=v[4], max=v[5]), fixed_ms=dict(mean=v[6], min=v[7], max=v[8]))


def PEGSX(Y, X, Z_list, maxit=500, logtol=-8.0, covbend=1.1, covMinEv=10e-4, cores=1, verbose=False, df0=1.1, NNC=False, InnerGS=False, NoInv=False,
          XFA=False, NumXFA=3, *, device=0, cnv_trace=False, **kw):
    """PEGSX(Y, X, Z_list, ...), src/RcppEigenX20251203.cpp:197-573 (R/RcppExports.R:284): Y = X b + sum_r Z_r u_r + E for k correlated
    traits (NaN in Y = missing) -- a fixed design X (n x f, an intercept is a column of it; nothing is centred) beside the random effects of
    Z_list, each an effect as `dense` and `sparse` describe and swept as PEGSZ sweeps it.  list(TrZSZ, b, u, vb_list, GC_list, ve, hat, its, cnv, bend)
    as a dict: TrZSZ, u, vb_list and GC_list are lists with one entry per effect, b is f x k, bend a vector.  Y, X, dense Z and the real
    options are rounded to float as the reference receives them; the engine is fp64.  The marker order of sweep s is em_order(m, s) per effect.
    InnerGS=True and NoInv=True are refused; cores and verbose are accepted and ignored; XFA=True with NumXFA <= 0 is XFA=False.
    cnv_trace=True adds "cnv_trace", cnv after every sweep."""
    with _pegs_effects(list(Z_list), dict(kw, device=device), True) as (effs, ce, ps):   # (a dense Z is a float matrix there, :266)
        f32 = lambda v: float(np.float32(v))   # the real options are floats there
        Ym = np.asarray(Y, np.float64)
        if Ym.ndim == 1:
            Ym = Ym[:, None]
        Xm = np.asarray(X, np.float64)
        if Xm.ndim == 1:
            Xm = Xm[:, None]
        if Ym.ndim != 2 or Xm.ndim != 2:
            raise BwgrError(1, "pegsx: Y has shape %s and X %s; both must be matrices" % (Ym.shape, Xm.shape))
        Yf = np.asfortranarray(Ym.astype(np.float32).astype(np.float64))
        with np.errstate(over="ignore"):
            Xf = np.asfortranarray(Xm.astype(np.float32).astype(np.float64))
        n, k = Yf.shape
        if Xf.shape[0] != n:
            raise BwgrError(1, "pegsx: X has %d rows, Y %d; nrow(X) must equal nrow(Y)" % (Xf.shape[0], n))
        rows = [_eff_rows(E) for E in effs]
        if any(r != n for r in rows):
            raise BwgrError(1, "pegsx: the effects have %s rows, Y %d; all must have the same rows" % (rows, n))
        f, neff, kk = Xf.shape[1], len(effs), max(k, 1)
        Tr = np.zeros((max(neff, 1), kk)); b = np.zeros((max(f, 1), kk), order="F"); ve = np.zeros(kk); hat = np.zeros((n, kk), order="F"); bend = np.zeros(max(neff, 1))
        u = [np.zeros((p_, kk), order="F") for p_ in ps]
        vb = [np.zeros((kk, kk), order="F") for _ in ps]; GC = [np.zeros((kk, kk), order="F") for _ in ps]
        ptrs = lambda arrs: C.cast((C.c_void_p * max(neff, 1))(*[a.ctypes.data for a in arrs]), C.c_void_p)
        cnv = np.zeros(max(int(maxit), 1)); its = C.c_int()
        check(_lib.lib().bwgr_pegsx_ex(int(device), C.cast(ce, C.c_void_p), neff, _dp(Xf), max(n, 1), int(f), _dp(Yf), int(n), int(k), int(maxit), f32(logtol),
                                    f32(covbend), f32(covMinEv), f32(df0), int(bool(NNC)), int(bool(XFA)), int(NumXFA), int(bool(InnerGS)), int(bool(NoInv)),
                                    _dp(Tr), _dp(b), ptrs(u), ptrs(vb), ptrs(GC), _dp(ve), _dp(hat), C.byref(its), _dp(cnv), _dp(bend)))
        nit = int(its.value)
        out = dict(zip(PEGSX_KEYS, ([Tr[e].copy() for e in range(neff)], b, u, vb, GC, ve, hat, nit, float(cnv[max(nit, 1) - 1]), bend)))
        if cnv_trace:
            out["cnv_trace"] = cnv[:nit].copy()
        return out


# ---- per-trait ridge fits: solver1x / UVBETA, solver1xF / FUVBETA, XFUVBETA, ZFUVBETA (bwgr_uvbeta, include/bwgr.h) ----
UVB_VARIANTS = {"D": 0, "F": 1, "X": 2, "Z": 3}   # BWGR_UVB_*
UVB_KEYS = ("b", "mu", "h2", "ve", "vb", "its", "cnv")


def uvb_plan(n, p, k):
    """bwgr_debug_uvb_plan (host arithmetic, no GPU): dict(W, groups, solve_traits, ngl, solve_lds, pass_lds, pass_wg, ws_bytes)."""
    out = (C.c_int64 * 8)()
    check(_lib.lib().bwgr_debug_uvb_plan(int(n), int(p), int(k), out))
    return dict(zip(("W", "groups", "solve_traits", "ngl", "solve_lds", "pass_lds", "pass_wg", "ws_bytes"), [int(v) for v in out]))


def _uvb_variant(variant, who):
    if isinstance(variant, str) and variant not in UVB_VARIANTS:
        raise BwgrError(1, "%s: unknown variant %r (one of D, F, X, Z)" % (who, variant))
    return UVB_VARIANTS[variant] if isinstance(variant, str) else int(variant)   # (an integer is passed on: the library checks it)


def _uvb_inputs(Y, nrow, v, tol, df0, who):
    """Y as an n x k float64 matrix; for the float variants Y, tol and df0 rounded to float, as the reference receives them."""
    Ym = np.asarray(Y, np.float64)
    if Ym.ndim == 1:
        Ym = Ym[:, None]
    if Ym.ndim != 2 or Ym.shape[0] != nrow:
        raise BwgrError(1, "%s: Y has shape %s; nrow(Y) must equal nrow(X) = %d" % (who, Ym.shape, nrow))
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
                                 its.ctypes.data_as(C.POINTER(C.c_int)), _dp(cnv), _dp(xbm) if xb else None))
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
                                       _dp(b), _dp(mu), _dp(h2), _dp(ve), _dp(vb), its.ctypes.data_as(C.POINTER(C.c_int)), _dp(cnv)))
    return dict(zip(UVB_KEYS, (b, mu, h2, ve, vb, its, cnv)))


def uvbeta(Y, X, variant="D", maxit=100, tol=10e-7, df0=20.0, xb=False, **kw):
    """One ridge fit per column of Y on one X (bwgr_uvbeta): Y is n x k (NaN = missing) or a vector; variant "D" solver1x / UVBETA,
    "F" solver1xF / FUVBETA, "X" xsolver1xF / XFUVBETA, "Z" zsolver1xF / ZFUVBETA (src/RcppEigen20230423.cpp:1410-1816).  The float
    variants receive Y, tol and df0 rounded to float, as the reference does; the engine is fp64.  Returns dict(b [p x k], mu, h2, ve, vb,
    its, cnv[, xb [n x k] = X b on the raw genotypes]).  X is an array or a Panel."""
    v = _uvb_variant(variant, "uvbeta")
    P, own = _as_panel(X, **kw)
    try:
        Ym, tol, df0 = _uvb_inputs(Y, P.n, v, tol, df0, "uvbeta")
        return _uvb_panel(P, Ym, v, maxit, tol, df0, xb)
    finally:
        if own:
            P.close()


def uvbd_plan(n, q, k):
    """bwgr_debug_uvbd_plan (host arithmetic, no GPU): dict(lds_rows, e_in_lds, threads, lds_bytes, ws_bytes)."""
    out = (C.c_int64 * 5)()
    check(_lib.lib().bwgr_debug_uvbd_plan(int(n), int(q), int(k), out))
    return dict(zip(("lds_rows", "e_in_lds", "threads", "lds_bytes", "ws_bytes"), [int(v) for v in out]))


def uvbeta_dense(Y, Z, variant="D", maxit=100, tol=10e-7, df0=20.0, *, device=0):
    """uvbeta's fits on a small dense real-valued design Z (n x q float64; bwgr_uvbeta_dense): one workgroup per trait runs the trait's whole
    fit.  Same variants, rounding of Y, tol and df0, rules and return dict (b is q x k) as uvbeta."""
    v = _uvb_variant(variant, "uvbeta_dense")
    Zm = np.asarray(Z, np.float64)
    if Zm.ndim == 1:
        Zm = Zm[:, None]
    if Zm.ndim != 2:
        raise BwgrError(1, "uvbeta_dense: Z has shape %s; it must be n x q" % (Zm.shape,))
    Ym, tol, df0 = _uvb_inputs(Y, Zm.shape[0], v, tol, df0, "uvbeta_dense")
    return _uvb_dense(Ym, Zm, v, maxit, tol, df0, device)


def panel_xb(X, B, **kw):
    """X B on the raw int8 genotypes, n x k float64 (bwgr_panel_xb); X is an array or a Panel."""
    P, own = _as_panel(X, **kw)
    try:
        return P.xb(B)
    finally:
        if own:
            P.close()


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
    P, own = _as_panel(X, **panel_kw)
    try:
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
    finally:
        if own:
            P.close()


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
    Zf = np.asarray(Z, np.float64)
    if Zf.ndim == 1:
        Zf = Zf[:, None]
    if Zf.ndim != 2 or Zf.shape[0] != P.n:
        raise BwgrError(1, "uvbeta2: Z has shape %s; nrow(Z) must equal nrow(X) = %d" % (Zf.shape, P.n))
    q = Zf.shape[1]
    Zf = np.asfortranarray(Zf)
    k = Ym.shape[1]
    Yf = np.asfortranarray(Ym)
    kk = max(k, 1)
    b1, b2 = np.zeros((q, kk), order="F"), np.zeros((P.p, kk), order="F")
    mu, h2, ve, vb1, vb2, cnv = (np.zeros(kk) for _ in range(6))
    its = np.zeros(kk, np.int32)
    check(_lib.lib().bwgr_uvbeta2(P._h, _dp(Zf), int(q), int(P.n), _dp(Yf), int(k), int(maxit), float(tol), float(df0), _dp(b1), _dp(b2), _dp(mu),
                                  _dp(h2), _dp(ve), _dp(vb1), _dp(vb2), its.ctypes.data_as(C.POINTER(C.c_int)), _dp(cnv)))
    return dict(zip(UVB2_KEYS, (b1, b2, mu, h2, ve, vb1, vb2, its, cnv)))


def uvbeta2(Y, Z, X, maxit=100, tol=10e-7, df0=20.0, **kw):
    """solver2x for every column of Y (bwgr_uvbeta2): in each sweep the q columns of the dense design Z (n x q float64), then the markers of X,
    against one residual, each design with its own lambda; each trait on its own observed rows (NaN = missing), fp64.  Returns dict(b1 [q x k],
    b2 [p x k], mu, h2, ve, vb1, vb2, its, cnv).  X is a genotype matrix or a Panel."""
    P, own = _as_panel(X, **kw)
    try:
        Ym, tol, df0 = _uvb_inputs(Y, P.n, 0, tol, df0, "uvbeta2")
        return _uvb2_panel(P, Ym, Z, maxit, tol, df0)
    finally:
        if own:
            P.close()


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
    P, own = _as_panel(X, **panel_kw)
    try:
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
    finally:
        if own:
            P.close()


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
    X, _ = _kernel_input(X)
    if isinstance(X, Panel):
        return X, False
    return Panel(X, **panel_kw), True


def _kernel(kind, X, par, flag, device_out, panel_kw):
    P, own = _kernel_panel(X, panel_kw)
    try:
        return P.kernel(kind, par, flag, device_out=device_out)
    finally:
        if own:
            P.close()


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
    P, own = _kernel_panel(X, kw)
    try:
        return P.crossprod(device_out=device_out)
    finally:
        if own:
            P.close()


# ---- founder-by-sample kernels: EigenArcZ / EigenGauZ (R/RcppExports.R:248-254) ----
class _Panels2:
    """The founders' and the samples' int8 panels of one call, from Panels or matrices under _kernel_panel's rules.  Both inputs are checked,
    their column counts compared, before the library is touched; the same matrix on both sides makes one panel."""

    def __init__(self, Xf, Xs, who, panel_kw):
        self._own = []
        same = Xs is Xf
        Xf, pf = _kernel_input(Xf)
        Xs, ps = (Xf, pf) if same else _kernel_input(Xs)
        if pf != ps:
            raise ValueError("%s: the founders have %d columns (markers), the samples %d" % (who, pf, ps))
        try:
            self.f = self._panel(Xf, panel_kw)
            self.s = self.f if same else self._panel(Xs, panel_kw)
        except BaseException:
            self.close()
            raise

    def _panel(self, X, panel_kw):
        if isinstance(X, Panel):
            return X
        self._own.append(Panel(X, **panel_kw))
        return self._own[-1]

    def close(self):
        for P in self._own:
            P.close()
        self._own = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def crossprod2(Xf, Xs, *, device_out=False, **kw):
    """The exact X_f X_s' of integer genotypes over the same markers, n_f x n_s int64 (the product inside EigenArcZ / EigenGauZ)."""
    with _Panels2(Xf, Xs, "crossprod2", kw) as P:
        return P.f.crossprod2(P.s, device_out=device_out)


def _kernel2z(kind, Zfndr, Zsamp, par, parts, who, panel_kw):
    with _Panels2(Zfndr, Zsamp, who, panel_kw) as P:
        Kff, Kfs = P.f.kernel2(P.s, kind, par)
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
