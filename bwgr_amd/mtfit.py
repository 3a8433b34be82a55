"""The multi-trait fits: mrr / MRR3 / MRR3F on a panel or a dense design, K2X and mkr, PEGS / PEGSZ and their sparse forms, PEGSX (bwgr_mrr*,
bwgr_pegs*, bwgr_pegsx*), the effect markers `dense` and `sparse`, and the families' plan hooks."""
import contextlib
import ctypes as C
import numpy as np

from . import _lib
from ._lib import BwgrError, check
from ._marshal import HOST, DEVICE, _dp, _vp, _is_device_tensor, _matrix, _plan
from .panel import Panel, as_panel


# ---- multi-trait ridge regression: MRR3 / MRR3F, mrr / mrr_float (bwgr_mrr, include/bwgr.h) ----
_MRR_OPTS = ["maxit", "tol", "TH", "NLfactor", "InnerGS", "NoInv", "HCS", "XFA", "ACS", "NumXFA", "R2", "gc0", "df0", "updateMu",
             "weight_prior_h2", "weight_prior_gc", "PenCor", "MinCor", "uncorH2below", "roundGCupFrom", "roundGCupTo", "roundGCdownFrom",
             "roundGCdownTo", "bucketGCfrom", "bucketGCto", "DeflateMax", "DeflateBy", "OneVarB", "OneVarE", "verbose"]   # BWGR_MRR_* order
MRR_KEYS = ("mu", "b", "hat", "h2", "GC", "vb", "ve", "MSx", "cnvB", "cnvH2", "cnvV", "b_Weights", "Its")


def _mrr_io(Yf, n, r, single, opts):
    """What bwgr_mrr and bwgr_mrr_dense share around their call for Y (n x k) on a design of r columns: the option vector, the pointers of the
    eleven output arrays (mu .. cnvV, padded to one row, column and sweep), the sweep counter, and the reference's list made of them."""
    k = Yf.shape[1]
    o = np.array([float(opts[name]) for name in _MRR_OPTS], np.float64)
    if single:
        o = o.astype(np.float32).astype(np.float64)
        o[_MRR_OPTS.index("maxit")] = int(opts["maxit"])
    kk, sweeps = max(k, 1), max(int(opts["maxit"]), 1)
    outs = (np.zeros(kk), np.zeros((max(r, 1), kk), order="F"), np.zeros((max(n, 1), kk), order="F"), np.zeros(kk), np.zeros((kk, kk), order="F"),
            np.zeros((kk, kk), order="F"), np.zeros(kk), np.zeros(kk), np.zeros(sweeps), np.zeros(sweeps), np.zeros(sweeps))
    its = C.c_int()

    def result():
        n_it = int(its.value)
        return dict(zip(MRR_KEYS, outs[:8] + tuple(c[:n_it].copy() for c in outs[8:]) + (np.ones((r, k)), n_it)))
    return o, [_dp(a) for a in outs], its, result


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
        ldx, xptr, loc = n, _vp(Xh), HOST
    Yf = np.asfortranarray(_matrix(Y, "mrr", n, single))
    o, outs, its, result = _mrr_io(Yf, n, r, single, opts)
    check(_lib.lib().bwgr_mrr_dense(device, xptr, loc, int(n), int(r), int(ldx), _dp(Yf), Yf.shape[1], _dp(o), len(o), *outs, C.byref(its)))
    return result()


def _mrr(Y, X, single, opts, panel_kw):
    """bwgr_mrr: Y is n x k (NaN = missing) or a vector (k = 1); returns the reference's list as a dict, in its order.  A design marked
    dense(X) goes to bwgr_mrr_dense; nothing else does.  MRR3F receives float matrices (src/RcppEigen20230423.cpp:704)."""
    if isinstance(X, dense):
        return _mrr_dense(Y, X, single, opts, dict(panel_kw))
    with as_panel(X, **panel_kw) as P:
        Yf = np.asfortranarray(_matrix(Y, "mrr", None, single))
        assert Yf.ndim == 2 and Yf.shape[0] == P.n, "nrow(Y) must equal nrow(X)"
        o, outs, its, result = _mrr_io(Yf, P.n, P.p, single, opts)      # (a panel has n >= 2, p >= 1: nothing is padded)
        check(_lib.lib().bwgr_mrr(P._h, _dp(Yf), Yf.shape[1], _dp(o), len(o), *outs, C.byref(its)))
        return result()


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
    names = ("ld", "nblk", "edge", "tiles", "pass_wg", "trips", "cols_wg", "hat_wg", "linv_lds", "ngl", "lds_gram", "lds_pass", "lds_solve", "lds_linv", "ws_bytes")
    return _plan("bwgr_debug_mrr_dense_plan", names, n, r, k, npat)


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
        Zm = _matrix(Z, "dense")
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
    names = ("setup_threads", "setup_wg", "serial_threads", "serial_wg", "disjoint_threads", "disjoint_wg", "trip_cols", "leg", "ws_bytes")
    r = _plan("bwgr_debug_pegs_sparse_plan", names, n, q, nnz, max_col_nnz, k, bool(disjoint))
    r["leg"] = "disjoint" if r["leg"] else "serial"
    return r


def pegs_plan(n, q, k):
    """bwgr_debug_pegs_plan (host arithmetic, no GPU): dict(threads, lds_bytes, ws_bytes) of the dense leg."""
    return _plan("bwgr_debug_pegs_plan", ("threads", "lds_bytes", "ws_bytes"), n, q, k)


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


def _ptrs(arrs):
    """the arrays' addresses as one array of pointers (of one entry where there is none): a per-effect output of bwgr_pegs / bwgr_pegsx"""
    return C.cast((C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs]), C.c_void_p)


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
        rows = [_eff_rows(E) for E in effs]
        n = rows[0]
        if any(r != n for r in rows):
            raise BwgrError(1, "pegs: the effects have %s rows; all must have the same" % (rows,))
        Yf = np.asfortranarray(_matrix(Y, "pegs", n, True))   # PEGS receives float matrices (src/RcppEigenX20251203.cpp:10)
        k = Yf.shape[1]
        neff, kk = len(effs), max(k, 1)
        f32 = lambda v: float(np.float32(v))   # the real options are floats there
        mu = np.zeros(kk); hat = np.zeros((n, kk), order="F"); h2 = np.zeros(kk); bend = np.zeros(neff)
        b = [np.zeros((p_, kk), order="F") for p_ in ps]; GC = [np.zeros((kk, kk), order="F") for _ in ps]
        cnv = np.zeros(max(int(maxit), 1)); its = C.c_int()
        check(_lib.lib().bwgr_pegs_ex(int(device), C.cast(ce, C.c_void_p), neff, _dp(Yf), int(n), int(k), int(maxit), f32(logtol), f32(covbend), f32(covMinEv),
                                   int(XFA), int(bool(NNC)), int(text), _dp(mu), _ptrs(b), _dp(hat), _dp(h2), _ptrs(GC),
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
    return _plan("bwgr_debug_pegsx_plan", ("threads", "lds_bytes", "ws_bytes", "jc", "fc", "trace_lds_bytes"), n, f, k)


def pegs_launch_plan(n, m):
    """bwgr_debug_pegs_launch_plan (host arithmetic, no GPU) for n rows and an effect of m columns: dict(trace_wg, trace_cols, setup_wg,
    setup_cols, leg_threads, fixed_threads) -- the trace kernels' workgroups and the columns one trip of them covers, the same of
    k_pegs_dense_setup, the threads of k_pegs_dense_leg and of k_pegsx_fixed."""
    return _plan("bwgr_debug_pegs_launch_plan", ("trace_wg", "trace_cols", "setup_wg", "setup_cols", "leg_threads", "fixed_threads"), n, m)


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
        Ym, Xm = _matrix(Y, "pegsx"), _matrix(X, "pegsx")
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
        cnv = np.zeros(max(int(maxit), 1)); its = C.c_int()
        check(_lib.lib().bwgr_pegsx_ex(int(device), C.cast(ce, C.c_void_p), neff, _dp(Xf), max(n, 1), int(f), _dp(Yf), int(n), int(k), int(maxit), f32(logtol),
                                    f32(covbend), f32(covMinEv), f32(df0), int(bool(NNC)), int(bool(XFA)), int(NumXFA), int(bool(InnerGS)), int(bool(NoInv)),
                                    _dp(Tr), _dp(b), _ptrs(u), _ptrs(vb), _ptrs(GC), _dp(ve), _dp(hat), C.byref(its), _dp(cnv), _dp(bend)))
        nit = int(its.value)
        out = dict(zip(PEGSX_KEYS, ([Tr[e].copy() for e in range(neff)], b, u, vb, GC, ve, hat, nit, float(cnv[max(nit, 1) - 1]), bend)))
        if cnv_trace:
            out["cnv_trace"] = cnv[:nit].copy()
        return out
