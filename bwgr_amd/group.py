"""Group: one fused-sampler chain over several GPUs of this process (bwgr_group_*)."""
import ctypes as C
import numpy as np

from . import _lib
from ._lib import check
from ._marshal import X_I8, X_F32, X_F64, HOST, DEVICE, _seed, _fp, _vp, _plan
from .samplers import MODELS, _PER_MARKER_VB


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
            xptr = _vp(self._X)
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
        out = _plan("bwgr_group_info", ("devices", "rounds_per_sweep", "markers_per_round", "rccl"), self._h)
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
