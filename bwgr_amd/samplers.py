"""The fused Gibbs samplers: Chain, BayesA .. BayesDpi and their two-panel forms, fit_many, mcmcCV, KMUP / KMUP2 (bwgr_chain_*, bwgr_bayes2,
bwgr_kmup*), and the debug hooks of a sweep."""
import ctypes as C
import numpy as np

from . import _lib
from ._lib import BwgrError, check
from ._marshal import HOST, DEVICE, _seed, _fp, _dp, _ip, _vp, _plan
from .panel import Panel, as_panel


MODELS = {"BayesA": 0, "BayesB": 1, "BayesC": 2, "BayesL": 3, "BayesRR": 4, "BayesCpi": 5, "BayesDpi": 6}
_PER_MARKER_VB = {"BayesA", "BayesB", "BayesL", "BayesDpi"}


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
            yptr, loc = _vp(self._y), HOST
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
    with as_panel(X, **panel_kw) as P:
        ch = Chain(P, model, y, it, bi, pi, df, R2, seed, rng_mode)
        try:
            ch.run(int(it))
            out = ch.result()
            if return_state:
                out["last"] = ch.state()
            return out
        finally:
            ch.close()


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
    with as_panel(X, **panel_kw) as P:
        return _fit_many(P, jobs, concurrent, chunk, pair)


def _fit_many(P, jobs, concurrent, chunk, pair):
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


def _fused2(base, y, X1, X2, it, bi, pi, df, R2, seed, rng_mode, **panel_kw):
    """BayesA2 / BayesB2 / BayesRR2(y, X1, X2, ...), src/Rcpp20260726ai.cpp:990-1218: two panels, one residual."""
    own1, own2 = not isinstance(X1, Panel), not isinstance(X2, Panel)
    P1 = Panel(X1, **panel_kw) if own1 else X1
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
                                       _ip(out)))
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
        with as_panel(np.ascontiguousarray(gen[keep]), **panel_kw) as P:
            B = np.zeros((p, 7))
            ytr = y[keep].astype(np.float32)
            jobs = [dict(model=model, y=ytr, it=it, bi=bi, df=df, R2=R2, seed=(base + 1000003 * (c + 1) + i) & 0x7FFFFFFFFFFFFFFF,
                         **({"pi": pi} if model in ("BayesB", "BayesC") else {})) for i, model in enumerate(_CV_FITS)]
            for i, fit in enumerate(fit_many(P, jobs)):   # the seven chains side by side on the fold's training panel
                B[:, i] = fit["b"]
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
    with as_panel(X, **panel_kw) as P:
        b = np.array(b, np.float32); d = np.array(d, np.float32); e = np.array(e, np.float32)
        xx = np.ascontiguousarray(xx, np.float32); L = np.ascontiguousarray(L, np.float32)
        assert b.size == P.p and d.size == P.p and xx.size == P.p and L.size == P.p and e.size == P.n
        check(_lib.lib().bwgr_kmup(P._h, _fp(b), _fp(d), _fp(xx), _fp(e), _fp(L), float(Ve), float(pi),
                                    C.c_uint64(_seed(seed)), C.c_uint32(int(it)), int(rng_mode)))
        return {"b": b, "d": d, "e": e}


def KMUP2(X, Use, b, d, xx, E, L, Ve, pi, *, seed=None, it=0, rng_mode=0, **panel_kw):
    """One Gibbs sweep on the row subsample Use (0-based, as wgr passes it: sort(sample(n, n*bag, rp)) - 1, R/wgr.R:68);
    returns list(b=, d=, e=) like src/Rcpp20260726ai.cpp:76 (e: the subsample's residuals).  Inputs are not modified."""
    with as_panel(X, **panel_kw) as P:
        use = np.ascontiguousarray(np.asarray(Use), np.int32)
        b = np.array(b, np.float32); d = np.array(d, np.float32); E = np.ascontiguousarray(E, np.float32)
        xx = np.ascontiguousarray(xx, np.float32); L = np.ascontiguousarray(L, np.float32)
        assert b.size == P.p and d.size == P.p and xx.size == P.p and L.size == P.p and E.size == P.n
        e = np.zeros(use.size, np.float32)
        check(_lib.lib().bwgr_kmup2(P._h, _ip(use), int(use.size), _fp(b), _fp(d), _fp(xx), _fp(E),
                                     _fp(e), _fp(L), float(Ve), float(pi), C.c_uint64(_seed(seed)), C.c_uint32(int(it)), int(rng_mode)))
        return {"b": b, "d": d, "e": e}


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
    return _plan("bwgr_debug_sweep_plan", SWEEP_PLAN_FIELDS, bool(is_f32), n, p, block, nwg, kind, xmax, bool(gram16), flags, blk_begin, blk_end, mode, state)
