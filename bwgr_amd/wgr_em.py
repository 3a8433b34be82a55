"""wgr and the EM / Gauss-Seidel family (bwgr_wgr*, bwgr_em)."""
import ctypes as C
import numpy as np

from . import _lib
from ._lib import check
from ._marshal import _seed, _fp, _dp, _ip
from .panel import Panel, as_panel


_EM = {"emRR": 0, "emBA": 1, "emDE": 2, "emML": 3, "emBB": 4, "emBC": 5, "emBCpi": 6, "emBL": 7, "emEN": 8, "lasso": 9}


def _em(model, y, gen, df=10.0, R2=0.5, par=0.0, D=None, maxit=0, **panel_kw):
    """The EM / Gauss-Seidel family over bwgr_em (include/bwgr.h); returns dict(mu, b, d, hat, vbvec, scal, iters)."""
    with as_panel(gen, **panel_kw) as P:
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
    check(_lib.lib().bwgr_em_order(int(p), int(upto), _ip(out)))
    return out


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
    with as_panel(X, **panel_kw) as P:
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
