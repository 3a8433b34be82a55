"""The inputs of tests/test_gpu_kernel_codes.py: int8 panels whose codes go beyond 0 / 1 / 2, for the finishes of the relationship kernels
(k_kfin_*, k_kfin2_* and the host scalars of bwgr_panel_kernel / bwgr_panel_kernel2), which read the panel raw with code of their own: the
column sums s (k_kfin_colstats), the row sums X s (k_kfin_xs) and the samples' row squares q_s (k_kfin2_rowsq).  Kept in one place, in the
style of tests/code_cases.py and tests/pair_cases.py, so that tests/test_kernel_code_cases_cpu.py can check without a GPU that every case
is well defined, reaches the plan it is listed for, and bites: a byte read as unsigned in any one of the three places moves every centred
kernel far beyond the tests' bounds.

Two references.  The float64 restatements (tests/kernels_restatement.py, tests/kernels2_restatement.py) use the library's centring identity
and stay the parity reference.  The long double kernels at the end of this file follow the reference's formulas directly -- centre first,
multiply afterwards -- and share nothing with the identity, so they see what it loses where |G| is far above |ZZ'|.

Every panel keeps the int32 Gram bound n * max|x|^2 < 2^31 (include/bwgr.h, at bwgr_panel_create)."""
import ctypes as C
import functools

import numpy as np

import kernels_restatement as KR
import kernels2_restatement as K2
import pegs_cases as PC

LD = np.longdouble


def _i8(A):
    A = np.asarray(A)
    assert A.min() >= -128 and A.max() <= 127
    X = np.asfortranarray(A.astype(np.int8))
    X.setflags(write=False)
    return X


def _uniform(seed, n, p, lo, hi):
    """integers(lo, hi + 1) from the case's own seed"""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(n, p))


def _full():
    return PC._panel("full")          # 300 x 200 uniform in -128..127, both ends in column 0: tests/test_gpu_mrr.py's full-range panel


def _hold_dup():
    A = np.array(_full(), dtype=np.int16)
    A[:, 5], A[:, 9] = -128, 127
    A[7] = A[3]
    return A


# tag -> the panel, Panel()'s keywords, what the case is there for
CASES = {
    "pm1":      dict(make=lambda: PC._panel("signed"), kw={}),            # tpod - 1, 196 x 376: the usual centred coding
    "tpod100":  dict(make=lambda: PC._panel("offset"), kw={}),            # tpod + 100: the centring identity under cancellation, |G| / |ZZ'| ~ 3e4
    "full":     dict(make=_full, kw={}),                                  # the whole byte range
    "full3":    dict(make=lambda: PC._panel("full_slabs"), kw={"nwg": 3}),      # the same codes, 700 x 900: three slabs, partial last block
    "pm127":    dict(make=lambda: np.where(np.random.default_rng(2931).random((257, 129)) < 0.5, -127, 127), kw={}),
                                                                          # largest squares without -128; n, p one past a tile / two blocks
    "dos100":   dict(make=lambda: _uniform(2932, 130, 65, 0, 100), kw={}),      # dosage x 100: large means, unsigned
    "hold_dup": dict(make=_hold_dup, kw={}),                              # zero-variance columns at -128 and 127; row 7 := row 3: an exact
                                                                          # zero distance off the diagonal, under sqrt and exp
    "n2":       dict(make=lambda: _uniform(2933, 2, 63, -128, 127), kw={}),     # smallest n the entry accepts: k_kfin_apply's diagonal branch
    "n3p1":     dict(make=lambda: np.array([[-128], [127], [5]]), kw={}),       # p = 1: one marker, one column workgroup, (p + 3) / 4 = 1
    "n129p1":   dict(make=lambda: _uniform(2934, 129, 1, -3, 3), kw={}),        # the product's edge shapes, now through the finishes
    "n130p63":  dict(make=lambda: _uniform(2935, 130, 63, -3, 3), kw={}),
    "n257p65":  dict(make=lambda: _uniform(2936, 257, 65, -3, 3), kw={}),
}
TAGS = list(CASES)
# One marker with seven codes over 129 rows: rows repeat by counting alone, and a row of 0 makes the uncentred EigenARC 0 / 0 in the
# reference's own formula.  The guards state both as what they are (tests/test_kernel_code_cases_cpu.py) instead of hiding the case.
SHIFTED = ("pm1", "tpod", "tpod100")      # X - mean is the same matrix on all three ("tpod": the golden panel itself, codes 0 / 1 / 2)


def _sample_full():
    A = _uniform(2941, 170, 200, -128, 127)
    A[7] = -128            # the largest q_s there is: p * 2^14
    return A


# tag -> (founders, samples): a one-panel tag, or a maker; kwf / kws: Panel()'s keywords
PAIRS = {
    "pair_pm1":   dict(f=lambda: data("pm1")[:130], s=lambda: data("pm1")[130:], kwf={}, kws={}),      # the tpod split, signed
    "pair_full":  dict(f=lambda: data("full"), s=_sample_full, kwf={}, kws={}),                        # largest q_s; k_kfin2_rowsq on negative bytes
    "pair_mixed": dict(f=lambda: _uniform(2942, 300, 200, 0, 2), s=lambda: _uniform(2943, 170, 200, -128, 127), kwf={}, kws={}),
                                                                     # panels of different ranges; samples centred by means that are not theirs
    "pair_slabs": dict(f=lambda: data("full3"), s=lambda: _uniform(2944, 300, 900, -100, 100), kwf={"nwg": 3}, kws={"nwg": 3}),
                                                                     # three founder slabs of 256 rows against three sample slabs of 128 (the default
                                                                     # rule gives 300 rows slabs of 256 too: nwg = 3 is what makes the heights differ)
    "pair_ns2":   dict(f=lambda: data("full"), s=lambda: _uniform(2945, 2, 200, -128, 127), kwf={}, kws={}),      # a sample panel of two rows
}
ORIENTATIONS = [(tag, swapped) for tag in PAIRS for swapped in (False, True)]      # (swapped pair_ns2: two founders, the smallest n_f)
PAIR_KINDS = [("ARC", 1.0), ("GAU", 1.0), ("GAU", 0.5)]


@functools.lru_cache(maxsize=None)
def data(tag):
    """the panel of a one-panel case (or "tpod"): int8, column-major, read-only"""
    if tag == "tpod":
        return _i8(PC.tpod())
    return _i8(CASES[tag]["make"]())


@functools.lru_cache(maxsize=None)
def _pair(tag):
    c = PAIRS[tag]
    return _i8(c["f"]()), _i8(c["s"]())


def pair_data(tag, swapped=False):
    """(X_f, X_s, Panel keywords of the founders, of the samples)"""
    c = PAIRS[tag]
    F, S = _pair(tag)
    return (S, F, c["kws"], c["kwf"]) if swapped else (F, S, c["kwf"], c["kws"])


def xmax(X):
    return int(np.abs(np.asarray(X).astype(np.int16)).max())


def has_negative(X):
    return bool(np.asarray(X).min() < 0)


# ---- plans (host arithmetic, no GPU) ----------------------------------------------------------------------------------------------------
XXT_FIELDS = ("chunk", "nchunks", "tiles", "wgs", "ws_bytes", "T", "sub", "piece")
XYT_FIELDS = ("chunk", "nchunks", "tiles", "wgs", "ws_bytes", "Tr", "Tc", "sub", "piece")


def panel_plan(X, kw):
    """K, R, ld of bwgr_debug_panel_plan for this int8 panel with its own largest |x|"""
    from bwgr_amd import _lib
    out = (C.c_int64 * 25)()
    rc = _lib.lib().bwgr_debug_panel_plan(0, int(X.shape[0]), int(X.shape[1]), int(kw.get("block", 0)), int(kw.get("nwg", 0)), 0, xmax(X), 0, out)
    assert rc == 0, _lib.lib().bwgr_last_error().decode()
    return dict(K=int(out[1]), R=int(out[2]), ld=int(out[3]))


def xxt_plan(X, kchunk=0):
    from bwgr_amd import _lib
    out = (C.c_int64 * len(XXT_FIELDS))()
    rc = _lib.lib().bwgr_debug_xxt_plan(int(X.shape[0]), int(X.shape[1]), xmax(X), int(kchunk), out)
    assert rc == 0, _lib.lib().bwgr_last_error().decode()
    return dict(zip(XXT_FIELDS, (int(v) for v in out)))


def xyt_plan(F, S, kchunk=0):
    from bwgr_amd import _lib
    out = (C.c_int64 * len(XYT_FIELDS))()
    rc = _lib.lib().bwgr_debug_xyt_plan(int(F.shape[0]), int(S.shape[0]), int(F.shape[1]), xmax(F), xmax(S), int(kchunk), out)
    assert rc == 0, _lib.lib().bwgr_last_error().decode()
    return dict(zip(XYT_FIELDS, (int(v) for v in out)))


def rows_grid(ld, p):
    """kfin_rows_grid of kernels_host.hip.h: (row workgroups, column workgroups) of k_kfin_xs / k_kfin2_rowsq"""
    ysplit = max(1, min(65535, (p + 511) // 512, 2048 // (ld // 128) + 1))
    cpw = -(-p // ysplit)
    return ld // 128, -(-p // cpw)


# ---- the float64 restatements, once per case ----------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def restated(tag, k):
    """KR.restate of KR.KINDS[k] on the case (or "tpod"); read-only"""
    kind, kw = KR.KINDS[k]
    with np.errstate(invalid="ignore", divide="ignore"):
        return _frozen(KR.restate(kind, data(tag), **kw))[0]


@functools.lru_cache(maxsize=None)
def restated2(tag, swapped, kind, phi):
    F, S = pair_data(tag, swapped)[:2]
    return _frozen(*K2.kernels(kind, F, S, phi))


def kind_id(k):
    kind, kw = KR.KINDS[k]
    return "%s-%s" % (kind, "-".join("%s" % v for v in kw.values()))


def centred_kind(k):
    """the kinds that depend on X through X - mean alone (GRM's Code012 divides by the raw means: centred product, uncentred scale)"""
    kind, kw = KR.KINDS[k]
    return (kind == "GRM" and not kw["Code012"]) or (kind in ("EigenGRM", "EigenARC") and list(kw.values())[0])


def uses_sums(k):
    """the kinds whose finish reads the column sums and X s (cen of bwgr_panel_kernel): the unsigned-byte guard speaks of these"""
    kind, kw = KR.KINDS[k]
    return kind == "GRM" or (kind in ("EigenGRM", "EigenARC") and list(kw.values())[0])


def zero_rows(X):
    return ~np.asarray(X).any(1)


def undefined(tag, k):
    """Where the reference's own formula is 0 / 0: the uncentred EigenARC divides by sqrt(G_ii G_jj 1.001), which is 0 on a row of zeros.
    A boolean n x n mask; all False for every other kind and for every panel without such a row."""
    X = data(tag)
    z = zero_rows(X)
    kind, kw = KR.KINDS[k]
    if kind == "EigenARC" and not kw["centralizeX"]:
        return z[:, None] | z[None, :]
    return np.zeros((X.shape[0],) * 2, bool)


# ---- the long double reference: the reference's formulas, directly -----------------------------------------------------------------------
# The literals are the double values the library and the restatements use.
PI_ARC, PI_ARCZ, SLACK = LD(3.1416), LD(3.14159), LD(1.001)


def _ldot(A, B):
    """A B' in long double (numpy has no BLAS for it; einsum's loop is its fastest)"""
    return np.einsum("ik,jk->ij", np.ascontiguousarray(A), np.ascontiguousarray(B))


@functools.lru_cache(maxsize=None)
def _ld_products(tag):
    """(X X', Z Z') in long double, Z = X - mean formed first: X X' holds exact integers"""
    X = data(tag).astype(LD)
    Z = X - X.mean(0)
    return _frozen(KR.crossprod(data(tag)).astype(LD), _ldot(Z, Z))


def _ld_arc(A, da, db, pi):
    N = np.sqrt(da[:, None] * db[None, :] * SLACK)
    th = np.arccos(A / N)
    return N, th, np.sin(th) + (pi - th) * np.cos(th)


def _ld_dist2(G):
    d = np.diag(G)
    return d[:, None] + d[None, :] - 2 * G


@functools.lru_cache(maxsize=None)
def reference(tag, k):
    """KR.KINDS[k] of the case in long double; read-only"""
    kind, kw = KR.KINDS[k]
    X = data(tag).astype(LD)
    n = X.shape[0]
    G, ZZ = _ld_products(tag)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == "GRM":
            m = X.mean(0)
            D = np.sum(m * m / 2) if kw["Code012"] else np.sum(((X - m) ** 2).sum(0) / (n - 1))
            K = ZZ / D
        elif kind == "GAU":
            d2 = _ld_dist2(G)
            K = np.exp(-d2 / (d2.sum() / (LD(n) * (n - 1))))
        elif kind == "EigenGRM":
            A = np.array(ZZ if kw["centralizeZ"] else G)
            A[np.diag_indices(n)] += 1
            K = A * (1 / np.mean(np.diag(A)))
        elif kind == "EigenGAU":
            d = np.sqrt(_ld_dist2(G))
            np.fill_diagonal(d, 0)
            K = np.exp(d * (LD(kw["phi"]) * (-(LD(n) * (n - 1))) / d.sum()))
        else:
            A = ZZ if kw["centralizeX"] else G
            A = A * (1 / np.mean(np.diag(A)))
            dg = np.diag(A)
            N, _, J = _ld_arc(A, dg, dg, PI_ARC)
            K = N / PI_ARC * J
    return _frozen(K)[0]


@functools.lru_cache(maxsize=None)
def reference2(tag, swapped, kind, phi):
    """(K_ff, K_fs) of EigenArcZ / EigenGauZ in long double: both matrices centred by the founders' means, then multiplied"""
    Fi, Si = pair_data(tag, swapped)[:2]
    F, S = Fi.astype(LD), Si.astype(LD)
    nf = F.shape[0]
    if kind == "ARC":
        m = F.mean(0)
        Zf, Zs = F - m, S - m
        Aff, Afs = _ldot(Zf, Zf), _ldot(Zf, Zs)
        df, ds = np.diag(Aff).copy(), (Zs * Zs).sum(1)
        Nff, _, Jff = _ld_arc(Aff, df, df, PI_ARCZ)
        Nfs, _, Jfs = _ld_arc(Afs, df, ds, PI_ARCZ)
        Kff, Kfs = Nff * Jff / PI_ARCZ, Nfs * Jfs / PI_ARCZ
        ks = 1 / np.mean(np.diag(Kff))
        return _frozen(Kff * ks, Kfs * ks)
    Gff, Gfs = K2.crossprod2(Fi, Fi).astype(LD), K2.crossprod2(Fi, Si).astype(LD)
    dff, qs = np.diag(Gff), (S * S).sum(1)
    Dfs = np.sqrt(dff[:, None] + qs[None, :] - 2 * Gfs)
    Dff = np.sqrt(dff[:, None] + dff[None, :] - 2 * Gff)
    np.fill_diagonal(Dff, 0)
    t = LD(phi) * (-(LD(nf) * (nf - 1))) / Dff.sum()
    return _frozen(np.exp(Dff * t), np.exp(Dfs * t))


def arc_argument(tag, centred):
    """max |acos argument| of EigenARC on the case, in long double, over the entries where it is defined"""
    G, ZZ = _ld_products(tag)
    A = ZZ if centred else G
    dg = np.diag(A)
    with np.errstate(invalid="ignore", divide="ignore"):
        arg = np.abs(A / np.sqrt(dg[:, None] * dg[None, :] * SLACK))
    return float(np.nanmax(arg))


def err(a, b, mask=None):
    """KR.scaled_err of a (float64) against the long double b, formed in long double, over the entries outside mask"""
    a, b = np.asarray(a).astype(LD), np.asarray(b, LD)
    if mask is not None:
        a, b = a[~mask], b[~mask]
    den = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (den if den > 0 else 1))


# ---- the restatement with the bytes read as unsigned in one place only --------------------------------------------------------------------
MISREADS = ("s", "Xs", "qs")


def _u8(X):
    return np.asarray(X).view(np.uint8).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _gram(tag):
    return _frozen(KR.crossprod(data(tag)))[0]


def misread_zz(tag, where):
    """KR.zz_identity with the column sums (where = "s") or the panel under the row sums X s ("Xs") read as unsigned bytes; the product
    itself is read right"""
    X = data(tag)
    Xi = X.astype(np.int64)
    n = Xi.shape[0]
    s = (_u8(X) if where == "s" else Xi).sum(0)
    r = ((_u8(X) if where == "Xs" else Xi) @ s).astype(np.float64) / n
    c = float(np.sum((s.astype(np.float64) / n) ** 2))
    return _gram(tag).astype(np.float64) - (r[:, None] + r[None, :]) + c


def misread(k, tag, where):
    """KR.restate of KR.KINDS[k] (a kind of uses_sums) with that one misreading; GRM's scale follows the misread sums, as the library's would"""
    kind, kw = KR.KINDS[k]
    X = data(tag)
    A = misread_zz(tag, where)
    n = A.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == "GRM":
            Xi = np.asarray(X).astype(np.int64)
            s = (_u8(X) if where == "s" else Xi).sum(0).astype(np.float64)
            q = (Xi * Xi).sum(0).astype(np.float64)
            return A / (float(np.sum((s / n) ** 2 / 2.0)) if kw["Code012"] else float(np.sum((q - s * s / n) / (n - 1.0))))
        if kind == "EigenGRM":
            A[np.diag_indices_from(A)] += 1.0
            return A * (1.0 / np.mean(np.diag(A)))
        A = A * (1.0 / np.mean(np.diag(A)))
        dg = np.diag(A)
        N = np.sqrt(dg[:, None] * dg[None, :] * 1.001)
        th = np.arccos(A / N)
        return N / 3.1416 * (np.sin(th) + (3.1416 - th) * np.cos(th))


@functools.lru_cache(maxsize=None)
def _grams2(tag, swapped):
    F, S = pair_data(tag, swapped)[:2]
    return _frozen(K2.crossprod2(F, F), K2.crossprod2(F, S))


def misread2(kind, tag, swapped, where, phi=1.0):
    """K2.kernels with one misreading: the founders' column sums ("s"), the panels under X_f s and X_s s ("Xs"), the samples' row squares
    ("qs"); the two products are read right"""
    F, S = pair_data(tag, swapped)[:2]
    Fi, Si = F.astype(np.int64), S.astype(np.int64)
    nf = Fi.shape[0]
    qs = ((_u8(S) ** 2) if where == "qs" else (Si * Si)).sum(1)
    Gff, Gfs = _grams2(tag, swapped)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == "GAU":
            dff = np.diag(Gff)
            Dfs = np.sqrt((dff[:, None] + qs[None, :] - 2 * Gfs).astype(np.float64))
            Dff = np.sqrt((dff[:, None] + dff[None, :] - 2 * Gff).astype(np.float64))
            np.fill_diagonal(Dff, 0.0)
            t = phi * (-(nf * (nf - 1.0))) / Dff.sum()
            return np.exp(Dff * t), np.exp(Dfs * t)
        s = (_u8(F) if where == "s" else Fi).sum(0)
        rf = ((_u8(F) if where == "Xs" else Fi) @ s).astype(np.float64) / nf
        rs = ((_u8(S) if where == "Xs" else Si) @ s).astype(np.float64) / nf
        c = float(np.sum((s.astype(np.float64) / nf) ** 2))
        Aff = Gff.astype(np.float64) - (rf[:, None] + rf[None, :]) + c
        Afs = Gfs.astype(np.float64) - rf[:, None] - rs[None, :] + c
        df, ds = np.diag(Aff).copy(), qs.astype(np.float64) - 2.0 * rs + c
        Kff, Kfs = K2._arc(Aff, df, df), K2._arc(Afs, df, ds)
        ks = 1.0 / np.mean(np.diag(Kff))
        return Kff * ks, Kfs * ks


def moved(a, b):
    """KR.scaled_err, with an entry that stops being a number counted as moved without bound"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not np.all(np.isfinite(a)):
        return np.inf
    return KR.scaled_err(a, b)
