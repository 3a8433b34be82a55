"""The cases of the mkr / mrr(Y, dense(X)) tests, in one place: tests/test_gpu_mkr.py fits them on the GPU against tests/mrr_restatement.py, and
tests/test_mkr_cpu.py checks on the CPU that the restatement alone stays finite and runs at least three sweeps on each, and that the library's
plan (bwgr_debug_mrr_dense_plan) gives each the blocks, edge widths, row-tile trips and ngl < npat it is there for.
The second round (SOLVE .. OPTION below) walks the solve's five LDS regimes, the row counts beside the tile, the trip and the eight-at-a-time
sum, the column kernels' second trip, degenerate columns and rows, and the options where ngl < npat.

A case is (Y, X, opts): Y n x k with NaN = missing, X the n x r float64 design fed alike to the library and to the restatement."""
import numpy as np


def genotypes(n, p, seed):
    return np.random.default_rng(seed).integers(0, 3, size=(n, p)).astype(np.float64)


def grm(Z):
    """the centred genomic relationship matrix of a 0/1/2 matrix, Zc Zc' / sum_j var(z_j) (the restated GRM; rank n - 1)"""
    Zc = Z - Z.mean(0)
    return (Zc @ Zc.T) / Zc.var(0).sum()


def grm150():
    return grm(genotypes(150, 400, 7))


def traits(X, k, seed, frac=0.0, patterns=None):
    """k correlated traits with signal in the columns of X; `frac`: every record missing with that chance (k distinct patterns);
    `patterns`: per trait, the chance of its own missing rows (0: fully observed)."""
    rng = np.random.default_rng(seed)
    n, r = X.shape
    Xc = X - X.mean(0)
    G = Xc @ (rng.normal(size=(r, k)) / np.sqrt(r))
    sd = G.std(0)
    Y = G / np.where(sd > 0, sd, 1.0) + rng.normal(size=(n, k)) + 3.0
    if patterns is not None:
        for t, fr in enumerate(patterns):
            if fr > 0:
                Y[rng.random(n) < fr, t] = np.nan
    elif frac > 0:
        Y[rng.random((n, k)) < frac] = np.nan
    return Y


def shared_traits(X, ids, seed, frac=0.1):
    """len(ids) fully generated traits with prescribed shared missingness: one random mask per pattern id (every record of it missing with
    chance `frac`), applied to every trait with that id.  The ids are numbered in order of first appearance, as find_patterns numbers them,
    so trait t's pattern index in the library is ids[t]."""
    ids = list(ids)
    seen = []
    for g in ids:
        if g not in seen:
            seen.append(g)
    assert seen == list(range(len(seen))), ids
    Y = traits(X, len(ids), seed)
    rng = np.random.default_rng(seed + 1000)
    masks = [rng.random(X.shape[0]) < frac for _ in seen]
    for t, g in enumerate(ids):
        Y[masks[g], t] = np.nan
    return Y


def regime(linv_lds, ngl, npat):
    """k_mrrd_solve's five regimes, numbered as tests/mrr_cases.py numbers k_mrr_solve's: the inverses in LDS with every Gram there (1), some (2),
    none (3); the inverses in global memory with every Gram in LDS (4), some (5)"""
    if linv_lds:
        return 3 if ngl == 0 else (1 if ngl == npat else 2)
    return 4 if ngl == npat else 5


def real_design(n, r, seed):
    """real-valued columns of unequal scale and non-zero means"""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.normal(size=(n, r)) * rng.uniform(0.5, 2.0, size=r) + rng.normal(size=r))


def npat(Y):
    """the distinct missingness patterns of Y's traits"""
    obs = ~np.isnan(Y if Y.ndim == 2 else Y[:, None])
    return len({obs[:, t].tobytes() for t in range(obs.shape[1])})


# name -> (n, r, k, settings).  The plan facts a case is there for are asserted in tests/test_mkr_cpu.py.
def case(name):
    import bwgr_amd
    if name == "grm150":             # r = 149: blocks of 64, 64, 21; 150 rows: tiles of 64, 64, 22 (and one of padding); the defaults
        X = bwgr_amd.K2X(grm150())
        return traits(X, 3, 21, frac=0.15), X, {}
    if name in _NEW:
        return _new_case(name)
    if name.startswith("r"):         # r1, r64, r65, r130 at n = 200
        r = int(name[1:])
        X = real_design(200, r, 30 + r)
        return traits(X, 3, 40 + r, frac=0.1), X, dict(maxit=20)
    if name == "tall":               # 2 304 padded rows = 36 tiles on 32 workgroups: a second trip
        X = real_design(2200, 70, 51)
        return traits(X, 2, 52, frac=0.1), X, dict(maxit=10)
    if name == "k1":
        X = real_design(200, 70, 61)
        return traits(X, 1, 62, frac=0.2)[:, 0], X, dict(maxit=20)
    if name == "k16":                # sixteen distinct patterns: ngl < npat, the inverses from global memory
        X = real_design(200, 70, 63)
        return traits(X, 16, 64, frac=0.1), X, dict(maxit=10)
    if name == "k4full":             # no missing record: one pattern
        X = real_design(200, 70, 65)
        return traits(X, 4, 66), X, dict(maxit=20)
    if name in ("TH", "updateMu", "XFA"):
        X = real_design(200, 130, 71)
        opt = {"TH": dict(TH=True), "updateMu": dict(updateMu=True), "XFA": dict(XFA=True, NumXFA=2)}[name]
        Y = traits(X, 4, 72, patterns=[0.1, 0.0, 0.3, 0.0])
        Y[np.isnan(Y[:, 0]), 3] = np.nan          # traits 0 and 3 share a pattern: three patterns for four traits
        return Y, X, dict(maxit=20, **opt)
    if name == "int012":             # the design both engines take: 300 x 500 0/1/2
        X = np.asfortranarray(genotypes(300, 500, 81))
        return traits(X, 3, 82, frac=0.1), X, dict(maxit=15)
    raise KeyError(name)


# ---- the second round -------------------------------------------------------------------------------------------------------------------
# (k, npat) of the solve-regime cases: n = 200, r = 70 (two blocks of 64 and 6), 10 % missing, maxit = 10.  npat = k: k distinct patterns.
SOLVE = {"solve_k4p4": (4, 4), "solve_k7p7": (7, 7), "solve_k8p8": (8, 8), "solve_k11p11": (11, 11), "solve_k12p12": (12, 12),
         "solve_k13p13": (13, 13), "solve_k14p14": (14, 14), "solve_k15p15": (15, 15), "solve_k15p1": (15, 1), "solve_k16p2": (16, 2)}
# traits that share patterns across the ngl line: trait t's Gram row comes from LDS where ids[t] < ngl, from global memory otherwise
SHARED = {"shared_k6": [0, 1, 2, 3, 0, 3], "shared_k10": [0, 1, 2, 1, 3, 0, 4, 2, 4, 3]}
# row counts at r = 70, k = 2, maxit = 6; the two smallest shapes (fully observed, k = 2) are n2r1 and n3r2
ROWS = {"n%d" % n: n for n in (63, 64, 65, 127, 128, 129, 512, 513, 2048, 2049, 4100)}
SMALLEST = {"n2r1": (2, 1), "n3r2": (3, 2)}
WIDE = ["wide"]                      # r = 32 800 > 4 * 8192: the column kernels' second trip
DEGENERATE = ["deg_const_cols", "deg_const_on_trait", "deg_dead_rows", "deg_dead_tile", "deg_scales", "deg_default_tol"]
OPTION = {"opt_HCS": dict(HCS=True), "opt_ACS": dict(ACS=True, NumXFA=2), "opt_OneVarB": dict(OneVarB=True), "opt_OneVarE": dict(OneVarE=True),
          "opt_TH_updateMu": dict(TH=True, updateMu=True)}
_NEW = set(SOLVE) | set(SHARED) | set(ROWS) | set(SMALLEST) | set(WIDE) | set(DEGENERATE) | set(OPTION)


def _new_case(name):
    if name in SOLVE:
        k, npt = SOLVE[name]
        X = real_design(200, 70, 100 + 16 * k + npt)
        if npt == k:
            return traits(X, k, 400 + 16 * k + npt, frac=0.1), X, dict(maxit=10)
        ids = [t % npt for t in range(k)]             # (15, 1): one shared pattern; (16, 2): [0, 1] * 8
        return shared_traits(X, ids, 400 + 16 * k + npt), X, dict(maxit=10)
    if name in SHARED or name in OPTION:
        ids = SHARED.get(name, SHARED["shared_k6"])
        X = real_design(200, 70, 700 + len(ids))
        return shared_traits(X, ids, 720 + len(ids)), X, dict(maxit=10, **OPTION.get(name, {}))
    if name in ROWS:
        n = ROWS[name]
        X = real_design(n, 70, 800 + n % 97)
        return traits(X, 2, 900 + n % 97, frac=0.1), X, dict(maxit=6)
    if name in SMALLEST:
        n, r = SMALLEST[name]
        X = real_design(n, r, 950 + n)
        return traits(X, 2, 960 + n), X, dict(maxit=6)
    if name == "wide":                # 513 blocks, the last of 32 columns; columns 32 768 .. 32 799 on the column kernels' second trip
        X = real_design(130, 32800, 970)
        return traits(X, 2, 971, frac=0.1), X, dict(maxit=3)
    # the degenerate inputs: n = 200, r = 70, k = 3, 10 % missing, maxit = 10
    X = real_design(200, 70, 980)
    Y = traits(X, 3, 981, frac=0.1)
    opts = dict(maxit=10)
    if name == "deg_const_cols":      # monomorphic columns: all zero after centring, XX = XSX = 0, LHS = iG, b = 0
        X[:, 5] = 2.5
        X[:, 66] = 0.0
    elif name == "deg_const_on_trait":   # constant on exactly trait 1's observed rows: that trait's XSX of the column is 0 but for rounding
        X[~np.isnan(Y[:, 1]), 17] = 1.0
    elif name == "deg_dead_rows":     # rows 10 .. 74 missing for every trait: tile 0 keeps its first ten rows, tile 64..127 loses its first eleven
        Y[10:75, :] = np.nan
    elif name == "deg_dead_tile":     # a whole 64-row tile with z = 0
        Y[64:128, :] = np.nan
    elif name == "deg_scales":        # column scales over two decades
        X = np.asfortranarray(X * np.logspace(-1, 1, 70))
    elif name == "deg_default_tol":   # the default maxit and tol: the fit stops by its tolerance, Its < maxit
        opts = {}
    else:
        raise KeyError(name)
    return Y, X, opts


NEW_CASES = list(SOLVE) + list(SHARED) + list(ROWS) + list(SMALLEST) + WIDE + DEGENERATE + list(OPTION)
CASES = ["grm150", "r1", "r64", "r65", "r130", "tall", "k1", "k16", "k4full", "TH", "updateMu", "XFA", "int012"]
ALL_CASES = CASES + NEW_CASES
