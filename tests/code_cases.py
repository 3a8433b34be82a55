"""The inputs of tests/test_gpu_codes.py: int8 panels whose codes go beyond 0/1/2, up to the whole byte range, and the two panels either side of
the int32 Gram bound n * max|x|^2 < 2^31 (include/bwgr.h, at bwgr_panel_create).  Kept in one place, as tests/driver_cases.py is, so that
tests/test_code_cases_cpu.py can check without a GPU that every case reaches the plan it is listed for (bwgr_debug_panel_plan with the case's own
largest |x|) and that every job with inclusion decisions is one the oracle decides alike in both of its flavours.

What the largest |x| of a panel (PanelData::xmax) feeds: the fixed-point scale of k_sweep3 / k_sweep3f / k_sweep3p and of k_sweep2w's fixed-point
streamers (k_escale: |x * drej| < 2^(e3_dex - 126 + xbits), xbits = ceil(log2 xmax)); the 16-bit verdict and the byte planes follow the size and sign
of the Gram entries (uint16 or int32 staging, engine 4 or 2 for the affine sweeps).
"""
import ctypes as C
import functools

import numpy as np

SEED = 7      # every case's generator seed


def codes_panel(n, p, lo, hi, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(lo, hi + 1, size=(n, p)).astype(np.int8)
    bt = np.zeros(p); idx = rng.choice(p, max(1, p // 20), replace=False); bt[idx] = rng.normal(size=idx.size)
    g = X.astype(float) @ bt; g = (g - g.mean()) / g.std()
    y = g * np.sqrt(.5) + rng.normal(size=n) * np.sqrt(.5) + 2.0
    return np.asfortranarray(X), y


# tag -> n, p, the codes lo..hi, columns held at -128 (set after the generator ran: y is the generator's)
CASES = {
    "c15":    dict(n=200,    p=300, lo=0,    hi=15,  hold=()),       # xbits 4 from an xmax that is no power of two
    "c16":    dict(n=200,    p=300, lo=0,    hi=16,  hold=()),       # xmax a power of two: xbits 4; entries <= 51 200: 16-bit staging
    "c17":    dict(n=200,    p=300, lo=0,    hi=17,  hold=()),       # xbits 5; entries <= 57 800: still 16-bit; k_sweep3f; affine sweeps on k_sweep2w
    "pm1":    dict(n=700,    p=600, lo=-1,   hi=1,   hold=()),       # the usual centred coding: negative entries, 32-bit staging
    "s127":   dict(n=300,    p=300, lo=-127, hi=127, hold=()),       # xbits 7, 32-bit staging
    "full":   dict(n=300,    p=300, lo=-128, hi=127, hold=(5,)),     # xmax 128
    "dos100": dict(n=1500,   p=400, lo=0,    hi=100, hold=()),       # dosage x 100: six slabs, four blocks, cross arrays to distance 3
    "tall":   dict(n=63700,  p=260, lo=-128, hi=127, hold=(5,)),     # the largest k_sweep3 geometry (K3 = 249 streamers of 256 rows) on full-range bytes
    "edge":   dict(n=131071, p=32,  lo=-3,   hi=3,   hold=(0, 1)),   # n * xmax^2 = 2^31 - 16 384: the last panel the int32 Gram holds
    "over":   dict(n=131072, p=32,  lo=-3,   hi=3,   hold=(0, 1)),   # n * xmax^2 = 2^31: refused
}

# the plan each case is there for (bwgr_debug_panel_plan with the case's xmax and 16-bit verdict); D: k_sweep3's fold-in lag
EXPECT = {
    "c15":    dict(K=1,   R=256, nblocks=3, pipelined=1, fits3=1),
    "c16":    dict(K=1,   R=256, nblocks=3, pipelined=1, fits3=1),
    "c17":    dict(K=1,   R=256, nblocks=3, pipelined=1, fits3=1),
    "pm1":    dict(K=3,   R=256, nblocks=5, pipelined=1, fits3=1),
    "s127":   dict(K=2,   R=256, nblocks=3, pipelined=1, fits3=1),
    "full":   dict(K=2,   R=256, nblocks=3, pipelined=1, fits3=1),
    "dos100": dict(K=6,   R=256, nblocks=4, pipelined=1, fits3=1, D=4, xdist=3),
    "tall":   dict(K=249, R=256, nblocks=3, pipelined=1, fits3=1, D=3, K3=249, R3=256),
    "edge":   dict(K=147, R=896, nblocks=1, pipelined=1, fits3=0),      # (32-marker blocks: 1 029 streamers of 128 rows would be k_sweep3's, so k_sweep2)
    "over":   dict(K=147, R=896, nblocks=1, pipelined=1, fits3=0),
}
XMAX = {"c15": 15, "c16": 16, "c17": 17, "pm1": 1, "s127": 127, "full": 128, "dos100": 100, "tall": 128, "edge": 128, "over": 128}
GRAM16 = {"c15": 1, "c16": 1, "c17": 1, "dos100": 0}      # (every other case has negative entries; dos100's reach 1500 * 100^2)
TALL_STEP = 45      # tall's n + 45 rows are 250 slabs of 256: beyond the pipelined engines' grid

PLAN_FIELDS = ("m", "K", "R", "ld", "nblocks", "pstride", "nfeed", "lag4_ok", "lds", "lds2", "ldsw", "x_bytes", "gram_bytes", "pipelined", "xdist",
               "has16", "wdist", "try3", "fits3", "R3", "sub3", "K3", "D", "lds3", "solo3")


def panel_plan(n, p, xmax, gram16, kind=0):
    """Every field of bwgr_debug_panel_plan for an int8 panel at the default block (host arithmetic, no GPU)."""
    from bwgr_amd import _lib
    out = (C.c_int64 * len(PLAN_FIELDS))()
    rc = _lib.lib().bwgr_debug_panel_plan(0, int(n), int(p), 0, 0, int(kind), int(xmax), int(gram16), out)
    assert rc == 0, _lib.lib().bwgr_last_error().decode()
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def plan(tag):
    c = CASES[tag]
    return panel_plan(c["n"], c["p"], XMAX[tag], GRAM16.get(tag, 0))


@functools.lru_cache(maxsize=None)
def data(tag):
    """(X, y) of a case, from the fixed generator; not to be written to."""
    c = CASES[tag]
    X, y = codes_panel(c["n"], c["p"], c["lo"], c["hi"], SEED)
    for j in c["hold"]:
        X[:, j] = -128
    X.setflags(write=False); y.setflags(write=False)
    return X, y


# ---- chains -----------------------------------------------------------------------------------------------------------------------------
ALL_MODELS = ["BayesA", "BayesB", "BayesC", "BayesL", "BayesRR", "BayesCpi", "BayesDpi"]
SELECTION = ("BayesB", "BayesC", "BayesCpi", "BayesDpi")
CHAIN_TAGS = ["c16", "c17", "pm1", "s127", "full", "dos100"]
CHAIN_KW = dict(it=8, bi=2, pi=0.9, seed=21)
# the selection jobs the oracle's two flavours must decide alike: these, and `full` x BayesDpi
DECIDE_MODELS = ("BayesB", "BayesC", "BayesCpi")
DECIDE_JOBS = [(tag, m) for tag in ["c15"] + CHAIN_TAGS for m in DECIDE_MODELS] + [("full", "BayesDpi")]
# seeds 21 and 33 are the listed ones.  At 33 the oracle's flavours agree on the chain's state -- what the GPU is compared on at this size -- but part on
# marker 30 in the second iteration and meet again in the third; 34, the next seed at which they decide alike throughout, runs beside it
TALL_JOBS = [("BayesB", 21), ("BayesB", 33), ("BayesB", 34), ("BayesA", 21), ("BayesA", 33)]
TALL_ALIKE_ON_STATE_ONLY = (33,)
TALL_KW = dict(it=3, bi=0, pi=0.9)
REDO_JOBS = [(tag, m) for tag in ("s127", "c17") for m in ("BayesB", "BayesA")]
CENTRED_JOBS = [(tag, m, pi) for tag in ("s127", "dos100") for m, pi in (("BayesB", 0.9), ("BayesCpi", 0.0))]
CENTRED_SEED = 41      # test_implicit_centring_is_the_chain_on_the_centred_columns'
EDGE_JOBS = [("BayesB", 0.8), ("BayesRR", 0.0)]
EDGE_KW = dict(it=2, bi=0, seed=21)
PAIR_TAGS = ["c17", "s127"]


@functools.lru_cache(maxsize=None)
def oracle_chain(tag, model, **kw):
    """The oracle's chain (flavour "w") of a job, computed once and shared by every test that compares against it; not to be written to."""
    from oracle import oracle as O
    X, y = data(tag)
    return O.bayes(model, y, X, **kw)


def centred_f32(X):
    Xd = X.astype(np.float64)
    return np.asfortranarray((Xd - Xd.mean(0)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def oracle_centred_chain(tag, model, pi):
    from oracle import oracle as O
    X, y = data(tag)
    return O.bayes(model, y, centred_f32(X), it=CHAIN_KW["it"], bi=CHAIN_KW["bi"], pi=pi, seed=CENTRED_SEED)


# ---- KMUP, KMUP2, wgr, EM ---------------------------------------------------------------------------------------------------------------
KMUP_TAGS = ["c17", "s127", "full", "dos100"]
KMUP2_TAGS = ["c17", "s127", "dos100"]
KMUP_VE = 0.03
KMUP_SEED, KMUP2_SEED = 77, 78      # test_kmup_sweep_tpod's, test_kmup2_tpod's
WGR_TAGS = ["c17", "s127"]
WGR_SETTINGS = {"BRR": {}, "BayesB": {"iv": True, "pi": 0.5}, "bag": {"bag": 0.5}, "bag_over": {"bag": 1.5, "rp": True}}
WGR_BASE = dict(it=8, bi=2, seed=21)
EM_TAGS = ["c17", "full"]
EM_MODELS = ["emRR", "emBA", "emBB", "emBC", "emBCpi", "emDE", "emBL", "emEN", "emML", "lasso"]


def last_redo():
    """Sweeps the last KMUP / KMUP2 / wgr call of this thread redid on the fp64 residual (bwgr_debug_last_redo): those entry points have no chain
    to ask."""
    from bwgr_amd import _lib
    k = C.c_int(-1)
    _lib.check(_lib.lib().bwgr_debug_last_redo(C.byref(k)))
    return k.value


def kmup_inputs(tag):
    """b, d, xx, e, L as test_kmup_sweep_tpod makes them, on this case."""
    X, y = data(tag)
    p = X.shape[1]
    rs = np.random.RandomState(5)
    Xd = X.astype(np.float64)
    xx = (Xd ** 2).sum(0)
    b = rs.normal(size=p) * 0.01
    e = y - y.mean() - Xd @ b
    L = np.full(p, 120.0) * rs.uniform(0.5, 2.0, p)
    return dict(b=b, d=np.ones(p), xx=xx, e=e, L=L)


def kmup_tiny_inputs(tag, escale):
    """... and as test_kmup_with_a_zero_or_tiny_residual makes them: a residual of zero, or far below the steps."""
    X, _ = data(tag)
    n, p = X.shape
    rs = np.random.RandomState(4)
    xx = (X.astype(np.float64) ** 2).sum(0)
    b = rs.normal(size=p) * 0.02
    e = rs.normal(size=n) * escale
    L = np.full(p, 200.0) * rs.uniform(0.5, 2.0, p)
    return dict(b=b, d=np.ones(p), xx=xx, e=e, L=L, Ve=0.04, seed=17, it=2)


def kmup2_use(tag, variant):
    """Use: "half" of the rows, sorted, without repeats; "over": one and a half times the rows, sorted, with repeats."""
    n = CASES[tag]["n"]
    rs = np.random.RandomState(9)
    if variant == "half":
        return np.sort(rs.choice(n, n // 2, replace=False)).astype(np.int32)
    return np.sort(rs.choice(n, n + n // 2, replace=True)).astype(np.int32)


def kmup2_inputs(tag, variant, zero_e):
    k = kmup_inputs(tag)
    use = kmup2_use(tag, variant)
    E = np.zeros_like(k["e"]) if zero_e else k["e"]
    return dict(Use=use, b=k["b"], d=k["d"], xx=k["xx"] * (use.size / float(CASES[tag]["n"])), E=E, L=k["L"])


def em_y(tag):
    return np.asarray(data(tag)[1], np.float32)


# ---- KMUP2 beyond the bound: 140 000 rows drawn from a 70 000 x 32 panel with a column at -128 ------------------------------------------
def kmup2_over_inputs():
    """X, and KMUP2's inputs as kmup2_inputs makes them (xx = colSums(X^2) * nuse / n)."""
    n, p, nuse = 70000, 32, 140000
    X, y = codes_panel(n, p, -3, 3, SEED)
    X[:, 0] = -128
    assert n * 128 * 128 < 2 ** 31 <= nuse * 128 * 128
    use = np.sort(np.random.RandomState(9).choice(n, nuse, replace=True)).astype(np.int32)
    rs = np.random.RandomState(5)
    Xd = X.astype(np.float64)
    b = rs.normal(size=p) * 0.01
    return X, dict(Use=use, b=b, d=np.ones(p), xx=(Xd ** 2).sum(0), E=y - y.mean() - Xd @ b, L=np.full(p, 120.0) * rs.uniform(0.5, 2.0, p))
