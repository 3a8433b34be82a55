"""The shapes and settings of the driver parity tests (tests/test_gpu_drivers.py), kept in one place so that tests/test_driver_cases_cpu.py can
check, without a GPU, (1) that every shape still reaches the launch regime it is listed for, under the library's own host arithmetic
(bwgr_debug_panel_plan for the geometry of a main panel and of the row-subset scratch panel, bwgr_debug_aux_plan for the two-stage product
X * coef and the row gather), and (2) that every setting with inclusion decisions is one the reference itself decides the same way in both of
its flavours (no near-tie in u < p_include), so that an unequal decision on the GPU is a defect and not a coin toss.

The regimes:
  gemv    column chunks = min(512 int8 / 64 float, p / 512), at least 1; columns per chunk rounded up, the last chunk takes what is left;
          row workgroups of 256 threads x 16 rows (int8) or 4 rows (float)
  gather  float: element-wise.  int8: mpw = min(8, 32768 / ld) columns staged in LDS per workgroup while ld <= 65536 (mpw * ld bytes),
          element-wise above; a ragged last group when p % mpw != 0.  The subsample panel has its own slab count and, below block 128, its own
          slab height
"""
import ctypes as C
import functools

import numpy as np

from conftest import synth_small

MAIN, ROWS = 0, 1

# tag -> f32, n, p, block (0 = the default), seed of the genotypes
CASES = {
    "mid":     dict(f32=0, n=1500,  p=1300,  block=0,  seed=2800),
    "mid16":   dict(f32=0, n=2000,  p=300,   block=16, seed=2801),
    "tall9k":  dict(f32=0, n=9000,  p=1100,  block=0,  seed=2802),
    "tall40k": dict(f32=0, n=40000, p=300,   block=0,  seed=2803),
    "tall70k": dict(f32=0, n=70000, p=100,   block=16, seed=2804),
    "wide":    dict(f32=0, n=300,   p=70000, block=0,  seed=2805),
    "flt":     dict(f32=1, n=1300,  p=1101,  block=0,  seed=2806),
    "signed":  dict(f32=0, n=700,   p=1031,  block=0,  seed=2807),
}

# What each shape is there for, as the plans must report it.  K, R: slabs and their height; last_block: markers of the last block; chunks, cpc,
# last_chunk, row_wgs: the product; gather: 0 element-wise, else mpw; gather_lds in bytes; ragged: p % mpw.
EXPECT = {
    "mid":     dict(K=6, R=256, nblocks=11, last_block=20, chunks=2, cpc=650, last_chunk=650, row_wgs=1, gather=8, ragged=4),
    "mid16":   dict(K=2, R=1024, nblocks=19, last_block=12, chunks=1, cpc=300, last_chunk=300, row_wgs=1, gather=8, ragged=4),
    "tall9k":  dict(K=36, R=256, ld=9216, chunks=2, cpc=550, last_chunk=550, row_wgs=3, gather=3, ragged=2),
    "tall40k": dict(K=157, R=256, ld=40192, chunks=1, row_wgs=10, gather=1, gather_lds=40192),
    "tall70k": dict(K=55, R=1280, ld=70400, chunks=1, row_wgs=18, gather=0, gather_lds=0),
    "wide":    dict(K=2, R=256, nblocks=547, chunks=136, cpc=515, last_chunk=475, row_wgs=1, gather=8),
    "flt":     dict(K=11, R=128, m=64, nblocks=18, last_block=13, chunks=2, cpc=551, last_chunk=550, row_wgs=2, gather=0),
    "signed":  dict(K=3, R=256, nblocks=9, last_block=7, chunks=2, cpc=516, last_chunk=515, row_wgs=1, gather=8, ragged=7),
}

# row subsamples: (tag, rows) -> K, R of the scratch panel, against the base panel's
SUBSAMPLES = {
    ("mid", 750):      dict(K=3, R=256),     # same height, fewer slabs
    ("mid", 2250):     dict(K=9, R=256),     # bag = 1.5 with replacement: taller than the base
    ("mid16", 600):    dict(K=1, R=640),     # another slab height: Ro != Rb in the gather
    ("mid16", 1000):   dict(K=1, R=1024),
    ("tall9k", 4500):  dict(K=18, R=256),
    ("tall40k", 20000): dict(K=79, R=256),
    ("tall70k", 35000): dict(K=28, R=1280),
    ("flt", 650):      dict(K=6, R=128),
    # all but a twentieth of the rows: the base panel's own geometry
    ("mid", 1425): dict(K=6, R=256), ("mid16", 1900): dict(K=2, R=1024), ("tall9k", 8550): dict(K=34, R=256),
    ("tall40k", 38000): dict(K=149, R=256), ("tall70k", 66500): dict(K=52, R=1280), ("flt", 1235): dict(K=10, R=128),
}


def panel_plan(f32, n, p, block=0, kind=MAIN):
    """m, K, R, ld, nblocks of bwgr_debug_panel_plan (host arithmetic, no GPU)."""
    from bwgr_amd import _lib
    out = (C.c_int64 * 25)()
    rc = _lib.lib().bwgr_debug_panel_plan(int(f32), int(n), int(p), int(block), 0, int(kind), -1, 1, out)
    assert rc == 0, _lib.lib().bwgr_last_error().decode()
    pl = dict(zip(("m", "K", "R", "ld", "nblocks"), (int(v) for v in out[:5])))
    pl["last_block"] = p - (pl["nblocks"] - 1) * pl["m"]
    return pl


AUX_FIELDS = ("chunks", "cpc", "row_wgs", "gather", "gather_lds")


def aux_plan(f32, p, ld):
    """(status, dict) of bwgr_debug_aux_plan: column chunks, columns per chunk, row workgroups of the product; path and LDS bytes of the gather."""
    from bwgr_amd import _lib
    out = (C.c_int64 * len(AUX_FIELDS))(*([-1] * len(AUX_FIELDS)))
    rc = _lib.lib().bwgr_debug_aux_plan(int(f32), int(p), int(ld), out)
    pl = dict(zip(AUX_FIELDS, (int(v) for v in out)))
    if rc == 0:
        pl["last_chunk"] = p - (pl["chunks"] - 1) * pl["cpc"]
        pl["ragged"] = p % pl["gather"] if pl["gather"] else 0
    return rc, pl


def plans(tag):
    c = CASES[tag]
    pl = panel_plan(c["f32"], c["n"], c["p"], c["block"])
    rc, ax = aux_plan(c["f32"], c["p"], pl["ld"])
    assert rc == 0
    pl.update(ax)
    return pl


def panel_kw(tag):
    return {"block": CASES[tag]["block"]} if CASES[tag]["block"] else {}


@functools.lru_cache(maxsize=None)
def data(tag):
    """(X, y): the genotypes as the panel takes them (int8, or float32 for "flt") and a phenotype, from fixed seeds."""
    c = CASES[tag]
    if tag == "signed":     # signed bytes: -2 .. 2
        rng = np.random.default_rng(c["seed"])
        X = np.asfortranarray(rng.integers(-2, 3, size=(c["n"], c["p"])).astype(np.int8))
        y = X[:, :25].astype(np.float64) @ rng.normal(size=25) * 0.3 + rng.normal(size=c["n"]) + 1.0
        return X, y
    X, y = synth_small(c["n"], c["p"], seed=c["seed"])
    y = y + 2.0             # synth_small's phenotype has mean zero: an intercept away from zero, so that the relative tolerance on mu means something
    if tag == "flt":        # centred and scaled genotypes, as test_float_panel_chains makes them
        Xd = X.astype(np.float64)
        return np.asfortranarray(((Xd - Xd.mean(0)) / (Xd.std(0) + 0.5)).astype(np.float32)), y
    return X, y


# ---- wgr ------------------------------------------------------------------------------------------------------------------------------------
# the six settings of test_wgr_tpod (man/wgr.Rd:82) and the three of test_wgr_bagging_tpod
WGR_SETTINGS = {"BRR": {}, "BayesA": {"iv": True}, "BayesB": {"iv": True, "pi": 0.5}, "BayesC": {"pi": 0.5}, "BayesL": {"de": True},
                "thin": {"th": 3, "bi": 4}}
BAG_SETTINGS = {"bag": {"bag": 0.5}, "bag_rp_B": {"bag": 0.8, "rp": True, "iv": True, "pi": 0.5}, "bag_C": {"bag": 0.7, "pi": 0.3}}
WGR_BASE = dict(it=12, bi=3, th=1, df=5, R2=0.5, seed=21)
WGR_TALL = dict(it=4, bi=1, seed=17)      # the tall shapes reach their branch in the first iteration


def _jobs(tags, settings, base, prefix=""):
    out = []
    for tag in tags:
        for name, kw in settings.items():
            args = dict(base); args.update(kw)
            out.append(("%s-%s%s" % (tag, prefix, name), tag, args))
    return out


WGR_JOBS = _jobs(["mid", "flt", "signed"], WGR_SETTINGS, WGR_BASE) + \
    _jobs(["wide"], {k: WGR_SETTINGS[k] for k in ("BRR", "BayesC")}, dict(WGR_BASE, it=6, bi=2))
BAG_JOBS = _jobs(["mid", "mid16", "tall9k", "flt"], BAG_SETTINGS, dict(it=10, bi=3, seed=17)) + \
    [("mid-bag_over", "mid", dict(it=10, bi=3, seed=17, bag=1.5, rp=True))] + \
    _jobs(["tall40k"], {k: BAG_SETTINGS[k] for k in ("bag", "bag_C")}, WGR_TALL) + \
    _jobs(["tall70k"], {k: BAG_SETTINGS[k] for k in ("bag", "bag_C")}, WGR_TALL)
# seeds replaced where the reference's own two flavours decide differently at the seed above (tests/test_driver_cases_cpu.py finds that without a
# GPU).  Seeds were tried counting upwards from the default and the FIRST at which the flavours agree was taken, never a later one; of the 30 bagging
# settings 4 needed another seed: the second tried for three of them, the fifth for tall40k-bag_C
_RESEED = {"tall9k-bag_rp_B": 18, "tall40k-bag_C": 21, "tall70k-bag_C": 18, "flt-bag_rp_B": 18}
BAG_JOBS = [(name, tag, dict(args, seed=_RESEED.get(name, args["seed"]))) for name, tag, args in BAG_JOBS]


@functools.lru_cache(maxsize=None)
def mid_eigk():
    """eigen(K) of the centred `mid` genotypes, K scaled to a mean diagonal of one, as test_gpu_parity._tpod_eigk makes it."""
    Z = data("mid")[0].astype(np.float64); Z = Z - Z.mean(0)
    K = Z @ Z.T; K = K / np.mean(np.diag(K))
    w, v = np.linalg.eigh(K); o = np.argsort(-w)
    return {"values": w[o], "vectors": v[:, o]}


def eigk_case(which):
    """(eigK, VarK, pk): VarK 0.5 and 0.1 truncate to several float blocks and to less than one; "pk5" is a hand-truncated list."""
    eig = mid_eigk()
    if which == "pk5":
        eig = {"values": eig["values"][:5], "vectors": eig["vectors"][:, :5]}
        cs = np.cumsum(eig["values"]) / 5.0
        vark = float(0.5 * (cs[3] + cs[4]))      # the fifth value is the first to pass it
    else:
        vark = float(which)
    V = eig["values"]
    return eig, vark, int(np.argmax((np.cumsum(V) / V.size) > vark)) + 1


EIGK_PK = {"0.5": 239, "0.1": 36, "pk5": 5}
EIGK_SETTINGS = {"BRR": {}, "BayesB": {"iv": True, "pi": 0.5}}     # both settings of test_wgr_polygenic_term_tpod
EIGK_BASE = dict(it=10, bi=3, seed=13)


# missing phenotypes and genotypes on `mid` (R/wgr.R:12-18, 34-39): the rows dropped sit on both sides of slab boundaries (256, 512, 1024)
MISSING_KW = dict(it=10, bi=3, seed=9)
MISSING_ROWS = [3, 255, 256, 257, 511, 700, 1023, 1024, 1499]
MISSING_CELLS = [(7, 11), (100, 200), (256, 0), (1400, 1299), (1499, 640)]


def missing_case():
    """(y, X) with NaNs as the caller passes them, and the mean-imputed X and the rows kept, as the reference makes them."""
    X, y = data("mid")
    X = X.astype(np.float64); y = y.copy()
    y[MISSING_ROWS] = np.nan
    for i, j in MISSING_CELLS:
        X[i, j] = np.nan
    Xi = X.copy(); cm = np.nanmean(Xi, axis=0); idx = np.where(np.isnan(Xi)); Xi[idx] = cm[idx[1]]
    return y, X, Xi, ~np.isnan(y)


# ---- KMUP, KMUP2 ------------------------------------------------------------------------------------------------------------------------
KMUP_TAGS = ["mid", "tall9k", "flt", "signed"]
KMUP2_TAGS = ["mid", "mid16", "tall9k", "tall40k", "tall70k", "flt"]
KMUP2_ROWS = {"mid": 750, "mid16": 600, "tall9k": 4500, "tall40k": 20000, "tall70k": 35000, "flt": 650}
KMUP2_VARIANTS = ["sorted", "repeats", "unsorted", "over", "most"]     # "over": more rows than the panel has; "most": all but a twentieth
KMUP_VE = 0.03
KMUP2_SEED = {("tall9k", "over"): 81, ("tall40k", "sorted"): 79, ("tall40k", "unsorted"): 80, ("tall40k", "most"): 79, ("tall70k", "sorted"): 79,
              ("tall70k", "unsorted"): 79}      # default 78, test_kmup2_tpod's; replaced as _RESEED above: 6 of 30 cases, all on the tall
# shapes (one flip among 300 or 100 decisions on 20 000+ rows): the second seed tried for four, the third for one, the fourth for one


def kmup2_seed(tag, variant):
    return KMUP2_SEED.get((tag, variant), 78)


def kmup_inputs(tag):
    """b, d, xx, e, L of test_kmup_sweep_tpod on this shape."""
    X, y = data(tag)
    p = X.shape[1]
    rs = np.random.RandomState(5)
    Xd = X.astype(np.float64)
    xx = (Xd ** 2).sum(0)
    b = rs.normal(size=p) * 0.01
    e = y - y.mean() - Xd @ b
    L = np.full(p, 120.0) * rs.uniform(0.5, 2.0, p)
    return dict(b=b, d=np.ones(p), xx=xx, e=e, L=L)


def kmup2_use(tag, variant):
    n = CASES[tag]["n"]; k = KMUP2_ROWS[tag]
    rs = np.random.RandomState(9)
    if variant == "sorted":
        return np.sort(rs.choice(n, k, replace=False)).astype(np.int32)
    if variant == "repeats":
        return np.sort(rs.choice(n, k, replace=True)).astype(np.int32)
    if variant == "unsorted":
        return rs.choice(n, k, replace=True).astype(np.int32)
    if variant == "most":
        return np.sort(rs.choice(n, n - n // 20, replace=False)).astype(np.int32)
    return np.sort(rs.choice(n, n + n // 10 + 3, replace=True)).astype(np.int32)


def kmup2_inputs(tag, variant):
    """Use, b, d, xx, E, L as test_kmup2_tpod makes them (xx = colSums(X^2) * nuse / n, as wgr passes it)."""
    k = kmup_inputs(tag)
    use = kmup2_use(tag, variant)
    return dict(Use=use, b=k["b"], d=k["d"], xx=k["xx"] * (use.size / float(CASES[tag]["n"])), E=k["e"], L=k["L"])


# ---- fused chains -----------------------------------------------------------------------------------------------------------------------
ALL_MODELS = ["BayesA", "BayesB", "BayesC", "BayesL", "BayesRR", "BayesCpi", "BayesDpi"]
SELECTION = ("BayesB", "BayesC", "BayesCpi", "BayesDpi")
CHAIN_JOBS = [(tag, m) for tag in ("mid", "signed") for m in ALL_MODELS] + [(tag, m) for tag in ("flt", "wide") for m in ("BayesA", "BayesB", "BayesCpi")]
CHAIN_KW = dict(it=12, bi=3, pi=0.9, df=5, R2=0.5)
# default 11, test_short_chain_tpod's; replaced as _RESEED above: 3 of 14 selection chains, the second seed tried for two, the third for wide BayesB
CHAIN_SEED = {("wide", "BayesB"): 13, ("wide", "BayesCpi"): 12, ("flt", "BayesB"): 12}
# 70 000 decisions per iteration on 300 rows: over twelve iterations the reference's two flavours parted at 28 of the 29 seeds tried for BayesCpi, so no
# seed was picked at that length; at six iterations the seeds above are the third and the second tried
CHAIN_WIDE = dict(it=6, bi=2)
CAUSAL = 7          # the marker made strongly causal: in the model in every iteration the reference keeps


def chain_kw(tag, model):
    return dict(CHAIN_KW, seed=CHAIN_SEED.get((tag, model), 11), **(CHAIN_WIDE if tag == "wide" else {}))


@functools.lru_cache(maxsize=None)
def chain_y(tag):
    X, y = data(tag)
    x = X[:, CAUSAL].astype(np.float64)
    return y + 6.0 * float(np.std(y)) * (x - x.mean()) / x.std()


# model, pi, seed: on `mid` with set_centred(True); 41 is the existing test's seed, 42 the second tried for BayesCpi (as _RESEED above)
CENTRED_JOBS = [("BayesB", 0.9, 41), ("BayesCpi", 0.0, 42)]
CENTRED_KW = dict(it=10, bi=2)


def centred_f32(X):
    Xd = X.astype(np.float64)
    return np.asfortranarray((Xd - Xd.mean(0)).astype(np.float32))


# ---- two-effect samplers ----------------------------------------------------------------------------------------------------------------
def bayes2_inputs():
    X1, y = data("mid")
    rng = np.random.default_rng(5)
    X2 = rng.normal(size=(X1.shape[0], 200)).astype(np.float32)
    y2 = (y + 0.7 * X2[:, 0]).astype(np.float32)
    return X1.astype(np.float32), X2, y2


BAYES2_KW = dict(it=12, bi=3, seed=22)      # (test_two_effect_samplers' 21 parts the flavours on BayesB2's d1: the second seed tried)
BAYES2_PI = 0.7
