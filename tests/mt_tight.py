"""The yardstick of tests/test_mt_tight_cpu.py and tests/test_gpu_mt_tight.py: the multi-trait fp64 fits (mrr / mrr_float on the int8 train,
mrr(Y, dense(X)) and mkr on the dense train, PEGS and PEGSZ with panel, dense and sparse effects, PEGS_sparse and PEGSZ_sparse, PEGSX) held to
bounds that come from the restatements alone, as tests/uvb_tight.py holds the per-trait fits; scaled_err, perms, MARGIN, NRUNS and FLOOR are
its.

For a case of tests/mt_tight_cases.py, ref(name) is the restatement (mrr_restatement.mrr, pegs_restatement.pegsz -- with mu_div_n=True for
PEGSZ_sparse's text --, pegsx_restatement.pegsx) run in long double, with
the k x k routines of tests/ld_linalg.py.  yard(name)[key] is the largest scaled error against it over NRUNS float64 runs of the same
restatement: the rows as given and under eight fixed permutations of the rows, the same one for Y, for every design and for PEGSX's X, with hat put back in
the given order.  The marker orders are those of bwgr_amd.em_order, made once per case and handed to all ten runs.  A permutation changes the
order of every row sum and nothing else, so the spread of the nine runs around the long double result is what fp64 rounding alone does to
this case and this key, and the library is a tenth order:

    bound(name)[key] = kappa * max(MARGIN * yard[key], MARGIN * 2**-52),      MARGIN = 64.

kappa is 1 for the dense train, which centres its design explicitly, and for PEGS / PEGSZ / PEGSX, which do not centre: restatement and
kernels sum the same terms, and PEGSX's TrZSZ = sum z^2 - v'A v is the same difference in both.  A sparse effect is restated on its dense
copy with the values rounded to float, as the library stores them, and PEGSX's dense Z likewise.  The int8 train keeps raw
int8 columns and centres implicitly: where the restatement forms xc_J'e with xc = x - xbar, the library forms x_J'e - xbar_J sum(e), and its
block Gram is G - xbar_i S(j) - xbar_j S(i) + n_t xbar_i xbar_j.  Each of these is a difference of terms that are larger than the result by at
most sum x^2 / sum (x - xbar)^2 (Cauchy-Schwarz: |x'e| <= |x| |e| where |xc'e| <= |xc| |e|, and the same ratio for the Gram's diagonal), so
the rounding of the raw terms, relative to the result, is at most that ratio times the rounding of the centred ones.  For the int8 train

    kappa = max over the columns of sum x^2 / sum (x - xbar)^2 over all rows,

computed from the case's panel on the host (3.2 on 0/1/2 codes with allele frequencies up to 0.5, about 36 with frequencies up to 0.95).
No number from the GPU enters a bound.

Keys: mu, b, hat, h2, GC, vb, ve, MSx, cnvB, cnvH2, cnvV for mrr, mkr and the dense train; mu, hat, h2, cnv_trace and every effect's b, GC
and bend (b0, GC0, bend0, b1, ...) for PEGS / PEGSZ; b, ve, hat, cnv_trace and every effect's TrZSZ, u, vb, GC and bend for PEGSX; and hat_own: hat against the long double product of the same result's own b and mu
with the design (centred for mrr, raw for PEGS; for PEGSX the returned b with the float-rounded X plus every returned u with its design), so
that an error of the kernels that form hat (k_pegs_zb, the panel's hat kernels, k_pegs_sparse_hat) is not masked by b's own.  Its / numit must
be equal; NaN, +inf and -inf must stand in the same places.  Everything is computed once per session and left unchanged."""
import functools

import numpy as np

import mrr_restatement as MR
import mt_tight_cases as TC
import pegs_restatement as PR
import pegs_sparse_restatement as SR  # noqa: F401  (row_disjoint, for the tests)
import pegsx_restatement as XR
from uvb_tight import FLOOR, LD, MARGIN, NRUNS, f32, perms, scaled_err as _scaled_err

KEYS_MRR = ("mu", "b", "hat", "h2", "GC", "vb", "ve", "MSx", "cnvB", "cnvH2", "cnvV")


def scaled_err(a, b):
    """uvb_tight.scaled_err with +inf and -inf held to the same places (and compared as 0)"""
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    assert a.shape == b.shape, (a.shape, b.shape)
    for v in (np.inf, -np.inf):
        assert np.array_equal(a == v, b == v), (a, b)
    fin = ~np.isinf(b)
    return _scaled_err(np.where(fin, a, 0), np.where(fin, b, 0))


KEYS_PEGSX_EFFECT = ("TrZSZ", "u", "vb", "GC", "bend")


def keys(c):
    if c["family"] == "pegsx":
        return ("b", "ve", "hat", "cnv_trace") + tuple("%s%d" % (key, r) for r in range(len(c["effects"])) for key in KEYS_PEGSX_EFFECT) + ("hat_own",)
    if c["family"] == "pegs":
        return ("mu", "hat", "h2", "cnv_trace") + tuple("%s%d" % (key, f) for f in range(len(c["effects"])) for key in ("b", "GC", "bend")) + ("hat_own",)
    return KEYS_MRR + ("hat_own",)


def b_keys(c):
    if c["family"] == "pegsx":
        return ("b",) + tuple("u%d" % r for r in range(len(c["effects"])))
    return tuple("b%d" % f for f in range(len(c["effects"]))) if c["family"] == "pegs" else ("b",)


def kappa(c):
    return TC.kappa(c["X"]) if c["family"] == "mrr" else 1.0


def _design(c, e):
    """an effect as the library reads it: a sparse design's values are floats, and so is PEGSX's dense Z"""
    return f32(e[1]) if e[0] == "sparse" or (e[0] == "dense" and c["family"] == "pegsx") else e[1]


def designs(c):
    return [_design(c, e) for e in c["effects"]] if c["family"] in ("pegs", "pegsx") else [c["X"]]


class _Orders:
    """orders[s]: sweep s's marker order(s) from bwgr_amd.em_order, made when first asked for and kept"""

    def __init__(self, c):
        self.ps, self.pegs, self.made = [D.shape[1] for D in designs(c)], c["family"] in ("pegs", "pegsx"), {}

    def __getitem__(self, s):
        if s not in self.made:
            import bwgr_amd
            o = [bwgr_amd.em_order(p, s) for p in self.ps]
            self.made[s] = o if self.pegs else o[0]
        return self.made[s]


@functools.lru_cache(None)
def orders(name):
    return _Orders(TC.case(name))


@functools.lru_cache(None)
def _wide_designs(name):
    c = TC.case(name)
    Ds = [np.asarray(D, LD) for D in designs(c)]
    return Ds if c["family"] in ("pegs", "pegsx") else [Ds[0] - Ds[0].mean(0)]


@functools.lru_cache(None)
def _wide_fixed(name):
    return np.asarray(f32(TC.case(name)["X"]), LD)


def hat_of(name, r):
    """the long double product of a flat result's own b and mu with the case's designs: centred for mrr, raw for PEGS; for PEGSX of its b
    with the float-rounded X and of every u with its design"""
    Ds = _wide_designs(name)
    if "u0" in r:
        X = _wide_fixed(name)
        return X @ np.asarray(r["b"], LD).reshape(X.shape[1], -1) + sum(D @ np.asarray(r["u%d" % i], LD).reshape(D.shape[1], -1) for i, D in enumerate(Ds))
    bs = [r["b%d" % f] for f in range(len(Ds))] if "b0" in r else [r["b"]]
    return sum(D @ np.asarray(b, LD).reshape(D.shape[1], -1) for D, b in zip(Ds, bs)) + np.asarray(r["mu"], LD)


def flat(c, r):
    """a fit's dict, the library's or the restatement's, under the keys of keys(c) (hat_own excepted) and "its" """
    if c["family"] == "pegsx":
        ne = len(c["effects"])
        k = np.asarray(r["ve"]).size
        o = dict(b=np.asarray(r["b"]), ve=np.asarray(r["ve"]), hat=np.asarray(r["hat"]).reshape(-1, k), cnv_trace=np.asarray(r["cnv_trace"]), its=int(r["its"]))
        bend = np.asarray(r["bend"]).reshape(-1)
        for i in range(ne):
            o["TrZSZ%d" % i], o["u%d" % i], o["vb%d" % i], o["GC%d" % i], o["bend%d" % i] = (np.asarray(r["TrZSZ"][i]), np.asarray(r["u"][i]),
                                                                                             np.asarray(r["vb_list"][i]), np.asarray(r["GC_list"][i]), bend[i])
        return o
    if c["family"] != "pegs":
        k = np.asarray(r["mu"]).size
        return dict({key: np.asarray(r[key]) for key in KEYS_MRR}, hat=np.asarray(r["hat"]).reshape(-1, k), its=int(r["Its"]))
    ne = len(c["effects"])
    bs, GCs = (r["b"], r["GC"]) if isinstance(r["b"], list) else ([r["b"]], [r["GC"]])
    o = dict(mu=np.asarray(r["mu"]), hat=np.asarray(r["hat"]), h2=np.asarray(r["h2"]), cnv_trace=np.asarray(r["cnv_trace"]), its=int(r["numit"]))
    bend = np.asarray(r["bend"]).reshape(ne)
    for f in range(ne):
        o["b%d" % f], o["GC%d" % f], o["bend%d" % f] = np.asarray(bs[f]), np.asarray(GCs[f]), bend[f]
    return o


DEC = ("inflated", "MinDVb", "maxEv", "gap", "near0")


def run(name, dtype=np.float64, perm=None, dot=None, **mutant):
    """The restatement on a case, on what the library receives (float-rounded Y for mrr_float), with the rows permuted by perm and hat put
    back: the flat result, with "dec": the decisions of every sweep -- (bent, lam) for mrr, per effect (inflated, MinDVb, maxEv, gap, near0)
    for PEGS and PEGSX.  PEGSX adds "mm", per trait (eigenvalues of M'M kept, smallest kept ratio, largest dropped ratio or 0), and "floors",
    the names of every floor that was active anywhere in the fit; mutant: its fixed_dot= and trace_dot=."""
    c = TC.case(name)
    Y = f32(c["Y"]) if c.get("variant") == "F" else c["Y"]
    Ds, X = designs(c), c.get("X")
    if perm is not None:
        Y, Ds = Y[perm], [D[perm] for D in Ds]
        X = X[perm] if c["family"] == "pegsx" else X
    more = {}
    if c["family"] == "pegsx":
        r = XR.pegsx(Y, X, Ds, orders=orders(name), trace=True, dtype=dtype, dot=dot, **mutant, **c["kw"])
        dec = [[tuple(rec[key] for key in DEC) for rec in recs] for recs in r["trace"]]
        more["mm"] = [(m["kept"].size, m["kept"].min(initial=np.inf), m["dropped"].max(initial=0)) for m in r["mm"]]
        more["floors"] = set(r["floors0"]).union(*[rec["floors"] for recs in r["trace"] for rec in recs])
    elif c["family"] == "pegs":
        r = PR.pegsz(Y, Ds, own_text=c["entry"] in ("PEGS", "PEGS_sparse"), mu_div_n=c["entry"] == "PEGSZ_sparse", orders=orders(name), trace=True,
                     dtype=dtype, dot=dot, **c["kw"])
        dec = [[tuple(rec[key] for key in DEC) for rec in recs] for recs in r["trace"]]
    else:
        r = MR.mrr(Y, Ds[0], orders=orders(name), trace=True, dtype=dtype, dot=dot, **c["kw"])
        dec = [(t["bent"], t["lam"]) for t in r["trace"]]
    o = flat(c, r)
    if perm is not None:
        hat = np.empty_like(o["hat"])
        hat[perm] = o["hat"]
        o["hat"] = hat
    o["dec"] = dec
    o.update(more)
    return o


@functools.lru_cache(None)
def ref(name):
    return run(name, LD)


def errs(name, got, o):
    """key -> scaled_err(the flat result got, the long double result o); equal its asserted; hat_own against got's own product"""
    assert got["its"] == o["its"], (got["its"], o["its"])
    return {key: scaled_err(got["hat"], hat_of(name, got)) if key == "hat_own" else scaled_err(got[key], o[key]) for key in keys(TC.case(name))}


@functools.lru_cache(None)
def runs(name):
    """The NRUNS float64 runs against ref(name): a tuple of (errors, decisions, PEGSX's dict(mm, floors) or None)."""
    o, out = ref(name), []
    for pm in perms(TC.case(name)["Y"].shape[0]):
        r = run(name, perm=pm)
        out.append((errs(name, r, o), r["dec"], dict(mm=r["mm"], floors=r["floors"]) if "mm" in r else None))
    return tuple(out)


@functools.lru_cache(None)
def yard(name):
    return {key: max(r[0][key] for r in runs(name)) for key in keys(TC.case(name))}


def bound(name):
    kap = kappa(TC.case(name))
    return {key: kap * max(MARGIN * v, FLOOR) for key, v in yard(name).items()}


def float_dot(x, e):
    """The mutant: the step's dependent dot x_J'e through a float."""
    return (x @ e).astype(np.float32).astype(np.float64)


def float_tdot(M, e):
    """The mutants of PEGSX's fixed_dot= and trace_dot=: M'e (a vector e or a matrix of columns) through a float."""
    return float_dot(M.T, e)
