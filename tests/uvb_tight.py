"""The yardstick of tests/test_uvb_tight_cpu.py and tests/test_gpu_uvb_tight.py: the per-trait fp64 fits (uvbeta, uvbeta_dense, uvbeta2) held
to bounds that come from the restatements alone.

For a case of tests/uvb_tight_cases.py, ref(name) is the restatement run in long double (uvb_restatement / sem2_restatement with
dtype=np.longdouble: 64 bits of mantissa against float64's 53).  yard(name)[key] is the largest scaled error against it over NRUNS float64
runs of the same restatement: the rows as given and under eight fixed random permutations of the rows (the same one for Y, X and Z).  A
permutation changes the order of every row sum and nothing else, so the runs are nine summation orders of one fp64 recurrence, and their
spread around the long double result is what rounding alone does to this case and this key.  The library is a tenth order:

    bound(name)[key] = max(MARGIN * yard[key], MARGIN * 2**-52),      MARGIN = 64.

The margin covers the accumulation style (the kernels add tiles sequentially and in fixed trees, numpy pairwise: sqrt(n) to n against log2 n,
a ratio below 8 at these row counts) times the spread between draws (up to 8 in the scalar keys).  The floor is the margin on one rounding
of the result, for a yardstick that happens to come out exact.  No number from the GPU enters a bound.

scaled_err is max |a - b| / max |b| over the key's array, evaluated in long double with the long double result as b; NaN must stand in the
same places; its must be equal.  Everything is computed once per session and left unchanged."""
import functools

import numpy as np

import sem2_restatement as S2
import uvb_restatement as UR
import uvb_tight_cases as TC

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble is no wider than float64 here: it cannot be the yardstick"
MARGIN = 64
FLOOR = MARGIN * 2.0 ** -52
NRUNS = 9
KEYS = {"uvbeta": ("b", "mu", "ve", "vb", "h2", "cnv"), "dense": ("b", "mu", "ve", "vb", "h2", "cnv"),
        "uvbeta2": ("b1", "b2", "mu", "h2", "ve", "vb1", "vb2", "cnv")}


def f32(Y):
    return np.asarray(Y, np.float64).astype(np.float32).astype(np.float64)


def scaled_err(a, b):
    """max |a - b| / max |b| in long double, NaN in the same places (asserted; compared as 0)."""
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    if not b.size:
        return 0.0
    a, b = np.nan_to_num(a), np.nan_to_num(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), LD(1e-300)))


@functools.lru_cache(None)
def perms(n):
    """The rows as given (None) and eight fixed random permutations of them."""
    return (None,) + tuple(np.random.default_rng(7000 + i).permutation(n) for i in range(1, NRUNS))


def keys(c):
    return KEYS[c["entry"]] + (("xb",) if c.get("xb") else ())


def xb(X, b):
    """X b in long double."""
    return np.asarray(X, LD) @ np.asarray(b, LD)


def run(c, dtype=np.float64, perm=None, **mutant):
    """The restatement on a case: on what the library's variant receives (float-rounded Y for F, X and Z), on the case's columns of Y, with
    the rows permuted by perm.  With xb, out["xb"] is X b in dtype, on the rows as given."""
    Y = c["Y"] if c.get("cols") is None else c["Y"][:, list(c["cols"])]
    A = [Y if c.get("variant", "D") == "D" else f32(Y)] + [c[key] for key in ("Z", "X") if key in c]
    if perm is not None:
        A = [a[perm] for a in A]
    if c["entry"] == "uvbeta2":
        return S2.uvbeta2(*A, dtype=dtype, **c["kw"], **mutant)
    o = UR.uvbeta(*A, c["variant"], dtype=dtype, **c["kw"], **mutant)
    if c.get("xb"):
        o["xb"] = np.asarray(c["X"], dtype) @ o["b"]
    return o


@functools.lru_cache(None)
def ref(name):
    return run(TC.case(name), LD)


def errs(c, got, o):
    """key -> scaled_err(got, the long double result o); equal its asserted.  xb is held against the long double product of got's own b."""
    assert np.array_equal(got["its"], o["its"]), (got["its"], o["its"])
    return {key: scaled_err(got[key], xb(c["X"], got["b"]) if key == "xb" else o[key]) for key in keys(c)}


@functools.lru_cache(None)
def runs(name):
    """The NRUNS float64 runs' errors against ref(name): a tuple of dicts."""
    c, o = TC.case(name), ref(name)
    return tuple(errs(c, run(c, perm=pm), o) for pm in perms(c["Y"].shape[0]))


@functools.lru_cache(None)
def yard(name):
    return {key: max(r[key] for r in runs(name)) for key in keys(TC.case(name))}


def bound(name):
    return {key: max(MARGIN * v, FLOOR) for key, v in yard(name).items()}
