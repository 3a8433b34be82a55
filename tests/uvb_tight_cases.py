"""The cases of tests/test_uvb_tight_cpu.py and tests/test_gpu_uvb_tight.py: inputs on which the per-trait fp64 fits are held to the bounds of
tests/uvb_tight.py.  They are the shapes of tests/test_gpu_uvb.py, tests/test_gpu_uvbd.py and tests/sem2_cases.py, made by their generators,
at the sizes at which the kernels take another path; tol = 0 and six sweeps unless a case says otherwise.

A case is dict(entry, Y, kw, ...): entry "uvbeta" with X, variant[, panel_kw, xb, cols]; "dense" with Z, variant; "uvbeta2" with Z, X[,
panel_kw].  panel names the Panel a GPU module shares between the cases of one shape.  cols: the columns of Y that are compared (the library
fits all of them; the traits do not couple)."""
import functools

import numpy as np

import sem2_cases as C
from test_gpu_mrr import _traits, _traits_ids
from test_gpu_uvb import _f32, _slabs900, _stopping_case, _tpod, _W
from test_gpu_uvbd import _case as _dense_case, _lds_rows

SIX = dict(maxit=6, tol=0)
SLABS = dict(panel="slabs900", panel_kw=dict(nwg=3))


def _uvb(Y, X, variant, kw=SIX, panel=None, **more):
    return dict(entry="uvbeta", Y=Y, X=X, variant=variant, kw=dict(kw), panel=panel, **more)


def _tpod_variant(v):
    return _uvb(_traits(_tpod(), 3, 0.1, seed=11), _tpod(), v, panel="tpod")


def _slabs_k5(v):
    """700 x 900 with nwg = 3: three row slabs, a last block of 4 markers; four patterns and one fully observed trait."""
    return _uvb(_traits(_slabs900(), 5, 0, seed=5, patterns=[0.1, 0.0, 0.25, 0.05, 0.4]), _slabs900(), v, xb=True, **SLABS)


def _slabs_k17():
    """One pattern per trait: the first solve workgroup holds 16 patterns, nine Gram matrices in LDS slots and seven read from global memory."""
    Y = _traits(_slabs900(), 17, 0.15, seed=31)
    assert len({np.isnan(Y[:, t]).tobytes() for t in range(17)}) == 17
    return _uvb(Y, _slabs900(), "D", **SLABS)


def k65_cols():
    W = _W()
    return (0, 8, 9, 15, 16, W - 1, W)


def _slabs_k65():
    """k = W + 1: two groups, the second with one trait.  Compared on k65_cols(): the first trait, both sides of the ninth Gram slot and of the
    first solve workgroup's end, the last trait of the first group and the trait of the second."""
    k = _W() + 1
    return _uvb(_traits(_slabs900(), k, 0.15, seed=33), _slabs900(), "D", kw=dict(maxit=3, tol=0), cols=k65_cols(), **SLABS)


def _shared(v):
    """test_gpu_uvb.test_shared_patterns_and_awkward_rows: shared patterns, four rows nobody has, one pattern observed on five rows over three
    slabs (more than 100 markers have XX = 0 for it: tests/test_uvb_tight_cpu.py asserts it).  Y is float-representable."""
    ids = (0, 1, 0, 2, 1, 3, 2, 3, 0)
    Y = _f32(_traits_ids(_slabs900(), ids, 0.2, seed=41, all_missing=(10, 200, 400, 650), sparse=(3, (5, 130, 300, 450, 690))))
    return _uvb(Y, _slabs900(), v, **SLABS)


def _tpod_p(p):
    """tpod cut to p markers.  With one marker the fit settles at once, so p = 1 runs two sweeps, as test_gpu_uvb.test_marker_count_edges."""
    return _uvb(_traits(_tpod(), 3, 0.1, seed=71), np.asfortranarray(_tpod()[:, :p]), "D", kw=dict(maxit=2 if p == 1 else 6, tol=0),
                panel="tpod_p%d" % p)


def _signed():
    X = _tpod()
    return _uvb(_traits(X, 3, 0.1, seed=81), np.asfortranarray((X.astype(np.int16) - 1).astype(np.int8)), "D", panel="tpod_signed")


def _full_range():
    rng = np.random.default_rng(91)
    X = rng.integers(-128, 128, size=(300, 200)).astype(np.int8)
    X[0, 0], X[1, 0] = -128, 127
    X = np.asfortranarray(X)
    return _uvb(_traits(X, 5, 0.1, seed=92), X, "D", panel="full_range")


def _stopping():
    return _uvb(_stopping_case("D")[0], _tpod(), "D", kw=dict(maxit=100, tol=10e-7), panel="tpod")


def _row_tiles():
    """1300 x 130 in the default slabs: several row tiles per pass workgroup."""
    X = C._genotypes(1300, 130, 61)
    return _uvb(_traits(X, 4, 0.1, seed=62), X, "Z", xb=True, panel="rows1300")


def _dense(Y, Z, variant, kw=SIX):
    return dict(entry="dense", Y=Y, Z=Z, variant=variant, kw=dict(kw))


def _dense_missing(v):
    """test_gpu_uvbd.test_missingness: a fifth of every trait missing; traits 0 and 2 share their pattern; trait 3 has no observed row."""
    Y, Z = _dense_case(300, 6, 5, seed=6, frac=0.2)
    Y[np.isnan(Y[:, 0]), 2] = np.nan
    Y[~np.isnan(Y[:, 0]) & np.isnan(Y[:, 2]), 2] = 1.0
    Y[:, 3] = np.nan
    return _dense(Y, Z, v)


def _dense_constant(v):
    """test_gpu_uvbd.test_a_column_constant_on_one_traits_rows: XX = 0 exactly for trait 1 in column 2."""
    Y, Z = _dense_case(196, 4, 3, seed=7, frac=0.2)
    Z[~np.isnan(Y[:, 1]), 2] = 1.5
    return _dense(Y, Z, v)


def _dense_lds(off):
    """lds_rows - 27 rows: e in LDS; lds_rows + 37: e in global memory."""
    return _dense(*_dense_case(_lds_rows() + off, 2, 2, seed=4), "D", kw=dict(maxit=2, tol=0))


def _uvb2(name):
    c = dict(C.engine(name), entry="uvbeta2")
    c["panel_kw"] = dict(nwg=c.pop("nwg")) if "nwg" in c else {}
    c["panel"] = "slabs900" if name == "slabs_defaults" else "tpod" if c["X"] is C.tpod() else "tpod_" + name
    return c


def _uvb2_residual(off):
    """sem2_cases.residual_path on both sides of lds_rows, with a signal on Z added to its traits: as it stands b1 is the noise of 20 000
    rows around zero, a sum that cancels by sqrt(n), and its yardstick (1.5e-13) leaves the bound on b1 only just below 1e-11."""
    c = C.residual_path(_lds_rows() + off)
    Y = c["Y"] + (c["Z"] - c["Z"].mean(0)) / c["Z"].std(0) @ np.array([[0.5, -0.3], [0.2, 0.4]])
    return dict(c, Y=Y, entry="uvbeta2", panel="residual%+d" % off, panel_kw={})


CASES = {}
for _v in "DFXZ":
    CASES["uvbeta/tpod_" + _v] = functools.partial(_tpod_variant, _v)
for _v in "DZ":
    CASES["uvbeta/slabs900_k5_" + _v] = functools.partial(_slabs_k5, _v)
CASES["uvbeta/slabs900_k17"] = _slabs_k17
CASES["uvbeta/slabs900_k65"] = _slabs_k65
for _v in "DF":
    CASES["uvbeta/shared_patterns_" + _v] = functools.partial(_shared, _v)
for _p in (1, 63, 64, 65):
    CASES["uvbeta/tpod_p%d" % _p] = functools.partial(_tpod_p, _p)
CASES["uvbeta/tpod_signed"] = _signed
CASES["uvbeta/full_range_int8"] = _full_range
CASES["uvbeta/stopping"] = _stopping
CASES["uvbeta/rows1300_Z"] = _row_tiles
for _v in "DFXZ":
    CASES["dense/n300_q5_" + _v] = functools.partial(lambda v: _dense(*_dense_case(300, 5, 3, seed=1), v), _v)
for _q in (1, 70):
    CASES["dense/q%d" % _q] = functools.partial(lambda q: _dense(*_dense_case(300, q, 3, seed=2), "D"), _q)
for _n in (63, 1023, 1025):
    CASES["dense/n%d" % _n] = functools.partial(lambda n: _dense(*_dense_case(n, 3, 2, seed=3), "Z"), _n)
for _v in "DX":
    CASES["dense/missingness_" + _v] = functools.partial(_dense_missing, _v)
CASES["dense/e_in_lds"] = functools.partial(_dense_lds, -27)
CASES["dense/e_in_global_memory"] = functools.partial(_dense_lds, 37)
for _v in "DFZ":
    CASES["dense/constant_column_" + _v] = functools.partial(_dense_constant, _v)
for _name in ("k3_q3", "q1", "q7_beyond_k", "k17_two_solve_workgroups", "p1", "p63", "p64", "p65", "one_pattern", "full_and_masked",
              "all_nan_trait", "xx1_zero", "trx1_zero", "maxit1", "slabs_defaults"):
    CASES["uvbeta2/" + _name] = functools.partial(_uvb2, _name)
CASES["uvbeta2/residual_in_lds"] = functools.partial(_uvb2_residual, -27)
CASES["uvbeta2/residual_in_global_memory"] = functools.partial(_uvb2_residual, 37)
NAMES = tuple(CASES)


@functools.lru_cache(None)
def case(name):
    c = CASES[name]()
    for key in ("Y", "Z", "X"):
        if key in c:
            c[key].setflags(write=False)
    return c
