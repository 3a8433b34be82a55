"""CPU: the yardstick of tests/test_gpu_uvb_tight.py (tests/uvb_tight.py) on every case of tests/uvb_tight_cases.py: it is finite, it puts the
bound on the coefficients at least five orders below the suite's 1e-6, and it bites: the restatement with one float temporary in the step's
dependent dot e'x_J -- what a float partial sum in a kernel's dot does -- lands at least a hundred bounds away.  The cases' own preconditions
(the patterns, the exact zeros, no cnv near log10(tol)) are asserted here too, on the long double and on the float64 runs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uvb_tight as T  # noqa: E402
import uvb_tight_cases as TC  # noqa: E402

B_BOUND = 1e-11     # the bound on b must not exceed this: a condition on the inputs
BITE = 100          # the mutant moves b by at least this many bounds


def _float_dot(e, x):
    """The mutant: the dependent dot through a float."""
    return np.float64(np.float32(e @ x))


# entry -> (the restatement's argument that takes the mutant, the coefficients it must move), once per leg
LEGS = {"uvbeta": (("dot", "b"),), "dense": (("dot", "b"),), "uvbeta2": (("dot1", "b1"), ("dot2", "b2"))}


@pytest.mark.parametrize("name", TC.NAMES)
def test_yardstick_is_finite_tight_and_bites(name):
    c = TC.case(name)
    o, yard, bound = T.ref(name), T.yard(name), T.bound(name)
    assert o["b1" if c["entry"] == "uvbeta2" else "b"].dtype == T.LD
    print(name, {key: "%.1e" % v for key, v in yard.items()})
    for key in T.keys(c):
        assert np.isfinite(yard[key]) and np.isfinite(bound[key]) and bound[key] >= T.FLOOR, (key, yard[key])
    for arg, key in LEGS[c["entry"]]:
        assert bound[key] <= B_BOUND, (key, bound[key])
        moved = T.errs(c, T.run(c, **{arg: _float_dot}), o)[key]
        print(name, arg, key, "mutant %.2e, bound %.2e, ratio %.0f" % (moved, bound[key], moved / bound[key]))
        assert moved >= BITE * bound[key], (key, moved, bound[key])


def test_a_long_double_run_leaves_nothing_in_float64():
    for name in ("uvbeta/tpod_F", "uvbeta/slabs900_k5_Z", "dense/n300_q5_X", "uvbeta2/k3_q3", "uvbeta2/trx1_zero"):
        o = T.ref(name)
        for key in T.keys(TC.case(name)) + (("XX",) if "XX" in o else ()):
            assert np.asarray(o[key]).dtype == T.LD, (name, key)
        for tr in o["trace"]:
            assert all(isinstance(v, T.LD) for v in tr), name
        assert np.asarray(o["its"]).dtype == np.int32
    # ... nor on the way: the start values and every sweep's sums and updates, as the restatements record them
    c = TC.case("uvbeta2/k3_q3")
    w = ~np.isnan(c["Y"][:, 0])
    rec1, rec2 = {}, {}
    T.UR.solver(c["Y"][w, 0], c["X"][w], "F", maxit=3, record=rec1, dtype=T.LD)
    T.S2.solver2x(c["Y"][w, 0], c["Z"][w], c["X"][w], maxit=3, record=rec2, dtype=T.LD)
    for rec in (rec1, rec2):
        assert len(rec["sweeps"]) == 3
        for d in [rec] + rec["sweeps"]:
            for key, v in d.items():
                assert isinstance(v, (T.LD, int, bool, np.bool_, list)), (key, type(v))


def test_case_preconditions():
    W = TC._W()
    assert TC.k65_cols() == (0, 8, 9, 15, 16, 63, 64) and W == 64
    c = TC.case("uvbeta/slabs900_k65")
    assert c["Y"].shape == (700, W + 1) and len({np.isnan(c["Y"][:, t]).tobytes() for t in range(W + 1)}) == W + 1
    c = TC.case("uvbeta/slabs900_k5_D")
    assert not np.isnan(c["Y"][:, 1]).any() and len({np.isnan(c["Y"][:, t]).tobytes() for t in range(5)}) == 5
    for v in "DF":
        c, o = TC.case("uvbeta/shared_patterns_" + v), T.ref("uvbeta/shared_patterns_" + v)
        assert np.isnan(c["Y"][[10, 200, 400, 650]]).all() and np.sum(~np.isnan(c["Y"][:, 5])) == 5
        assert len({np.isnan(c["Y"][:, t]).tobytes() for t in range(9)}) == 4
        assert np.sum(o["XX"][:, 5] == 0) > 100
    c = TC.case("uvbeta/tpod_signed")
    assert c["X"].min() == -1 and c["X"].max() == 1
    c = TC.case("uvbeta/full_range_int8")
    assert c["X"].min() == -128 and c["X"].max() == 127 and c["X"].shape == (300, 200)
    # the stopping cases: no cnv of any sweep within 0.02 of log10(tol), in the long double run and in the float64 run on the rows as given
    # (the permuted float64 runs are held to the long double run's its by uvb_tight.errs), and the traits stop at different sweeps
    for name, counts in (("uvbeta/stopping", None), ("uvbeta2/slabs_defaults", 4)):
        for o in (T.ref(name), T.run(TC.case(name))):
            near = min(abs(float(v) - np.log10(10e-7)) for tr in o["trace"] for v in tr)
            assert near >= 0.02 and o["its"].max() < 100, (name, near, o["its"])
            assert len(set(o["its"])) == counts if counts else len(set(o["its"])) > 1, (name, o["its"])
    for v in "DFZ":
        o = T.ref("dense/constant_column_" + v)
        assert o["XX"][2, 1] == 0 and o["XX"][2, 0] > 1 and o["XX"][2, 2] > 1 and o["b"][2, 1] == 0
    o = T.ref("dense/missingness_D")
    assert list(o["its"]) == [6, 6, 6, 0, 6]
    assert TC.case("dense/e_in_lds")["Y"].shape[0] == TC._lds_rows() - 27 and TC.case("dense/e_in_global_memory")["Y"].shape[0] == TC._lds_rows() + 37
    o = T.ref("uvbeta2/xx1_zero")
    assert o["b1"][1, 0] == 0 and o["b1"][1, 1] != 0
    o = T.ref("uvbeta2/trx1_zero")
    assert not o["b1"][:, 1].any() and np.isnan(o["vb1"][1])
