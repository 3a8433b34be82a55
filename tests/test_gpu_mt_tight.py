"""GPU: the multi-trait fp64 fits -- mrr / mrr_float on the int8 launch train (mrr.hip.h), mrr(Y, dense(X)) and mkr on the dense train
(mrr_dense.hip.h), PEGS and PEGSZ (the int8 train uncentred, and k_pegs_dense_leg), the sparse legs (pegs_sparse.hip.h: set-up, the serial and
the disjoint column step, hat) and PEGSX (pegsx.hip.h: the fixed step, the three trace kernels, k_pegs_zb on X) -- held to what fp64 rounding
alone allows.

tests/test_gpu_mrr.py, test_gpu_mkr.py, test_gpu_pegs.py and test_gpu_tall.py assert scaled_err <= 1e-6 against the float64 restatements,
eight orders above what these kernels deliver: a float temporary in a dot, a dropped partial or a Gram entry of the wrong pattern moves b by
1e-8 or less and passes them.  Here every returned key of every case of tests/mt_tight_cases.py is compared with the long double restatement
under the bound of tests/mt_tight.py,

    kappa * max(64 * yard[key], 64 * 2**-52),    yard[key] = the largest error of nine float64 runs of the restatement, under row permutations,

which is computed from the restatements and the case's panel alone, per case and per key (kappa = 1 but for the implicitly centred int8
train; tests/test_mt_tight_cpu.py shows that the bound is finite, at most 1e-11 on b, and that a float dot lands a hundred bounds away or
further).  Its / numit must be equal; NaN and the infinities must stand in the same places; hat is also held (hat_own) against the long
double product of the returned b and mu with the design, centred for mrr and raw for PEGS (PEGSX: of b with X and of every u with its design).  Every figure is printed before anything is
asserted: case, key, error, bound, error / bound.  One Panel per shape serves the module.

A case's time is the yardstick's ten restatement runs on the host (the long double run inverts a sweep's k x k systems in one batched call);
the library's own call takes milliseconds.  Measured on the MI355X machine: 0.43 s for the slowest case (k = 6 on 700 x 132, the module's first,
after 1.5 s of set-up for the first Panel), 0.34 s for the next (k = 16, ten shared patterns), under 0.3 s for the rest, 9.3 s for the module's
49 cases; none of them is among the 25 slowest tests of the GPU suite.  The 31 cases of PEGSX and the sparse legs, same machine: 1.39 s for
pegsx/f70_k5_inflated (five long double Jacobis of a 70 x 70 M'M; 2.2 s on an eight-core host), 1.16 s for
sparse/ps_q4133 (two sweeps over 4 133 columns in numpy, ten times; 2.3 s on that host), 0.42 s for pegsx/f1 and 0.32 s for pegsx/k16_shared,
0.16 s or less for each of the others (at most 0.5 s on that host), 7.6 s for the 31 together.  The measured errors are in DESIGN.md sections
4.5, 4.10 to 4.13: no key of any case is above 0.040 of its bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mt_tight as T  # noqa: E402
import mt_tight_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def panel():
    """(name, X, kwargs) -> the Panel of that shape, made once for this module and closed after its last test."""
    import bwgr_amd
    live = bwgr_amd.debug_live()
    made = {}

    def get(name, X, kw):
        if name not in made:
            made[name] = (bwgr_amd.Panel(X, **kw), X, dict(kw))
        P, X0, kw0 = made[name]
        assert (X0 is X or np.array_equal(X0, X)) and kw0 == dict(kw), name
        if "nwg" in kw:
            assert P.nwg == kw["nwg"]
        return P

    yield get
    for P, _, _ in made.values():
        P.close()
    assert bwgr_amd.debug_live() == live


def _effect(e, panel, serial):
    """an effect of a case as the library takes it: the module's Panel of that shape, dense(Z), or sparse(...) from the column-compressed
    arrays of the stored entries (serial=True: on the one-wave leg whatever its rows)"""
    import bwgr_amd
    if e[0] == "panel":
        return panel(e[3], e[1], e[2])
    if e[0] == "dense":
        return bwgr_amd.dense(e[1])
    return bwgr_amd.sparse(T.SR.csc(e[1], e[2] if len(e) > 2 else None), shape=e[1].shape, serial=serial)


def _library(c, panel):
    import bwgr_amd
    if c["family"] == "mrr":
        fit = bwgr_amd.mrr_float if c["variant"] == "F" else bwgr_amd.mrr
        return fit(c["Y"], panel(c["panel"], c["X"], c["panel_kw"]), **c["kw"])
    if c["family"] == "dense":
        if "K" in c:
            assert np.array_equal(bwgr_amd.K2X(c["K"]), c["X"])
            return bwgr_amd.mkr(c["Y"], c["K"], **c["kw"])
        if c.get("device"):
            import torch
            Xd = torch.tensor(c["X"], device="cuda")
            assert Xd.is_cuda and Xd.dtype == torch.float64
            g = bwgr_amd.mrr(c["Y"], bwgr_amd.dense(Xd), **c["kw"])
            assert np.array_equal(Xd.cpu().numpy(), c["X"])
            return g
        return bwgr_amd.mrr(c["Y"], bwgr_amd.dense(c["X"]), **c["kw"])
    effs = [_effect(e, panel, c.get("serial", False)) for e in c["effects"]]
    if c["family"] == "pegsx":
        return bwgr_amd.PEGSX(c["Y"], c["X"], effs, cnv_trace=True, **c["kw"])
    if c["entry"] in ("PEGS", "PEGS_sparse"):
        return getattr(bwgr_amd, c["entry"])(c["Y"], effs[0], cnv_trace=True, **c["kw"])
    return getattr(bwgr_amd, c["entry"])(c["Y"], effs, cnv_trace=True, **c["kw"])


@pytest.mark.parametrize("name", TC.NAMES)
def test_within_the_bound_of_fp64_rounding(name, panel):
    c = TC.case(name)
    o, bound = T.ref(name), T.bound(name)
    g = T.flat(c, _library(c, panel))
    assert g["hat"].shape == o["hat"].shape and all(np.asarray(g[key]).shape == np.asarray(o[key]).shape for key in T.b_keys(c))
    errs = T.errs(name, g, o)
    for key in T.keys(c):
        print("%s %s err %.3e bound %.3e ratio %.4f" % (name, key, errs[key], bound[key], errs[key] / bound[key]))
    over = {key: (errs[key], bound[key]) for key in T.keys(c) if not errs[key] <= bound[key]}
    assert not over, over
