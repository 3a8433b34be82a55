"""GPU: the per-trait fp64 fits (bwgr_uvbeta in its four variants, bwgr_uvbeta_dense, bwgr_uvbeta2) held to what fp64 rounding alone allows.

tests/test_gpu_uvb.py, test_gpu_uvbd.py and test_gpu_sem2.py assert scaled_err <= 1e-6 against the float64 restatements, eight orders above
what these kernels deliver: a float temporary in a dot, or a dropped partial, moves b by about 1e-8 and passes them.  Here every returned key
of every case of tests/uvb_tight_cases.py is compared with the long double restatement under the bound of tests/uvb_tight.py,

    max(64 * yard[key], 64 * 2**-52),    yard[key] = the largest error of nine float64 runs of the restatement, under row permutations,

which is computed from the restatements alone, per case and per key (1e-14 to 2e-13 on b; tests/test_uvb_tight_cpu.py shows that it is
finite, below 1e-11 on b, and that a float dot lands a hundred bounds away or further).  its must be equal, NaN must stand in the same
places; xb, where a case asks for it, is held against the long double product X b of the returned b.  Every figure is printed before it is
asserted: case, key, error, bound, error / bound.  One Panel per shape serves the module.

A case's time is the yardstick's ten restatement runs on the host; the library's own call takes milliseconds.  Measured with the suite on the
MI355X machine: 4.3 s for the slowest case (k = 17 on 700 x 900, all 17 traits compared: nine Gram matrices in LDS slots, seven in global
memory, one in the second workgroup), 2.4 s for the next, under 2 s for the rest, 22 s for the module.  The measured errors are in DESIGN.md
sections 4.7 to 4.9."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uvb_tight as T  # noqa: E402
import uvb_tight_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def panel():
    """case -> the Panel of its shape, made once for this module and closed after its last test."""
    import bwgr_amd
    live = bwgr_amd.debug_live()
    made = {}

    def get(c):
        if c["panel"] not in made:
            made[c["panel"]] = (bwgr_amd.Panel(c["X"], **c.get("panel_kw", {})), c["X"])
        P, X = made[c["panel"]]
        assert X is c["X"] or np.array_equal(X, c["X"]), c["panel"]
        if "nwg" in c.get("panel_kw", {}):
            assert P.nwg == c["panel_kw"]["nwg"]
        return P

    yield get
    for P, _ in made.values():
        P.close()
    assert bwgr_amd.debug_live() == live


def _library(c, panel):
    import bwgr_amd
    if c["entry"] == "dense":
        g = bwgr_amd.uvbeta_dense(c["Y"], c["Z"], c["variant"], **c["kw"])
    elif c["entry"] == "uvbeta2":
        g = bwgr_amd.uvbeta2(c["Y"], c["Z"], panel(c), **c["kw"])
    else:
        g = bwgr_amd.uvbeta(c["Y"], panel(c), c["variant"], xb=bool(c.get("xb")), **c["kw"])
    k = c["Y"].shape[1]
    assert all(np.asarray(g[key]).shape[-1] == k for key in T.keys(c) + ("its",))
    if c.get("cols") is not None:
        g = {key: np.asarray(v)[..., list(c["cols"])] for key, v in g.items()}
    return g


@pytest.mark.parametrize("name", TC.NAMES)
def test_within_the_bound_of_fp64_rounding(name, panel):
    c = TC.case(name)
    o, bound = T.ref(name), T.bound(name)
    g = _library(c, panel)
    errs = T.errs(c, g, o)
    for key in T.keys(c):
        print("%s %s err %.3e bound %.3e ratio %.4f" % (name, key, errs[key], bound[key], errs[key] / bound[key]))
    over = {key: (errs[key], bound[key]) for key in T.keys(c) if not errs[key] <= bound[key]}
    assert not over, over
