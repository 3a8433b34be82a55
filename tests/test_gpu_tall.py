"""GPU: the fp64 families -- uvbeta, mrr, panel_xb, the relationship kernels, XSEMF / ZSEMF / YSEMF, uvbeta2, MEGA / GSEM, PEGS / PEGSZ / PEGSX -- against their float64 restatements on
the shapes of tests/tall_cases.py: tall panels on which the tail reductions and the passes take a second and a third trip, slabs of 1 280
and 1 024 rows (and one slab of 1 152: kern1100s, where the slab base is always 0), row tiles of panel_xb across slabs, wide panels on which the marker reductions take a second trip.
tests/test_tall_cases_cpu.py proves without a GPU that each shape reaches what it is listed for.

The bounds are the project's: mrr_restatement.scaled_err <= 1e-6 for the fits and the kernels (NaN in the same places, equal sweep counts),
1e-12 for the products (exact integers times doubles, fp64 sums), bit equality for X X' and between calls.  One Panel per shape serves the
whole module; test_state_between_calls_tall checks that sharing it hides nothing.

PEGS, PEGSZ and PEGSX run the jobs of tall_cases.PEGS_JOBS: the trace kernels past one grid (wide33k, dense q = 16 500 and 16 501), the
uncentred launch train where the reductions take further trips and on the other slab heights, a dense effect beside a panel that pads
further than it would alone (tall9k, in both orders), row loops of nine and five trips at 1 024 threads, f = 17 and f = 256.
Largest scaled error measured over these jobs on an MI355X: 9.9e-14 (`bend` of PEGSX on tall9k; 9.5e-14 on `vb_list` at f = 256, 5.6e-14 on
`bend` of PEGS and PEGSZ on wide33k), at most 3.5e-14 on every other figure; TrZSZ alone at most 3.5e-14 (f = 256); the normal equations
5.8e-17 and 2.0e-17 of ||M_t|| ||y_t|| (bar 1e-9).

tall9k_sparse and slab1280_sparse put sparse effects beside those panels (ld 216 and 120 rows past n, R = 256 and 1 280, a level of more
than 4 096 rows across slab edges, 36 and 20 workgroups of k_pegs_sparse_hat), under PEGSZ, PEGSX and, on slab1280, PEGSZ_sparse's text.
Measured: 3.5e-13 (`b` of PEGSZ on tall9k_sparse), 1.2e-13 and 1.1e-13 (`vb_list` and `bend` of PEGSX there), at most 6.4e-14 on every other
figure; the normal equations 5.3e-17 and 3.9e-17."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernels_restatement as KR  # noqa: E402
import mrr_restatement as MR  # noqa: E402
import pegs_cases as PC  # noqa: E402
import pegsx_cases as XC  # noqa: E402
import pegsx_restatement as XR  # noqa: E402
import sem_restatement as SR  # noqa: E402
import tall_cases as tc  # noqa: E402
import uvb_restatement as UR  # noqa: E402
from test_gpu_drivers import _raw_panel  # noqa: E402
from test_gpu_mrr import _check as _mrr_check, _traits  # noqa: E402
from test_gpu_pegs import _errs as _pegs_errs  # noqa: E402
from test_gpu_pegsx import _errs as _pegsx_errs, _normal_equations  # noqa: E402
from test_gpu_sem import _check as _sem_check, _strong, _well_posed  # noqa: E402
from test_gpu_sem2 import _check as _uvb2_check, _check_driver  # noqa: E402
from test_gpu_uvb import _check, _f32, _ref, _W  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6
X_I8, DEVICE = 0, 1


@pytest.fixture(scope="module")
def panel():
    """tag -> the shape's Panel, made once for this module and closed after its last test."""
    import bwgr_amd
    live = bwgr_amd.debug_live()
    made = {}

    def get(tag):
        if tag not in made:
            made[tag] = bwgr_amd.Panel(tc.data(tag), **tc.panel_kw(tag))
            pl = tc.plans(tag)
            assert (made[tag].ld, made[tag].slab_rows) == (pl["ld"], pl["R"]), tag
        return made[tag]

    yield get
    for P in made.values():
        P.close()
    assert bwgr_amd.debug_live() == live


# ---- uvbeta ----
# rows missing in every trait: in the first and the last slab, on both sides of a slab boundary, and (tall9k) beyond k_uvb_rows' first trip
ALL_MISSING = tc.ALL_MISSING
UVB_MAXIT = {"tall9k": 4, "slab1280": 6, "slab1024": 5}
UVB_JOBS = [("tall9k", v) for v in "DZFX"] + [(t, v) for t in ("slab1280", "slab1024") for v in "DZ"]


@functools.lru_cache(None)
def _uvb_traits(tag):
    """five traits: four missingness patterns and one complete trait (but for the four rows nobody has)"""
    Y = _traits(tc.data(tag), 5, 0, seed=tc.CASES[tag]["seed"] + 50, patterns=[0.1, 0.0, 0.25, 0.05, 0.4])
    Y[list(ALL_MISSING[tag])] = np.nan
    assert np.sum(np.isnan(Y[:, 1])) == 4 and len({np.isnan(Y[:, t]).tobytes() for t in range(5)}) == 5
    Y.setflags(write=False)
    return Y


@functools.lru_cache(None)
def _uvb_ref(tag, variant):
    return _ref(_uvb_traits(tag), tc.data(tag), variant, maxit=UVB_MAXIT[tag], tol=0)


@pytest.mark.parametrize("tag,variant", UVB_JOBS, ids=["%s-%s" % j for j in UVB_JOBS])
def test_uvbeta(panel, tag, variant):
    import bwgr_amd
    X, Y = tc.data(tag), _uvb_traits(tag)
    g = bwgr_amd.uvbeta(Y, panel(tag), variant, maxit=UVB_MAXIT[tag], tol=0, xb=True)
    print(tag, variant, end=" ")
    _check(g, _uvb_ref(tag, variant))
    assert list(g["its"]) == [UVB_MAXIT[tag]] * 5
    err = MR.scaled_err(g["xb"], X.astype(np.float64) @ g["b"])
    print("xb", err)
    assert g["xb"].shape == Y.shape and err <= 1e-12


def test_uvbeta_two_groups_on_tall_slabs(panel):
    """k = W + 1 on the 1 280-row slabs: a full group and a group of one trait, every trait its own pattern."""
    import bwgr_amd
    tag, k = "slab1280", _W() + 1
    X = tc.data(tag)
    Y = _traits(X, k, 0.15, seed=2961)
    assert len({np.isnan(Y[:, t]).tobytes() for t in range(k)}) == k
    g = bwgr_amd.uvbeta(Y, panel(tag), "D", maxit=4, tol=0, xb=True)
    _check(g, UR.uvbeta(Y, X, "D", maxit=4, tol=0))
    assert MR.scaled_err(g["xb"], X.astype(np.float64) @ g["b"]) <= 1e-12


# ---- mrr / MRR3 ----
MRR_JOBS = {"tall16k": dict(k=4, maxit=3), "slab1280": dict(k=3, maxit=4), "wide33k": dict(k=3, maxit=2)}


@functools.lru_cache(None)
def _mrr_traits(tag):
    k = MRR_JOBS[tag]["k"]
    Y = _traits(tc.data(tag), k, 0, seed=tc.CASES[tag]["seed"] + 60, patterns=[0.1, 0.0, 0.25, 0.05][:k])
    assert len({np.isnan(Y[:, t]).tobytes() for t in range(k)}) == k
    Y.setflags(write=False)
    return Y


@pytest.mark.parametrize("tag", list(MRR_JOBS))
def test_mrr(panel, tag):
    import bwgr_amd
    X, Y, maxit = tc.data(tag), _mrr_traits(tag), MRR_JOBS[tag]["maxit"]
    g = bwgr_amd.MRR3(Y, panel(tag), maxit=maxit, tol=0)
    errs = _mrr_check(g, MR.mrr(Y, X, maxit=maxit, tol=0))
    print(tag, errs)
    assert g["Its"] == maxit and g["hat"].shape == Y.shape and np.all(np.isfinite(g["hat"]))


def test_mrr_float_on_tall_slabs(panel):
    import bwgr_amd
    tag = "slab1280"
    X, Y = tc.data(tag), _mrr_traits(tag)
    g = bwgr_amd.mrr_float(Y, panel(tag), maxit=4, tol=0)
    print(_mrr_check(g, MR.mrr(_f32(Y), X, maxit=4, tol=0)))


# ---- panel_xb ----
XB_TAGS = ["tall9k", "slab1280", "slab1024", "xbwide"]


@pytest.mark.parametrize("k", [1, 17])
@pytest.mark.parametrize("tag", XB_TAGS)
def test_xb(panel, tag, k):
    X = tc.data(tag)
    B = np.random.default_rng(k + tc.CASES[tag]["seed"]).normal(size=(X.shape[1], k))
    P = panel(tag)
    a, b = P.xb(B), P.xb(B)
    err = MR.scaled_err(a, X.astype(np.float64) @ B)
    print(tag, k, err)
    assert a.shape == (X.shape[0], k) and err <= 1e-12
    assert np.array_equal(a, b)


def test_xb_signed_codes_on_tall_slabs():
    """codes -2 .. 2 on the 5 000 x 200 shape in 1 280-row slabs: the sign of a byte survives every row tile"""
    import bwgr_amd
    c = tc.CASES["slab1280"]
    rng = np.random.default_rng(2971)
    X = np.asfortranarray(rng.integers(-2, 3, size=(c["n"], c["p"])).astype(np.int8))
    B = rng.normal(size=(c["p"], 17))
    P = bwgr_amd.Panel(X, block=c["block"])
    try:
        assert P.slab_rows == 1280
        a, b = P.xb(B), P.xb(B)
    finally:
        P.close()
    assert MR.scaled_err(a, X.astype(np.float64) @ B) <= 1e-12 and np.array_equal(a, b)


@pytest.mark.parametrize("tag", ["tall9k", "slab1280"])
def test_xb_on_a_device_resident_padded_matrix(panel, tag):
    """The panel made from a (p, ldx) device matrix with ldx > n, its padding filled with a code that must never be read."""
    import torch
    X = tc.data(tag)
    n, p = X.shape
    ldx = n + 36
    Xd = torch.full((p, ldx), 2, dtype=torch.int8, device="cuda")
    Xd[:, :n] = torch.from_numpy(np.array(X.T, order="C")).cuda()
    torch.cuda.synchronize()
    B = np.random.default_rng(2972).normal(size=(p, 17))
    P = _raw_panel(C.c_void_p(Xd.data_ptr()), X_I8, DEVICE, n, p, ldx, block=tc.CASES[tag]["block"])
    try:
        assert (P.n, P.ld, P.slab_rows) == (n, panel(tag).ld, panel(tag).slab_rows)
        a = P.xb(B)
    finally:
        P.close()
    assert MR.scaled_err(a, X.astype(np.float64) @ B) <= 1e-12
    assert np.array_equal(a, panel(tag).xb(B))


# ---- the relationship kernels ----
KERN_TAGS = ["kern1100", "kern1100s", "slab1024"]
KERN_JOBS = [("kern1100", kind, kw) for kind, kw in KR.KINDS] + \
    [(tag, kind, kw) for tag in ("kern1100s", "slab1024") for kind, kw in (("GRM", {"Code012": False}), ("EigenGAU", {"phi": 1.0}))]


@functools.lru_cache(None)
def _crossprod_ref(tag):
    if tag == "kern1100s":
        return _crossprod_ref("kern1100")
    G = KR.crossprod(tc.data(tag))
    G.setflags(write=False)
    return G


@pytest.mark.parametrize("tag", KERN_TAGS)
def test_crossprod(panel, tag):
    """bit-equal to the int64 product, twice, on the device, and into a host array with ldg = n + 5 whose padding stays as it was"""
    from bwgr_amd import _lib
    P, ref = panel(tag), _crossprod_ref(tag)
    n = P.n
    G = P.crossprod()
    assert G.dtype == np.int64 and np.array_equal(G, ref), "max |diff| = %d" % np.abs(G - ref).max()
    assert np.array_equal(P.crossprod(), G)
    assert np.array_equal(P.crossprod(device_out=True).cpu().numpy(), G)
    Gp = np.full((n, n + 5), -9, np.int64)
    assert _lib.lib().bwgr_panel_crossprod(P._h, Gp.ctypes.data_as(C.c_void_p), n + 5, 0) == 0
    assert np.array_equal(Gp[:, n:], np.full((n, 5), -9)) and np.array_equal(Gp[:, :n], ref)


def test_crossprod_and_kernel_in_forced_chunks(panel, monkeypatch):
    """Three chunks of markers add into the zeroed n x n array: k_xxt_zero runs, and 1 100^2 entries are more than its grid covers in two
    trips.  Integer sums: the same bits as the one-chunk product, in G and in a kernel made from it."""
    import bwgr_amd
    tag = "kern1100"
    pl = tc.plans(tag)
    assert pl["forced_chunks"] == 3 and pl["xxt_zero"] == 3
    monkeypatch.setenv("BWGR_KCHUNK", str(pl["kchunk"]))     # read when the root panel is made
    P = bwgr_amd.Panel(tc.data(tag))
    # (a device array of the caller's that holds -9 everywhere beforehand: an entry that is added to without having been zeroed shows there,
    # whatever a fresh allocation of the library's own happens to hold)
    import torch
    from bwgr_amd import _lib
    Gd = torch.full((P.n, P.n), -9, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        G, K = P.crossprod(), P.kernel("GRM")
        assert _lib.lib().bwgr_panel_crossprod(P._h, C.c_void_p(Gd.data_ptr()), P.n, DEVICE) == 0
    finally:
        P.close()
    assert np.array_equal(G, _crossprod_ref(tag)) and np.array_equal(Gd.cpu().numpy(), G)
    assert np.array_equal(K, panel(tag).kernel("GRM"))


@pytest.mark.parametrize("tag,kind,kw", KERN_JOBS, ids=["%s-%s-%s" % (t, k, "-".join("%s" % v for v in kw.values())) for t, k, kw in KERN_JOBS])
def test_kernel(panel, tag, kind, kw):
    import bwgr_amd
    from bwgr_amd import api
    from bwgr_amd import _lib
    P = panel(tag)
    n = P.n
    K = getattr(bwgr_amd, kind)(P, **kw)
    K2 = getattr(bwgr_amd, kind)(P, **kw)
    Kd = getattr(bwgr_amd, kind)(P, device_out=True, **kw)
    ref = KR.restate(kind, np.ascontiguousarray(tc.data(tag)), **kw)
    err = MR.scaled_err(K, ref)
    print("%s %s %s: scaled_err = %.3e" % (tag, kind, kw, err))
    assert K.dtype == np.float64 and K.shape == ref.shape and np.all(np.isfinite(K))
    assert err <= TOL, err
    assert np.array_equal(K, K.T)
    assert np.array_equal(K, K2)
    assert np.array_equal(Kd.cpu().numpy(), K)
    # ldk = n + 5: the padding is left as it was
    par = float(kw.get("phi", 1.0))
    flag = int(bool(next(iter(kw.values())))) if kw and "phi" not in kw else 0
    Kp = np.full((n, n + 5), -7.25)
    assert _lib.lib().bwgr_panel_kernel(P._h, api.KERNELS[kind], par, flag, Kp.ctypes.data_as(C.c_void_p), n + 5, 0) == 0
    assert np.array_equal(Kp[:, n:], np.full((n, 5), -7.25)) and np.array_equal(Kp[:, :n], K)


# ---- XSEMF / ZSEMF / YSEMF ----
SEM_SEED = {"slab1280": 2981, "tall9k": 2991}


@functools.lru_cache(None)
def _sem_traits(tag):
    Y = _strong(tc.data(tag), 3, seed=SEM_SEED[tag])
    Y.setflags(write=False)
    return Y


@pytest.mark.parametrize("name", ["XSEMF", "ZSEMF", "YSEMF"])
def test_sem_on_tall_slabs(panel, name):
    """5 000 x 200 in 1 280-row slabs, k = 3, six sweeps per stage.  The trait seed was picked on the CPU, the first tried: the smallest gap
    between neighbouring singular values of G is 0.246 of the largest for XSEMF and 0.271 for ZSEMF and YSEMF (the precondition asks 0.05)."""
    import bwgr_amd
    tag = "slab1280"
    X, Y = tc.data(tag), _sem_traits(tag)
    o = getattr(SR, name)(Y, X, 0, maxit=6, tol=0)
    print(name, "gap", _well_posed(o))
    g = getattr(bwgr_amd, name)(Y, panel(tag), 0, maxit=6, tol=0)
    _sem_check(name, g, o)


@pytest.mark.parametrize("name", ["XSEMF", "ZSEMF", "YSEMF"])
def test_sem_with_the_references_defaults_on_a_tall_panel(panel, name):
    """9 000 x 200, maxit = 100, tol = 10e-7: every stage stops by its own test (after 2 to 6 sweeps), and no trait's cnv comes nearer than 0.02
    to log10(tol) at any sweep of any stage of the restatement (asserted; the nearest is 0.091 for XSEMF and 0.051 for ZSEMF and YSEMF), so the
    sweep counts agree.  The trait seed was picked on the CPU, the first tried; the gaps of G's singular values are 0.216 and 0.237."""
    import bwgr_amd
    tag = "tall9k"
    X, Y = tc.data(tag), _sem_traits(tag)
    o = getattr(SR, name)(Y, X)
    _well_posed(o)
    stages = [o["BETA"], o["second"]] + ([o["third"]] if name == "YSEMF" else [])
    logtol = np.log10(float(np.float32(10e-7)))
    near = min(abs(c - logtol) for d in stages for tr in d["trace"] for c in tr)
    print(name, [list(d["its"]) for d in stages], near)
    assert near >= 0.02 and all(d["its"].max() < 100 for d in stages) and o["npc"] == 3
    g = getattr(bwgr_amd, name)(Y, panel(tag))
    _sem_check(name, g, o)


# ---- uvbeta2 / MEGA / GSEM ----
UVB2_JOBS = [("tall9k", 3), ("slab1280", 3), ("slab1280", 65)]


@pytest.mark.parametrize("tag,k", UVB2_JOBS, ids=["%s-k%d" % j for j in UVB2_JOBS])
def test_uvbeta2(panel, tag, k):
    """solver2x per trait, q = 3, 10 % missing, six sweeps: tall9k (three tiles per pass workgroup, a second trip of k_uvb_rows, 216 padding
    rows) and slab1280 (slabs of 1 280 rows, 120 padding rows); k = 65 there is two groups of traits, the dense leg launched per group
    against rows of E that lie ld apart."""
    import bwgr_amd
    c = tc.uvb2_case(tag, k)
    g = bwgr_amd.uvbeta2(c["Y"], c["Z"], panel(tag), **c["kw"])
    _uvb2_check(g, tc.uvb2_ref(tag, k), "%s k=%d" % (tag, k))
    assert g["b1"].shape == (3, k) and g["b2"].shape == (tc.CASES[tag]["p"], k) and list(g["its"]) == [6] * k


@pytest.mark.parametrize("name", ["MEGA", "GSEM"])
def test_two_design_drivers_on_tall_slabs(panel, name):
    """5 000 x 200 in 1 280-row slabs, three traits, six sweeps per stage: three (MEGA) or two panel fits, panel_xb and uvbeta2 chained on one
    panel.  tests/test_tall_cases_cpu.py asserts the preconditions on the restatement (finite, singular values apart)."""
    import bwgr_amd
    tag = "slab1280"
    g = getattr(bwgr_amd, name)(tc.driver_traits(tag), panel(tag), **tc.SEM2_DRIVERS[tag]["kw"])
    _check_driver(name, g, tc.driver_ref(name, tag))


@pytest.mark.parametrize("name", ["MEGA", "GSEM"])
def test_two_design_drivers_with_the_references_defaults_on_a_tall_panel(panel, name):
    """9 000 x 200, maxit = 100, tol = 10e-7: every stage stops by its own test after 2 to 6 sweeps and no cnv of the restatement comes nearer
    than 0.02 to log10(tol) (tests/test_tall_cases_cpu.py asserts it; the nearest is 0.112), so the sweep counts agree.  The panel that was
    passed in stays usable."""
    import bwgr_amd
    tag = "tall9k"
    X, P = tc.data(tag), panel(tag)
    g = getattr(bwgr_amd, name)(tc.driver_traits(tag), P)
    _check_driver(name, g, tc.driver_ref(name, tag))
    again = P.xb(g["b"])
    assert MR.scaled_err(again, X.astype(np.float64) @ g["b"]) <= 1e-12
    if name == "MEGA":
        assert MR.scaled_err(again + g["mu"], g["gebv"]) <= 1e-12


# ---- PEGS / PEGSZ / PEGSX ----
class _Effects:
    """a job's effects as the entries take them: the module's shared Panel where the job's shape is on the table, a Panel of its own (closed
    on exit) for the 700 x 900 three-slab panel, dense(Z) for a dense effect, sparse(S) in CSC for a sparse one"""

    def __init__(self, panel, case, effects):
        import bwgr_amd
        tag = tc.PEGS_JOBS[case["job"]]["tag"]
        self.own, self.effs = [], []
        for e in effects:
            if e[0] != "panel":
                self.effs.extend(tc.gpu_effects([e], []))
            elif tag in tc.CASES:
                self.effs.append(panel(tag))
            else:
                self.own.append(bwgr_amd.Panel(e[1], **e[2]))
                self.effs.append(self.own[-1])

    def __enter__(self):
        return self.effs

    def __exit__(self, *exc):
        for P in self.own:
            P.close()


def _pegs_job(panel, entry, job):
    import bwgr_amd
    case = tc.pegs_case(entry, job)
    Y, effects, o = PC.restate(case)
    with _Effects(panel, case, effects) as effs:
        g = bwgr_amd.PEGS(Y, effs[0], **case["kw"]) if entry == "PEGS" else getattr(bwgr_amd, entry)(Y, effs, **case["kw"])
    errs = _pegs_errs(g, o, "PEGS" if entry == "PEGS" else "PEGSZ")
    print(entry, job, "numit", g["numit"], {k: "%.2e" % v for k, v in errs.items()}, "largest %.2e" % max(errs.values()))
    assert g["numit"] == o["numit"] == case["kw"]["maxit"]
    assert all(v <= TOL for v in errs.values()), errs
    assert g["hat"].shape == Y.shape and np.all(np.isfinite(g["hat"]))      # a row for every individual, missing records included
    bs = [g["b"]] if entry == "PEGS" else g["b"]
    assert [b.shape for b in bs] == [(e[1].shape[1], Y.shape[1]) for e in effects]


@pytest.mark.parametrize("job", tc.pegs_jobs("PEGS"))
def test_pegs(panel, job):
    _pegs_job(panel, "PEGS", job)


@pytest.mark.parametrize("job", tc.pegs_jobs("PEGSZ"))
def test_pegsz(panel, job):
    _pegs_job(panel, "PEGSZ", job)


@pytest.mark.parametrize("job", tc.pegs_jobs("PEGSZ_sparse"))
def test_pegsz_sparse(panel, job):
    """text 2 beside a panel: the intercept step of PEGSZ_sparse on a residual of the panel's stride"""
    _pegs_job(panel, "PEGSZ_sparse", job)


@pytest.mark.parametrize("job", tc.pegs_jobs("PEGSX"))
def test_pegsx(panel, job):
    """the fit against the restatement; on NORMAL_EQUATIONS also M_t'(Y - hat)_t = 0, which does not depend on the restatement"""
    import bwgr_amd
    case = tc.pegs_case("PEGSX", job)
    Y, X, effects, o = XC.restate(case)
    with _Effects(panel, case, effects) as effs:
        g = bwgr_amd.PEGSX(Y, X, effs, **case["kw"])
    errs = _pegsx_errs(g, o)
    print("PEGSX", job, "its", g["its"], {k: "%.2e" % v for k, v in errs.items()}, "largest %.2e" % max(errs.values()))
    assert g["its"] == o["its"] == case["kw"]["maxit"]
    assert all(v <= TOL for v in errs.values()), errs
    assert g["hat"].shape == Y.shape and np.all(np.isfinite(g["hat"]))
    assert g["b"].shape == (X.shape[1], Y.shape[1]) and [u.shape for u in g["u"]] == [(e[1].shape[1], Y.shape[1]) for e in effects]
    if job in tc.NORMAL_EQUATIONS:
        worst = _normal_equations(Y, X, g["hat"])
        print("PEGSX", job, "normal equations %.2e" % worst)
        assert worst <= 1e-9


@pytest.mark.parametrize("job", tc.TRZSZ_ALONE)
def test_pegsx_trzsz_alone(panel, job):
    """maxit = 0: the trace kernels apart from the sweeps, as tests/test_gpu_pegsx.py's test_trzsz_alone -- three trips of the panel kernel
    and two of the dense one at 1 024 workgroups, a last group of one column on the second trip, f = 256"""
    import bwgr_amd
    case = tc.pegs_case("PEGSX", job)
    Y, X, effects, o = XC.restate(case, maxit=0)
    with _Effects(panel, case, effects) as effs:
        g = bwgr_amd.PEGSX(Y, X, effs, **dict(case["kw"], maxit=0))
    err = max(XR.scaled_err(a, b) for a, b in zip(g["TrZSZ"], o["TrZSZ"]))
    print("PEGSX", job, "TrZSZ alone %.2e" % err)
    assert g["its"] == 0 and g["cnv"] == 10.0 and err <= TOL
    assert all(np.all(u == 0) for u in g["u"]) and XR.scaled_err(g["b"], o["b"]) <= TOL and XR.scaled_err(g["hat"], o["hat"]) <= TOL


# ---- state ----
def _mrr_around_a_pegsx_call(panel):
    """mrr on tall16k (a second trip of k_mrr_ey, 65 slabs, centred) before and after a PEGSX call on the same Panel, which runs the same
    launch train uncentred: the same bits."""
    import bwgr_amd
    tag = "tall16k"
    Y, P = _mrr_traits(tag), panel(tag)
    Yx, X, _ = tc.pegs_case("PEGSX", tag)["data"]()
    a = bwgr_amd.MRR3(Y, P, maxit=2, tol=0)
    x = bwgr_amd.PEGSX(Yx, X, [P], maxit=1, logtol=XC.NOSTOP)
    b = bwgr_amd.MRR3(Y, P, maxit=2, tol=0)
    assert x["its"] == 1
    for key in bwgr_amd.api.MRR_KEYS:
        assert np.array_equal(a[key], b[key]), key


def test_state_between_calls_tall(panel):
    """uvbeta, mrr, xb and uvbeta again on the module's tall9k panel, then uvbeta on a fresh one: the same bits every time.  Then mrr on the
    tall16k panel before and after a PEGSX call on it."""
    import bwgr_amd
    tag = "tall9k"
    X, Y = tc.data(tag), _uvb_traits(tag)
    P = panel(tag)
    a = bwgr_amd.uvbeta(Y, P, "D", maxit=3, tol=0, xb=True)
    m = bwgr_amd.MRR3(Y[:, :3], P, maxit=2, tol=0)
    x = P.xb(a["b"])
    b = bwgr_amd.uvbeta(Y, P, "D", maxit=3, tol=0, xb=True)
    Q = bwgr_amd.Panel(X)
    try:
        c = bwgr_amd.uvbeta(Y, Q, "D", maxit=3, tol=0, xb=True)
        m2 = bwgr_amd.MRR3(Y[:, :3], Q, maxit=2, tol=0)
    finally:
        Q.close()
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
        assert np.array_equal(a[key], c[key], equal_nan=True), key
    assert MR.scaled_err(x, a["xb"]) <= 1e-12      # (k_pxb and uvbeta's row-serial product add in different orders)
    for key in ("b", "hat", "vb", "ve"):
        assert np.array_equal(m[key], m2[key]), key
    _mrr_around_a_pegsx_call(panel)
