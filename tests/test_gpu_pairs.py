"""GPU: the founder-by-sample entries -- crossprod2, Panel.kernel2, EigenArcZ / EigenGauZ -- on the pairs of tests/pair_cases.py, both ways
round: more entries of K_ff and of K_fs than one grid of k_kfin2_apply covers, the rectangular k_xxt_zero over three trips, 1 024-row slabs with
a second slab as either operand of k_xyt_mfma_i8, k_kfin2_rowsq and k_kfin_xs over 16 row workgroups in two slabs.
tests/test_pair_cases_cpu.py proves without a GPU that each orientation reaches what it is listed for.

The bounds are those of tests/test_gpu_kernels2.py: bit equality for the product and between calls, scaled_err <= 1e-6 against
tests/kernels2_restatement.py for the finishes and the coordinates.  One pair of Panels per shape serves the whole module."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernels2_restatement as K2   # noqa: E402
import pair_cases as pc   # noqa: E402
from conftest import scaled_err   # noqa: E402
from test_gpu_kernels2 import TOL, _same   # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = [("ARC", 1.0), ("GAU", 1.0), ("GAU", 0.5)]
DEVICE, KZ_ARC = 1, 0      # include/bwgr.h: BWGR_DEVICE, BWGR_KZ_ARC
IDS = ["%s%s" % (t, "-swapped" if s else "") for t, s in pc.ORIENTATIONS]
JOBS = [(t, s, kind, phi) for t, s in pc.ORIENTATIONS for kind, phi in KINDS]


@pytest.fixture(scope="module")
def pair():
    """(tag, swapped) -> (founders, samples): the shape's two Panels, made once for this module and closed after its last test."""
    import bwgr_amd
    live = bwgr_amd.debug_live()
    made = {}

    def get(tag, swapped=False):
        if tag not in made:
            c = pc.CASES[tag]
            made[tag] = tuple(bwgr_amd.Panel(pc._data(tag, w), **pc.panel_kw(c[w])) for w in "ab")
        a, b = made[tag]
        Pf, Ps = (b, a) if swapped else (a, b)
        pl = pc.plans(tag, swapped)
        assert (Pf.n, Pf.ld // Pf.slab_rows, Pf.slab_rows, Pf.ld) == pl["f"] and (Ps.n, Ps.ld // Ps.slab_rows, Ps.slab_rows, Ps.ld) == pl["s"], (tag, swapped)
        return Pf, Ps

    yield get
    for ps in made.values():
        for P in ps:
            P.close()
    assert bwgr_amd.debug_live() == live


@functools.lru_cache(None)
def _product_ref(tag, swapped=False):
    """X_f X_s', exact: the float64 BLAS product of the codes (every partial sum is an integer below 2^53, so any order of summation gives
    it) cast to int64; numpy's int64 matmul would take seconds at these sizes."""
    if swapped:
        G = np.ascontiguousarray(_product_ref(tag).T)
    else:
        F, S = pc.data(tag)
        Gd = F.astype(np.float64) @ S.astype(np.float64).T
        G = Gd.astype(np.int64)
        assert np.array_equal(G, Gd) and 0 < G.max() <= 4 * pc.P
        rows = np.array([0, 1, 255, 256, 1023, 1024, F.shape[0] - 1])
        assert np.array_equal(G[rows], K2.crossprod2(F[rows], S))       # the int64 product itself, on rows either side of every slab boundary
    G.setflags(write=False)
    return G


@functools.lru_cache(None)
def _restated(tag, swapped, kind, phi):
    """(Kff, Kfs) of the restatement, computed once per case and shared (read-only)"""
    F, S = pc.data(tag, swapped)
    out = tuple(K2.kernels(kind, np.ascontiguousarray(F), np.ascontiguousarray(S), phi))
    for a in out:
        a.setflags(write=False)
    return out


# ---- the product ----
@pytest.mark.parametrize("tag,swapped", pc.ORIENTATIONS, ids=IDS)
def test_crossprod2(pair, tag, swapped):
    """bit-equal to the exact product, twice, and on the device"""
    Pf, Ps = pair(tag, swapped)
    G = Pf.crossprod2(Ps)
    _same(G, _product_ref(tag, swapped))
    assert np.array_equal(Pf.crossprod2(Ps), G)
    assert np.array_equal(Pf.crossprod2(Ps, device_out=True).cpu().numpy(), G)


@pytest.mark.parametrize("tag", list(pc.CASES))
def test_crossprod2_swapped_is_the_transpose(pair, tag):
    Pf, Ps = pair(tag)
    Gfs, Gsf = Pf.crossprod2(Ps), Ps.crossprod2(Pf)
    assert Gfs.shape == (Pf.n, Ps.n) and Gsf.shape == (Ps.n, Pf.n) and np.array_equal(Gfs, Gsf.T)


@pytest.mark.parametrize("swapped", [False, True], ids=["pair1100", "pair1100-swapped"])
def test_forced_chunks_give_the_same_bits(pair, swapped, monkeypatch):
    """Three chunks of markers add into the zeroed n_f x n_s array: the rectangular k_xxt_zero runs, and 1 100 000 entries are more than its
    grid covers in two trips.  Integer sums: the same bits as the one-chunk product, in G and in the two kernels made from it (K_ff's
    product is zeroed and accumulated likewise, upper = 1), to the caller's device arrays and to the host."""
    import torch
    import bwgr_amd
    from bwgr_amd import _lib
    L = _lib.lib()
    tag = "pair1100"
    pl = pc.plans(tag, swapped)
    assert pl["forced_chunks"] == 3 and pl["zero_fs"] == 3
    Pf, Ps = pair(tag, swapped)
    nf, ns = Pf.n, Ps.n
    monkeypatch.setenv("BWGR_KCHUNK", str(pl["kchunk"]))     # read when the founders' root panel is made
    Qf = bwgr_amd.Panel(pc.data(tag, swapped)[0], **pc.panel_kw(pc.sides(tag, swapped)[0]))
    # The caller's device arrays hold -9 everywhere when the library gets them: an entry that is added to without having been zeroed shows.
    # (An array the library allocates itself for a host result is fresh device memory, which may well hold zeros already.)
    Gd = torch.full((nf, ns), -9, dtype=torch.int64, device="cuda")
    Kffd, Kfsd = (torch.full(sh, -9, dtype=torch.int64, device="cuda") for sh in ((nf, nf), (nf, ns)))
    torch.cuda.synchronize()
    try:
        assert L.bwgr_panel_crossprod2(Qf._h, Ps._h, C.c_void_p(Gd.data_ptr()), ns, DEVICE) == 0
        assert L.bwgr_panel_kernel2(Qf._h, Ps._h, KZ_ARC, 1.0, C.c_void_p(Kffd.data_ptr()), nf, C.c_void_p(Kfsd.data_ptr()), ns, DEVICE) == 0
        Gh = Qf.crossprod2(Ps)
    finally:
        Qf.close()
    G = Gd.cpu().numpy()
    _same(G, _product_ref(tag, swapped))
    assert np.array_equal(Gh, G) and np.array_equal(G, Pf.crossprod2(Ps))
    Kff1, Kfs1 = Pf.kernel2(Ps, "ARC")
    assert np.array_equal(Kffd.view(torch.float64).cpu().numpy(), Kff1) and np.array_equal(Kfsd.view(torch.float64).cpu().numpy(), Kfs1)


# ---- the finishes ----
@pytest.mark.parametrize("tag,swapped,kind,phi", JOBS, ids=["%s%s-%s-%s" % (t, "-swapped" if s else "", k, f) for t, s, k, f in JOBS])
def test_kernel2(pair, tag, swapped, kind, phi):
    """Against the restatement at test_gpu_kernels2's bound, to the host and to the device; K_ff exactly symmetric.  Under GAU K_ff is also
    the founders' own EigenGAU kernel bit for bit: the two finishes evaluate exp(sqrt(G_ii + G_jj - 2 G_ij) t) with the same t from
    kfin_gau_t over the same exact product -- a check that does not pass through the restatement."""
    Pf, Ps = pair(tag, swapped)
    Kff, Kfs = Pf.kernel2(Ps, kind, phi)
    Kff2, Kfs2 = Pf.kernel2(Ps, kind, phi)
    Dff, Dfs = Pf.kernel2(Ps, kind, phi, device_out=True)
    rff, rfs = _restated(tag, swapped, kind, phi)
    eff, efs = scaled_err(Kff, rff), scaled_err(Kfs, rfs)
    print("%s%s %s phi=%s: scaled_err Kff = %.3e, Kfs = %.3e" % (tag, " swapped" if swapped else "", kind, phi, eff, efs))
    assert Kff.dtype == np.float64 and Kff.shape == rff.shape == (Pf.n, Pf.n) and Kfs.dtype == np.float64 and Kfs.shape == rfs.shape == (Pf.n, Ps.n)
    assert np.all(np.isfinite(Kff)) and np.all(np.isfinite(Kfs))
    assert eff <= TOL, eff
    assert efs <= TOL, efs
    assert np.array_equal(Kff, Kff.T)
    assert np.array_equal(Kff, Kff2) and np.array_equal(Kfs, Kfs2)      # two calls: identical bits
    assert np.array_equal(Dff.cpu().numpy(), Kff) and np.array_equal(Dfs.cpu().numpy(), Kfs)
    if kind == "GAU":
        assert np.array_equal(Kff, Pf.kernel("EigenGAU", phi))


# ---- the drivers ----
@pytest.mark.parametrize("kind,phi", KINDS, ids=["ARC", "GAU-1.0", "GAU-0.5"])
def test_driver_projection(pair, kind, phi):
    """EigenArcZ / EigenGauZ on pair1100 as test_gpu_kernels2's test_driver_parts_and_projection compares them: Z (V sqrt(L))' = K_fs' and
    Z Z' = K_fs' K_ff^-1 K_fs of the restatement -- projections, which the signs and rotations of eigenvectors do not touch.  The restated
    K_ff is well conditioned (asserted: 2.7e3 for ARC, 1.0e3 and 3.1e3 for GAU)."""
    import bwgr_amd
    Pf, Ps = pair("pair1100")
    r = bwgr_amd.EigenArcZ(Pf, Ps, parts=True) if kind == "ARC" else bwgr_amd.EigenGauZ(Pf, Ps, phi, parts=True)
    assert sorted(r) == ["Kff", "Kfs", "Z", "values", "vectors"]
    Z, w, V = r["Z"], r["values"], r["vectors"]
    assert Z.dtype == np.float64 and Z.shape == (Ps.n, Pf.n) and np.all(np.diff(w) >= 0) and w[0] > 0
    e1 = scaled_err(Z @ (V * np.sqrt(w)).T, r["Kfs"].T)
    rff, rfs = _restated("pair1100", False, kind, phi)
    cond = np.linalg.cond(rff)
    assert cond <= 1e5, cond           # a condition on the inputs
    e2 = scaled_err(Z @ Z.T, rfs.T @ np.linalg.solve(rff, rfs))
    print("pair1100 %s phi=%s: Z (V sqrt(L))' against Kfs' %.3e; Z Z' against Kfs' Kff^-1 Kfs %.3e (cond %.3g)" % (kind, phi, e1, e2, cond))
    assert e1 <= TOL, e1
    assert e2 <= TOL, e2
    Kff, Kfs = Pf.kernel2(Ps, kind, phi)
    assert np.array_equal(r["Kff"], Kff) and np.array_equal(r["Kfs"], Kfs)
