"""GPU: the finishes of the relationship kernels (k_kfin_colstats, k_kfin_xs, k_kfin2_rowsq, k_kfin_diag, k_kfin_sumd_*, k_kfin_apply,
k_kfin2_apply and the host scalars of bwgr_panel_kernel / bwgr_panel_kernel2) on int8 codes beyond 0 / 1 / 2: the panels of
tests/kernel_code_cases.py, whose CPU guards (tests/test_kernel_code_cases_cpu.py) show that a byte read as unsigned in the column sums, the
row sums or the samples' row squares moves a centred kernel by 1e-2 or more.  Three kinds of check: parity with the float64 restatement at
the project's bound; the long double reference, which centres first and so shares no rounding with the library's centring identity; and
identities that need no tolerance at all."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernels_restatement as KR   # noqa: E402
import kernels2_restatement as K2   # noqa: E402
import kernel_code_cases as KC   # noqa: E402
from conftest import scaled_err   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6           # the project's parity bound for fp64 engines against fp64 restatements (tests/test_gpu_kernels.py)
LD_BOUND = 1e-9      # against the long double reference: see tests/test_kernel_code_cases_cpu.py
KS = list(range(len(KR.KINDS)))
KIDS = [KC.kind_id(k) for k in KS]


@pytest.fixture(scope="module")
def panels():
    """one resident panel per case, made on first use and shared by every test of this file"""
    import bwgr_amd
    made = {}

    def get(tag, X=None, kw=None):
        if tag not in made:
            made[tag] = bwgr_amd.Panel(KC.data(tag) if X is None else X, **(KC.CASES.get(tag, {}).get("kw", {}) if kw is None else kw))
        return made[tag]
    yield get
    for P in made.values():
        P.close()


def _pair_panels(panels, tag, swapped):
    F, S, kwf, kws = KC.pair_data(tag, swapped)
    names = ("%s/f" % tag, "%s/s" % tag)
    nf, ns = names[::-1] if swapped else names
    return panels(nf, F, kwf), panels(ns, S, kws)


def _call(P, k, **extra):
    import bwgr_amd
    kind, kw = KR.KINDS[k]
    return getattr(bwgr_amd, kind)(P, **kw, **extra)


def _bits(A):
    return np.ascontiguousarray(A).view(np.uint64)


# ---- parity, and the long double reference ----
@pytest.mark.parametrize("k", KS, ids=KIDS)
@pytest.mark.parametrize("tag", KC.TAGS)
def test_kernel_on_codes(panels, tag, k):
    P = panels(tag)
    K, Kagain = _call(P, k), _call(P, k)
    ref, ld, mask = KC.restated(tag, k), KC.reference(tag, k), KC.undefined(tag, k)
    assert K.dtype == np.float64 and K.shape == ref.shape
    assert np.array_equal(np.isfinite(K), ~mask)          # (all finite, but for the reference's own 0 / 0: KC.undefined)
    e_par, e_ld = scaled_err(K[~mask], ref[~mask]), KC.err(K, ld, mask)
    print("%-8s %-16s parity %.3e, against long double %.3e" % (tag, KIDS[k], e_par, e_ld))
    assert e_par <= TOL, e_par
    assert e_ld <= LD_BOUND, e_ld
    assert np.array_equal(_bits(K), _bits(K.T))
    assert np.array_equal(_bits(K), _bits(Kagain))        # two calls: identical bits
    if KR.KINDS[k][0] in ("GAU", "EigenGAU"):
        assert np.array_equal(np.diag(K), np.ones(K.shape[0]))


@pytest.mark.parametrize("kind,phi", KC.PAIR_KINDS, ids=["%s-%s" % kp for kp in KC.PAIR_KINDS])
@pytest.mark.parametrize("tag,swapped", KC.ORIENTATIONS, ids=["%s%s" % (t, "-swapped" if s else "") for t, s in KC.ORIENTATIONS])
def test_kernel2_on_codes(panels, tag, swapped, kind, phi):
    import torch   # noqa: F401  (device_out)
    Pf, Ps = _pair_panels(panels, tag, swapped)
    host = Pf.kernel2(Ps, kind, phi)
    again = Pf.kernel2(Ps, kind, phi)
    dev = tuple(d.cpu().numpy() for d in Pf.kernel2(Ps, kind, phi, device_out=True))
    ref, ld = KC.restated2(tag, swapped, kind, phi), KC.reference2(tag, swapped, kind, phi)
    for where, (Kff, Kfs) in (("host", host), ("device", dev)):
        assert Kff.dtype == np.float64 and Kff.shape == ref[0].shape and Kfs.dtype == np.float64 and Kfs.shape == ref[1].shape
        assert np.all(np.isfinite(Kff)) and np.all(np.isfinite(Kfs))
        par = scaled_err(Kff, ref[0]), scaled_err(Kfs, ref[1])
        eld = KC.err(Kff, ld[0]), KC.err(Kfs, ld[1])
        print("%-10s %-7s %s phi=%s %-6s parity Kff %.3e Kfs %.3e, against long double Kff %.3e Kfs %.3e"
              % (tag, "swapped" if swapped else "", kind, phi, where, par[0], par[1], eld[0], eld[1]))
        assert max(par) <= TOL, par
        assert max(eld) <= LD_BOUND, eld
        assert np.array_equal(Kff, Kff.T)
        if kind == "GAU":
            assert np.array_equal(np.diag(Kff), np.ones(Kff.shape[0]))
    for a, b, c in zip(host, again, dev):
        assert np.array_equal(a, b) and np.array_equal(a, c)      # two calls, and the device result: identical bits


# ---- identities that need no tolerance ----
@pytest.mark.parametrize("k", KS, ids=KIDS)
def test_a_duplicated_row_gives_identical_rows_and_columns(panels, k):
    """hold_dup's row 7 is row 3: every entry of either row is formed from the same integers.  EigenGRM adds 1 to the diagonal before it
    normalises (the reference's :49), so there K[3, 3] and K[7, 7] stand apart from K[3, 7]: the two rows are compared outside these
    columns, and the two diagonal entries with each other."""
    K = _call(panels("hold_dup"), k)
    cols = np.ones(K.shape[0], bool)
    if KR.KINDS[k][0] == "EigenGRM":
        cols[[3, 7]] = False
        assert K[3, 3] == K[7, 7] and K[3, 7] == K[7, 3] and K[3, 3] > K[3, 7]
    assert np.array_equal(K[3, cols], K[7, cols]) and np.array_equal(K[cols, 3], K[cols, 7])
    if KR.KINDS[k][0] in ("GAU", "EigenGAU"):
        assert K[3, 7] == 1.0                  # an exact zero distance off the diagonal


PERMUTED = [k for k in KS if KIDS[k] in ("GAU-", "EigenGAU-1.0", "EigenGAU-0.5", "EigenGRM-False", "EigenARC-False")]


@pytest.mark.parametrize("k", PERMUTED, ids=[KIDS[k] for k in PERMUTED])
@pytest.mark.parametrize("tag", ["tpod100", "dos100"])
def test_kernel_follows_a_row_permutation(panels, tag, k):
    """The asymmetric check of test_crossprod_follows_a_row_permutation through the finish: the kinds whose scalars are exact sums of
    integers (GAU's md, the mean diagonal of the uncentred EigenGRM / EigenARC) or a sum over the whole matrix (EigenGAU's) on a freshly
    made panel of the rows in another order."""
    import bwgr_amd
    X = KC.data(tag)
    perm = np.random.default_rng(5).permutation(X.shape[0])
    K = _call(panels(tag), k)
    Q = bwgr_amd.Panel(np.ascontiguousarray(X[perm]), **KC.CASES[tag]["kw"])
    try:
        Kp = _call(Q, k)
    finally:
        Q.close()
    want = K[np.ix_(perm, perm)]
    print("%s %s: permuted rows, max |diff| = %.3e" % (tag, KIDS[k], np.abs(Kp - want).max()))
    assert np.array_equal(Kp, want)


@pytest.mark.parametrize("phi", [1.0, 0.5])
def test_pair_gau_of_a_panel_with_itself_is_eigengau(panels, phi):
    P = panels("full")
    Kff, Kfs = P.kernel2(P, "GAU", phi)
    off = ~np.eye(P.n, dtype=bool)
    assert np.array_equal(Kfs[off], Kff[off])
    assert np.array_equal(Kff, P.kernel("EigenGAU", phi))


def test_eigenarcz_of_full_with_itself_reproduces_kff(panels):
    """tests/test_gpu_kernels2.py's test_eigenarcz_of_the_founders_reproduces_kff, at its bounds, on the whole byte range"""
    import bwgr_amd
    P = panels("full")
    r = bwgr_amd.EigenArcZ(P, P, parts=True)
    err = scaled_err(r["Z"] @ r["Z"].T, r["Kff"])
    print("full EigenArcZ(F, F): Z Z' against Kff", err)
    assert err <= TOL, err
    assert scaled_err(r["Kfs"], r["Kff"]) <= 1e-12
    assert scaled_err(r["Kff"], K2.arc_kernels(KC.data("full"), KC.data("full"))[0]) <= TOL


# ---- shift invariance, library against library ----
SHIFT_FREE = [k for k in KS if KC.centred_kind(k) or KR.KINDS[k][0] in ("GAU", "EigenGAU")]      # (the other kinds depend on the codes' mean)


@pytest.mark.parametrize("k", SHIFT_FREE, ids=[KIDS[k] for k in SHIFT_FREE])
def test_shifted_codes_give_the_same_kernel(panels, k):
    """pm1, tpod and tpod100 are one matrix after centring, and one set of integer distances.  The centred kinds agree within the long
    double bound (the identity's cancellation on tpod100 is all that parts them); GAU and EigenGAU bit for bit."""
    kind = KR.KINDS[k][0]
    Ks = {tag: _call(panels(tag), k) for tag in KC.SHIFTED}
    for a, b in (("pm1", "tpod"), ("pm1", "tpod100"), ("tpod", "tpod100")):
        if kind in ("GAU", "EigenGAU"):
            assert np.array_equal(Ks[a], Ks[b]), (a, b)
        else:
            e = scaled_err(Ks[a], Ks[b])
            print("%-16s %s against %s: %.3e" % (KIDS[k], a, b, e))
            assert e <= LD_BOUND, (a, b, e)


# ---- slabs and chunks ----
@pytest.mark.parametrize("kchunk", ["64", "100"])
def test_forced_chunks_give_the_same_bits_on_full3(panels, kchunk, monkeypatch):
    import bwgr_amd
    ks = [KIDS.index("GRM-False"), KIDS.index("EigenGAU-1.0")]
    K0 = [_call(panels("full3"), k) for k in ks]
    monkeypatch.setenv("BWGR_KCHUNK", kchunk)     # read when the root panel is made
    Q = bwgr_amd.Panel(KC.data("full3"), **KC.CASES["full3"]["kw"])
    try:
        K1 = [_call(Q, k) for k in ks]
    finally:
        Q.close()
    for a, b in zip(K0, K1):
        assert np.array_equal(a, b)


def test_clone_centred_panel_and_padding_on_full3(panels):
    from bwgr_amd import _lib
    L = _lib.lib()
    P = panels("full3")
    n = P.n
    assert P.slab_rows == 256 and P.ld == 768
    ks = [KIDS.index("GRM-False"), KIDS.index("EigenGAU-1.0")]
    K0 = [_call(P, k) for k in ks]
    Q = P.clone()
    try:
        for k, a in zip(ks, K0):
            assert np.array_equal(_call(Q, k), a)
    finally:
        Q.close()
    P.set_centred(True)
    try:
        for k, a in zip(ks, K0):
            assert np.array_equal(_call(P, k), a)
    finally:
        P.set_centred(False)
    ld = n + 5
    for (kind, par), a in zip(((0, 1.0), (3, 1.0)), K0):      # BWGR_K_GRM, BWGR_K_EIGEN_GAU
        K = np.full((n, ld), -7.25)
        assert L.bwgr_panel_kernel(P._h, kind, par, 0, K.ctypes.data_as(C.c_void_p), ld, 0) == 0
        assert np.array_equal(K[:, n:], np.full((n, 5), -7.25))
        assert np.array_equal(K[:, :n], a)
