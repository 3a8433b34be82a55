"""GPU: MLM and its projection (bwgr_amd.mlm).
  parity:        every key of every case of tests/mlm_cases.py against the float64 restatement (tests/mlm_restatement.py) at 1e-6 scaled, the
                 project's parity tolerance, `its` equal
  projection:    project() elementwise against Zp formed in long double (tests/ld_linalg.py), within a bound that does not come from the code
                 under test (test_projection_within_its_bound); the same bits for two calls, a host and a device Z, a column alone and within a
                 wider call, panels of three slab heights, and a panel and its dense copy
  orthogonality: X'project(Z, X) against the same product of the long-double Zp
  the fit on a panel and on dense(Z) of the same numbers; the stopping rule; the refusals, a valid call after each; two calls, a clone on a
  caller's stream"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ld_linalg as LD  # noqa: E402
import mlm_cases as MC  # noqa: E402
import mlm_restatement as LR  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6
U = 2.0 ** -53
PROJ = ("k3_p65_f1", "k4_p130_f3", "k6_p400_f17", "k2_f256", "dense_k3", "two_slabs")


def _Z(name):
    """Z as the entries take it: the int8 matrix, or dense(Z) for a dense case"""
    import bwgr_amd
    Z = MC.data(name)[2]
    return bwgr_amd.dense(Z) if MC.CASES[name].get("dense") else Z


def _mlm(name, Z=None, **kw):
    from bwgr_amd import mlm
    Y, X, _ = MC.data(name)
    args = dict(MC.fit_kw(name), **MC.CASES[name].get("panel_kw", {}))
    args.update(kw)
    return mlm.MLM(Y, X, _Z(name) if Z is None else Z, **args)


def _check(g, o, keys=MC.KEYS):
    assert g["its"] == o["its"] >= 3
    errs = {k: LR.scaled_err(np.asarray(g[k]).reshape(np.asarray(o[k]).shape), o[k]) for k in keys}
    print("scaled errors:", {k: "%.2e" % v for k, v in errs.items()})
    assert all(np.all(np.isfinite(np.asarray(g[k]))) for k in keys)
    assert all(v <= TOL for v in errs.values()), errs
    return max(errs.values())


def _same_bits(a, b, keys=MC.KEYS + ("its",)):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


# ---- parity ----

@pytest.mark.parametrize("name", list(MC.CASES))
def test_parity(name):
    """largest scaled error measured over all cases and keys: 7.4e-11 (k2_f256; 1.9e-12 on two_slabs, at most 1.5e-13 on the others)"""
    from bwgr_amd import mlm
    c = MC.CASES[name]
    o = MC.ref(name)
    g = _mlm(name)
    assert tuple(g) == mlm.MLM_KEYS == tuple(o)[:9]
    assert g["b"].shape == (c["f"], c["k"]) and g["u"].shape == (c["p"], c["k"]) and g["hat"].shape == (c["n"], c["k"]) and g["vb"].shape == (c["k"], c["k"])
    print(name, "largest scaled error %.2e" % _check(g, o))
    if name == "k2_f256":
        assert sum(t["lam"] < 0.001 for t in MC.ref(name, True)["trace"]) >= c["maxit"] - 2


def test_maxit_zero_returns_the_start():
    Y, X, Z = MC.data("k4_p130_f3")
    g, o = _mlm("k4_p130_f3", maxit=0), LR.fit(Y, X, Z.astype(np.float64), maxit=0)
    assert g["its"] == 0 and g["cnv"] == 10.0 and not g["u"].any() and np.allclose(g["h2"], 0.5, rtol=0, atol=1e-15)
    for k in ("b", "hat", "GC", "vb", "ve"):
        assert LR.scaled_err(g[k], o[k]) <= TOL, k


# ---- the projection alone ----

@functools.lru_cache(maxsize=None)
def _ld_projection(name):
    """(Zp, C, a bound on A^-1's 2-norm, a bound on A's condition number) in long double from the float-rounded X and Z.  The two bounds are the
    Frobenius norms, ||A^-1||_F >= ||A^-1||_2 and kappa_F = ||A||_F ||A^-1||_F >= kappa_2, with A^-1 by Cholesky in long double: a Jacobi
    eigen-decomposition of a 256 x 256 matrix in long double takes ten seconds here, these a fifth of one, and a larger kappa only widens
    the bound by a factor of at most f."""
    _, X, Z = MC.data(name)
    Xl, Zl = X.astype(np.longdouble), Z.astype(np.longdouble)
    A = Xl.T @ Xl
    Cl = LD.solve(A, Xl.T @ Zl)
    iA = LD.inv(A)
    inorm = float(np.sqrt((iA * iA).sum()))
    return Zl - Xl @ Cl, Cl, inorm, float(np.sqrt((A * A).sum())) * inorm


def _projection_bound(name):
    """The elementwise bound on |project(Z, X) - Zp| (Zp in long double), in two parts.
    (1) The chain acc = z; acc = fma(-x_l, c_l, acc), l = 0 .. f-1, is f fused operations on f + 1 terms, each rounded once: at most
        (f + 1) 2^-53 (|z_ij| + sum_l |x_il| |c_lj|), plus 2^-53 |Zp_ij| for rounding the long double Zp itself to compare.
    (2) The device's C differs from the long double C.  With A = X'X, kappa = ||A||_F ||A^-1||_F in long double (at least lambda_max / lambda_min; ||A^-1||_2 is bounded by ||A^-1||_F likewise) and u = 2^-53:
        Z'X is summed over n terms in fp64, an error of at most n u |X|'|z_j| per entry, which A^-1 carries into c_j with norm at most
        n u ||A^-1||_2 || |X|'|z_j| ||_2; A itself is summed over n terms (||dA||_2 <= n u || |X|'|X| ||_2 <= n u f ||A||_2, since
        || |X|'|X| ||_2 <= trace A <= f lambda_max), its symmetric eigen-decomposition is backward stable with a constant of the order of f^2
        (cyclic Jacobi: f^2 / 2 rotations per sweep, about ten sweeps: 64 f^2 u ||A||_2 is taken), and a perturbation dA of A moves
        c_j = A^-1 (X'z_j) by at most kappa (||dA|| / ||A||) ||c_j||_2 to first order; the f-term products of A^-1 with Z'X add at most
        f u sqrt(f) ||A^-1||_2 ||X'z_j||_2.  Together
            ||dc_j||_2 <= u (kappa (n f + 64 f^2) ||c_j||_2 + (n + f sqrt f) ||A^-1||_2 || |X|'|z_j| ||_2),
        and element (i, j) moves by at most ||x_i||_2 ||dc_j||_2.
    Returns (bound, the chain's part alone)."""
    _, X, Z = MC.data(name)
    n, f = X.shape
    Zp, Cl, inorm, kappa = _ld_projection(name)
    Cf, Zf = np.abs(Cl.astype(np.float64)), np.abs(Z.astype(np.float64))
    chain = (f + 1) * U * (Zf + np.abs(X) @ Cf) + U * np.abs(Zp.astype(np.float64))
    dc = U * (kappa * (n * f + 64 * f * f) * np.sqrt((Cf ** 2).sum(0)) + (n + f * np.sqrt(f)) * inorm * np.sqrt(((np.abs(X).T @ Zf) ** 2).sum(0)))
    return chain + np.sqrt((X ** 2).sum(1))[:, None] * dc[None, :], chain


@pytest.mark.parametrize("name", PROJ)
def test_projection_within_its_bound(name):
    """Measured with the 2-norm kappa (1 to 604 on these cases), largest error / bound over the elements: k3_p65_f1 0.022, k4_p130_f3 9.3e-4,
    k6_p400_f17 3.1e-5, k2_f256 2.9e-8, dense_k3 6.0e-4, two_slabs 3.9e-4 (the Frobenius kappa widens the bound by up to f); against the chain's
    part alone the error is 0.35 of it at f = 1 and up to 4.1 of it where f > 1: the device's C is not the long double one."""
    from bwgr_amd import mlm
    _, X, _ = MC.data(name)
    Zp = _ld_projection(name)[0]
    bound, chain = _projection_bound(name)
    g = mlm.project(_Z(name), X, **MC.CASES[name].get("panel_kw", {}))
    assert g.shape == Zp.shape and g.dtype == np.float64 and np.all(np.isfinite(g))
    err = np.abs((g.astype(np.longdouble) - Zp).astype(np.float64))
    print(name, "kappa %.3g  largest error %.3g  error / bound %.3g  error / chain bound %.3g" % (_ld_projection(name)[3], err.max(), (err / bound).max(), (err / chain).max()))
    assert np.all(err <= bound)


def test_projection_gives_the_same_bits_however_it_is_asked():
    import torch
    import bwgr_amd
    from bwgr_amd import mlm
    from bwgr_amd.panel import as_panel
    _, X, Z = MC.data("two_slabs")
    Zf = np.asfortranarray(Z.astype(np.float64))
    cols = [5, 64, 129]
    with as_panel(Z) as P:
        base = mlm.project(P, X)
        assert P.slab_rows == 256 and np.array_equal(mlm.project(P, X), base)                         # two calls
        dev = mlm.project(P, X, device_out=True)
        assert dev.is_cuda and tuple(dev.shape) == Z.shape and np.array_equal(dev.cpu().numpy(), base)
    for kw, R in zip(MC.OTHER_SLABS, (128, 384)):                                                     # another slab height
        with as_panel(Z, **kw) as Q:
            assert Q.slab_rows == R and np.array_equal(mlm.project(Q, X), base)
    host = mlm.project(bwgr_amd.dense(Zf), X)
    assert np.array_equal(host, base)                                                                 # a panel and its dense copy
    Zd = torch.from_numpy(Zf.T.copy()).cuda().t()                                                     # column-major on the device
    got = mlm.project(bwgr_amd.dense(Zd), X)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), host)                                    # a host and a device Z
    Zw = torch.zeros((Z.shape[1], Z.shape[0] + 5), dtype=torch.float64, device="cuda")
    Zw[:, :Z.shape[0]] = Zd.t()
    assert np.array_equal(mlm.project(bwgr_amd.dense(Zw.t()[:Z.shape[0]]), X).cpu().numpy(), host)    # a column stride beyond n
    assert np.array_equal(mlm.project(bwgr_amd.dense(Zf[:, cols]), X), host[:, cols])                 # columns alone and within a wider call
    assert np.array_equal(mlm.project(Z[:, cols], X), base[:, cols])
    _, Xr, Zr = MC.data("dense_k3")                                                                   # real values, host and device
    a = mlm.project(bwgr_amd.dense(Zr), Xr)
    b = mlm.project(bwgr_amd.dense(torch.from_numpy(Zr.T.copy()).cuda().t()), Xr)
    assert np.array_equal(a, b.cpu().numpy()) and np.array_equal(mlm.project(bwgr_amd.dense(Zr[:, 7:8]), Xr), a[:, 7:8])


@pytest.mark.parametrize("name", ("k6_p400_f17", "k2_f256", "dense_k3"))
def test_projection_is_orthogonal_to_the_covariates(name):
    """X'project(Z, X) against X' times the long double Zp rounded to fp64, both products in fp64: they differ by at most |X|'E, E the
    projection's own bound, plus 8 x the fp64 product's n 2^-53 |X|'|Zp|.  Measured max |X'Zp| / max |X'Z|: 3.5e-15 (k6_p400_f17), 3.8e-14
    (k2_f256), 6.4e-16 (dense_k3); the long double Zp rounded to fp64 gives 2e-17 to 8e-17; largest difference / limit 5.8e-4."""
    from bwgr_amd import mlm
    _, X, Z = MC.data(name)
    n = X.shape[0]
    Zp = _ld_projection(name)[0].astype(np.float64)
    E = _projection_bound(name)[0]
    g = mlm.project(_Z(name), X)
    r_dev, r_ld = X.T @ g, X.T @ Zp
    lim = np.abs(X).T @ E + 8 * n * U * (np.abs(X).T @ np.abs(Zp))
    scale = np.abs(X.T @ Z.astype(np.float64)).max()
    print(name, "max |X'Zp| / max |X'Z|: device %.3g, long double %.3g; largest difference / limit %.3g" % (np.abs(r_dev).max() / scale, np.abs(r_ld).max() / scale,
                                                                                                           (np.abs(r_dev - r_ld) / lim).max()))
    assert np.all(np.abs(r_dev - r_ld) <= lim)
    assert np.abs(r_dev).max() <= 1e-12 * scale


# ---- the fit ----

def test_panel_against_dense():
    """the same numbers as a panel and as dense(Z): the projection gives the same bits, and so does everything after it (measured difference: 0)"""
    import bwgr_amd
    for name in ("k4_p130_f3", "k16_p200_f5"):
        Z = MC.data(name)[2]
        a = _mlm(name)
        b = _mlm(name, Z=bwgr_amd.dense(Z.astype(np.float64)))
        diff = {k: LR.scaled_err(b[k], a[k]) for k in MC.KEYS}
        print(name, "panel against dense:", {k: "%.1e" % v for k, v in diff.items()})
        assert a["its"] == b["its"] and max(diff.values()) <= TOL


def test_stopping_rule():
    """verb=False stops only on a NaN: it runs every sweep it is given, long after cnv < logtol; verb=True stops where the restatement stops"""
    o = MC.ref("k2_conv_verb")
    assert 5 <= o["its"] < 25
    g = _mlm("k2_conv_verb", verb=False, maxit=25)
    assert g["its"] == 25 and g["cnv"] < -8
    Y, X, Z = MC.data("k2_conv_verb")
    _check(g, LR.fit(Y, X, Z.astype(np.float64), maxit=25, verb=False))
    v = _mlm("k2_conv_verb", verb=True)
    assert v["its"] == o["its"] and v["cnv"] < -8
    _check(v, o)


def test_two_calls_a_clone_and_a_callers_stream_give_the_same_bits():
    import torch
    from bwgr_amd.panel import as_panel
    a, b = _mlm("k6_p400_f17", maxit=6), _mlm("k6_p400_f17", maxit=6)
    _same_bits(a, b)
    d1, d2 = _mlm("dense_k3", maxit=6), _mlm("dense_k3", maxit=6)
    _same_bits(d1, d2)
    Z = MC.data("k6_p400_f17")[2]
    s = torch.cuda.Stream()
    with as_panel(Z) as P:
        _same_bits(_mlm("k6_p400_f17", Z=P, maxit=6), a)
        q = P.clone()
        q.set_stream(s.cuda_stream)
        _same_bits(_mlm("k6_p400_f17", Z=q, maxit=6), a)
        q.close()
        P.set_stream(s.cuda_stream)
        _same_bits(_mlm("k6_p400_f17", Z=P, maxit=6), a)
        P.set_stream(0)


# ---- refusals ----

def test_refusals_leave_the_device_usable():
    """every refusal of bwgr_mlm comes through the Python layer as code 1 with a message that names f, the trait or the entry; a valid call right
    after each gives the bits of the first"""
    import bwgr_amd
    from bwgr_amd import mlm, BwgrError
    Y, X, Z = MC.data("k1_p64_f2")
    n, p = Z.shape
    Zf = Z.astype(np.float64)
    rng = np.random.default_rng(11)
    base = mlm.MLM(Y, X, Z, maxit=3)
    based = mlm.MLM(Y, X, bwgr_amd.dense(Zf), maxit=3)

    def w(a, i, j, v):
        a = np.array(a, np.float64)
        a[i, j] = v
        return a
    Yfew = np.array(Y); Yfew[2:, 0] = np.nan                      # two records, f = 2
    lev = (np.arange(n) < n // 2).astype(np.float64)
    Xlev = np.column_stack([np.ones(n), lev]); Ylev = np.array(Y); Ylev[n // 2:, 0] = np.nan      # trait 0 sees one level only
    bad = [
        (lambda: mlm.MLM(Y, np.ones((n, 0)), Z), "f = 0"),
        (lambda: mlm.MLM(Y, rng.normal(size=(n, 257)), Z), "f = 257"),
        (lambda: mlm.MLM(Y, w(X, 3, 1, np.inf), Z), "X[3, 1]"),
        (lambda: mlm.MLM(Y, X, bwgr_amd.dense(w(Zf, 4, 2, np.nan))), "Z[4, 2]"),
        (lambda: mlm.MLM(Yfew, X, Z), "trait 0"),
        (lambda: mlm.MLM(Ylev, Xlev, Z), "trait 0"),
        (lambda: mlm.MLM(Y, np.ones((n, 2)), Z), "trait 0"),
        (lambda: mlm.MLM(np.zeros((n, 0)), X, Z), "k = 0"),
        (lambda: mlm.MLM(rng.normal(size=(n, 17)), X, Z), "k = 17"),
        (lambda: mlm.MLM(Y, X, Z, maxit=-1), "maxit = -1"),
        (lambda: mlm.MLM(Y, X, bwgr_amd.Panel(Z.astype(np.float32), as_int8=False)), "fp32"),
        (lambda: mlm.MLM(Y, X, Z[:-1]), "nrow"),
        (lambda: mlm.MLM(Y, X, bwgr_amd.dense(Zf[:-1])), "nrow"),
        (lambda: mlm.project(bwgr_amd.Panel(Z.astype(np.float32), as_int8=False), X), "fp32"),
        (lambda: mlm.project(Z, np.ones((n, 2))), "all rows"),
    ]
    for i, (call, word) in enumerate(bad):
        with pytest.raises(BwgrError) as ei:
            call()
        assert ei.value.code == 1 and word in str(ei.value), (i, word, str(ei.value))
        _same_bits(mlm.MLM(Y, X, bwgr_amd.dense(Zf), maxit=3) if i % 2 else mlm.MLM(Y, X, Z, maxit=3), based if i % 2 else base)
    # the null pointers, through the C entry
    from bwgr_amd import _lib
    L = _lib.lib()
    Xf, Yf, Zc = np.asfortranarray(X), np.asfortranarray(Y), np.asfortranarray(Zf)
    u, its = np.zeros((p, 1)), C.c_int()
    dp, vp = (lambda a: None if a is None else a.ctypes.data_as(_lib.c_d)), (lambda a: None if a is None else a.ctypes.data_as(C.c_void_p))
    for args in (dict(Z=None), dict(X=None), dict(Y=None), dict(u=None), dict(its=None)):
        a = dict(dict(Z=Zc, X=Xf, Y=Yf, u=u, its=its), **args)
        rc = L.bwgr_mlm(0, None, vp(a["Z"]), 0, n, p, n, dp(a["X"]), 2, n, dp(a["Y"]), 1, 3, -8.0, 1.1, 0, None, dp(a["u"]), None, None, None, None, None, None,
                        None if a["its"] is None else C.byref(a["its"]))
        assert rc == 1 and "mlm: null pointer" in L.bwgr_last_error().decode(), args
    _same_bits(mlm.MLM(Y, X, Z, maxit=3), base)
    # the workspace: from the plan hook only
    pl = mlm.mlm_plan(10000, 1000000, 8, 4, 4)
    assert pl["ws_bytes"] >= 80 * 10 ** 9
