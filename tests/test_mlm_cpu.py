"""CPU: MLM without a GPU -- the surface (signature, defaults and key order as the reference's R/RcppExports.R:192 has them; the header, the ABI
table, bwgr_amd.mlm beside an unchanged bwgr_amd.__all__); the soundness of the cases of tests/mlm_cases.py under bwgr_amd.em_order; the
restatement's identities; the plan hook at the edges of every case; the refusals that need no device; and the host tail
(bwgr_amd/csrc/mlm_tail.h) as a program of its own under AddressSanitizer and UBSan against the restatement's trace."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlm_cases as MC  # noqa: E402
import mlm_restatement as LR  # noqa: E402
from test_devbufs_cpu import CSRC, FLAGS, ROOT, _sanitizing_compiler  # noqa: E402

# R/RcppExports.R:192 -- MLM's parameters and defaults (500L, -8, 1L, FALSE, 1.1) and the names of the list it returns (:1394-1402)
REF_PARAMS = [("Y", None), ("X", None), ("Z", None), ("maxit", 500), ("logtol", -8), ("cores", 1), ("verb", False), ("df0", 1.1)]
REF_KEYS = ("b", "u", "hat", "h2", "GC", "vb", "ve", "cnv", "its")


# ---- the surface ----

def test_signature_defaults_and_key_order():
    from bwgr_amd import mlm
    E = inspect.Parameter.empty
    pos = [(q.name, None if q.default is E else q.default) for q in inspect.signature(mlm.MLM).parameters.values() if q.kind == q.POSITIONAL_OR_KEYWORD]
    assert pos == REF_PARAMS
    assert mlm.MLM_KEYS == LR.MLM_KEYS == REF_KEYS
    sig = inspect.signature(mlm.project)
    assert list(sig.parameters)[:2] == ["Z", "X"] and sig.parameters["device_out"].kind == inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["device_out"].default is False
    assert list(inspect.signature(mlm.mlm_plan).parameters) == ["n", "p", "f", "k", "npat"]
    Y, X, Z = MC.data("k1_p64_f2")
    assert tuple(LR.fit(Y, X, Z.astype(float), maxit=2)) == REF_KEYS


def test_header_and_abi_table():
    from bwgr_amd import _lib
    from test_abi_table_cpu import prototypes
    protos = prototypes()
    assert protos["bwgr_project"] == ("int", ["int", "pointer", "pointer", "int", "int64_t", "int64_t", "int64_t", "pointer", "int64_t", "int64_t", "pointer", "int", "int64_t"])
    assert protos["bwgr_mlm"] == ("int", ["int", "pointer", "pointer", "int", "int64_t", "int64_t", "int64_t", "pointer", "int64_t", "int64_t", "pointer", "int", "int",
                                          "double", "double", "int"] + ["pointer"] * 9)
    assert protos["bwgr_debug_mlm_plan"] == ("int", ["int64_t", "int64_t", "int64_t", "int", "int", "pointer"])
    for name in ("bwgr_project", "bwgr_mlm", "bwgr_debug_mlm_plan"):
        assert len(_lib.ABI[name]) == len(protos[name][1]) and hasattr(_lib.lib(), name)
    assert "#define BWGR_MLM_PLAN_NOUT 24" in open(os.path.join(ROOT, "include", "bwgr.h")).read()


def test_module_is_importable_and_the_package_surface_is_unchanged():
    code = ("import sys; sys.path.insert(0, %r); import bwgr_amd; before = list(bwgr_amd.__all__); import bwgr_amd.mlm as M; "
            "assert list(bwgr_amd.__all__) == before and 'MLM' not in before and 'project' not in before and not hasattr(bwgr_amd.Panel, 'project'); "
            "assert callable(M.MLM) and callable(M.project) and callable(M.mlm_plan); "
            "sys.exit(1 if 'torch' in sys.modules else 0)" % ROOT)
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0


def test_documents_no_longer_call_mlm_out_of_scope():
    for rel in ("include/bwgr.h", "DESIGN.md", "README.md", os.path.join("bwgr_amd", "csrc", "kernels.hip.h")):
        txt = open(os.path.join(ROOT, rel)).read()
        assert "makes the int8 panel dense" not in txt, rel
        for m in re.finditer(r"[Oo]ut of scope[^.\n]*|Not here:[^.\n]*", txt):
            assert "MLM" not in m.group(0), (rel, m.group(0))


# ---- the cases ----

def test_case_table_is_the_issues():
    want = {"k3_p65_f1": (66, 65, 3, 1), "k4_p130_f3": (131, 130, 4, 3), "k1_p64_f2": (65, 64, 1, 2), "k16_p200_f5": (150, 200, 16, 5),
            "k6_p400_f17": (300, 400, 6, 17), "k2_f256": (330, 100, 2, 256), "k5_shared_f4": (120, 350, 5, 4), "k2_conv_verb": (200, 60, 2, 2)}
    assert set(MC.TABLE) == set(want)
    for name, shape in want.items():
        c = MC.CASES[name]
        assert (c["n"], c["p"], c["k"], c["f"]) == shape
        assert c["maxit"] <= (500 if name == "k2_conv_verb" else 20 if name == "k2_f256" else 30)
    assert MC.CASES["k2_conv_verb"]["verb"] is True and MC.CASES["k2_conv_verb"]["maxit"] == 500
    Y = MC.data("k16_p200_f5")[0]
    assert MC.npat(Y) == 16 and MC.npat(MC.data("k5_shared_f4")[0]) == 1
    assert MC.data("dense_k3")[2].dtype == np.float64 and not np.all(MC.data("dense_k3")[2] == np.rint(MC.data("dense_k3")[2]))
    n, p = MC.CASES["two_slabs"]["n"], MC.CASES["two_slabs"]["p"]
    R = MC.slab_rows(n, p, **MC.CASES["two_slabs"]["panel_kw"])
    assert R % 128 == 0 and -(-n // R) == 2
    assert sorted(MC.slab_rows(n, p, **kw) for kw in MC.OTHER_SLABS) == [128, 384] and R not in (128, 384)      # three slabs, and one
    its = MC.ref("k2_conv_verb")["its"]
    assert 5 <= its <= 25, its
    bends = sum(t["lam"] < 0.001 for t in MC.ref("k2_f256", True)["trace"])
    assert bends >= MC.CASES["k2_f256"]["maxit"] - 2


@pytest.mark.parametrize("name", list(MC.CASES))
def test_case_is_sound(name):
    """n_t - f >= 17; the smallest ve of any sweep is at least 0.22; a relative perturbation of Y by 2^-40 moves no output by more than 1e-8 of
    its scale; every compared output is finite"""
    Y, X, Z = MC.data(name)
    f = X.shape[1]
    assert ((~np.isnan(Y)).sum(0) - f).min() >= 17
    assert np.array_equal(LR.f32(Y), Y, equal_nan=True) and np.array_equal(LR.f32(X), X) and np.array_equal(LR.f32(Z), Z.astype(np.float64))
    o = MC.ref(name, True)
    assert len(o["trace"]) == o["its"] and min(t["ve"].min() for t in o["trace"]) >= 0.22
    assert all(np.all(np.isfinite(o[k])) for k in MC.KEYS)
    rng = np.random.default_rng(0)
    Y2 = Y * (1.0 + 2.0 ** -40 * rng.choice([-1.0, 1.0], Y.shape))
    keep = LR.f32
    LR.f32 = lambda a: np.asarray(a, np.float64)          # (the perturbed Y is no float: it goes in as it is, and so does its twin)
    try:
        o1 = LR.fit(Y, X, Z.astype(np.float64), **MC.fit_kw(name))
        o2 = LR.fit(Y2, X, Z.astype(np.float64), **MC.fit_kw(name))
    finally:
        LR.f32 = keep
    assert o1["its"] == o2["its"] == o["its"]
    moves = {k: LR.scaled_err(o2[k], o1[k]) for k in MC.KEYS}
    print(name, {k: "%.1e" % v for k, v in moves.items()})
    assert max(moves.values()) <= 1e-8, moves


# ---- the restatement ----

def test_restatement_identities():
    for name in ("k4_p130_f3", "k6_p400_f17", "dense_k3"):
        Y, X, Z = MC.data(name)
        Zp, C = LR.project(Z.astype(np.float64), X)
        assert np.abs(X.T @ Zp).max() <= 1e-10 * np.abs(X.T @ Z.astype(np.float64)).max()            # X'Zp = 0
        W, MU, y = LR.fixed(Y, X)
        for t in range(Y.shape[1]):
            M = X * W[:, t:t + 1]
            assert np.abs(M.T @ y[:, t]).max() <= 1e-10 * np.abs(M.T @ np.nan_to_num(Y[:, t])).max()  # M_t'y_t = 0
            assert np.all(y[W[:, t] == 0, t] == 0)
    Y, X, Z = MC.data("k3_p65_f1")                                                                     # f = 1: the column-centred Z
    Zf = Z.astype(np.float64)
    assert np.all(X == 1.0) and np.abs(LR.project(Zf, X)[0] - (Zf - Zf.mean(0))).max() <= 1e-13
    o = MC.ref("k3_p65_f1")
    assert np.abs(o["hat"] - (LR.project(Zf, X)[0] @ o["u"] + X @ o["b"])).max() <= 1e-12
    start = LR.fit(Y, X, Zf, maxit=0)
    assert start["its"] == 0 and start["cnv"] == 10.0 and not start["u"].any() and np.allclose(start["h2"], 0.5)


def test_bending_only_grows():
    tr = MC.ref("k2_f256", True)["trace"]
    infl = [t["inflate"] for t in tr]
    assert all(b >= a for a, b in zip(infl, infl[1:])) and infl[-1] > 0
    vb, inflate, lam = LR.bend(np.array([[1.0, 2.0], [2.0, 1.0]]), 0.5)          # smallest eigenvalue -1: fabs(1.1 * -1) = 1.1 replaces 0.5
    assert lam == pytest.approx(-1.0) and inflate == pytest.approx(1.1) and vb[0, 0] == pytest.approx(2.1)
    vb, inflate, lam = LR.bend(np.array([[1.0, 0.9995], [0.9995, 1.0]]), 0.5)     # 0.0005 < 0.001, but 0.00055 does not exceed 0.5: it stays, and is added
    assert inflate == 0.5 and vb[1, 1] == pytest.approx(1.5)
    vb, inflate, lam = LR.bend(np.eye(2), 0.25)                                   # nothing to bend: the carried inflate still goes on
    assert inflate == 0.25 and vb[0, 0] == 1.25


# ---- the plan hook ----

@pytest.mark.parametrize("name", list(MC.CASES))
def test_plan_edges(name):
    from bwgr_amd import mlm
    from bwgr_amd.mtfit import mrr_dense_plan
    c = MC.CASES[name]
    n, p, k, f = c["n"], c["p"], c["k"], c["f"]
    g = MC.npat(MC.data(name)[0])
    pl = mlm.mlm_plan(n, p, f, k, g)
    tp = mrr_dense_plan(n, p, k, g)
    assert all(pl[key] == tp[key] for key in tp if key != "ws_bytes") and pl["train_bytes"] == tp["ws_bytes"]
    assert pl["ld"] == -(-n // 128) * 128 and pl["nblk"] == -(-p // 64) and pl["edge"] == p - (pl["nblk"] - 1) * 64
    assert pl["proj_blocks"] == pl["nblk"]
    tiles = pl["ld"] // 64
    assert pl["proj_row_wg"] == min(tiles, 16) and pl["proj_trips"] == -(-tiles // pl["proj_row_wg"]) and pl["proj_row_wg"] * pl["proj_trips"] >= tiles
    assert pl["f_piece"] == min(f, 64) and pl["f_pieces"] == -(-f // 64) and pl["f_piece"] * pl["f_pieces"] >= f
    assert pl["proj_lds"] == 2 * pl["f_piece"] * 64 * 8 <= 64 * 1024
    assert pl["ztx_groups"] == -(-f // 16)
    assert pl["proj_bytes"] == 8 * (n * f + pl["ztx_groups"] * pl["ld"] * 16 + 2 * p * f)
    assert pl["ws_bytes"] == pl["train_bytes"] + pl["proj_bytes"] >= 8 * pl["ld"] * p
    if name == "k2_f256":
        assert pl["f_pieces"] == 4 and pl["proj_lds"] == 65536 and pl["ztx_groups"] == 16
    if name == "k6_p400_f17":
        assert pl["ztx_groups"] == 2
    if name == "k3_p65_f1":
        assert pl["nblk"] == 2 and pl["edge"] == 1 and n % 64 == 2
    if name == "k4_p130_f3":
        assert pl["nblk"] == 3 and pl["ld"] == 256 > n > 128
    if name == "k1_p64_f2":
        assert pl["nblk"] == 1 and pl["edge"] == 64


def test_plan_shows_the_price_of_the_copy():
    from bwgr_amd import mlm
    assert mlm.mlm_plan(5000, 50000, 8, 4, 4)["ws_bytes"] >= 5000 * 50000 * 8                    # config 2: 2 GB
    big = mlm.mlm_plan(10000, 1000000, 8, 4, 4)
    assert big["ws_bytes"] >= 80 * 10 ** 9 and big["proj_blocks"] == 15625 and big["proj_row_wg"] == 16


def test_plan_refusals():
    from bwgr_amd import mlm, BwgrError
    for bad in ((1, 5, 1, 1, 1), (5, 0, 1, 1, 1), (5, 2 ** 31, 1, 1, 1), (5, 5, 0, 1, 1), (5, 5, 257, 1, 1), (5, 5, 1, 0, 1), (5, 5, 1, 17, 1), (5, 5, 1, 2, 3),
                (5, 5, 1, 2, 0)):
        with pytest.raises(BwgrError) as ei:
            mlm.mlm_plan(*bad)
        assert ei.value.code == 1 and "mlm plan" in str(ei.value)
    assert mlm.mlm_plan(5, 5, 256, 16, 16)["f_pieces"] == 4


def test_timing_hook_needs_no_device():
    import ctypes as C
    from bwgr_amd import _lib
    L = _lib.lib()
    out = (C.c_double * 5)(*([-1.0] * 5))
    assert "#define BWGR_PROJECT_TIMING_NOUT 4" in open(os.path.join(ROOT, "include", "bwgr.h")).read()
    assert L.bwgr_debug_project_timing(1, out) == 0 and all(v >= 0.0 for v in out[:4]) and out[4] == -1.0
    assert L.bwgr_debug_project_timing(0, None) == 0
    assert L.bwgr_debug_project_timing(2, out) == 1 and b"project timing" in L.bwgr_last_error()


# ---- refusals that need no device ----

def test_python_refusals_come_before_the_library():
    code = """
import sys; sys.path.insert(0, %r)
import numpy as np
import bwgr_amd, bwgr_amd.mlm as M
from bwgr_amd import _lib, BwgrError
def no_lib(): raise AssertionError("the library was loaded")
_lib.lib = no_lib
Z = np.zeros((6, 4), np.int8); Y = np.zeros((6, 2)); X = np.ones((6, 1)); D = bwgr_amd.dense(np.zeros((6, 4)))
bad = [(lambda: M.MLM(Y, X, Z + 0.5), "dense(Z)"), (lambda: M.MLM(Y, X, Z.astype(float) + 300.0), "dense(Z)"),
       (lambda: M.MLM(Y, np.ones((5, 1)), Z), "nrow(X)"), (lambda: M.MLM(np.zeros((5, 2)), X, Z), "nrow(Y)"),
       (lambda: M.MLM(Y, np.ones((6, 0)), Z), "f = 0"), (lambda: M.MLM(Y, np.ones((6, 257)), D), "f = 257"),
       (lambda: M.MLM(np.zeros((6, 17)), X, Z), "k = 17"), (lambda: M.MLM(np.zeros((6, 0)), X, Z), "k = 0"),
       (lambda: M.MLM(Y, X, Z, maxit=-1), "maxit = -1"), (lambda: M.MLM(Y, X, D, block=16), "dense Z"),
       (lambda: M.MLM(Y, X, np.zeros(6, np.int8)), "n x p"),
       (lambda: M.project(Z + 0.25, X), "dense(Z)"), (lambda: M.project(Z, np.ones((7, 1))), "nrow(X)"),
       (lambda: M.project(D, np.ones((6, 300))), "f = 300"), (lambda: M.project(D, X, nwg=2), "dense Z")]
for i, (f, word) in enumerate(bad):
    try:
        f()
    except BwgrError as e:
        assert e.code == 1 and word in str(e), (i, word, e)
    else:
        raise SystemExit("case %%d was not refused" %% i)
""" % ROOT
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]


def test_c_entry_refusals_without_a_device():
    """what bwgr_mlm and bwgr_project refuse before they ask for a device: code 1 and a message that names the entry or the trait"""
    import ctypes as C
    from bwgr_amd import _lib
    L = _lib.lib()
    n, p, f, k = 40, 6, 2, 2
    rng = np.random.default_rng(5)
    Z = np.asfortranarray(rng.normal(size=(n, p))); X = np.asfortranarray(np.column_stack([np.ones(n), rng.normal(size=n)])); Y = np.asfortranarray(rng.normal(size=(n, k)))
    u = np.zeros((p, k), order="F"); its = C.c_int(); out = np.zeros((n, p), order="F")
    dp, vp = (lambda a: a.ctypes.data_as(_lib.c_d)), (lambda a: a.ctypes.data_as(C.c_void_p))

    def mlm(Z=Z, X=X, Y=Y, n=n, p=p, f=f, k=k, ldz=n, zloc=0, maxit=3, u=u, its=its):
        return L.bwgr_mlm(0, None, None if Z is None else vp(Z), zloc, n, p, ldz, None if X is None else dp(X), f, n, None if Y is None else dp(Y), k, maxit, -8.0, 1.1, 0,
                          None, None if u is None else dp(u), None, None, None, None, None, None, None if its is None else C.byref(its))

    def refused(rc, *words):
        msg = L.bwgr_last_error().decode()
        assert rc == 1 and all(w in msg for w in words), (rc, msg)

    refused(mlm(Z=None), "mlm", "null pointer"); refused(mlm(X=None), "null pointer"); refused(mlm(Y=None), "null pointer")
    refused(mlm(u=None), "null pointer"); refused(mlm(its=None), "null pointer")
    refused(mlm(f=0), "f = 0"); refused(mlm(f=257), "f = 257"); refused(mlm(k=0), "k = 0"); refused(mlm(k=17), "k = 17"); refused(mlm(maxit=-1), "maxit = -1")
    refused(mlm(ldz=n - 1), "mlm", "n = 40"); refused(mlm(zloc=7), "memloc"); refused(mlm(p=0), "p = 0")
    Xb = X.copy(order="F"); Xb[3, 1] = np.inf
    refused(mlm(X=Xb), "X[3, 1]", "not finite")
    Zb = Z.copy(order="F"); Zb[5, 2] = np.nan
    refused(mlm(Z=Zb), "Z[5, 2]", "not finite")
    Yb = Y.copy(order="F"); Yb[2:, 1] = np.nan                                      # two records, f = 2
    refused(mlm(Y=Yb), "trait 1", "n_t = 2", "f = 2")
    Xd = np.asfortranarray(np.column_stack([np.ones(n), np.ones(n)]))      # collinear over all rows: every trait's design fails the rank rule
    refused(mlm(X=Xd), "trait 0", "rank-deficient")
    lev = (np.arange(n) < 20).astype(float)                                # full rank over all rows, collinear on trait 1's rows (one level only)
    Xl = np.asfortranarray(np.column_stack([np.ones(n), lev])); Yl = Y.copy(order="F"); Yl[:20, 1] = np.nan
    refused(mlm(X=Xl, Y=Yl), "trait 1", "rank-deficient")

    def proj(Z=Z, X=X, f=f, out=out, ldo=n, oloc=0):
        return L.bwgr_project(0, None, None if Z is None else vp(Z), 0, n, p, n, None if X is None else dp(X), f, n, None if out is None else vp(out), oloc, ldo)
    refused(proj(out=None), "project", "null pointer"); refused(proj(Z=None), "project", "null pointer"); refused(proj(f=257), "f = 257")
    refused(proj(ldo=n - 1), "ldo"); refused(proj(oloc=5), "memloc"); refused(proj(X=Xb), "X[3, 1]"); refused(proj(Z=Zb), "Z[5, 2]")
    refused(proj(X=Xd), "all rows", "rank-deficient")


# ---- the tail header ----

def _fmt(v):
    return " ".join("%.17g" % x for x in np.asarray(v, np.float64).ravel())


def _tail_input():
    texts, raised, ks = [], 0, set()
    for name in ("k3_p65_f1", "k16_p200_f5", "k2_f256", "k1_p64_f2", "k5_shared_f4"):
        c = MC.CASES[name]
        Y, X, Z = MC.data(name)
        o = MC.ref(name, True)
        st, tr = o["start"], o["trace"]
        k, f = c["k"], c["f"]
        df0 = float(np.float32(1.1))
        iN = 1.0 / (st["nt"] - f)
        ve0 = st["vy"] * 0.5
        out = ["%d %d %d %.17g" % (k, f, len(tr), df0), _fmt(st["nt"]), _fmt(st["ssy"]), _fmt(st["Tr"]), _fmt(st["vy"]), _fmt(ve0),
               _fmt(np.diag(ve0 / (st["Tr"] * iN))), _fmt(ve0 * df0), _fmt(1.0 / (st["nt"] + df0 - f))]
        before = 0.0
        for t in tr:
            w = np.abs(np.linalg.eigvalsh(t["vb"]))
            with np.errstate(divide="ignore"):
                cnv = np.log10(t["db2"])
            out += [_fmt(t["ey"]), _fmt(t["TH"]), "%.17g" % t["db2"], _fmt(t["ve"]), _fmt(t["vb"]), _fmt(t["iG"]),
                    "%.17g %.17g %.17g" % (t["inflate"], cnv, w.max() / max(w.min(), 1e-300))]
            raised += t["inflate"] > before
            before = t["inflate"]
        out += [_fmt(o["h2"]), _fmt(o["GC"])]
        texts.append("\n".join(out)); ks.add(k)
    assert raised >= 3 and ks >= {1, 2, 3, 5, 16}
    return "%d\n" % len(texts) + "\n".join(texts) + "\n"


def test_tail_under_sanitizers(tmp_path):
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible: no sanitizer build runs on a GPU machine")
    cxx = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no C++ compiler with the AddressSanitizer and UBSan runtimes")
    exe, cases = str(tmp_path / "mlm_tail_check"), str(tmp_path / "cases.txt")
    built = subprocess.run([cxx] + FLAGS + ["-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "mlm_tail_check.cpp")], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    with open(cases, "w") as f:
        f.write(_tail_input())
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "" and run.stdout.strip() == "mlm_tail_check ok", (run.returncode, run.stdout, run.stderr[-2000:])


def test_tail_header_is_plain_cxx():
    txt = open(os.path.join(CSRC, "mlm_tail.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", txt) and "__global__" not in txt and "__device__" not in txt
    hip = open(os.path.join(CSRC, "bwgr_hip.hip")).read()
    assert '#include "mlm_tail.h"' in hip and '#include "project.hip.h"' in hip and '#include "mlm_host.hip.h"' in hip
