"""CPU: mrr_svd and the transpose product X'A without a GPU -- the host tail (bwgr_amd/csrc/mrr_svd_tail.h) as a program of its own under
AddressSanitizer and UBSan against tests/mrr_svd_restatement.py; the plan of bwgr_panel_xta at the edges of every case of tests/mrr_svd_cases.py;
the surface (header, ABI table, bwgr_amd.svd without torch, the refusals made before the library loads); and the case table's soundness: every
fit's restatement is stable against a perturbation of its design, and the rank rule separates the kept from the dropped directions."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrr_svd_cases as MC  # noqa: E402
import mrr_svd_restatement as SR  # noqa: E402
from test_devbufs_cpu import CSRC, FLAGS, ROOT, _sanitizing_compiler  # noqa: E402

KEYS = ("mu", "b", "hat", "h2", "GC", "vb", "ve", "cnvB", "cnvH2", "cnvV")


# ---- the tail header ----

def _fmt(v):
    return " ".join("%.17g" % x for x in np.asarray(v, np.float64).ravel())


def _tail_sweep(TH, Tr):
    vb, iG, bent, lam = SR.tail(TH, Tr)
    w = np.abs(np.linalg.eigvalsh(vb))
    return [_fmt(TH), _fmt(Tr), _fmt(vb), _fmt(iG), "%d %.17g %.17g" % (int(bent), lam, w.max() / max(w.min(), 1e-300))], vb, bent


def _tail_case(rng, k, sweeps):
    """a case's text from (TH, Tr) pairs; returns (text, how many sweeps bent)"""
    nt = rng.integers(5, 200, k).astype(float)
    vy, MSx = rng.uniform(0.5, 3.0, k), rng.uniform(1.0, 50.0, k)
    ve = vy * 0.5
    out = ["%d %d" % (k, len(sweeps)), _fmt(nt), _fmt(vy), _fmt(MSx), _fmt(ve), _fmt(np.diag(ve / MSx)), _fmt(np.diag(MSx / ve)), _fmt(1 - ve / vy),
           _fmt(1 / (nt - 1))]
    nbent, vb = 0, np.eye(k)
    for TH, Tr in sweeps:
        lines, vb, bent = _tail_sweep(TH, Tr)
        out += lines
        nbent += int(bent)
    db2, h20, h2 = rng.uniform(1e-9, 1e-3, k), rng.uniform(0.1, 0.9, k), rng.uniform(0.1, 0.9, k)
    vb0 = vb + rng.normal(size=(k, k)) * 1e-3
    vbp = vb + np.eye(k) * (abs(np.linalg.eigvalsh(vb).min()) + 0.1)          # a positive diagonal for the correlations
    cnv = [np.log10(db2.sum()), np.log10(((h20 - h2) ** 2).sum()), np.log10(((vb0 - vbp) ** 2).sum())]
    sd = np.sqrt(np.diag(vbp))
    out += [_fmt(db2), _fmt(h20), _fmt(h2), _fmt(vb0), _fmt(vbp), _fmt(cnv), _fmt(vbp / np.outer(sd, sd))]
    return "\n".join(out), nbent


def _tail_input():
    rng = np.random.default_rng(20230423)
    texts, bent, ks = [], 0, set()
    for name in ("k3_r65", "k16_r149", "k1_r64_converges"):          # what the fits' sweeps left
        tr = MC.engine_ref(name)[2]["trace"][:12]
        t, nb = _tail_case(rng, MC.FIT[name]["k"], [(r["TH"], r["Tr"]) for r in tr])
        texts.append(t); bent += nb; ks.add(MC.FIT[name]["k"])
    for k in (1, 2, 5, 16):                                          # random TildeHat / Tr: about half of them bend for k > 1
        sweeps = []
        for _ in range(8):
            B = rng.normal(size=(k, k))
            TH = B @ B.T * rng.uniform(0.2, 2.0) + rng.normal(size=(k, k)) * (0.8 if k > 1 else 0.0)
            sweeps.append((TH, rng.uniform(5.0, 500.0, k)))
        t, nb = _tail_case(rng, k, sweeps)
        texts.append(t); bent += nb; ks.add(k)
    assert bent >= 5 and ks >= {1, 2, 3, 5, 16}
    return "%d\n" % len(texts) + "\n".join(texts) + "\n"


def test_tail_under_sanitizers(tmp_path):
    import bwgr_amd
    if bwgr_amd.device_count() > 0:
        pytest.skip("a GPU is visible: no sanitizer build runs on a GPU machine")
    cxx = _sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no C++ compiler with the AddressSanitizer and UBSan runtimes")
    exe, cases = str(tmp_path / "mrr_svd_tail_check"), str(tmp_path / "cases.txt")
    built = subprocess.run([cxx] + FLAGS + ["-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "mrr_svd_tail_check.cpp")], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    with open(cases, "w") as f:
        f.write(_tail_input())
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "" and run.stdout.strip() == "mrr_svd_tail_check ok", (run.returncode, run.stdout, run.stderr[-2000:])


def test_tail_header_is_plain_cxx():
    txt = open(os.path.join(CSRC, "mrr_svd_tail.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", txt) and "__global__" not in txt and "__device__" not in txt
    assert '#include "mrr_svd_tail.h"' in open(os.path.join(CSRC, "bwgr_hip.hip")).read()


# ---- the plan of bwgr_panel_xta ----

@pytest.mark.parametrize("name", list(MC.XTA))
def test_xta_plan_edges(name):
    from bwgr_amd import svd
    c = MC.XTA[name]
    n, p = c["n"], c["p"]
    R = MC.slab_rows(n, p, c["block"])
    assert R % 128 == 0
    slabs = -(-n // R)
    for k in MC.XTA_K:
        pl = svd.xta_plan(n, p, k, R)
        assert pl["groups"] == -(-k // 16) and pl["cols_wg"] == 64 and pl["cols_wave"] == 16 and pl["row_tile"] == 128
        nblk = -(-p // pl["cols_wg"])
        assert pl["grid"] == min(nblk, 1024) and pl["trips"] == -(-nblk // pl["grid"]) and pl["grid"] * pl["trips"] >= nblk
        assert pl["tiles"] * pl["row_tile"] == slabs * R >= n and R % pl["row_tile"] == 0
        assert pl["lds_bytes"] == 128 * 18 * 8 <= 64 * 1024
        assert pl["ws_bytes"] == 8 * (pl["groups"] * 16 * slabs * R + pl["groups"] * 16)
    # what each case is in the table for
    if name == "two_slabs":
        assert n % 64 != 0 and slabs == 2 and p % 64 != 0
    if name == "tall_slab":
        assert R == 1024 and slabs == 2
    if name == "padded_slab":
        assert slabs == 1 and R > n
    if name == "two_trips":
        assert svd.xta_plan(n, p, 1, R)["trips"] == 2 and -(-p // 64) == 1025
    if name == "int8_codes":
        W = MC.xta_W(name)
        assert W.min() == -128 and W.max() == 127 and sum(len(set(W[:, j])) == 1 for j in range(p)) >= 5


def test_xta_plan_refusals():
    from bwgr_amd import svd, BwgrError
    for bad in ((0, 5, 1, 128), (5, 0, 1, 128), (5, 5, 0, 128), (5, 5, 1, 64), (5, 5, 1, 192), (5, 5, 1, 8192), (5, 5, 65535 * 16 + 1, 128)):
        with pytest.raises(BwgrError):
            svd.xta_plan(*bad)
    assert svd.xta_plan(5, 5, 65535 * 16, 128)["groups"] == 65535


# ---- the surface ----

def test_header_and_abi_table():
    from bwgr_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_abi_table_cpu import prototypes
    protos = prototypes()
    assert protos["bwgr_panel_xta"] == ("int", ["pointer", "pointer", "int64_t", "int64_t", "int", "int", "pointer", "int64_t"])
    assert protos["bwgr_debug_xta_plan"] == ("int", ["int64_t"] * 4 + ["pointer"])
    assert protos["bwgr_mrr_svd_fit"] == ("int", ["int", "pointer", "int", "int64_t", "int64_t", "int64_t", "pointer", "int", "int", "double", "int"] + ["pointer"] * 11)
    for name in ("bwgr_panel_xta", "bwgr_debug_xta_plan", "bwgr_mrr_svd_fit"):
        assert len(_lib.ABI[name]) == len(protos[name][1]) and hasattr(_lib.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "bwgr.h")).read()
    assert "#define BWGR_XTA_PLAN_NOUT 9" in hdr


def test_svd_imports_without_torch_and_keeps_the_package_surface():
    code = ("import sys; sys.path.insert(0, %r); import bwgr_amd.svd as S; import bwgr_amd; "
            "assert not hasattr(bwgr_amd.Panel, 'xta') and 'mrr_svd' not in bwgr_amd.__all__; "
            "sys.exit(1 if 'torch' in sys.modules else 0)" % ROOT)
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0


def test_wmodel_keys_and_signatures():
    from bwgr_amd import svd
    assert svd.WMODEL_KEYS == SR.WMODEL_KEYS == ("Intercepts", "MarkerEffects", "FittedValues", "Heritability", "WCorrelations", "VarBeta", "VarResiduals",
                                                 "ConvergenceBeta", "ConvergenceH2", "ConvergenceVar", "NumOfIterations")
    sig = inspect.signature(svd.mrr_svd)
    assert list(sig.parameters)[:2] == ["Y", "W"]
    assert all(q.kind in (q.KEYWORD_ONLY, q.VAR_KEYWORD) for q in list(sig.parameters.values())[2:])
    assert sig.parameters["maxit"].default == 500 and sig.parameters["tol"].default == 10e-9
    sig = inspect.signature(svd.panel_xta)
    assert list(sig.parameters)[:3] == ["X", "A", "centre"] and sig.parameters["centre"].default is True
    assert sig.parameters["device_out"].kind == inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(svd.xta_plan).parameters) == ["n", "p", "k", "slab_rows"]


def test_python_refusals_come_before_the_library():
    """shape mismatches, dense(W) and a non-integer W are refused where no library can be loaded"""
    code = """
import sys; sys.path.insert(0, %r)
import numpy as np
import bwgr_amd, bwgr_amd.svd as S
from bwgr_amd import _lib, BwgrError
def no_lib(): raise AssertionError("the library was loaded")
_lib.lib = no_lib
W = np.zeros((6, 4), np.int8)
bad = [lambda: S.mrr_svd(np.zeros((5, 2)), W), lambda: S.mrr_svd(np.zeros((6, 2)), bwgr_amd.dense(np.zeros((6, 4)))),
       lambda: S.mrr_svd(np.zeros((6, 2)), W + 0.5), lambda: S.mrr_svd(np.zeros((6, 2)), W.astype(float) + 300.0),
       lambda: S.svd_design(bwgr_amd.dense(np.zeros((6, 4)))), lambda: S.svd_design(W + 0.25),
       lambda: S.panel_xta(W, np.zeros(5)), lambda: S.panel_xta(W, np.zeros((7, 2))), lambda: S.panel_xta(W + 0.5, np.zeros(6)),
       lambda: S.panel_xta(bwgr_amd.dense(np.zeros((6, 4))), np.zeros(6)), lambda: S.panel_xta(np.zeros(6, np.int8), np.zeros(6))]
for i, f in enumerate(bad):
    try:
        f()
    except BwgrError as e:
        assert e.code == 1, (i, e)
    else:
        raise SystemExit("case %%d was not refused" %% i)
""" % ROOT
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]


# ---- the case table ----

def test_case_table_covers_what_it_is_for():
    rs = {name: MC.engine_ref(name)[1].shape[1] for name in MC.FIT}
    assert {64, 65, 128, 129} <= set(rs.values())
    ks = {c["k"] for c in MC.FIT.values()}
    assert 1 in ks and 16 in ks
    pats = {name: MC.npat(MC.data(name)[1]) for name in MC.FIT}
    assert pats["k5_shared"] == 1 and MC.FIT["k5_shared"]["k"] == 5 and pats["k16_r149"] == 16 and pats["k3_r65"] == 3
    assert any(any(t["bent"] for t in MC.engine_ref(name)[2]["trace"]) for name in MC.FIT)
    assert rs["k16_p_lt_n"] == MC.FIT["k16_p_lt_n"]["p"] < MC.FIT["k16_p_lt_n"]["n"]
    for name, c in MC.FIT.items():
        its = MC.engine_ref(name)[2]["Its"]
        assert (3 <= its < c["maxit"]) if name.endswith("converges") else (its == c["maxit"] <= 40), (name, its)
    assert set(MC.DRIVER) <= set(MC.FIT)


@pytest.mark.parametrize("name", list(MC.FIT))
def test_case_is_sound(name):
    """the restatement of every case is stable: a relative perturbation of 2^-40 of the design moves every compared output by less than 1e-9"""
    Y, X, o = MC.engine_ref(name)
    rng = np.random.default_rng(0)
    o2 = SR.fit(Y, X * (1.0 + 2.0 ** -40 * rng.choice([-1.0, 1.0], X.shape)), maxit=MC.FIT[name]["maxit"])
    assert o2["Its"] == o["Its"]
    moves = {k: SR.scaled_err(o2[k], o[k]) for k in KEYS}
    print(name, {k: "%.1e" % v for k, v in moves.items()})
    assert all(np.all(np.isfinite(o[k])) for k in KEYS)
    assert max(moves.values()) < 1e-9, moves


@pytest.mark.parametrize("name", list(MC.FIT))
def test_rank_rule_separates(name):
    """the smallest kept singular value is at least 100 x the threshold, the largest dropped one at most a tenth of it; the eigh design and the SVD
    design keep the same directions"""
    W, _ = MC.data(name)
    n, p = W.shape
    De, Ds = SR.design_eigh(W), SR.design_svd(W)
    thr = np.sqrt(De["lam"][0]) * SR.rank_factor(n, p)
    r = De["r"]
    assert r == Ds["r"] == min(n - 1, p)
    assert De["d"][-1] >= 100 * thr
    if r < n:
        assert np.sqrt(np.abs(De["lam"][r:]).max()) <= 0.1 * thr
    assert SR.scaled_err(De["d"], Ds["d"]) <= 1e-10
    from bwgr_amd import svd
    assert svd.rank_threshold(n, p) == SR.rank_factor(n, p) ** 2


def test_restatement_identities():
    """V b = W_c'(U (b / d)), and W_c beta + mu = hat: what the driver's back-map and the GPU identities rest on"""
    W, Y, o = MC.driver_ref("k3_r65")
    D = SR.design_svd(W)
    f = SR.fit(Y, D["X"], maxit=MC.FIT["k3_r65"]["maxit"])
    beta = D["Wc"].T @ (D["U"] @ (f["b"] / D["d"][:, None]))
    assert SR.scaled_err(beta, o["MarkerEffects"]) <= 1e-10
    assert SR.scaled_err(D["Wc"] @ o["MarkerEffects"] + o["Intercepts"], o["FittedValues"]) <= 1e-10
    assert tuple(o) == SR.WMODEL_KEYS


def test_asum_restates_the_device_order():
    A = np.random.default_rng(3).normal(size=(700, 3))
    s = SR.asum(A)
    assert np.allclose(s, A.sum(0), rtol=1e-13) and s.shape == (3,)
    part = [sum(A[q::256, 1][i] for i in range(len(A[q::256, 1]))) for q in range(256)]
    tot = 0.0
    for q in range(256):
        tot = tot + part[q]
    assert tot == s[1]
