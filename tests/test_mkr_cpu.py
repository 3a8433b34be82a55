"""CPU: K2X's properties and refusals, the signatures of K2X and mkr, the dense train's plan (bwgr_debug_mrr_dense_plan) on every case of
tests/test_gpu_mkr.py, the refusals bwgr_mrr_dense makes before it asks for a device, and the restatement alone on every case."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mkr_cases as MC  # noqa: E402
import mrr_restatement as MR  # noqa: E402


def _k_grm():
    return MC.grm150()


def _k_full():
    A = np.random.default_rng(3).normal(size=(60, 90))
    return A @ A.T / 90 + np.eye(60)


def _k_indefinite():
    A = np.random.default_rng(4).normal(size=(50, 50))
    return (A + A.T) / 2


@pytest.mark.parametrize("make,npc", [(_k_grm, 149), (_k_full, 60), (_k_indefinite, 50)], ids=["grm", "full", "indefinite"])
def test_k2x_reproduces_k_squared(make, npc):
    """X = U[:, :NPC] diag(|lambda|) in float: n x NPC, columns by decreasing |lambda|, and X X' = K+ K+ (K+ = K without the dropped
    eigenvalues) within twice the float rounding of X's entries plus the eigensolver's own error."""
    import bwgr_amd
    K = make()
    w, V = np.linalg.eigh(K)
    aw = np.abs(w)
    # NPC is no rounding decision: every |eigenvalue| is far from MinEV = 1e-8
    assert np.all((aw >= 1e-4) | (aw <= 1e-12)), np.sort(aw)[:3]
    keep = aw > 1e-8
    assert int(keep.sum()) == npc
    X = bwgr_amd.K2X(K)
    assert X.shape == (K.shape[0], npc) and X.dtype == np.float64
    assert np.array_equal(X, X.astype(np.float32).astype(np.float64))          # float values
    norms = np.sqrt((X ** 2).sum(0))                                          # = |lambda| in decreasing order
    assert np.all(np.diff(norms) <= 1e-6 * norms[0])
    assert np.allclose(norms, np.sort(aw[keep])[::-1], rtol=1e-6, atol=0)
    Kp = (V[:, keep] * w[keep]) @ V[:, keep].T
    KK = Kp @ Kp
    d = np.sqrt(np.diag(KK))
    bound = 2.0 ** -22 * np.outer(d, d) + 1e-10 * np.abs(K @ K).max()
    err = np.abs(X @ X.T - KK)
    assert np.all(err <= bound), float((err / bound).max())
    # `cores` is ignored; a larger MinEV drops more
    assert np.array_equal(bwgr_amd.K2X(K, 1e-8, 4), X)
    assert bwgr_amd.K2X(K, MinEV=float(np.median(aw))).shape[1] == int((aw > np.median(aw)).sum())


def test_k2x_refusals():
    import bwgr_amd
    with pytest.raises(bwgr_amd.BwgrError, match="square"):
        bwgr_amd.K2X(np.zeros((4, 5)))
    with pytest.raises(bwgr_amd.BwgrError, match="square"):
        bwgr_amd.K2X(np.zeros(4))
    K = _k_full()
    K[2, 7] += 1e-3
    with pytest.raises(bwgr_amd.BwgrError, match="symmetric"):
        bwgr_amd.K2X(K)
    K = _k_full()
    K[2, 7] += 1e-9                 # within 1e-6 of the largest entry: taken
    assert bwgr_amd.K2X(K).shape == (60, 60)


def test_signatures_match_reference():
    """K2X(K, MinEV = 1e-8, cores = 1L), R/RcppExports.R:256; mkr = function(Y, K, ...) MRR3(Y, K2X(K), ...), R/mix.R:1275."""
    import bwgr_amd as B
    E = inspect.Parameter.empty
    P = inspect.Parameter

    def pos(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind == P.POSITIONAL_OR_KEYWORD]
    assert pos(B.K2X) == [("K", E), ("MinEV", 1e-8), ("cores", 1)]
    assert pos(B.mkr) == [("Y", E), ("K", E)]
    assert [p.kind for p in inspect.signature(B.mkr).parameters.values()][-1] == P.VAR_KEYWORD
    for name in ("K2X", "mkr", "mrr_dense_plan"):
        assert name in B.__all__ and hasattr(B, name)


def _shape(name):
    Y, X, _ = MC.case(name)
    k = 1 if Y.ndim == 1 else Y.shape[1]
    return X.shape[0], X.shape[1], k, MC.npat(Y)


@pytest.mark.parametrize("name", MC.ALL_CASES)
def test_plan_of_every_gpu_case(name):
    import bwgr_amd
    n, r, k, npat = _shape(name)
    pl = bwgr_amd.mrr_dense_plan(n, r, k, npat)
    assert pl["ld"] % 128 == 0 and 0 <= pl["ld"] - n < 128
    assert pl["nblk"] == -(-r // 64) and pl["edge"] == r - 64 * (pl["nblk"] - 1) and 1 <= pl["edge"] <= 64
    assert pl["tiles"] == pl["ld"] // 64 and pl["pass_wg"] == min(pl["tiles"], 32) and pl["trips"] == -(-pl["tiles"] // pl["pass_wg"])
    assert pl["cols_wg"] == min(-(-r // 4), 8192) and pl["hat_wg"] == -(-n // 256)
    assert 0 <= pl["ngl"] <= npat and pl["lds_solve"] <= 160 * 1024 and pl["lds_linv"] == 8 * 64 * k * k <= 160 * 1024
    assert pl["lds_gram"] <= 64 * 1024 and pl["lds_pass"] <= 64 * 1024
    assert pl["linv_lds"] == (1 if k < 16 else 0)
    # the solve stages whole 32 KB Gram matrices in what its fixed arrays and the inverses leave of 160 KB
    fixed = pl["lds_solve"] - 32768 * pl["ngl"]
    assert pl["ngl"] == min(npat, (160 * 1024 - fixed) // 32768)
    assert pl["ws_bytes"] >= 8 * (pl["ld"] * r + pl["nblk"] * npat * 4096 + 2 * k * pl["ld"])
    want = {
        "grm150": dict(nblk=3, edge=21, tiles=4, trips=1, ngl=3),
        "r1": dict(nblk=1, edge=1), "r64": dict(nblk=1, edge=64), "r65": dict(nblk=2, edge=1), "r130": dict(nblk=3, edge=2),
        "tall": dict(tiles=36, pass_wg=32, trips=2),
        "k1": dict(ngl=1), "k16": dict(linv_lds=0, ngl=3), "k4full": dict(ngl=1),
        # the row counts: beside one tile, beside ld = 128, the eight-at-a-time sum of the partials with and without a remainder, the last
        # single trip, a second trip that only workgroups 0 and 1 take, a third trip
        "n63": dict(ld=128, tiles=2, pass_wg=2, trips=1), "n64": dict(ld=128, tiles=2, pass_wg=2, trips=1),
        "n65": dict(ld=128, tiles=2, pass_wg=2, trips=1), "n127": dict(ld=128, tiles=2, pass_wg=2, trips=1),
        "n128": dict(ld=128, tiles=2, pass_wg=2, trips=1), "n129": dict(ld=256, tiles=4, pass_wg=4, trips=1),
        "n512": dict(ld=512, tiles=8, pass_wg=8, trips=1), "n513": dict(ld=640, tiles=10, pass_wg=10, trips=1),
        "n2048": dict(ld=2048, tiles=32, pass_wg=32, trips=1), "n2049": dict(ld=2176, tiles=34, pass_wg=32, trips=2),
        "n4100": dict(ld=4224, tiles=66, pass_wg=32, trips=3),
        "n2r1": dict(ld=128, tiles=2, pass_wg=2, trips=1, nblk=1, edge=1, cols_wg=1, hat_wg=1, ngl=1),
        "n3r2": dict(ld=128, tiles=2, pass_wg=2, trips=1, nblk=1, edge=2, cols_wg=1, hat_wg=1, ngl=1),
        "wide": dict(cols_wg=8192, nblk=513, edge=32, ld=256, tiles=4, trips=1),
    }.get(name, {})
    if name in MC.ROWS:
        want = dict(want, nblk=2, edge=6, ngl=2, linv_lds=1)
        assert (n, r, k, npat) == (MC.ROWS[name], 70, 2, 2)
    if name in MC.SMALLEST:
        assert (n, r, k, npat) == MC.SMALLEST[name] + (2, 1)
    if name == "wide":
        assert (n, r, k) == (130, 32800, 2) and r > 4 * pl["cols_wg"] and r - 4 * pl["cols_wg"] == 32     # columns 32 768 .. 32 799: a second trip
        assert pl["ws_bytes"] < 110e6
    if name in MC.SOLVE:
        ngl, reg = {"solve_k4p4": (3, 2), "solve_k7p7": (3, 2), "solve_k8p8": (2, 2), "solve_k11p11": (2, 2), "solve_k12p12": (1, 2),
                    "solve_k13p13": (1, 2), "solve_k14p14": (0, 3), "solve_k15p15": (0, 3), "solve_k15p1": (0, 3), "solve_k16p2": (2, 4)}[name]
        assert (n, r, k, npat) == (200, 70) + MC.SOLVE[name]
        want = dict(nblk=2, edge=6, tiles=4, trips=1, ngl=ngl, linv_lds=1 if k < 16 else 0)
        assert MC.regime(pl["linv_lds"], pl["ngl"], npat) == reg
    if name in MC.SHARED or name in MC.OPTION:
        ids = MC.SHARED.get(name, MC.SHARED["shared_k6"])
        assert (n, r, k, npat) == (200, 70, len(ids), max(ids) + 1)
        want = dict(nblk=2, edge=6, ngl={6: 3, 10: 2}[k], linv_lds=1)
        assert MC.regime(pl["linv_lds"], pl["ngl"], npat) == 2
        # one trait's Gram row comes from LDS and another's from global memory, and so do two neighbours'
        assert min(ids) < pl["ngl"] <= max(ids)
        assert any((ids[t] < pl["ngl"]) != (ids[t + 1] < pl["ngl"]) for t in range(k - 1))
        assert _pattern_ids(MC.case(name)[0]) == ids
    if name in MC.DEGENERATE:
        assert (n, r, k, npat) == (200, 70, 3, 3)
        want = dict(nblk=2, edge=6, tiles=4, ngl=3, linv_lds=1)
    for key, v in want.items():
        assert pl[key] == v, (key, pl)
    if name == "grm150":
        assert (n, r, npat) == (150, 149, 3)
    if name == "k16":
        assert npat == 16 and pl["ngl"] < npat
    if name == "k4full":
        assert npat == 1
    if name in ("TH", "updateMu", "XFA"):
        assert npat == 3 and k == 4          # two traits share a pattern


def _pattern_ids(Y):
    """the traits' pattern ids, numbered in order of first appearance (find_patterns)"""
    obs = ~np.isnan(Y)
    seen, ids = [], []
    for t in range(Y.shape[1]):
        key = obs[:, t].tobytes()
        if key not in seen:
            seen.append(key)
        ids.append(seen.index(key))
    return ids


def test_the_plan_table_of_the_solve():
    """linv_lds and the cap on ngl for every k, as DESIGN.md section 4.13 states them: 32 KB per pattern's Gram beside the fixed arrays and 64 k^2
    doubles of inverses in 160 KB"""
    import bwgr_amd
    for k in range(1, 17):
        pl = bwgr_amd.mrr_dense_plan(200, 70, k, k)
        cap = 3 if k <= 7 else 2 if k <= 11 else 1 if k <= 13 else 0 if k <= 15 else 3
        assert pl["linv_lds"] == (1 if k <= 15 else 0) and pl["ngl"] == min(k, cap), (k, pl)
        assert pl["lds_solve"] <= 160 * 1024


def test_the_cases_reach_every_regime():
    """all five regimes of k_mrrd_solve, regime 2 at ngl = 1, 2 and 3, and every option where ngl < npat"""
    import bwgr_amd
    reached = {}
    for name in MC.ALL_CASES:
        n, r, k, npat = _shape(name)
        pl = bwgr_amd.mrr_dense_plan(n, r, k, npat)
        reached.setdefault(MC.regime(pl["linv_lds"], pl["ngl"], npat), set()).add(pl["ngl"])
    assert sorted(reached) == [1, 2, 3, 4, 5], reached
    assert {1, 2, 3} <= reached[2] and reached[3] == {0}, reached
    for name in MC.OPTION:
        n, r, k, npat = _shape(name)
        assert bwgr_amd.mrr_dense_plan(n, r, k, npat)["ngl"] < npat


def test_the_degenerate_cases_are_what_they_say():
    Y, X, _ = MC.case("deg_const_cols")
    assert np.all(X[:, 5] == 2.5) and np.all(X[:, 66] == 0.0)
    o = MR.mrr(Y, X, maxit=10)
    assert np.all(o["b"][[5, 66]] == 0.0) and np.count_nonzero(o["b"]) == 68 * 3
    Y, X, _ = MC.case("deg_const_on_trait")
    on = ~np.isnan(Y[:, 1])
    assert np.all(X[on, 17] == 1.0) and not np.any(X[~on, 17] == 1.0) and 0 < (~on).sum()
    Y, X, _ = MC.case("deg_dead_rows")
    seen = (~np.isnan(Y)).any(1)
    assert not seen[10:75].any() and seen[:10].all() and seen[75:128].all()      # tile 0 keeps ten rows, tile 1 loses its first eleven
    Y, X, _ = MC.case("deg_dead_tile")
    seen = (~np.isnan(Y)).any(1)
    assert not seen[64:128].any() and seen[:64].any() and seen[128:].any()
    Y, X, _ = MC.case("deg_scales")
    sd = X.std(0)
    assert 20 < sd.max() / sd.min() < 1e4
    Y, X, opts = MC.case("deg_default_tol")
    assert opts == {}
    assert 3 <= MR.mrr(Y, X)["Its"] < 500


def test_plan_refusals():
    import bwgr_amd
    for bad in [(1, 10, 2, 1), (10, 0, 2, 1), (10, 10, 0, 1), (10, 10, 17, 1), (10, 10, 3, 0), (10, 10, 3, 4)]:
        with pytest.raises(bwgr_amd.BwgrError, match="mrr_dense plan"):
            bwgr_amd.mrr_dense_plan(*bad)


def test_refusals_before_the_device():
    """what bwgr_mrr_dense refuses of its arguments needs no GPU, and names the argument"""
    import bwgr_amd as B
    rng = np.random.default_rng(5)
    X = rng.normal(size=(40, 6))
    Y = rng.normal(size=(40, 2))
    with pytest.raises(B.BwgrError, match="k = 17"):
        B.mrr(rng.normal(size=(40, 17)), B.dense(X))
    with pytest.raises(B.BwgrError, match="nrow"):
        B.mrr(Y[:39], B.dense(X))
    Xn = X.copy()
    Xn[3, 4] = np.nan
    with pytest.raises(B.BwgrError, match=r"X\[3, 4\]"):
        B.mrr(Y, B.dense(Xn))
    with pytest.raises(B.BwgrError, match="r = 0"):
        B.mrr(Y, B.dense(np.zeros((40, 0))))
    with pytest.raises(B.BwgrError, match="n = 1"):
        B.mrr(Y[:1], B.dense(X[:1]))
    with pytest.raises(B.BwgrError, match="InnerGS"):
        B.mrr(Y, B.dense(X), InnerGS=True)
    with pytest.raises(B.BwgrError, match="NonLinearFactor"):
        B.mrr_float(Y, B.dense(X), NonLinearFactor=0.5)
    with pytest.raises(B.BwgrError, match="dense design"):
        B.mrr(Y, B.dense(X), nwg=3)
    # a plain float matrix is not taken for a dense design: it goes the panel's way, which has no place for these values
    with pytest.raises(Exception) as ei:
        B.mrr(Y, X)
    assert "mrr_dense" not in str(ei.value)


@pytest.mark.parametrize("name", MC.ALL_CASES)
def test_restatement_alone(name):
    """the reference of the GPU tests stays finite and runs at least three sweeps on every case"""
    Y, X, opts = MC.case(name)
    o = MR.mrr(Y, X, **opts)
    assert o["Its"] >= 3, o["Its"]
    for key in ("mu", "b", "hat", "h2", "GC", "vb", "ve", "MSx", "cnvB", "cnvH2", "cnvV"):
        assert np.all(np.isfinite(o[key])), key
    assert len(o["cnvB"]) == o["Its"]
    if name in MC.NEW_CASES and "maxit" in opts:          # every sweep of its maxit: no early stop hides a sweep from the comparison
        assert o["Its"] == opts["maxit"]
