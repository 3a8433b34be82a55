"""GPU: what the handles and the one-call entry points own on the device comes and goes with them.

Every handle (panel data, panel, chain, group) and every call holds its device arrays, streams and long-lived events in one holder
(bwgr_amd/csrc/devbufs.h); bwgr_amd.debug_live() counts what the holders of this process own.  These tests assert on those counts and on
status codes only -- on the tpod panel (196 x 376 int8: three 128-marker blocks, one slab); the parity of the results is the other GPU
tests' job, and the failure paths of the holder run on the CPU (test_devbufs_cpu.py).  The multi-trait fits stand in both tables with a
sparse effect beside the panel: what a call's effects own goes with the call, also when it is refused on the device after they exist."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL = 1


def live():
    import bwgr_amd
    gc.collect()   # (a handle some earlier test dropped without closing goes now, not in the middle of a count)
    return bwgr_amd.debug_live()


def _above(now, start):
    return all(a > b for a, b in zip(now, start))


def _family(tpod, monkeypatch):
    """Root panel, BayesB chain alone on it (k_sweep3 at the shipped gate, its range snapshot, the variates drawn ahead on their stream
    between their two events); then a clone with a BayesA chain (the affine engine's winv / qsumw); then a fresh panel, implicitly centred,
    with a BayesC chain (csum / xxc, cpre).  Returns the counts at the start, while everything is alive, and after the teardown."""
    import bwgr_amd
    monkeypatch.delenv("BWGR_ENG3_THR", raising=False)   # the shipped engine gate (read when a panel is made)
    y, X = tpod["y"], tpod["gen"]
    start = live()
    root = bwgr_amd.Panel(X)
    c_root = bwgr_amd.Chain(root, "BayesB", y, it=3, bi=1, seed=11)
    before_run = live()
    c_root.run(3)
    c_root.sync()
    after_run = live()
    # the range snapshot (e, b, d, vb: four arrays) and the draws group (one array, one stream, two events), each taken whole.  The events of
    # the sweep path, by rule: two (a timing pair) per sweep launched since the chain's last sweep_ms, up to the pool's 2048 pairs; one guard
    # event per handle whose sweeps went through the occupancy guard; one hand-over event per handle that has been handed from one stream to
    # another (none here).  Three sweeps and the root's guard event beside the two of the draws group: 2 + 3 * 2 + 1.
    assert after_run == (before_run[0] + 5, before_run[1] + 1, before_run[2] + 9), (before_run, after_run)
    clone = root.clone()
    c_clone = bwgr_amd.Chain(clone, "BayesA", y, it=3, bi=1, seed=12)
    before_run = live()
    c_clone.run(3)
    c_clone.sync()
    # winv and qsumw, and the range snapshot of the fixed-point streamers; no draws ahead beside another handle.  Events: three timing pairs
    # and the clone's guard event, 3 * 2 + 1
    assert live() == (before_run[0] + 6, before_run[1], before_run[2] + 7), (before_run, live())
    cen = bwgr_amd.Panel(X)
    before_cen = live()
    cen.set_centred(True)
    assert live()[0] == before_cen[0] + 2   # csum and xxc, together
    cen.set_centred(True)
    assert live()[0] == before_cen[0] + 2   # ... once
    c_cen = bwgr_amd.Chain(cen, "BayesC", y, it=3, bi=1, seed=13)
    c_cen.run(3)
    c_cen.sync()
    peak = live()
    assert _above(peak, start), (start, peak)
    for c in (c_root, c_clone, c_cen):
        c.close()
    clone.close()
    root.close()
    assert _above(live(), start)   # (the centred panel is still there)
    cen.close()
    return start, peak, live()


def test_family_made_run_and_torn_down(tpod, monkeypatch):
    start, peak, end = _family(tpod, monkeypatch)
    assert end == start, (start, peak, end)
    start2, peak2, end2 = _family(tpod, monkeypatch)
    assert start2 == start and peak2 == peak and end2 == start, (start, peak, end, start2, peak2, end2)


def test_timing_pairs_are_reused(tpod):
    """A chain's timing pairs are made as its sweeps reach new slots of the pool, and handed out again after every sweep_ms."""
    import bwgr_amd
    y, X = tpod["y"], tpod["gen"]
    start = live()
    P = bwgr_amd.Panel(X)
    ch = bwgr_amd.Chain(P, "BayesC", y, it=8, bi=1, seed=41)
    ch.run(3)
    ch.sync()
    held = live()
    ms, launches = ch.sweep_ms()
    assert launches == 3 and np.isfinite(ms) and ms > 0, (ms, launches)
    assert live() == held   # read and kept
    ch.run(3)
    ch.sync()
    assert live() == held   # the same three pairs again: nothing grows
    ch.run(2)
    assert ch.sweep_ms()[1] == 5
    ch.close()
    P.close()
    assert live() == start


FOLD_IT = 2048 + 52   # the pool's capacity (bwgr_amd/csrc/devbufs.h, EventPairs::kCapacity) and some


def test_timing_pairs_fold_at_the_capacity(tpod):
    """More sweeps than the pool has pairs, with no sweep_ms in between: the library reads the full pool itself (the fold) and hands the same pairs
    out again, so the live events stay within the capacity, the launches are counted across the fold, and the chain is the one it is
    when its timing is read every 100 iterations."""
    import bwgr_amd
    y, X = tpod["y"], tpod["gen"]
    start = live()
    P = bwgr_amd.Panel(X)
    kw = dict(it=FOLD_IT, bi=100, seed=43)
    ch = bwgr_amd.Chain(P, "BayesC", y, **kw)
    before = live()
    ch.run(FOLD_IT)
    ch.sync()
    after = live()
    # at most the pool, and the handle's guard event (no hand-over here) and the two events of its draws group
    assert before[2] < after[2] <= before[2] + 2 * 2048 + 1 + 0 + 2, (before, after)
    ms, launches = ch.sweep_ms()
    assert launches == FOLD_IT and np.isfinite(ms) and ms > 0, (ms, launches)
    b_whole = ch.result()["b"]
    ch.close()
    ch = bwgr_amd.Chain(P, "BayesC", y, **kw)
    total = 0
    for _ in range(FOLD_IT // 100):
        ch.run(100)
        total += ch.sweep_ms()[1]
    assert total == FOLD_IT
    b_parts = ch.result()["b"]
    ch.close()
    P.close()
    assert np.array_equal(b_whole, b_parts)
    assert live() == start


def _incidence(n, q):
    """row r on level r mod q"""
    A = np.zeros((n, q))
    A[np.arange(n), np.arange(n) % q] = 1.0
    return A


def test_refused_call_owns_nothing_new(tpod):
    import bwgr_amd
    y, X = tpod["y"], tpod["gen"]
    rng = np.random.default_rng(5)
    start = live()
    P = bwgr_amd.Panel(X)
    ch = bwgr_amd.Chain(P, "BayesB", y, it=3, bi=1, seed=3)
    held = live()
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        P.close()
    assert ei.value.code == EINVAL and live() == held
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.mrr(rng.standard_normal((X.shape[0], 17)), P, maxit=2)
    assert ei.value.code == EINVAL and live() == held
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.uvbeta(rng.standard_normal((X.shape[0], 2)), P, 7, maxit=2)   # (an integer variant reaches the library)
    assert ei.value.code == EINVAL and "variant" in str(ei.value) and live() == held
    ch.close()
    # a sparse effect beside the panel: one refusal found on the host, while the matrix is checked, and one found on the device, after the
    # effect's arrays exist (a constant column: TrXSX = 0).  A fit that ran before them has left P whatever scratch its sweeps keep.
    n = X.shape[0]
    A = _incidence(n, 12)
    Y = rng.standard_normal((n, 2))
    assert bwgr_amd.PEGSZ(Y, [P, bwgr_amd.sparse(A)], maxit=1)["numit"] == 1
    held = live()
    rows, cols = np.nonzero(A.T)[::-1]
    ptr = np.concatenate([[0], np.cumsum(A.sum(0))]).astype(np.int64)
    dup = rows.astype(np.int32)
    dup[1] = dup[0]
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.PEGSZ(Y, [P, bwgr_amd.sparse((np.ones(len(dup)), dup, ptr), shape=A.shape)], maxit=2)
    assert ei.value.code == EINVAL and live() == held, (held, live())
    with pytest.raises(bwgr_amd.BwgrError) as ei:
        bwgr_amd.PEGSZ(Y, [P, bwgr_amd.sparse(np.ones((n, 1)))], maxit=2)
    assert ei.value.code == EINVAL and live() == held, (held, live())
    P.close()
    assert live() == start


def test_one_call_entry_points_give_back_what_they_took(tpod):
    import bwgr_amd
    y, X = tpod["y"], tpod["gen"]
    n, p = X.shape
    rng = np.random.default_rng(6)
    use = np.sort(rng.choice(n, 120, replace=False))
    e = (y - y.mean()).astype(np.float32)
    xx_use = (X[use].astype(np.float64) ** 2).sum(0)
    A, Y2 = _incidence(n, 12), rng.standard_normal((n, 2))
    X2 = np.column_stack([np.ones(n), rng.standard_normal(n)])
    start = live()
    P = bwgr_amd.Panel(X)
    calls = {
        "emRR": lambda: bwgr_amd.emRR(y, P, maxit=2),
        "emBB": lambda: bwgr_amd.emBB(y, P, maxit=2),
        "mrr": lambda: bwgr_amd.mrr(rng.standard_normal((n, 2)), P, maxit=2),
        "uvbeta": lambda: bwgr_amd.uvbeta(rng.standard_normal((n, 3)), P, "D", maxit=2, xb=True),
        "GRM": lambda: bwgr_amd.GRM(P),
        "KMUP2": lambda: bwgr_amd.KMUP2(P, use, np.zeros(p), np.ones(p), xx_use, e, np.ones(p), 1.0, 0.0, seed=7, it=1),
        "wgr": lambda: bwgr_amd.wgr(y, P, it=6, bi=2, bag=0.8, seed=8),
        # the multi-trait fits with a sparse effect: its arrays (both copies of the matrix, XX, XSX, tilde, b, d2, Linv, the order) are the call's
        "PEGSZ": lambda: bwgr_amd.PEGSZ(Y2, [P, bwgr_amd.sparse(A)], maxit=2),
        "PEGSX": lambda: bwgr_amd.PEGSX(Y2, X2, [P, bwgr_amd.sparse(A)], maxit=2),
        "PEGS_sparse": lambda: bwgr_amd.PEGS_sparse(Y2, A, maxit=2),      # (no panel: nothing is kept)
    }
    # The calls that do not sweep on P itself give everything back the first time.  A sweep on P may leave the PANEL arrays that it keeps (the
    # scratch that comes with the first sweep that needs it: never a stream or an event here, where P is not alone in a chain of its own), so
    # those calls are counted exactly the second time.
    for name, call in calls.items():
        before = live()
        call()
        first = live()
        if name in ("emRR", "mrr", "uvbeta", "GRM", "PEGS_sparse"):
            assert first == before, (name, before, first)
        assert first[0] >= before[0] and first[1:] == before[1:], (name, before, first)
        call()
        assert live() == first, (name, first, live())
    P.close()
    assert live() == start


def test_pair_run(tpod):
    import bwgr_amd
    y, X = tpod["y"], tpod["gen"]
    start = live()
    root = bwgr_amd.Panel(X)
    clone = root.clone()
    c0 = bwgr_amd.Chain(root, "BayesC", y, it=14, bi=1, seed=21)
    c1 = bwgr_amd.Chain(clone, "BayesC", y, it=14, bi=1, seed=22)
    before = live()
    c0.run_pair(c1, 3)
    c0.sync(); c1.sync()
    assert live()[1] == before[1] + 1, (before, live())   # the pair stream, which lives in the data

    def rest_of_cycle():
        """... of: a pair run, one iteration of each chain alone (each handle back on its own stream), a second pair run (onto the pair's again)"""
        assert c0.sweep_ms()[1] == 3 and c1.sweep_ms()[1] == 3   # both chains time the launch they share
        c0.run(1); c1.run(1)
        c0.run_pair(c1, 3)
        c0.sync(); c1.sync()
        assert c0.sweep_ms()[1] == 4 and c1.sweep_ms()[1] == 4
        return live()
    first = rest_of_cycle()
    # by now each handle has its hand-over event and its guard event, and each chain four timing pairs (the rule of _family; no draws ahead
    # beside a clone): the second cycle makes nothing
    assert first[1:] == (before[1] + 1, before[2] + 2 * 4 * 2 + 2 + 2), (before, first)
    c0.run_pair(c1, 3)
    c0.sync(); c1.sync()
    assert rest_of_cycle() == first
    c0.close(); c1.close()
    clone.close()
    assert live()[1] >= start[1] + 1   # ... and outlives the clone
    root.close()
    assert live() == start


def test_a_pair_that_forms_again_takes_an_idle_pair_stream(tpod):
    """Two pairs on one resident panel, each on a pair stream of its own.  A pair whose handles both went back to their own streams takes a pair
    stream that nobody is on when it forms again -- no new one, while the other pair keeps running on its own -- and every chain stays the
    chain it is alone."""
    import bwgr_amd
    y, X = tpod["y"], tpod["gen"]
    start = live()
    root = bwgr_amd.Panel(X)
    handles = [root] + [root.clone() for _ in range(3)]
    kw = dict(it=7, bi=1)
    solo = []
    for i, h in enumerate(handles):
        ch = bwgr_amd.Chain(h, "BayesC", y, seed=50 + i, **kw)
        ch.run(7)
        solo.append(ch.state())
        ch.close()
    c = [bwgr_amd.Chain(h, "BayesC", y, seed=50 + i, **kw) for i, h in enumerate(handles)]
    before = live()
    c[0].run_pair(c[1], 2); c[2].run_pair(c[3], 2)
    assert live()[1] == before[1] + 2   # a pair stream each
    for k in range(2):
        a, b = (0, 2) if k == 0 else (2, 0)   # pair a leaves and forms again while pair b runs on
        c[a].run(1); c[a + 1].run(1)
        c[b].run_pair(c[b + 1], 1)
        c[a].run_pair(c[a + 1], 1)
        c[b].run_pair(c[b + 1], 1 if k == 0 else 2)
        for ch in c:
            ch.sync()
        assert live()[1] == before[1] + 2, (k, before, live())
    c[2].run(1); c[3].run(1)
    for ch, want in zip(c, solo):
        got = ch.state()
        assert ch.sweep_ms()[1] == 7
        assert np.array_equal(got["b"], want["b"]) and np.array_equal(got["d"], want["d"]) and np.array_equal(got["e"], want["e"])
        ch.close()
    for h in handles[::-1]:
        h.close()
    assert live() == start


def test_group_of_two_shards_on_one_device(tpod):
    import bwgr_amd
    y, X = tpod["y"], tpod["gen"]
    start = live()
    g = bwgr_amd.Group("BayesB", y.astype(np.float32), X, devices=[0, 0], it=3, bi=1, pi=0.95, seed=31, centre=True)
    assert g.implicit_centring and g.info()["rccl"] == 0 and g.info()["devices"] == 2
    g.run(3)
    g.sync()
    assert _above(live(), start)
    g.close()
    assert live() == start
