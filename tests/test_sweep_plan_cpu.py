"""CPU: plan_sweep decides every sweep of tests/sweep_plan_cases.py as it did before the plan took a mode, carried its redo and named its
helper kernels: bwgr_debug_sweep_plan against tests/golden/sweep_plan_parent.txt, which tools/sweep_plan_table.py recorded from the parent's
plan_sweep (called unchanged, on a host-only panel, with force3 set for the pairs) at the commit its first line names.  A differing entry is
a changed decision: restore it, do not re-record."""
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_plan_cases as S  # noqa: E402

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_plan_parent.txt")
INF_BITS = 0x7F800000


@functools.lru_cache(None)
def _parent():
    return S.read_table(TABLE)


@functools.lru_cache(None)
def _now():
    return S.table()


def _rows(tab):
    return [(k, dict(zip(S.FIELDS, v))) for k, v in tab.items() if v is not None]


def test_the_table_covers_exactly_the_cases():
    with open(TABLE) as f:
        first = f.readline()
    assert first.startswith("#") and "commit" in first, first
    assert list(_parent()) == [S.key(*c) for c in S.cases()]
    assert len(S.FIELDS) == 67 and all(v is None or len(v) == len(S.FIELDS) for v in _parent().values())


@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_every_plan_is_the_parents(shape):
    """entry by entry, the refusals included"""
    differ = []
    for c in S.cases():
        if c[0] != shape:
            continue
        k = S.key(*c)
        got, want = _now()[k], _parent()[k]
        if got != want:
            differ.append((k, None if got is None or want is None else [(f, w, g) for f, w, g in zip(S.FIELDS, want, got) if w != g]))
    assert not differ, differ[:5]


def test_the_table_reaches_every_branch():
    rows = _rows(_parent())
    assert {r["engine"] for _, r in rows} == {1, 2, 3, 4}                      # all four engines
    assert {r["gate"] for _, r in rows} == {0, 1, 2}                           # no gate, a finite one, an infinite one
    assert all((r["gate"] == 2) == (r["gate3_bits"] == INF_BITS) and (r["gate"] == 0) == (r["gate3_bits"] == 0) for _, r in rows)
    e3 = [r for _, r in rows if r["engine"] == 3 and r["spin0_kernel"] not in S.K_SWEEP3P]
    assert {r["fixed3"] for r in e3} == {0, 1}
    assert {r["spin0_kernel"] for r in e3 if r["fixed3"]} == {S.KERNELS.index("k_sweep3f")}
    assert {r["pf"] >= 0 for r in e3} == {False, True} and {r["pf2"] >= 0 for r in e3} == {False, True}
    assert {r["fx"] for _, r in rows if r["engine"] == 4} == {0, 1}
    assert {r["guarded"] for _, r in rows} == {0, 1}
    assert any(r["spin0_kernel"] in S.K_SWEEP3P for _, r in rows)              # the pair launch
    assert {r["dbg3"] & (S.DMA4 | S.DMA3) for r in e3} == {0, S.DMA4}          # both streamer families
    used = {r["spin%d_kernel" % i] for _, r in rows for i in range(3)} - {-1}
    assert len(used) >= 14, sorted(S.KERNELS[i] for i in used)
    refused = [k for k, v in _parent().items() if v is None]
    assert refused and all(" | redo | " in k or " | pair | " in k or "centre" in k or " rows | " in k or " em | " in k for k in refused)


def test_a_pair_is_one_k_sweep3p_launch_without_redo():
    """mode 2 is what the parent planned with force3 set on the handle (the table's pair entries, compared above), and that is: every
    sweep k_sweep3's, one launch of K3 + 2 workgroups on the 256-row-or-planned streamers, no fallback and no redo"""
    pairs = [(k, r) for k, r in _rows(_parent()) if " | pair | " in k]
    assert len(pairs) >= 20
    for k, r in pairs:
        assert r["engine"] == 3 and r["gate"] == 2 and r["nspins"] == 1 and not r["guarded"] and r["spin_run"] == -1, k
        assert r["spin0_kernel"] == (15 if r["g16"] else 16) and r["spin0_grid"] == r["spin0_resident"] == r["K3"] + 2, k
        assert r["fixed3"] == 0 and r["pf"] == -1 and r["pf2"] == -1, k
    assert {k: v for k, v in _now().items() if " | pair | " in k} == {k: v for k, v in _parent().items() if " | pair | " in k}


def test_a_guarded_plan_holds_its_redo_in_full():
    """the redo of a guarded sweep alone is the plan the parent made a second time in launch_sweep_kernel: the mode-1 entry of the same case"""
    tab = _parent()
    n = 0
    for c in S.cases():
        k, v = S.key(*c), tab[S.key(*c)]
        if v is None or c[2] != "alone" or c[4] is not None:
            continue
        r = dict(zip(S.FIELDS, v))
        redo = tab[S.key(c[0], c[1], "redo", c[3], None)]
        assert (redo is not None) == bool(r["guarded"]), k
        if redo is None:
            continue
        q = dict(zip(S.FIELDS, redo))
        n += 1
        for f in ("engine", "lag", "nfeed", "g16", "fx", "nd", "npf", "ahead", "nq", "wsub", "wK3"):
            assert r["redo_" + f] == q[f], (k, f)
        i = r["spin_redo"]
        assert i == r["nspins"] - 1 and q["nspins"] == 1
        assert [r["spin%d_%s" % (i, f)] for f in ("kernel", "grid", "resident", "threads", "lds")] == [q["spin0_" + f] for f in ("kernel", "grid", "resident", "threads", "lds")], k
        assert r["cen_redo"] == q["cen_run"] and r["redo_spec"] == q["redo_spec"] and r["redo_cen"] == q["redo_cen"], k
    assert n >= 50
