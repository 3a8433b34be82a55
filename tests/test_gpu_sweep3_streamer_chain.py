"""GPU: the DMA streamers of k_sweep3f / k_sweep3 give the bits they gave before their update waves' step was reordered.

Everything a streamer computes is exact integer arithmetic (int32 MFMA sums, the 64-bit residual, 64-bit atomics), so a reordering of its work
must leave every bit where it was.  tests/golden/sweep3_streamer_parent.npz holds Chain.state() (b, d, e, ve, mu) and Chain.result() (b, hat, ve)
of every case below after it = 5, bi = 1, seed 23, as the commit BEFORE that change computed them on an MI355X (tools/make_sweep3_streamer_golden.py
writes the file from whatever library is loaded: run it against a build of the commit to compare with, never against the code under test).  Every
array of every case is compared with np.array_equal.

Cases, n = 600 rows (the suite's conftest forces k_sweep3 for every selection sweep):
  nwg = 5: 128-row slabs, a streamer each;  nwg = 3: 256-row slabs cut into two 128-row streamers
  p = 1536: twelve whole blocks, D at full depth;  p = 1600: a last block of 64;  p = 1764: a last block of 100;  p = 640: D clamped to 5
  pi = 0.99: lists of 0-3 markers (the prefetched columns are the whole fold);  pi = 0.7: about 38 markers a block (fold_list continues behind the
  four prefetched entries and takes a second pass of 31);  pi = 0.5 at p = 1536: about 64 markers a block (three passes)
  p = 4096 with BWGR_D3 = 4 and 16 at pi = 0.98: lists are late often at the short lag and never at the long one
BayesC as well for the first two shapes.  The default cases must have run k_sweep3f; one case runs again with BWGR_FIXED3=0, must have run
k_sweep3 and is held to the same arrays.  Against a stale fixture, one case's golden arrays are compared with the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import scaled_err, synth_small

pytestmark = pytest.mark.gpu
TOL = 1e-6   # (tests/test_gpu_parity.py)
N, IT, BI, SEED = 600, 5, 1, 23
GENERIC, FIXED = 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep3_streamer_parent.npz")
STATE_KEYS, RESULT_KEYS = ("b", "d", "e", "ve", "mu"), ("b", "hat", "ve")

# (model, p, nwg, pi, BWGR_D3 or 0)
CASES = [("BayesB", p, nwg, pi, 0) for p in (1536, 1600, 1764, 640) for nwg in (5, 3) for pi in (0.99, 0.7)]
CASES += [("BayesB", 1536, nwg, 0.5, 0) for nwg in (5, 3)]
CASES += [("BayesB", 4096, nwg, 0.98, d3) for nwg in (5, 3) for d3 in (4, 16)]
CASES += [("BayesC", p, nwg, pi, 0) for p in (1536, 1600) for nwg in (5, 3) for pi in (0.99, 0.7)]
GENERIC_CASE = ("BayesB", 1764, 5, 0.7, 0)   # (runs once more as k_sweep3)
ORACLE_CASE = ("BayesB", 1600, 3, 0.7, 0)


def case_id(case):
    return "%s-p%d-nwg%d-pi%g-D%d" % case


_data = {}


def inputs(p):
    if p not in _data:
        _data[p] = synth_small(N, p, seed=100 + p)
    return _data[p]


def run_case(case, setenv, delenv, fixed=True):
    """One chain of `case` on the loaded library: (which kernel the selection sweeps ran as, the arrays the fixture keeps).  setenv / delenv set
    the switches (they are read when the root panel is made)."""
    import bwgr_amd
    from bwgr_amd import _lib
    model, p, nwg, pi, d3 = case
    if d3:
        setenv("BWGR_D3", str(d3))
    else:
        delenv("BWGR_D3")
    if fixed:
        delenv("BWGR_FIXED3")
    else:
        setenv("BWGR_FIXED3", "0")
    X, y = inputs(p)
    P = bwgr_amd.Panel(X, nwg=nwg)
    w = C.c_int(-1)
    _lib.check(_lib.lib().bwgr_debug_sweep3_kernel(P._h, C.byref(w)))
    ch = bwgr_amd.Chain(P, model, y, it=IT, bi=BI, pi=pi, df=5, R2=0.5, seed=SEED)
    ch.run(IT)
    st, res = ch.state(), ch.result()
    ch.close(); P.close()
    out = {"state_" + k: np.asarray(st[k]) for k in STATE_KEYS}
    out.update({"result_" + k: np.asarray(res[k]) for k in RESULT_KEYS})
    return w.value, out


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _check(case, got, golden):
    cid = case_id(case)
    for k in ["state_" + s for s in STATE_KEYS] + ["result_" + s for s in RESULT_KEYS]:
        want = golden[cid + "/" + k]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (cid, k)
        assert np.array_equal(got[k], want), (cid, k, int(np.sum(got[k] != want)))


def _env(monkeypatch):
    return monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fixed_kernel_gives_the_parent_commits_bits(case, golden, monkeypatch):
    which, got = run_case(case, *_env(monkeypatch))
    assert which == FIXED
    _check(case, got, golden)
    if case[3] <= 0.7:   # the dense settings do go past the four prefetched entries (0.7: a second pass too; 0.5: a third)
        d = got["state_d"]
        assert max(d[j:j + 128].sum() for j in range(0, case[1], 128)) > (31 if case[3] == 0.7 else 62)


def test_generic_kernel_gives_the_parent_commits_bits(golden, monkeypatch):
    which, got = run_case(GENERIC_CASE, *_env(monkeypatch), fixed=False)
    assert which == GENERIC
    _check(GENERIC_CASE, got, golden)


def test_fixture_is_the_oracles_chain(golden):
    """A stale or foreign fixture would not be the chain the CPU oracle runs: the same decisions, b and e to test_gpu_parity.py's 1e-6."""
    from oracle import oracle as O
    model, p, nwg, pi, d3 = ORACLE_CASE
    X, y = inputs(p)
    o = O.bayes(model, y, X, it=IT, bi=BI, pi=pi, df=5, R2=0.5, seed=SEED)
    cid = case_id(ORACLE_CASE)
    assert np.array_equal(golden[cid + "/state_d"], o["last"]["d"])
    assert scaled_err(golden[cid + "/state_b"], o["last"]["b"]) < TOL
    assert scaled_err(golden[cid + "/state_e"], o["last"]["e"]) < TOL
    assert scaled_err(golden[cid + "/result_b"], o["b"]) < TOL
