"""Sparse-effect timing probe (GPU box), at BASELINE config 2's row count (n = 5 000; the panel is config 2's 50 000 markers), 20 % missing,
k = 4 and k = 16, on the incidence matrix of a factor with q = 500 and q = 5 000 levels.

    python tools/pegs_sparse_probe.py [--quick]        one JSON line per measurement

legs    ms per sweep of a PEGSZ fit on the one effect, `reps` repeats each (a repeat times a fit of 2 + its sweeps and one of 2 and divides
        the difference by its, so the set-up cancels): sparse(S) on the disjoint leg, sparse(S, serial=True) on the one-wave leg and
        dense(S) on the dense leg.  Each sweep carries the same fixed part beside its leg (the linv kernel, the residual sums, the k x k
        tail on the host, the mu shift), so the difference of two is the difference of their legs; the serial leg's time per column is
        its sweep minus the disjoint one's over q (the disjoint leg's own time is left in: a slight underestimate).
        Bar: the disjoint leg's sweep is at most the dense leg's on the same matrix.
mixed   ms per sweep of PEGSZ([panel, sparse(S)]) beside PEGSZ([panel]) in the same run.  Bar: at most the panel's sweep, plus twice the
        sparse leg alone -- taken as the whole sweep of the one-effect fit above, fixed part included, an upper bound --, plus three times
        the panel sweep's run-to-run spread (max - min over its repeats); "within_3_spreads" says whether it holds without the leg's term.
Every timed fit is checked to have run every sweep it was asked for.  --quick: k = 4 only and 3 repeats."""
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (before bwgr_amd: see bwgr_amd/_lib.py)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bwgr_amd  # noqa: E402
from bwgr_amd import dense, sparse, synth  # noqa: E402
from pegs_probe import NOSTOP, per_sweep, stats, traits  # noqa: E402


def incidence(n, q, seed, serial=False):
    """every row in one of q levels, drawn uniformly: built column-compressed, never dense"""
    lev = np.random.default_rng(seed).integers(0, q, size=n)
    rows = np.argsort(lev, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(lev, minlength=q))])
    return sparse((np.ones(n), rows, ptr), shape=(n, q), serial=serial)


def main(quick):
    n, p, frac = 5000, 50000, 0.2
    reps, its = (3, 3) if quick else (5, 4)
    X = synth.genotypes(n, p, device=0)
    P = bwgr_amd.Panel(X, n=n, device=0)
    numit = lambda r: r["numit"]
    for k in ([4] if quick else [4, 16]):
        Y = traits(X, n, k, frac, seed=100)
        sweep = lambda effs, sw=its: per_sweep(lambda s: bwgr_amd.PEGSZ(Y, effs, maxit=s, logtol=NOSTOP), numit, sw, reps)
        panel = sweep([P])
        spread = max(panel) - min(panel)
        print(json.dumps({"probe": "yardsticks", "n": n, "p": p, "k": k, "missing": frac, "panel_ms_per_sweep": stats(panel), "panel_spread_ms": round(spread, 3)}), flush=True)
        for q in (500, 5000):
            S = incidence(n, q, q)
            nnz, longest = int(S.indptr[-1]), int(np.diff(S.indptr).max())
            pl = bwgr_amd.pegs_sparse_plan(n, q, nnz, longest, k, True)
            d = sweep([S], 20)
            s = sweep([incidence(n, q, q, serial=True)], 20)
            z = sweep([dense(S.toarray())], 4 if q > 1000 else 20) if 8.0 * n * q <= 4e9 else None
            leg = float(np.mean(d))
            out = {"probe": "legs", "n": n, "q": q, "k": k, "nnz": nnz, "longest_column": longest, "trips": -(-q // pl["trip_cols"]),
                   "sparse_ws_bytes": pl["ws_bytes"], "dense_ws_bytes": bwgr_amd.pegs_plan(n, q, k)["ws_bytes"],
                   "disjoint_ms_per_sweep": stats(d), "serial_ms_per_sweep": stats(s), "serial_us_per_column": round(1e3 * (float(np.mean(s)) - leg) / q, 3)}
            if z is not None:
                out.update({"dense_ms_per_sweep": stats(z), "dense_us_per_column": round(1e3 * (float(np.mean(z)) - leg) / q, 3), "bar_disjoint_at_most_dense": bool(np.mean(d) <= np.mean(z))})
            print(json.dumps(out), flush=True)
            m = sweep([P, S])
            bar = float(np.mean(panel)) + 2 * leg + 3 * spread
            print(json.dumps({"probe": "mixed", "n": n, "p": p, "q": q, "k": k, "panel_sparse_ms_per_sweep": stats(m), "panel_ms_per_sweep": round(float(np.mean(panel)), 3),
                              "diff_ms": round(float(np.mean(m) - np.mean(panel)), 3), "bar_ms": round(bar, 3), "bar_holds": bool(np.mean(m) <= bar),
                              "within_3_spreads": bool(np.mean(m) - np.mean(panel) <= 3 * spread)}), flush=True)
    P.close()


if __name__ == "__main__":
    main("--quick" in sys.argv)
