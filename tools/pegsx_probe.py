"""PEGSX timing probe (GPU box), at BASELINE config 2's shape (n = 5 000, p = 50 000, 20 % missing), k = 4 and 16, f = 1, 8 and 64.

    python tools/pegsx_probe.py [--quick]        one JSON line per measurement

The yardstick in every comparison is the existing code, never the code under test:
sweep   ms per sweep of PEGSX(Y, X, [panel]) beside PEGSZ(Y, [panel]) on the same panel in the same process.  PEGSZ: `reps` repeats, each
        timing a fit of 2 + its sweeps and one of 2 and dividing the difference by its (its set-up cancels).  PEGSX pays the projected trace
        once per call -- far more than a sweep -- so a difference of two calls would be its noise; instead the library's own clock times every
        sweep of one call (pegsx_timing mode 1: the host clock around a sweep, which ends in a synchronous copy anyway; the first sweep, which
        is the first launch of the sweep's kernels in that call, is in the figures).
fixed   the fixed step alone: k_pegsx_fixed bracketed with events (pegsx_timing mode 2) in a fit on a four-column dense effect -- the step
        depends on n, f and k only.
bar     a PEGSX sweep costs at most the PEGSZ sweep, plus twice the fixed step alone, plus three times PEGSZ's run-to-run spread (max - min
        over its repeats): the fixed step adds no hidden synchronisation.
trace   the trace set-up (k_pegsx_trace_panel, once per call) beside k_mrr_setup_cols in the same call, both with events: reported, not
        barred.  X is read unmasked (n x f doubles, once for all patterns) through L2.
--quick: k = 4, f = 1 and 8, and 3 repeats."""
import json
import os
import sys

import numpy as np
import torch  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bwgr_amd  # noqa: E402
from bwgr_amd import synth  # noqa: E402
from pegs_probe import NOSTOP, per_sweep, stats, traits  # noqa: E402


def main(quick):
    n, p, frac = 5000, 50000, 0.2
    reps, its = (3, 3) if quick else (5, 4)
    Xg = synth.genotypes(n, p, device=0)
    P = bwgr_amd.Panel(Xg, n=n, device=0)
    rng = np.random.default_rng(5)
    Xall = np.asfortranarray(np.column_stack([np.ones(n), rng.normal(size=(n, 63))]))
    D4 = bwgr_amd.dense(rng.normal(size=(n, 4)))
    ok = True
    for k in ([4] if quick else [4, 16]):
        Y = traits(Xg, n, k, frac, seed=100)
        z = per_sweep(lambda s: bwgr_amd.PEGSZ(Y, [P], maxit=s, logtol=NOSTOP), lambda r: r["numit"], its, reps)
        spread = max(z) - min(z)
        for f in ([1, 8] if quick else [1, 8, 64]):
            X = Xall[:, :f]
            bwgr_amd.pegsx_timing(2)
            r = bwgr_amd.PEGSX(Y, X, [D4], maxit=20, logtol=NOSTOP)
            fx = bwgr_amd.pegsx_timing(1)
            assert r["its"] == 20 and fx["sweeps"] == 20
            r = bwgr_amd.PEGSX(Y, X, [P], maxit=2 + its, logtol=NOSTOP)
            t = bwgr_amd.pegsx_timing(0)
            assert r["its"] == 2 + its and t["sweeps"] == 2 + its
            bar = float(np.mean(z)) + 2 * fx["fixed_ms"]["mean"] + 3 * spread
            within = bool(t["sweep_ms"]["mean"] <= bar)
            ok &= within
            pl = bwgr_amd.pegsx_plan(n, f, k)
            print(json.dumps({"probe": "pegsx", "n": n, "p": p, "k": k, "f": f, "missing": frac, "pegsz_ms_per_sweep": stats(z), "pegsz_spread_ms": round(spread, 3),
                              "pegsx_ms_per_sweep": {q: round(v, 3) for q, v in t["sweep_ms"].items()}, "sweeps_timed": t["sweeps"],
                              "fixed_step_alone_ms": {q: round(v, 4) for q, v in fx["fixed_ms"].items()}, "fixed_threads": pl["threads"],
                              "bar_ms": round(bar, 3), "within_bar": within, "trace_setup_ms": round(t["trace_ms"], 2),
                              "mrr_setup_cols_ms": round(t["setup_cols_ms"], 2), "x_bytes_read_through_l2": 8 * n * f}), flush=True)
    P.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main("--quick" in sys.argv))
