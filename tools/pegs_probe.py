"""PEGS / PEGSZ timing probe (GPU box), at BASELINE config 2's shape (n = 5 000, p = 50 000, 20 % missing), k = 4 and k = 16.

    python tools/pegs_probe.py [--quick]        one JSON line per measurement

panel   ms per sweep of PEGS against mrr(updateMu=True) per iteration, on the same panel in the same process, `reps` repeats each (a repeat
        times a fit of 2 + its sweeps and one of 2 and divides the difference by its, so the set-up cancels).  The two run the same kernels;
        "within" says whether the means differ by at most three times mrr's own run-to-run spread (max - min over its repeats).
dense   microseconds per column step of the dense leg (a dense-only PEGSZ fit, q = 16 and 64; the sweep's fixed part included, and the
        marginal figure per further column from the two), beside uvbeta_dense's per-step figure for one
        trait times k (its workgroups run the traits side by side; the dense leg of PEGS runs the k traits of a column in one workgroup,
        because their solve couples them).
full    one PEGSZ([X, Z]) fit at k = 4 with the default logtol: wall time, sweeps, and the panel leg's share (its per-sweep time above).
Every timed fit is checked to have run every sweep it was asked for.  --quick: k = 4 only and 3 repeats."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bwgr_amd  # noqa: E402
from bwgr_amd import synth  # noqa: E402

NOSTOP = float("-inf")


def traits(X, n, k, frac, seed):
    G = np.stack([synth.phenotype(X, n, seed=seed + t).cpu().numpy() for t in range(k)], 1)
    G = (G - G.mean(0)) / G.std(0)
    rng = np.random.default_rng(seed)
    Y = G + rng.normal(size=(n, k))
    Y[rng.random((n, k)) < frac] = np.nan
    return Y


def timed(f, sweeps, its_of):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f(sweeps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert its_of(r) == sweeps, (its_of(r), sweeps)
    return dt


def per_sweep(f, its_of, its, reps):
    f(1)
    return [1e3 * (timed(f, 2 + its, its_of) - timed(f, 2, its_of)) / its for _ in range(reps)]


def stats(ms):
    return {"mean": round(float(np.mean(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "reps": len(ms)}


def main(quick):
    n, p, frac = 5000, 50000, 0.2
    reps, its = (3, 3) if quick else (5, 4)
    X = synth.genotypes(n, p, device=0)
    P = bwgr_amd.Panel(X, n=n, device=0)
    panel_ms = {}
    for k in ([4] if quick else [4, 16]):
        Y = traits(X, n, k, frac, seed=100)
        Yf = Y.astype(np.float32).astype(np.float64)      # (what PEGS makes of Y; mrr gets the same values)
        m = per_sweep(lambda s: bwgr_amd.mrr(Yf, P, maxit=s, tol=0, updateMu=True), lambda r: r["Its"], its, reps)
        g = per_sweep(lambda s: bwgr_amd.PEGS(Y, P, maxit=s, logtol=NOSTOP), lambda r: r["numit"], its, reps)
        spread = max(m) - min(m)
        panel_ms[k] = float(np.mean(g))
        print(json.dumps({"probe": "panel", "n": n, "p": p, "k": k, "missing": frac, "mrr_updateMu_ms_per_iter": stats(m), "pegs_ms_per_sweep": stats(g),
                          "mrr_spread_ms": round(spread, 3), "diff_ms": round(float(np.mean(g) - np.mean(m)), 3),
                          "within_3_spreads": bool(abs(np.mean(g) - np.mean(m)) <= 3 * spread)}), flush=True)
        dense_ms = {}
        for q in (16, 64):
            Z = np.asfortranarray(np.random.default_rng(q).normal(size=(n, q)))
            dits = 20
            d = per_sweep(lambda s: bwgr_amd.PEGSZ(Y, [bwgr_amd.dense(Z)], maxit=s, logtol=NOSTOP), lambda r: r["numit"], dits, reps)
            u = per_sweep(lambda s: bwgr_amd.uvbeta_dense(Y[:, 0], Z, maxit=s, tol=0), lambda r: int(r["its"][0]), dits, reps)
            print(json.dumps({"probe": "dense", "n": n, "q": q, "k": k, "threads": bwgr_amd.pegs_plan(n, q, k)["threads"],
                              "pegs_us_per_column_step": round(1e3 * float(np.mean(d)) / q, 3), "pegs_ms_per_sweep": stats(d),
                              "uvbeta_dense_us_per_step_one_trait": round(1e3 * float(np.mean(u)) / q, 3),
                              "uvbeta_dense_us_per_step_times_k": round(1e3 * float(np.mean(u)) / q * k, 3)}), flush=True)
            dense_ms[q] = float(np.mean(d))
        print(json.dumps({"probe": "dense_marginal", "n": n, "k": k, "us_per_further_column": round(1e3 * (dense_ms[64] - dense_ms[16]) / 48, 3),
                          "fixed_ms_per_sweep": round(dense_ms[16] - 16 * (dense_ms[64] - dense_ms[16]) / 48, 3)}), flush=True)
    k = 4
    Y = traits(X, n, k, frac, seed=100)
    Z = np.asfortranarray(np.random.default_rng(7).normal(size=(n, 64)))
    bwgr_amd.PEGSZ(Y, [P, Z], maxit=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = bwgr_amd.PEGSZ(Y, [P, Z])
    wall = time.perf_counter() - t0
    print(json.dumps({"probe": "full", "n": n, "p": p, "q": 64, "k": k, "wall_s": round(wall, 3), "numit": r["numit"], "cnv": round(r["cnv"], 3),
                      "panel_leg_share": round(r["numit"] * panel_ms[k] * 1e-3 / wall, 3), "bend": [float(v) for v in r["bend"]]}), flush=True)
    P.close()


if __name__ == "__main__":
    main("--quick" in sys.argv)
