"""mkr timing probe (GPU box): the dense fp64 train of mrr(Y, dense(X)) / mkr against the dense leg of PEGSZ on the same design.

    python tools/mkr_probe.py [--quick]        one JSON line per measurement

The design is K2X(GRM(panel)) of BASELINE config 2's panel (n = 5 000, p = 50 000), so n = 5 000 and r = 4 999; 20 % missing records; k = 4 and
k = 16.  Both fits read the same float-rounded matrix in the same process.
k2x     the GRM and K2X's eigendecomposition on the device (seconds), r
sweep   ms per sweep of mrr(Y, dense(X)) on the device-resident design, and of PEGSZ(Y, [dense(X)]) (the dense leg, one workgroup walking the
        columns): `reps` repeats each; a repeat times a fit of 2 + its sweeps and one of 2 and divides the difference by its, so the set-up
        cancels.  "bar": the train's mean sweep costs no more than the dense leg's.  Also ms per 64-column block, the Gram's share (the
        train timed again with every trait on one shared pattern; the Gram's work is proportional to the patterns, so
        (t_npat - t_1) npat / (npat - 1) estimates it), the one-off part (a fit of no sweep: allocation, centring, set-up, fitted values) and the
        plan's workspace.
Every timed fit is checked to have run every sweep it was asked for.  --quick: k = 4 only, 3 repeats."""
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


def traits(X, n, k, frac, seed, shared):
    G = np.stack([synth.phenotype(X, n, seed=seed + t).cpu().numpy() for t in range(k)], 1)
    G = (G - G.mean(0)) / G.std(0)
    rng = np.random.default_rng(seed)
    Y = G + rng.normal(size=(n, k))
    if shared:
        Y[rng.random(n) < frac, :] = np.nan
    else:
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
    reps = 3 if quick else 5
    Xg = synth.genotypes(n, p, device=0)
    P = bwgr_amd.Panel(Xg, n=n, device=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    K = bwgr_amd.GRM(P, device_out=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    Xd = bwgr_amd.K2X(K)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    r = int(Xd.shape[1])
    print(json.dumps({"probe": "k2x", "n": n, "p": p, "r": r, "grm_s": round(t1 - t0, 3), "k2x_s": round(t2 - t1, 3)}), flush=True)
    Xh = np.asfortranarray(Xd.cpu().numpy())
    D, Dh = bwgr_amd.dense(Xd), bwgr_amd.dense(Xh)
    for k in ([4] if quick else [4, 16]):
        Y = traits(Xg, n, k, frac, seed=100, shared=False)
        Y1 = traits(Xg, n, k, frac, seed=100, shared=True)
        Yf = Y.astype(np.float32).astype(np.float64)       # (what PEGSZ makes of Y; mrr gets the same values)
        pl = bwgr_amd.mrr_dense_plan(n, r, k, k)
        m = per_sweep(lambda s: bwgr_amd.mrr(Yf, D, maxit=s, tol=0), lambda q: q["Its"], 6, reps)
        m1 = per_sweep(lambda s: bwgr_amd.mrr(Y1, D, maxit=s, tol=0), lambda q: q["Its"], 6, reps)
        g = per_sweep(lambda s: bwgr_amd.PEGSZ(Y, [Dh], maxit=s, logtol=NOSTOP), lambda q: q["numit"], 2, reps)
        once = [1e3 * timed(lambda s: bwgr_amd.mrr(Yf, D, maxit=s, tol=0), 0, lambda q: q["Its"]) for _ in range(reps)]
        mm, m1m, gm = float(np.mean(m)), float(np.mean(m1)), float(np.mean(g))
        gram = (mm - m1m) * k / (k - 1)
        print(json.dumps({"probe": "sweep", "n": n, "r": r, "k": k, "npat": k, "missing": frac, "train_ms_per_sweep": stats(m),
                          "train_one_pattern_ms_per_sweep": stats(m1), "dense_leg_ms_per_sweep": stats(g), "speedup": round(gm / mm, 2),
                          "bar_train_no_slower": bool(mm <= gm), "blocks": pl["nblk"], "train_ms_per_block": round(mm / pl["nblk"], 4),
                          "gram_ms_per_sweep_est": round(gram, 3), "gram_share_est": round(gram / mm, 3), "one_off_ms": stats(once),
                          "ngl": pl["ngl"], "ws_bytes": pl["ws_bytes"]}), flush=True)
    P.close()


if __name__ == "__main__":
    main("--quick" in sys.argv)
