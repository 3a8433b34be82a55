"""uvbeta timing probe (GPU box): ms per sweep of the per-trait ridge engine on BASELINE config 2's shape (n = 5 000, p = 50 000, 20 %
missing, one missingness pattern per trait) for k = 1, 16, 64, 256, beside two yardsticks measured in the same process: mrr's ms per
iteration at k = 16 on the first 16 columns, and emRR's ms per sweep (what one unmasked trait costs on the single-trait engine).

    python tools/uvb_probe.py [--quick]        one JSON line per measurement, then a summary line

ms per sweep is the difference of two tol = 0 runs (maxit = 2 + its and maxit = 2) after a warm-up call, so the set-up (k_uvb_setup, the
uploads) and xb cancel.  uvbeta and mrr at k = 16 alternate three times each; the summary prints medians and spread.  Per sweep the engine
launches k_permute_cols once and, per group of 64 traits, k_mrr_gram, then k_uvb_pass + k_uvb_solve for each of the ceil(p/64) blocks and
one closing pass, then k_uvb_rows, k_uvb_cols and two k_mrr_finish, and one k_uvb_mu_shift: groups * (2 * ceil(p/64) + 7) + 1 kernels.
The Gram's share is estimated from a second k = 16 run without missing values (one pattern: a sixteenth of the Gram work; its solve reads
the one matrix from LDS) -- an estimate, not a profile.  --quick: k = 16 only, one repetition.  Exit status 1 when uvbeta at k = 16 takes
longer per sweep than mrr per iteration at k = 16 beyond the spread the run shows: that is a defect to find, not a number to report."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bwgr_amd  # noqa: E402
from bwgr_amd import synth  # noqa: E402


def timed(f, *a, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f(*a, **kw)
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def per_sweep(f, Y, P, its, **kw):
    _, ta = timed(f, Y, P, maxit=2 + its, tol=0, **kw)
    _, tb = timed(f, Y, P, maxit=2, tol=0, **kw)
    return 1e3 * (ta - tb) / its


def probe(n=5000, p=50000, ks=(1, 16, 64, 256), its=3, reps=3, frac=0.2):
    X = synth.genotypes(n, p, device=0)
    P = bwgr_amd.Panel(X, n=n, device=0)
    rng = np.random.default_rng(100)
    kmax = max(ks)
    G = np.stack([synth.phenotype(X, n, seed=100 + t).cpu().numpy() for t in range(4)], 1)
    G = (G - G.mean(0)) / G.std(0)
    Yfull = G[:, rng.integers(0, 4, kmax)] * rng.uniform(0.5, 1.0, kmax) + rng.normal(size=(n, kmax))
    Y = Yfull.copy()
    Y[rng.random((n, kmax)) < frac] = np.nan
    nblk = (p + 63) // 64
    y1 = synth.scale_phenotype(synth.phenotype(X, n)).cpu().numpy()
    bwgr_amd.emRR(y1, P, maxit=2)
    em = [per_sweep(lambda y, Pn, maxit, tol: bwgr_amd.emRR(y, Pn, maxit=maxit), y1, P, 6) for _ in range(reps)]
    print(json.dumps({"engine": "emRR", "ms_per_sweep": [round(v, 3) for v in em]}), flush=True)
    bwgr_amd.uvbeta(Y[:, :16], P, "D", maxit=1, tol=0)
    bwgr_amd.mrr(Y[:, :16], P, maxit=1, tol=0)
    uv16, mr16 = [], []
    for _ in range(reps):
        uv16.append(per_sweep(bwgr_amd.uvbeta, Y[:, :16], P, its, variant="D"))
        mr16.append(per_sweep(bwgr_amd.mrr, Y[:, :16], P, its))
    print(json.dumps({"engine": "uvbeta", "k": 16, "ms_per_sweep": [round(v, 3) for v in uv16]}), flush=True)
    print(json.dumps({"engine": "mrr", "k": 16, "ms_per_iter": [round(v, 3) for v in mr16]}), flush=True)
    one = [per_sweep(bwgr_amd.uvbeta, Yfull[:, :16], P, its, variant="D") for _ in range(reps)]
    print(json.dumps({"engine": "uvbeta", "k": 16, "patterns": 1, "ms_per_sweep": [round(v, 3) for v in one]}), flush=True)
    rows = {}
    for k in ks:
        if k == 16:
            rows[k] = uv16
            continue
        bwgr_amd.uvbeta(Y[:, :k], P, "D", maxit=1, tol=0)
        rows[k] = [per_sweep(bwgr_amd.uvbeta, Y[:, :k], P, its, variant="D") for _ in range(reps)]
        print(json.dumps({"engine": "uvbeta", "k": k, "ms_per_sweep": [round(v, 3) for v in rows[k]]}), flush=True)
    med = statistics.median
    spread = lambda v: round(max(v) - min(v), 3)   # noqa: E731
    W = bwgr_amd.uvb_plan(n, p, 1)["W"]
    gram16 = (med(uv16) - med(one)) * 16.0 / 15.0
    summary = {"n": n, "p": p, "missing": frac, "W": W, "emRR_ms_per_sweep": round(med(em), 3), "mrr_k16_ms_per_iter": round(med(mr16), 3),
               "mrr_k16_spread": spread(mr16), "uvbeta_k16_ms_per_sweep": round(med(uv16), 3), "uvbeta_k16_spread": spread(uv16),
               "uvbeta_k16_not_slower_than_mrr": bool(med(uv16) <= med(mr16) + spread(uv16) + spread(mr16)),
               "uvbeta_k16_one_pattern_ms": round(med(one), 3), "gram_share_k16_estimate": round(gram16 / med(uv16), 3),
               "uvbeta": {str(k): {"ms_per_sweep": round(med(v), 3), "spread": spread(v), "ms_per_trait_sweep": round(med(v) / k, 4),
                                   "launches_per_sweep": -(-k // W) * (2 * nblk + 7) + 1} for k, v in rows.items()}}
    print(json.dumps(summary), flush=True)
    P.close()
    del X
    torch.cuda.empty_cache()
    return summary


if __name__ == "__main__":
    if "--quick" in sys.argv:
        r = probe(ks=(16,), its=2, reps=1)
    else:
        r = probe()
    sys.exit(0 if r["uvbeta_k16_not_slower_than_mrr"] else 1)   # the required bar
