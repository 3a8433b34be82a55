"""mrr / mrr_float timing probe (GPU box): ms per iteration of the multi-trait engine on synthetic int8 panels, its launch count,
its HBM traffic against the n*p bytes one pass over the panel costs, and emRR's sweep on the same panel as a one-trait yardstick.

    python tools/mrr_probe.py [--quick]        one JSON line per shape

Shapes: BASELINE config 2 (n = 5 000, p = 50 000) with k = 1, 4, 8 and config 3's panel (n = 10 000, p = 500 000) with k = 4;
--quick runs config 2 with k = 4 only (for a rocprofv3 --kernel-trace --stats run of its own).  Per iteration the engine launches
k_permute_cols, k_mrr_gram, k_mrr_linv, then k_mrr_pass + k_mrr_solve for each of the ceil(p/64) blocks and one closing pass, then
k_mrr_ey + k_mrr_finish and k_mrr_tilde + k_mrr_finish: 2 * ceil(p/64) + 8 kernels (plus small copies).
Bytes per sweep: the pass kernel reads the gathered panel once (n p); the gather reads and writes it (2 n p, extra); the Gram
reads it once per missingness pattern (npat n p, extra; the four waves of a workgroup share their loads through the caches)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bwgr_amd  # noqa: E402
from bwgr_amd import synth  # noqa: E402

HBM_TBS = 8.0   # MI355X peak HBM3E bandwidth, TB/s


def traits(X, n, k, frac, seed):
    G = np.stack([synth.phenotype(X, n, seed=seed + t).cpu().numpy() for t in range(k)], 1)
    G = (G - G.mean(0)) / G.std(0)
    rng = np.random.default_rng(seed)
    Y = G + rng.normal(size=(n, k))
    Y[rng.random((n, k)) < frac] = np.nan
    return Y


def timed(f, *a, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f(*a, **kw)
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def probe(n, p, ks, its=6, frac=0.2):
    X = synth.genotypes(n, p, device=0)
    P = bwgr_amd.Panel(X, n=n, device=0)
    out = []
    y1 = synth.scale_phenotype(synth.phenotype(X, n)).cpu().numpy()
    bwgr_amd.emRR(y1, P, maxit=2)
    _, ta = timed(bwgr_amd.emRR, y1, P, maxit=2 + its)
    _, tb = timed(bwgr_amd.emRR, y1, P, maxit=2)
    em_ms = 1e3 * (ta - tb) / its
    for k in ks:
        Y = traits(X, n, k, frac, seed=100)
        npat = len({tuple(np.isnan(Y[:, t])) for t in range(k)})
        bwgr_amd.mrr(Y, P, maxit=1, tol=0)
        _, ta = timed(bwgr_amd.mrr, Y, P, maxit=2 + its, tol=0)
        _, tb = timed(bwgr_amd.mrr, Y, P, maxit=2, tol=0)
        ms = 1e3 * (ta - tb) / its
        nblk = (p + 63) // 64
        sweep_bytes = n * p
        extra = {"gather": 2 * n * p, "gram": npat * n * p}
        total = sweep_bytes + sum(extra.values())
        out.append({"n": n, "p": p, "k": k, "missing": frac, "patterns": npat, "ms_per_iter": round(ms, 3),
                    "launches_per_iter": 2 * nblk + 8, "engine": "per-block launch train",
                    "hbm_frac_np": round(sweep_bytes / (ms * 1e-3) / (HBM_TBS * 1e12), 5),
                    "hbm_frac_all": round(total / (ms * 1e-3) / (HBM_TBS * 1e12), 5),
                    "bytes": {"sweep_np": sweep_bytes, **extra}, "emRR_ms_per_sweep": round(em_ms, 3)})
        print(json.dumps(out[-1]), flush=True)
    P.close()
    del X
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    if "--quick" in sys.argv:
        probe(5000, 50000, [4], its=3)
    else:
        probe(5000, 50000, [1, 4, 8])
        probe(10000, 500000, [4], its=2)
