"""Latent-space fits timing probe: where ZSEMF's time goes on BASELINE config 2's shape (n = 5 000, p = 50 000, 20 % missing, one missingness
pattern per trait) at k = 16 and 64 with tol = 0, maxit = 20 -- the first stage (bwgr_uvbeta on the panel), G = X BETA (bwgr_panel_xb), the host
SVD of G, the dense second stage (bwgr_uvbeta_dense, total and per trait-sweep) and the final X b (bwgr_panel_xb) -- and bwgr_panel_xb alone at
10 000 x 1 000 000 with k = 16 beside the path it replaces, bwgr_uvbeta's row-serial xb.

    python tools/sem_probe.py [--quick]        one JSON line per measurement, then a summary line

tools/uvb_probe.py's method: every stage is called as the driver calls it, once as a warm-up and then three times; the summary prints medians
and spread (max - min).  The second stage's ms per trait-sweep is its time less the same call at maxit = 0 (set-up, uploads), over 20 k.
The product's effective rate is n p bytes of int8 genotypes over its time, beside the 8 TB/s of HBM.  The row-serial yardstick is
uvbeta(maxit = 0, xb = True) less uvbeta(maxit = 0) on the same panel and B = 0 (the product's cost does not depend on B's values).
--quick: k = 16 only, one repetition, the large product at p = 100 000.  Exit status 1 when everything after the first stage takes as long as
the first stage of the same run: the second stage does q / p of the first's marker steps, so that only happens to an engine whose shape is
wrong."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bwgr_amd  # noqa: E402
from bwgr_amd import uvfit as api, synth  # noqa: E402

med = statistics.median


def timed(f, *a, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f(*a, **kw)
    torch.cuda.synchronize()
    return r, 1e3 * (time.perf_counter() - t0)


def spread(v):
    return round(max(v) - min(v), 3)


def stages(P, Y, maxit, reps):
    """ZSEMF's stages on the panel, as bwgr_amd.uvfit._sem runs them; ms per stage, `reps` times after a warm-up."""
    v = api.UVB_VARIANTS["Z"]
    Ym, tol, df0 = api._uvb_inputs(Y, P.n, v, 0.0, 20.0, "probe")
    k = Ym.shape[1]
    names = ("first_stage", "xb", "svd", "second_stage", "second_setup", "final_xb")
    out = {nm: [] for nm in names}
    for rep in range(reps + 1):
        s1, t1 = timed(api._uvb_panel, P, Ym, v, maxit, tol, df0)
        G, t2 = timed(P.xb, s1["b"])
        (Z, V), t3 = timed(api._sem_latent, G, 0, "probe")
        s2, t4 = timed(api._uvb_dense, Ym, Z, v, maxit, tol, df0, P.device)
        _, t4s = timed(api._uvb_dense, Ym, Z, v, 0, tol, df0, P.device)
        b = s1["b"] @ (V @ s2["b"])
        _, t5 = timed(P.xb, b)
        assert np.all(s2["its"] == maxit) and np.all(np.isfinite(b))
        if rep:   # (the first round is the warm-up)
            for nm, t in zip(names, (t1, t2, t3, t4, t4s, t5)):
                out[nm].append(t)
    row = {"k": k, "q": int(Z.shape[1]), "maxit": maxit}
    for nm in names:
        row[nm + "_ms"] = round(med(out[nm]), 3); row[nm + "_spread"] = spread(out[nm])
    row["second_stage_us_per_trait_sweep"] = round(1e3 * (med(out["second_stage"]) - med(out["second_setup"])) / (maxit * k), 3)
    row["second_stage_us_per_marker_step"] = round(row["second_stage_us_per_trait_sweep"] / Z.shape[1] * k, 3)   # the k fits run side by side
    after = [sum(t) for t in zip(out["xb"], out["svd"], out["second_stage"], out["final_xb"])]
    row["after_first_stage_ms"] = round(med(after), 3)
    row["after_over_first"] = round(med(after) / med(out["first_stage"]), 5)
    return row


def product(n, p, k, reps):
    """bwgr_panel_xb alone, and bwgr_uvbeta's row-serial xb on the same panel."""
    X = synth.genotypes(n, p, device=0)
    P = bwgr_amd.Panel(X, n=n, device=0)
    del X
    torch.cuda.empty_cache()
    B = np.random.default_rng(1).normal(size=(p, k)) / np.sqrt(p)
    Y = np.random.default_rng(2).normal(size=(n, k))
    P.xb(B)
    new = [timed(P.xb, B)[1] for _ in range(reps)]
    api._uvb_panel(P, Y, 0, 0, 0.0, 20.0, xb=True)
    old = []
    for _ in range(reps):
        _, ta = timed(api._uvb_panel, P, Y, 0, 0, 0.0, 20.0, xb=True)
        _, tb = timed(api._uvb_panel, P, Y, 0, 0, 0.0, 20.0)
        old.append(ta - tb)
    P.close()
    torch.cuda.empty_cache()
    upload = 8.0 * p * k + 8.0 * n * k     # B up, the result down: part of the call
    return {"n": n, "p": p, "k": k, "panel_xb_ms": round(med(new), 3), "panel_xb_spread": spread(new),
            "panel_xb_TB_per_s": round(n * p / (1e-3 * med(new)) / 1e12, 3), "roofline_TB_per_s": 8.0, "host_copies_bytes": upload,
            "row_serial_xb_ms": round(med(old), 3), "row_serial_xb_spread": spread(old), "speedup": round(med(old) / med(new), 2)}


def probe(n=5000, p=50000, ks=(16, 64), maxit=20, reps=3, frac=0.2, big=(10000, 1000000, 16)):
    X = synth.genotypes(n, p, device=0)
    P = bwgr_amd.Panel(X, n=n, device=0)
    rng = np.random.default_rng(100)
    kmax = max(ks)
    G = np.stack([synth.phenotype(X, n, seed=100 + t).cpu().numpy() for t in range(8)], 1)
    G = (G - G.mean(0)) / G.std(0)
    mix = rng.normal(size=(8, kmax)) * np.linspace(2.0, 0.5, 8)[:, None]   # eight genetic factors of decreasing weight: a latent space to find
    Y = G @ mix + rng.normal(size=(n, kmax))
    Y[rng.random((n, kmax)) < frac] = np.nan
    rows = []
    for k in ks:
        rows.append(stages(P, Y[:, :k], maxit, reps))
        print(json.dumps(rows[-1]), flush=True)
    P.close()
    del X
    torch.cuda.empty_cache()
    prod = product(*big, reps=reps)
    print(json.dumps(prod), flush=True)
    summary = {"n": n, "p": p, "missing": frac, "stages": rows, "product": prod, "bar_holds": bool(all(r["after_over_first"] < 1.0 for r in rows))}
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    if "--quick" in sys.argv:
        r = probe(ks=(16,), reps=1, big=(10000, 100000, 16))
    else:
        r = probe()
    sys.exit(0 if r["bar_holds"] else 1)   # the required bar
