"""Two-design engine timing probe: what the dense leg adds to a sweep of bwgr_uvbeta2 beside bwgr_uvbeta (variant D) on BASELINE config 2's
shape (n = 5 000, p = 50 000, 20 % missing, one missingness pattern per trait) at k = q = 16 and 64, and MEGA and GSEM end to end at k = 16,
split by stage.

    python tools/sem2_probe.py [--quick]        one JSON line per measurement, then a summary line

tools/uvb_probe.py's method: ms per sweep is the difference of two tol = 0 runs (maxit = 3 and 1) after a warm-up, over the two sweeps
between them; medians of three, spread = max - min.  uvbeta2 and uvbeta D are alternated in one process on one panel, and every timed run
is checked to have run every trait through every sweep, so that the difference compares equal work (the bar fails otherwise).  The dense leg's
predicted cost is groups x q x the per-step time of bwgr_uvbeta_dense, measured in the same process at the same n, q and k (the difference
of its maxit = 40 and maxit = 20 runs over 20 q steps; the k fits run side by side).

The bar: uvbeta2's ms per sweep may exceed uvbeta D's of the same run by at most twice that predicted cost plus
three times the yardstick's spread -- the factor two is for what bwgr_uvbeta_dense does not pay per sweep, the load and store of E and a
launch per group.  Both sides are printed; exit status 1 when the bar fails.  --quick: k = 16 only, one repetition."""
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


def sweeps(P, Y, Z, reps, lo=1, hi=3, dlo=20, dhi=40):
    """ms per sweep of uvbeta2(Y, Z, P) and of uvbeta(Y, P, "D"), alternated; us per step of uvbeta_dense(Y, Z)."""
    k, q = Y.shape[1], Z.shape[1]
    two, one, step = [], [], []
    equal_work = True      # every trait ran every sweep of every timed run (a trait whose cnv goes NaN stops early: less work in the difference)
    for rep in range(reps + 1):
        ra3, a3 = timed(api._uvb2_panel, P, Y, Z, hi, 0.0, 20.0)
        rb3, b3 = timed(api._uvb_panel, P, Y, 0, hi, 0.0, 20.0)
        ra1, a1 = timed(api._uvb2_panel, P, Y, Z, lo, 0.0, 20.0)
        rb1, b1 = timed(api._uvb_panel, P, Y, 0, lo, 0.0, 20.0)
        equal_work = equal_work and all(bool(np.all(r["its"] == m)) for r, m in ((ra3, hi), (rb3, hi), (ra1, lo), (rb1, lo)))
        _, d2 = timed(api._uvb_dense, Y, Z, 0, dhi, 0.0, 20.0, P.device)
        _, d1 = timed(api._uvb_dense, Y, Z, 0, dlo, 0.0, 20.0, P.device)
        if rep:   # (the first round is the warm-up)
            two.append((a3 - a1) / (hi - lo)); one.append((b3 - b1) / (hi - lo)); step.append(1e3 * (d2 - d1) / ((dhi - dlo) * q))
    groups = (k + 63) // 64
    predicted = groups * q * med(step) * 1e-3
    row = {"k": k, "q": q, "groups": groups, "uvbeta2_ms_per_sweep": round(med(two), 3), "uvbeta2_spread": spread(two),
           "uvbeta_D_ms_per_sweep": round(med(one), 3), "uvbeta_D_spread": spread(one), "dense_us_per_step": round(med(step), 3),
           "dense_us_per_step_spread": spread(step), "leg_predicted_ms": round(predicted, 4)}
    row["excess_ms"] = round(med(two) - med(one), 3)
    row["allowed_ms"] = round(2.0 * predicted + 3.0 * (max(one) - min(one)), 3)
    row["every_trait_ran_every_sweep"] = equal_work
    row["bar_holds"] = bool(equal_work and row["excess_ms"] <= row["allowed_ms"])
    return row


def driver(which, P, Y, maxit, reps):
    """MEGA / GSEM as bwgr_amd.uvfit._sem2 runs them; ms per stage."""
    names = ("first_stage", "xb", "latent", "ls_beta", "two_design_fit", "products")
    out = {nm: [] for nm in names}
    k = Y.shape[1]
    for rep in range(reps + 1):
        s1, t1 = timed(api._uvb_panel, P, Y, 0, maxit, 0.0, 20.0)
        G, t2 = timed(P.xb, s1["b"])
        if which == "MEGA":
            LS, t3 = timed(api._mega_latent, Y, G, -1, "probe")
            lsb, t4 = timed(api._uvb_panel, P, LS, 0, maxit, 0.0, 20.0)
        else:
            (LS, V), t3 = timed(api._sem_latent, G, -1, "probe")
            t4 = 0.0
        s, t5 = timed(api._uvb2_panel, P, Y, LS, maxit, 0.0, 20.0)
        if which == "MEGA":
            b = lsb["b"] @ s["b1"] + s["b2"]
            _, t6 = timed(P.xb, np.hstack([s["b2"], b]))
        else:
            b = s1["b"] @ (V @ s["b1"]) + s["b2"]
            _, t6 = timed(P.xb, s["b2"])
        ran = int(np.sum(s["its"] == maxit))      # a trait whose variance update leaves the rails stops on its NaN cnv
        if rep:
            for nm, t in zip(names, (t1, t2, t3, t4, t5, t6)):
                out[nm].append(t)
    row = {"driver": which, "k": k, "npc": int(LS.shape[1]), "maxit": maxit, "traits_that_ran_maxit": ran, "its": [int(v) for v in s["its"]],
           "traits_with_finite_b": int(np.sum(np.isfinite(b).all(0)))}
    for nm in names:
        row[nm + "_ms"] = round(med(out[nm]), 3); row[nm + "_spread"] = spread(out[nm])
    row["total_ms"] = round(sum(med(out[nm]) for nm in names), 3)
    return row


def probe(n=5000, p=50000, ks=(16, 64), reps=3, frac=0.2, maxit=5):
    X = synth.genotypes(n, p, device=0)
    P = bwgr_amd.Panel(X, n=n, device=0)
    rng = np.random.default_rng(100)
    kmax = max(ks)
    G = np.stack([synth.phenotype(X, n, seed=100 + t).cpu().numpy() for t in range(8)], 1)
    G = (G - G.mean(0)) / G.std(0)
    mix = rng.normal(size=(8, kmax)) * np.linspace(2.0, 0.5, 8)[:, None]   # eight genetic factors of decreasing weight: a latent space to find
    Y = G @ mix + rng.normal(size=(n, kmax))
    Y[rng.random((n, kmax)) < frac] = np.nan
    rows, drivers = [], []
    for k in ks:
        Yk = np.asfortranarray(Y[:, :k])
        Z = rng.normal(size=(n, k)) * (4.0 / (1.0 + np.arange(k))) + rng.normal(size=k)
        rows.append(sweeps(P, Yk, Z, reps))              # q = k dense columns on falling scales, drawn apart from Y: a step's cost does not
                                                         # depend on Z's values, and a Z that spans y can send the variance updates off the rails
        print(json.dumps(rows[-1]), flush=True)
    Y16 = np.asfortranarray(Y[:, :16])
    for which in ("MEGA", "GSEM"):
        drivers.append(driver(which, P, Y16, maxit, reps))
        print(json.dumps(drivers[-1]), flush=True)
    P.close()
    summary = {"n": n, "p": p, "missing": frac, "sweeps": rows, "drivers": drivers, "bar_holds": bool(all(r["bar_holds"] for r in rows))}
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    r = probe(ks=(16,), reps=1) if "--quick" in sys.argv else probe()
    sys.exit(0 if r["bar_holds"] else 1)   # the required bar
