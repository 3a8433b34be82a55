"""Timing probe (GPU box) of MLM and of its projection (bwgr_amd.mlm).

    python tools/mlm_probe.py [--quick] [--out profiles/mlm_probe.json]     one JSON line per measurement, all of them in the file

(a) project  Zp = Z - X C on a bwgr_synth_genotypes panel of config 2's shape (n = 5 000, p = 50 000) for f = 1, 8, 64, 256: k_project alone
             (bwgr_debug_project_timing: the stream is waited for before and after, wall clock) and, alternating with it in the same run and
             timed the same way, the yardstick  Zd.double() - Xd @ C  in torch from the same int8 tensor and the same C.  Bar 2: at f = 8 the
             kernel's minimum is at most torch's minimum.  f = 1, 64 and 256 are reported, not barred.  Also the one-off costs of a call (X'X and
             its eigen-decomposition, Z'X, C on the host with its copies), the projection's achieved bytes per second (n p int8 bytes read plus
             n p 8 bytes written over the kernel's time, named as such: what moved, not what the memory system did) beside the 8 TB/s HBM rate,
             and the scaled difference to the yardstick.
(b) sweep    the same shape, 20 % missing, f = 8, k = 4 and 16: a sweep of MLM(Y, X, panel) and, in the same run, a sweep of
             mrr(Y, dense(Z)) on the fp64 copy of the same matrix -- the same kernels on a design of the same shape.  Bar 1: MLM's sweep is at
             most that yardstick's plus three of its min - max spreads.  A sweep is (a fit of 2 + its sweeps minus a fit of 2) / its, so the
             set-up cancels; every timed fit is checked to have run every sweep it was asked for.  Also the set-up of an MLM call (a fit of 0
             sweeps) and the plan's workspace.
Five repetitions, min - max.  --quick: f = 8 only in (a), k = 4 only in (b), three repetitions."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bwgr_amd  # noqa: E402
from bwgr_amd import _lib, mlm, synth  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def span(v):
    return {"min": round(min(v), 4), "max": round(max(v), 4), "mean": round(float(np.mean(v)), 4), "reps": len(v)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def covariates(n, f, seed):
    rng = np.random.default_rng(seed)
    nd = min(4, f - 1)
    cols = [np.ones(n)]
    if nd:
        lev = rng.permutation(np.arange(n) % (nd + 1))
        cols += [(lev == l + 1).astype(np.float64) for l in range(nd)]
    cols += [rng.normal(size=n) for _ in range(f - 1 - nd)]
    return np.asfortranarray(np.column_stack(cols).astype(np.float32).astype(np.float64))


def timing(mode=1):
    out = (C.c_double * 4)()
    _lib.check(_lib.lib().bwgr_debug_project_timing(mode, out))
    return [float(v) for v in out]


def project_part(X, P, n, p, fs, reps, emit):
    Zi = X[:, :n]                                      # (p, n) int8: row j = column j of Z
    for f in fs:
        Xh = covariates(n, f, 50 + f)
        Xd = torch.from_numpy(Xh).cuda()
        out = torch.empty((p, n), dtype=torch.float64, device="cuda").t()
        L = _lib.lib()

        def ours():
            _lib.check(L.bwgr_project(0, P._h, None, 0, n, p, n, Xh.ctypes.data_as(_lib.c_d), f, n, C.c_void_p(out.data_ptr()), 1, n))

        Zd = Zi.t().to(torch.float64)
        Cm = torch.linalg.solve(Xd.T @ Xd, Xd.T @ Zd)
        del Zd

        def theirs():
            return Zi.t().double() - Xd @ Cm

        timing(1)
        ours(); theirs(); ours(); theirs()
        ms = {"k_project": [], "torch": [], "host_design": [], "ztx": [], "c_and_copies": [], "call": []}
        for _ in range(reps):
            ms["call"].append(wall_ms(ours))
            t = timing(1)
            for key, v in zip(("host_design", "ztx", "c_and_copies", "k_project"), t):
                ms[key].append(v)
            ms["torch"].append(wall_ms(theirs))
        timing(0)
        ref = theirs()
        diff = float((out - ref).abs().max() / ref.abs().max())
        del ref
        moved = float(n) * p * (1 + 8)
        rec = {"probe": "project", "n": n, "p": p, "f": f, "plan": {k: v for k, v in mlm.mlm_plan(n, p, f, 4, 4).items() if k.startswith(("proj", "f_", "ztx"))},
               "k_project_ms": span(ms["k_project"]), "torch_ms": span(ms["torch"]), "host_design_ms": span(ms["host_design"]), "ztx_ms": span(ms["ztx"]),
               "c_and_copies_ms": span(ms["c_and_copies"]), "whole_call_ms": span(ms["call"]), "scaled_diff_to_torch": diff,
               "achieved_bytes_per_s": moved / (min(ms["k_project"]) * 1e-3), "hbm_bytes_per_s": HBM_BYTES_PER_S}
        rec["share_of_hbm_rate"] = round(rec["achieved_bytes_per_s"] / HBM_BYTES_PER_S, 4)
        if f == 8:
            rec["bar2_kernel_min_at_most_torch_min"] = bool(min(ms["k_project"]) <= min(ms["torch"]))
        emit(rec)
        del out, Cm
        torch.cuda.empty_cache()


def traits(X, n, k, frac, seed):
    G = np.stack([synth.phenotype(X, n, seed=seed + t).cpu().numpy() for t in range(k)], 1)
    G = (G - G.mean(0)) / G.std(0)
    rng = np.random.default_rng(seed)
    Y = G + rng.normal(size=(n, k))
    Y[rng.random((n, k)) < frac] = np.nan
    return Y.astype(np.float32).astype(np.float64)


def wall(f, sweeps, its_of):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f(sweeps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert its_of(r) == sweeps, (its_of(r), sweeps)
    return dt


def per_sweep(f, its_of, its, reps):
    f(1)
    return [1e3 * (wall(f, 2 + its, its_of) - wall(f, 2, its_of)) / its for _ in range(reps)]


def sweep_part(X, P, n, p, f, ks, reps, emit):
    Xh = covariates(n, f, 50 + f)
    Zd = X[:, :n].to(torch.float64).t()                # n x p fp64, column-major: the yardstick's design
    D = bwgr_amd.dense(Zd)
    for k in ks:
        its = 6 if k <= 4 else 3
        Y = traits(X, n, k, 0.2, seed=100)
        a = per_sweep(lambda s: mlm.MLM(Y, Xh, P, maxit=s), lambda q: q["its"], its, reps)
        y = per_sweep(lambda s: bwgr_amd.mrr(Y, D, maxit=s, tol=0), lambda q: q["Its"], its, reps)
        b = per_sweep(lambda s: mlm.MLM(Y, Xh, P, maxit=s), lambda q: q["its"], its, reps)
        setup = [1e3 * wall(lambda s: mlm.MLM(Y, Xh, P, maxit=s), 0, lambda q: q["its"]) for _ in range(reps)]
        both = a + b
        spread = max(y) - min(y)
        npat = len({tuple(np.isnan(Y[:, t])) for t in range(k)})
        emit({"probe": "sweep", "n": n, "p": p, "f": f, "k": k, "missing": 0.2, "mlm_ms_per_sweep": span(both), "mrr_dense_ms_per_sweep": span(y),
              "mlm_setup_ms": span(setup), "ws_bytes": mlm.mlm_plan(n, p, f, k, npat)["ws_bytes"], "bar_ms": round(float(np.mean(y)) + 3 * spread, 4),
              "bar1_mlm_sweep_at_most_yardstick_plus_three_spreads": bool(float(np.mean(both)) <= float(np.mean(y)) + 3 * spread)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "mlm_probe.json"))
    a = ap.parse_args()
    reps = 3 if a.quick else 5
    res = {"device": torch.cuda.get_device_name(0), "seed": synth.SEED, "records": []}

    def emit(rec):
        res["records"].append(rec)
        print(json.dumps(rec), flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    n, p = 5000, 50000
    X = synth.genotypes(n, p)                          # (p, ld) int8
    P = bwgr_amd.Panel(X, n=n)
    project_part(X, P, n, p, [8] if a.quick else [1, 8, 64, 256], reps, emit)
    sweep_part(X, P, n, p, 8, [4] if a.quick else [4, 16], reps, emit)
    P.close()


if __name__ == "__main__":
    main()
