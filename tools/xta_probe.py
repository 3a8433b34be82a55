"""Timing probe (GPU box) of the transpose product X_c'A (bwgr_panel_xta) and of mrr_svd on the resident panel.

    python tools/xta_probe.py [--quick] [--out profiles/xta_probe.json]     one JSON line per measurement, all of them in the file

(a) xta      bwgr_panel_xta, device to device, centred, on bwgr_synth_genotypes panels: 5 000 x 50 000 with k = 1, 4, 16 and 10 000 x 1 000 000
             with k = 16; five repetitions after a warm-up, device events, min - max.  At the first shape, in the same run and alternating
             with it, torch.mm(Xd.T, A) on an fp64 device copy Xd (n x p) of the same panel: the yardstick.  Bar: at k = 16 the int8 kernel's
             minimum is at most torch.mm's minimum (the same flops on an eighth of the bytes; min against min absorbs the run-to-run spread).
             Also the achieved fp64 FMA/s (n p k multiply-adds over the call's device time: the staging kernels are in it) beside the vector
             peak, 39.3e12 FMA/s (78.6 TFLOP/s fp64, half the fp32 vector rate of 157.3), and the genotype bytes per second.
(b) mrr_svd  config 2's shape (n = 5 000, p = 50 000), 20 % missing, k = 4 and 16: ms for the Gram matrix, the double centring and eigh, a sweep
             of bwgr_mrr_svd_fit on the device-resident design, and the back-map; a sweep of mkr's train (mrr(Y, dense(X))) on the same X in the
             same run -- bar: the new fit's sweep is at most mkr's plus three of mkr's min - max spreads (the same kernels; the reduction mode
             and the host tail differ) -- and, beside them and not barred, mrr's sweep on the panel.  A sweep is (a fit of 2 + its sweeps minus
             a fit of 2) / its, so the set-up cancels; every timed fit is checked to have run every sweep it was asked for.
--quick: the first shape only, k = 4 in (b), three repetitions."""
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
from bwgr_amd import _lib, svd, synth  # noqa: E402

FMA_PEAK = 39.3e12


def event_ms(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def span(v):
    return {"min": round(min(v), 4), "max": round(max(v), 4), "mean": round(float(np.mean(v)), 4), "reps": len(v)}


def xta_part(n, p, ks, reps, yardstick, emit):
    L = _lib.lib()
    X = synth.genotypes(n, p)                        # (p, ld) int8
    P = bwgr_amd.Panel(X, n=n)
    Xd = X[:, :n].t().to(torch.float64).contiguous() if yardstick else None      # n x p fp64
    for k in ks:
        g = torch.Generator(device="cuda").manual_seed(7 + k)
        A = torch.randn((k, n), dtype=torch.float64, device="cuda", generator=g).t()        # n x k, column-major
        out = torch.empty((k, p), dtype=torch.float64, device="cuda").t()                     # p x k, column-major
        torch.cuda.synchronize()

        def ours():
            _lib.check(L.bwgr_panel_xta(P._h, C.c_void_p(A.data_ptr()), n, k, 1, 1, C.c_void_p(out.data_ptr()), p))

        def theirs():
            return torch.mm(Xd.T, A)

        contenders = [("xta", ours)] + ([("torch_mm_fp64", theirs)] if yardstick else [])
        for _, f in contenders:
            f(); f()
        ms = {name: [] for name, _ in contenders}
        for _ in range(reps):
            for name, f in contenders:
                ms[name].append(event_ms(f))
        rec = {"probe": "xta", "n": n, "p": p, "k": k, "slab_rows": P.slab_rows, "plan": svd.xta_plan(n, p, k, P.slab_rows), "xta_ms": span(ms["xta"]),
               "fma_per_s": float(n) * p * k / (min(ms["xta"]) * 1e-3), "fma_peak": FMA_PEAK, "genotype_bytes_per_s": float(n) * p / (min(ms["xta"]) * 1e-3)}
        rec["share_of_fma_peak"] = round(rec["fma_per_s"] / FMA_PEAK, 4)
        if yardstick:
            ref = torch.mm(Xd.T, A) - torch.outer(Xd.mean(0), A.sum(0))
            ours()
            torch.cuda.synchronize()
            rec["scaled_diff_to_torch"] = float((out - ref).abs().max() / ref.abs().max())
            rec["torch_mm_fp64_ms"] = span(ms["torch_mm_fp64"])
            if k == 16:
                rec["bar_xta_min_at_most_torch_min"] = bool(min(ms["xta"]) <= min(ms["torch_mm_fp64"]))
        emit(rec)
    P.close()
    return X


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


def svd_part(X, n, p, ks, reps, emit):
    P = bwgr_amd.Panel(X, n=n)
    svd.svd_design(P)                                # warm-up: the product's and eigh's first calls
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    G = P.crossprod(device_out=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    D = svd.svd_design(P)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    Xd, r = D["X"], int(D["X"].shape[1])
    del G
    emit({"probe": "design", "n": n, "p": p, "r": r, "gram_ms": round(1e3 * (t1 - t0), 2), "gram_centring_eigh_ms": round(1e3 * (t2 - t1), 2)})
    for k in ks:
        Y = traits(X, n, k, 0.2, seed=100)
        fit = per_sweep(lambda s: svd.mrr_svd_fit(Y, Xd, maxit=s, tol=0.0), lambda q: q["Its"], 6, reps)
        mkr = per_sweep(lambda s: bwgr_amd.mrr(Y, bwgr_amd.dense(Xd), maxit=s, tol=0), lambda q: q["Its"], 6, reps)
        fit2 = per_sweep(lambda s: svd.mrr_svd_fit(Y, Xd, maxit=s, tol=0.0), lambda q: q["Its"], 6, reps)
        mrr = per_sweep(lambda s: bwgr_amd.mrr(Y, P, maxit=s, tol=0), lambda q: q["Its"], 2, max(2, reps // 2))
        f = svd.mrr_svd_fit(Y, Xd, maxit=3, tol=0.0)
        coef = D["U"] @ (torch.from_numpy(f["b"]).cuda() / D["d"][:, None])
        svd.panel_xta(P, coef, True)
        back = [event_ms(lambda: svd.panel_xta(P, coef, True)) for _ in range(reps)]
        both = fit + fit2
        spread = max(mkr) - min(mkr)
        emit({"probe": "mrr_svd", "n": n, "p": p, "r": r, "k": k, "missing": 0.2, "fit_ms_per_sweep": span(both), "mkr_ms_per_sweep": span(mkr),
              "mrr_panel_ms_per_sweep": span(mrr), "backmap_ms": span(back), "bar_ms": round(float(np.mean(mkr)) + 3 * spread, 4),
              "bar_fit_sweep_at_most_mkr_plus_three_spreads": bool(float(np.mean(both)) <= float(np.mean(mkr)) + 3 * spread)})
    P.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "xta_probe.json"))
    a = ap.parse_args()
    reps = 3 if a.quick else 5
    res = {"device": torch.cuda.get_device_name(0), "seed": synth.SEED, "records": []}

    def emit(rec):
        res["records"].append(rec)
        print(json.dumps(rec), flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    X = xta_part(5000, 50000, [1, 4, 16], reps, True, emit)
    svd_part(X, 5000, 50000, [4] if a.quick else [4, 16], reps, emit)
    del X
    torch.cuda.empty_cache()
    if not a.quick:
        xta_part(10000, 1000000, [16], reps, False, emit)


if __name__ == "__main__":
    main()
