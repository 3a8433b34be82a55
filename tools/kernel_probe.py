"""Speed of the exact X X' product (bwgr_panel_crossprod) beside what a user can do today on the same GPU without it: torch.mm on an fp32
copy of the panel (exact for 0/1/2 codes while the sums stay below 2^24), and an fp16-input torch.mm for information.  Also one full GRM call
(product + centring + finish, to a device and to a host array).

Panels: bwgr_synth_genotypes from the BASELINE seed.  Every shape is warmed up first; the contenders alternate within one process, `--reps`
times each; device events bracket synchronised work.  Operations are counted from the shapes -- n (n + 1) / 2 * p multiply-adds, two
operations each (the upper triangle with the diagonal) -- not from what the tiles issue.  The nominal int8 matrix peak (5 POP/s dense) is an
unmeasured figure: the share is labelled so.  Writes one JSON file.

    python tools/kernel_probe.py [--shapes 5000x50000,10000x100000] [--reps 5] [--out profiles/xxt_crossprod_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bwgr_amd  # noqa: E402
from bwgr_amd import _lib, synth  # noqa: E402

NOMINAL_INT8_OPS = 5.0e15


def timed(fn):
    """(device ms between two events on the current stream, wall ms) of fn(), which leaves the device idle"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v), "all_ms": v}


def probe(n, p, reps, with_f16):
    L = _lib.lib()
    X = synth.genotypes(n, p)                       # (p, ld) int8: row j = marker j
    P = bwgr_amd.Panel(X, n=n)
    G = torch.empty((n, n), dtype=torch.int64, device=X.device)
    K = torch.empty((n, n), dtype=torch.float64, device=X.device)
    Xf = X[:, :n].to(torch.float32)                 # (p, n): G = Xf' Xf
    Xh = X[:, :n].to(torch.float16) if with_f16 else None
    torch.cuda.synchronize()

    def ours():
        _lib.check(L.bwgr_panel_crossprod(P._h, C.c_void_p(G.data_ptr()), n, 1))

    def grm_dev():
        _lib.check(L.bwgr_panel_kernel(P._h, 0, 1.0, 0, C.c_void_p(K.data_ptr()), n, 1))

    out32 = torch.empty((n, n), dtype=torch.float32, device=X.device)
    out16 = torch.empty((n, n), dtype=torch.float16, device=X.device) if with_f16 else None
    contenders = [("crossprod", ours), ("torch_mm_f32", lambda: torch.mm(Xf.T, Xf, out=out32))]
    if with_f16:
        contenders.append(("torch_mm_f16", lambda: torch.mm(Xh.T, Xh, out=out16)))
    contenders.append(("grm_device_out", grm_dev))
    for _, f in contenders:                          # warm-up of every contender at this shape
        f(); f()
    torch.cuda.synchronize()
    exact = bool(torch.equal(G, out32.to(torch.int64)))   # fp32 sums of 0/1/2 codes are exact below 2^24
    dev = {k: [] for k, _ in contenders}
    for _ in range(reps):
        for k, f in contenders:
            dev[k].append(timed(f)[0])
    host = [timed(lambda: P.kernel("GRM"))[1] for _ in range(max(2, reps // 2))]   # product + centring + finish + copy to a host array (wall clock)
    res = {k: summary(v) for k, v in dev.items()}
    res["grm_host_out_wall"] = summary(host)
    ops = float(n) * (n + 1) / 2 * p * 2
    rate = ops / (res["crossprod"]["median_ms"] * 1e-3)
    a, b = res["crossprod"], res["torch_mm_f32"]
    info = {"n": n, "p": p, "geometry": {"block": P.block, "nwg": P.nwg, "slab_rows": P.slab_rows}, "reps": reps, "timings": res,
            "int8_ops_counted": ops, "int8_ops_per_s": rate, "share_of_nominal_5_POPs_unmeasured_peak": rate / NOMINAL_INT8_OPS,
            "x_bytes_read_per_call": "not measured", "crossprod_equals_fp32_mm": exact,
            "clearly_faster_than_f32_mm": bool(a["median_ms"] + a["spread_ms"] + b["spread_ms"] < b["median_ms"]),
            "speedup_over_f32_mm": b["median_ms"] / a["median_ms"]}
    P.close()
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5000x50000,10000x100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-f16", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "xxt_crossprod_probe.json"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least five alternating repeats"
    res = {"device": torch.cuda.get_device_name(0), "seed": synth.SEED, "shapes": []}
    for s in a.shapes.split(","):
        n, p = (int(v) for v in s.split("x"))
        r = probe(n, p, a.reps, not a.no_f16)
        res["shapes"].append(r)
        t = r["timings"]
        print("%d x %d: crossprod %.2f ms (spread %.2f), torch.mm f32 %.2f ms (spread %.2f), %.1f TOP/s = %.1f %% of nominal 5 POP/s (unmeasured peak), "
              "GRM device %.2f ms, GRM host %.1f ms, exact %s, clearly faster %s"
              % (n, p, t["crossprod"]["median_ms"], t["crossprod"]["spread_ms"], t["torch_mm_f32"]["median_ms"], t["torch_mm_f32"]["spread_ms"],
                 r["int8_ops_per_s"] / 1e12, 100 * r["share_of_nominal_5_POPs_unmeasured_peak"], t["grm_device_out"]["median_ms"],
                 t["grm_host_out_wall"]["median_ms"], r["crossprod_equals_fp32_mm"], r["clearly_faster_than_f32_mm"]), flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out, "ok": all(r["clearly_faster_than_f32_mm"] and r["crossprod_equals_fp32_mm"] for r in res["shapes"])}))


if __name__ == "__main__":
    main()
