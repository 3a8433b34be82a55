"""Speed of the exact rectangular product X_f X_s' (bwgr_panel_crossprod2) beside what a user could do without it: the symmetric product
(bwgr_panel_crossprod) of the stacked (n_f + n_s)-row panel, of which X_f X_s' is the off-diagonal block.  Also the founders' own X_f X_f'
and the full founder-by-sample kernels (bwgr_panel_kernel2, both kinds) with device outputs, for information.

Panels: bwgr_synth_genotypes from the BASELINE seed; the founders are the first n_f rows of the stacked panel and the samples the rest.  The
probe first checks that crossprod2 equals the stacked product's off-diagonal block bit for bit.  Every shape is warmed up first; the
contenders alternate within one process, `--reps` times each; device events bracket synchronised work.  Writes one JSON file.

    python tools/xyt_probe.py [--shapes 5000+5000x50000,10000+500x100000] [--reps 5] [--out profiles/xyt_probe.json]
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


def rows(X, lo, hi):
    """rows lo .. hi - 1 of the (p, ld) panel as a (p, ld') tensor of their own, zero-padded to a multiple of 128"""
    n = hi - lo
    out = torch.zeros((X.shape[0], (n + 127) // 128 * 128), dtype=torch.int8, device=X.device)
    out[:, :n] = X[:, lo:hi]
    return out


def probe(nf, ns, p, reps):
    L = _lib.lib()
    n = nf + ns
    X = synth.genotypes(n, p)                       # (p, ld) int8: row j = marker j
    Pall = bwgr_amd.Panel(X, n=n)
    Pf = bwgr_amd.Panel(rows(X, 0, nf), n=nf)
    Ps = bwgr_amd.Panel(rows(X, nf, n), n=ns)
    dev = X.device
    Gall = torch.empty((n, n), dtype=torch.int64, device=dev)
    Gfs = torch.empty((nf, ns), dtype=torch.int64, device=dev)
    Gff = torch.empty((nf, nf), dtype=torch.int64, device=dev)
    Kff = torch.empty((nf, nf), dtype=torch.float64, device=dev)
    Kfs = torch.empty((nf, ns), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731

    def ours():
        _lib.check(L.bwgr_panel_crossprod2(Pf._h, Ps._h, ptr(Gfs), ns, 1))

    def stacked():
        _lib.check(L.bwgr_panel_crossprod(Pall._h, ptr(Gall), n, 1))

    def founders():
        _lib.check(L.bwgr_panel_crossprod(Pf._h, ptr(Gff), nf, 1))

    def kernel2(kind):
        return lambda: _lib.check(L.bwgr_panel_kernel2(Pf._h, Ps._h, kind, 1.0, ptr(Kff), nf, ptr(Kfs), ns, 1))

    contenders = [("crossprod2", ours), ("crossprod_stacked", stacked), ("crossprod_founders", founders), ("kernel2_arc_device_out", kernel2(0)),
                  ("kernel2_gau_device_out", kernel2(1))]
    for _, f in contenders:                          # warm-up of every contender at this shape
        f(); f()
    torch.cuda.synchronize()
    exact = bool(torch.equal(Gfs, Gall[:nf, nf:]))
    dev_ms = {k: [] for k, _ in contenders}
    for _ in range(reps):
        for k, f in contenders:
            dev_ms[k].append(timed(f)[0])
    res = {k: summary(v) for k, v in dev_ms.items()}
    a, b = res["crossprod2"], res["crossprod_stacked"]
    plan = (C.c_int64 * 9)()
    _lib.check(L.bwgr_debug_xyt_plan(nf, ns, p, 2, 2, 0, plan))
    info = {"n_f": nf, "n_s": ns, "p": p, "reps": reps, "timings": res,
            "geometry": {"founders_slab_rows": Pf.slab_rows, "samples_slab_rows": Ps.slab_rows, "stacked_slab_rows": Pall.slab_rows},
            "plan": dict(zip(("chunk", "chunks", "tiles", "workgroups", "ws_bytes", "T_f", "T_s", "pieces", "piece"), (int(v) for v in plan))),
            "multiply_adds": {"crossprod2": float(nf) * ns * p, "crossprod_stacked": float(n) * (n + 1) / 2 * p},
            "crossprod2_ops_per_s": 2.0 * nf * ns * p / (a["median_ms"] * 1e-3),
            "crossprod2_equals_the_stacked_block": exact,
            "clearly_faster_than_stacked": bool(a["median_ms"] + a["spread_ms"] + b["spread_ms"] < b["median_ms"]),
            "speedup_over_stacked": b["median_ms"] / a["median_ms"]}
    Pall.close(); Pf.close(); Ps.close()
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5000+5000x50000,10000+500x100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "xyt_probe.json"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least five alternating repeats"
    res = {"device": torch.cuda.get_device_name(0), "seed": synth.SEED, "shapes": []}
    for s in a.shapes.split(","):
        nn, p = s.split("x")
        nf, ns = (int(v) for v in nn.split("+"))
        r = probe(nf, ns, int(p), a.reps)
        res["shapes"].append(r)
        t = r["timings"]
        print("%d + %d x %s: crossprod2 %.2f ms (spread %.2f), stacked crossprod %.2f ms (spread %.2f), founders' crossprod %.2f ms, "
              "kernel2 ARC %.2f ms, GAU %.2f ms (device outputs), %.1f TOP/s, equal bits %s, clearly faster %s"
              % (nf, ns, p, t["crossprod2"]["median_ms"], t["crossprod2"]["spread_ms"], t["crossprod_stacked"]["median_ms"],
                 t["crossprod_stacked"]["spread_ms"], t["crossprod_founders"]["median_ms"], t["kernel2_arc_device_out"]["median_ms"],
                 t["kernel2_gau_device_out"]["median_ms"], r["crossprod2_ops_per_s"] / 1e12, r["crossprod2_equals_the_stacked_block"],
                 r["clearly_faster_than_stacked"]), flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out, "ok": all(r["clearly_faster_than_stacked"] and r["crossprod2_equals_the_stacked_block"] for r in res["shapes"])}))


if __name__ == "__main__":
    main()
