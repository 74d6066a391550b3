#!/usr/bin/env python3
"""Times the cross-view variance aggregates 'var' and 'meanvar'  against what the library offered before them on the same
inputs -- 'mean' with variant='gather', and with visible_only for the visible form: forward, feature backward and geometry backward, fp32
planar features, B = 8, at the BASELINE configs[1] volume and map sizes and at the north-star ones.  All go through the registered ops
(torch.ops.mvhmr.*), are alternated in one process after a soak (as bench.py: an untimed second of the same work) and are timed with
device events; prints one JSON line with medians and spreads (ms).

    python scripts/time_moments.py [--reps 7 --warmup 2 --out profiles/r14_moments.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import ring_projections  # noqa: E402
from multiviewhmr_amd import _capi, aggregation  # noqa: E402,F401  (registers the ops)

SHAPES = {"configs1": dict(B=8, S=32, C=256, V=4, HW=96), "north_star": dict(B=8, S=64, C=256, V=4, HW=96)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def time_shape(name, a, dev):
    s = SHAPES[name]
    B, S, C, V, HW = s["B"], s["S"], s["C"], s["V"], s["HW"]
    torch.manual_seed(0)
    f = torch.randn(B, V, C, HW, HW, device=dev)
    p = torch.from_numpy(ring_projections(B, V, (HW, HW), seed=0)).to(dev)
    ax = torch.linspace(-1000.0, 1000.0, S, device=dev)
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
    c = torch.stack([grid + 15.0 * b for b in range(B)]).contiguous()
    g = torch.randn(B, 2 * C, S, S, S, device=dev)
    g1 = g[:, :C].contiguous()
    ones = torch.ones(B, V, dtype=torch.uint8, device=dev)
    tail = (_capi.AGG["mean"], _capi.F32, _capi.VARIANT["gather"])
    ops = torch.ops.mvhmr
    runs = {}
    for vis, tag in ((False, ""), (True, "visible ")):
        if vis:                                                                # the parent's visible form: the *_visible family (all views present)
            runs[tag + "mean fwd"] = lambda: ops.unprojection_visible(f, p, c, ones, *tail)
            runs[tag + "mean bwd_features"] = lambda: ops.unprojection_visible_backward(g1, f, p, c, ones, *tail)
            runs[tag + "mean bwd_geometry"] = lambda: ops.unprojection_visible_backward_geometry(g1, f, p, c, ones, *tail, True, True)
        else:
            runs[tag + "mean fwd"] = lambda: ops.unprojection(f, p, c, *tail)
            runs[tag + "mean bwd_features"] = lambda: ops.unprojection_backward(g1, f, p, c, *tail)
            runs[tag + "mean bwd_geometry"] = lambda: ops.unprojection_backward_geometry(g1, f, p, c, *tail, True, True)
        for m, mname, go in ((1, "var", g1), (2, "meanvar", g)):
            runs[tag + mname + " fwd"] = lambda vis=vis, m=m: ops.unprojection_moments(f, p, c, None, vis, m, *tail)
            runs[tag + mname + " bwd_features"] = lambda vis=vis, m=m, go=go: ops.unprojection_moments_backward(go, f, p, c, None, vis, m, *tail)
            runs[tag + mname + " bwd_geometry"] = lambda vis=vis, m=m, go=go: ops.unprojection_moments_backward_geometry(go, f, p, c, None, vis, m, *tail, True, True)
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.soak_ms:                      # untimed soak: clocks and caches as in the timed loop
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for i in range(a.warmup + a.reps):
        for k, fn in runs.items():
            t = _timed(fn)
            if i >= a.warmup:
                times[k].append(t)
    res = {"shape": "B%d S%d C%d V%d %dx%d mean" % (B, S, C, V, HW, HW)}
    for k, v in times.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
        res[k + "_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--soak-ms", type=float, default=1000.0)
    ap.add_argument("--shapes", default="configs1,north_star")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_moments.py needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"reps": a.reps, "warmup": a.warmup, "soak_ms": a.soak_ms}
    res.update({name: time_shape(name, a, dev) for name in a.shapes.split(",")})
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
