#!/usr/bin/env python3
"""Times the lens-distortion-aware un-projection against the plain variant='gather' call on the same inputs: forward,
feature backward and geometry backward, softmax, fp32 planar features, at the BASELINE configs[1] volume and map sizes and at the
north-star ones.  The lens is a barrel + tangential one (k1 = -0.2, k2 = 0.05, p1 = 0.001, p2 = -0.002) under the rig's own intrinsics.  Both
go through the registered ops (torch.ops.mvhmr.*), are alternated in one process after a soak (as bench.py: an untimed second of the same
work) and are timed with device events; prints one JSON line with medians and spreads (ms).

    python scripts/time_lens.py [--reps 7 --warmup 2 --method softmax --out profiles/r13_lens.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
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


def lens_records(B, V, HW):
    """one record per (sample, view): the feature-level intrinsics of bench.ring_projections' cameras (f = 1145 px and the principal point
    (512, 512) of a 1000 x 1000 sensor, cropped to (200, 200, 824, 824) and resized to the map), the script's coefficients"""
    k = (-0.2, 0.05, 0.001, -0.002, 0.0)
    rec = np.zeros((B, V, 10), np.float32)
    rec[..., :4] = (1145.0 * HW / 624.0, 1145.0 * HW / 624.0, 312.0 * HW / 624.0, 312.0 * HW / 624.0)
    rec[..., 4:9] = k
    rec[..., 9] = aggregation.lens_r2max(k[0], k[1], k[4])
    return rec


def time_shape(name, a, dev):
    s = SHAPES[name]
    B, S, C, V, HW = s["B"], s["S"], s["C"], s["V"], s["HW"]
    torch.manual_seed(0)
    f = torch.randn(B, V, C, HW, HW, device=dev)
    p = torch.from_numpy(ring_projections(B, V, (HW, HW), seed=0)).to(dev)
    lens = torch.from_numpy(lens_records(B, V, HW)).to(dev)
    ax = torch.linspace(-1000.0, 1000.0, S, device=dev)
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
    c = torch.stack([grid + 15.0 * b for b in range(B)]).contiguous()
    g = torch.randn(B, C, S, S, S, device=dev)
    tail = (_capi.AGG[a.method], _capi.F32, _capi.VARIANT["gather"])
    ops = torch.ops.mvhmr
    runs = {
        "plain fwd": lambda: ops.unprojection(f, p, c, *tail), "lens fwd": lambda: ops.unprojection_lens(f, p, c, lens, *tail),
        "plain bwd_features": lambda: ops.unprojection_backward(g, f, p, c, *tail),
        "lens bwd_features": lambda: ops.unprojection_lens_backward(g, f, p, c, lens, *tail),
        "plain bwd_geometry": lambda: ops.unprojection_backward_geometry(g, f, p, c, *tail, True, True),
        "lens bwd_geometry": lambda: ops.unprojection_lens_backward_geometry(g, f, p, c, lens, *tail, True, True),
    }
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
    res = {"shape": "B%d S%d C%d V%d %dx%d %s" % (B, S, C, V, HW, HW, a.method)}
    for k, v in times.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
        res[k + "_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", default="softmax")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--soak-ms", type=float, default=1000.0)
    ap.add_argument("--shapes", default="configs1,north_star")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lens.py needs a HIP device")
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
