#!/usr/bin/env python3
"""Times shared feature maps against what a caller had to do before: M volumes from B feature samples, B = 8, M = 32 (four
volumes per sample, unsorted), forward, feature backward and geometry backward of
    materialised   variant='gather' on features[idx] and proj[idx], as autograd runs it: the forward's timed region holds the index_select
                   of both inputs (whose results a caller keeps for the backward), the backwards' the index_add of the per-volume gradient
                   into the (B, ...) gradient
    shared         the feature_index call on the B samples
on the same inputs, at the BASELINE configs[1] volume and map sizes and at the north-star ones.  Both go through the registered ops
(torch.ops.mvhmr.*), are alternated in one process after a soak (as bench.py: an untimed second of the same work) and are timed with device
events; prints one JSON line with medians and spreads (ms).

    python scripts/time_shared_features.py [--reps 7 --warmup 2 --method softmax --out profiles/r12_shared_features.json]
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

SHAPES = {"configs1": dict(B=8, M=32, S=32, C=256, V=4, HW=96), "north_star": dict(B=8, M=32, S=64, C=256, V=4, HW=96)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def time_shape(name, a, dev):
    s = SHAPES[name]
    B, M, S, C, V, HW = s["B"], s["M"], s["S"], s["C"], s["V"], s["HW"]
    torch.manual_seed(0)
    f = torch.randn(B, V, C, HW, HW, device=dev)
    p = torch.from_numpy(ring_projections(B, V, (HW, HW), seed=0)).to(dev)
    idx = torch.randperm(M, generator=torch.Generator().manual_seed(1)).remainder(B).to(dev)        # every sample four times, unsorted
    idx32 = idx.to(torch.int32)
    ax = torch.linspace(-1000.0, 1000.0, S, device=dev)
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
    c = torch.stack([grid + 15.0 * m for m in range(M)]).contiguous()
    g = torch.randn(M, C, S, S, S, device=dev)
    tail = (_capi.AGG[a.method], _capi.F32, _capi.VARIANT["gather"])
    ops = torch.ops.mvhmr

    fm, pm = f.index_select(0, idx), p.index_select(0, idx)                  # what the materialised forward saves for its backward

    def mat_fwd():
        return ops.unprojection(f.index_select(0, idx), p.index_select(0, idx), c, *tail)

    def mat_bwd():
        return torch.zeros_like(f).index_add_(0, idx, ops.unprojection_backward(g, fm, pm, c, *tail))

    def mat_geo():
        gp, gc = ops.unprojection_backward_geometry(g, fm, pm, c, *tail, True, True)
        return torch.zeros_like(p).index_add_(0, idx, gp), gc

    runs = {
        "materialised fwd": mat_fwd, "shared fwd": lambda: ops.unprojection_shared(f, p, c, idx32, *tail),
        "materialised bwd_features": mat_bwd, "shared bwd_features": lambda: ops.unprojection_shared_backward(g, f, p, c, idx32, *tail),
        "materialised bwd_geometry": mat_geo, "shared bwd_geometry": lambda: ops.unprojection_shared_backward_geometry(g, f, p, c, idx32, *tail, True, True),
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
    res = {"shape": "B%d M%d S%d C%d V%d %dx%d %s" % (B, M, S, C, V, HW, HW, a.method)}
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
        raise SystemExit("time_shared_features.py needs a HIP device")
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
