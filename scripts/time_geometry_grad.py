#!/usr/bin/env python3
"""Times the geometric backward (mvhmr::unprojection_backward_geometry: k_bwd_geom + k_geom_reduce, after the channels-last layout
pass) against the feature backward (mvhmr::unprojection_backward) at the north-star shape, alternating the two in one process.
Device events around each call; prints one JSON line with the median milliseconds of both and the geometric pass's algorithmic
bytes (B C N sizeof(grad_out) + B V C Hf Wf sizeof(feat) + 2 B N 12 + 2 B V 48) over its median time.

    python scripts/time_geometry_grad.py [--batch 32 --grid 64 --channels 256 --views 4 --feat 96 --method softmax --reps 10]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import cuboid_volume, ring_projections  # noqa: E402
from multiviewhmr_amd import _capi, aggregation  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--feat", type=int, default=96)
    ap.add_argument("--method", default="softmax")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_geometry_grad.py needs a HIP device")
    dev = torch.device("cuda:0")
    B, S, C, V, HW = a.batch, a.grid, a.channels, a.views, a.feat
    N = S ** 3
    torch.manual_seed(0)
    f = torch.randn(B, V, C, HW, HW, device=dev)
    p = torch.from_numpy(ring_projections(B, V, (HW, HW), seed=0)).to(dev)
    c = torch.from_numpy(cuboid_volume(1, S)).to(dev).expand(B, S, S, S, 3).contiguous()
    g = torch.randn(B, C, S, S, S, device=dev)
    m = _capi.AGG[a.method]
    feat_bwd = lambda: torch.ops.mvhmr.unprojection_backward(g, f, p, c, m, _capi.F32, 0)                    # noqa: E731
    geom_bwd = lambda: torch.ops.mvhmr.unprojection_backward_geometry(g, f, p, c, m, _capi.F32, 0)           # noqa: E731
    times = {"feature_backward": [], "geometry_backward": []}
    for i in range(a.warmup + a.reps):
        for name, fn in (("feature_backward", feat_bwd), ("geometry_backward", geom_bwd)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    alg = B * C * N * 4 + B * V * C * HW * HW * 4 + 2 * B * N * 12 + 2 * B * V * 48
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"shape": "B%d S%d C%d V%d %dx%d %s" % (B, S, C, V, HW, HW, a.method),
                      "feature_backward_ms": med["feature_backward"], "geometry_backward_ms": med["geometry_backward"],
                      "geometry_spread_ms": [min(times["geometry_backward"]), max(times["geometry_backward"])],
                      "geometry_alg_bytes": alg, "geometry_alg_TBps": alg / med["geometry_backward"] / 1e9}))


if __name__ == "__main__":
    main()
