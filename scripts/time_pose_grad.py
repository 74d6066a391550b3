#!/usr/bin/env python3
"""Times the cuboid route's geometric backward (mvhmr::unprojection_cuboid_backward_geometry: k_bwd_geom with its pose epilogue,
k_geom_reduce, k_pose_reduce, after the channels-last layout pass) against the tensor route's (mvhmr::unprojection_backward_geometry)
at the north-star shape, alternating three ops in one process: the tensor-route op (grad_proj and grad_coords), the cuboid op with
proj, rot and center, and the cuboid op with rot and center only.  Also times the DLT backward (mvhmr::triangulate_dlt_backward) at
B 32, V 4.  Device events around each call; prints one JSON line with the medians and spreads.

    python scripts/time_pose_grad.py [--batch 32 --grid 64 --channels 256 --views 4 --feat 96 --method softmax --reps 10]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import ring_projections  # noqa: E402
from multiviewhmr_amd import _capi, aggregation, volumetric  # noqa: E402


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
        raise SystemExit("time_pose_grad.py needs a HIP device")
    dev = torch.device("cuda:0")
    B, S, C, V, HW = a.batch, a.grid, a.channels, a.views, a.feat
    torch.manual_seed(0)
    f = torch.randn(B, V, C, HW, HW, device=dev)
    p = torch.from_numpy(ring_projections(B, V, (HW, HW), seed=0)).to(dev)
    rng = np.random.default_rng(0)
    rot = torch.from_numpy(volumetric.get_rotation_matrices([0, 0, 1], rng.uniform(0, 2 * np.pi, B)).astype(np.float32)).to(dev)
    cen = torch.from_numpy(rng.normal(0, 100.0, (B, 3)).astype(np.float32)).to(dev)
    pos, sides = [-1250.0] * 3, [2500.0] * 3
    c = torch.empty(B, S, S, S, 3, dtype=torch.float32, device=dev)          # the same voxels as a coordinate tensor
    L = _capi.lib()
    _capi.check(L.mvhmr_build_coord_volumes(aggregation._ptr(c), aggregation._ptr(rot), aggregation._ptr(cen), B, S, (ctypes.c_double * 3)(*pos),
                                            (ctypes.c_double * 3)(*sides), aggregation._stream(dev)))
    g = torch.randn(B, C, S, S, S, device=dev)
    m = _capi.AGG[a.method]
    cub = (pos, sides, [S, S, S], m, _capi.F32, 0)
    uv = torch.full((V, 2), HW / 2.0, device=dev)
    gx = torch.randn(B, 3, device=dev)
    ops = {
        "tensor_geometry": lambda: torch.ops.mvhmr.unprojection_backward_geometry(g, f, p, c, m, _capi.F32, 0),
        "cuboid_proj_rot_center": lambda: torch.ops.mvhmr.unprojection_cuboid_backward_geometry(g, f, p, rot, cen, *cub, True, True, True),
        "cuboid_rot_center": lambda: torch.ops.mvhmr.unprojection_cuboid_backward_geometry(g, f, p, rot, cen, *cub, False, True, True),
        "dlt_backward": lambda: torch.ops.mvhmr.triangulate_dlt_backward(gx, p, uv, None),
    }
    times = {k: [] for k in ops}
    for i in range(a.warmup + a.reps):
        for name, fn in ops.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    res = {"shape": "B%d S%d C%d V%d %dx%d %s" % (B, S, C, V, HW, HW, a.method)}
    for k, v in times.items():
        res[k + "_ms"] = statistics.median(v)
        res[k + "_spread_ms"] = [min(v), max(v)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
