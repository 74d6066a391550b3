#!/usr/bin/env python3
"""Times the feature-gradient backward in its default form (mvhmr::unprojection_backward) and its deterministic form
(mvhmr::unprojection_backward_deterministic) at the north-star shape, alternating them in one process, the deterministic one with
torch's NaN fill of new memory on and off (torch.utils.deterministic.fill_uninitialized_memory: it applies to the op's output tensor;
the workspace bypasses it).  Also times one fused-route step (_FusedAggregate forward + backward: 1x1 conv, cuboid un-projection and their
gradients) with the deterministic flag off and on.  Device events around each call; prints one JSON line with the medians and spreads.

    python scripts/time_deterministic_bwd.py [--batch 32 --grid 64 --channels 256 --views 4 --feat 96 --method softmax --reps 5]
    python scripts/time_deterministic_bwd.py --only-deterministic --reps 2     # a short run for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.utils.deterministic  # noqa: E402

from bench import ring_projections  # noqa: E402
from multiviewhmr_amd import _capi, aggregation, volumetric  # noqa: E402


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--feat", type=int, default=96)
    ap.add_argument("--method", default="softmax")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only-deterministic", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_deterministic_bwd.py needs a HIP device")
    dev = torch.device("cuda:0")
    B, S, C, V, HW = a.batch, a.grid, a.channels, a.views, a.feat
    torch.manual_seed(0)
    f = torch.randn(B, V, C, HW, HW, device=dev)
    p = torch.from_numpy(ring_projections(B, V, (HW, HW), seed=0)).to(dev)
    ax = torch.linspace(-1000.0, 1000.0, S, device=dev)
    c = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)[None].expand(B, S, S, S, 3).contiguous()
    g = torch.randn(B, C, S, S, S, device=dev)
    m = _capi.AGG[a.method]

    def det(fill):
        def run():
            torch.use_deterministic_algorithms(True)
            torch.utils.deterministic.fill_uninitialized_memory = fill
            try:
                torch.ops.mvhmr.unprojection_backward_deterministic(g, f, p, c, m, _capi.F32, 0)
            finally:
                torch.use_deterministic_algorithms(False)
                torch.utils.deterministic.fill_uninitialized_memory = True
        return run

    ops = {"deterministic_fill_on": det(True), "deterministic_fill_off": det(False)}
    if not a.only_deterministic:
        ops = {"default": lambda: torch.ops.mvhmr.unprojection_backward(g, f, p, c, m, _capi.F32, 0), **ops}
    times = {k: [] for k in ops}
    for i in range(a.warmup + a.reps):
        for name, fn in ops.items():
            t = _timed(fn)
            if i >= a.warmup:
                times[name].append(t)
    res = {"shape": "B%d S%d C%d V%d %dx%d %s" % (B, S, C, V, HW, HW, a.method)}
    for k, v in times.items():
        res[k + "_ms"] = statistics.median(v)
        res[k + "_spread_ms"] = [min(v), max(v)]
    if "default_ms" in res:
        res["ratio_deterministic_fill_off"] = res["deterministic_fill_off_ms"] / res["default_ms"]
        # what torch's fill would cost if the workspace came from torch.empty: the fill of a buffer of the workspace's size
        import ctypes
        desc = aggregation._make_desc(f, c, m, torch.float32, _capi.LAYOUT_BVCHW, _capi.VARIANT["auto"])
        n = _capi.lib().mvhmr_unproject_backward_deterministic_workspace_bytes(ctypes.byref(desc))
        fills = []
        for i in range(a.warmup + a.reps):
            torch.use_deterministic_algorithms(True)
            try:
                t = _timed(lambda: torch.empty(n, dtype=torch.uint8, device=dev))
            finally:
                torch.use_deterministic_algorithms(False)
            if i >= a.warmup:
                fills.append(t)
        res["workspace_bytes"] = n
        res["workspace_fill_if_torch_empty_ms"] = statistics.median(fills)
    del g, f

    if not a.only_deterministic:
        # the fused route's step: conv 256 -> 256 (the deterministic wgrad applies: C_in, C_out % 128 == 0), the same volume and maps
        x = torch.randn(B, V, C, HW, HW, device=dev, requires_grad=True)
        w = (torch.randn(C, C, 1, 1, device=dev) * 0.05).requires_grad_(True)
        bias = torch.zeros(C, device=dev, requires_grad=True)
        rng = np.random.default_rng(0)
        rot = torch.from_numpy(volumetric.get_rotation_matrices([0, 0, 1], rng.uniform(0, 2 * np.pi, B)).astype(np.float32)).to(dev)
        cen = torch.from_numpy(rng.normal(0, 100.0, (B, 3)).astype(np.float32)).to(dev)
        go = torch.randn(B, C, S, S, S, device=dev)

        def step(flag):
            def run():
                out = aggregation._FusedAggregate.apply(x, w, bias, p, rot, cen, (-1250.0,) * 3, (2500.0,) * 3, (S, S, S), m)
                torch.use_deterministic_algorithms(flag)
                try:
                    out.backward(go)
                finally:
                    torch.use_deterministic_algorithms(False)
            return run

        steps = {"fused_step_default": step(False), "fused_step_deterministic": step(True)}
        st = {k: [] for k in steps}
        for i in range(a.warmup + a.reps):
            for name, fn in steps.items():
                x.grad = w.grad = bias.grad = None
                t = _timed(fn)
                if i >= a.warmup:
                    st[name].append(t)
        for k, v in st.items():
            res[k + "_ms"] = statistics.median(v)
            res[k + "_spread_ms"] = [min(v), max(v)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
