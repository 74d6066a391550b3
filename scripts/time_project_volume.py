#!/usr/bin/env python3
"""Times project_volume_cuboid against the torch recipe it replaces, on the same inputs: the points o + lambda_k d of
every pixel and sample built with torch ops from the op's own ranges, taken to the normalised grid, the 5-D grid_sample (bilinear, zeros,
align_corners=True), then the reduction over k.  The recipe is the baseline.  Shapes: the heat volumes of a batch (B 32, J 17, 64^3, four
64 x 64 maps, K 64) in float32 and bfloat16, and the 80 x 80 x 20 root volume with one channel; all three methods.  Each forward alone and
forward + backward w.r.t. the volume, the peak memory each adds to its inputs, and the op's kernels alone from a graph replay.  One
process, a soak, the candidates alternated, device events; prints one JSON line with medians and spreads (ms).

    python scripts/time_project_volume.py [--reps 5 --warmup 2 --out profiles/r18_project_volume.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from multiviewhmr_amd import aggregation, volproject  # noqa: E402

SHAPES = {"heat_f32": dict(B=32, C=17, shape=(64, 64, 64), dtype="float32"), "heat_bf16": dict(B=32, C=17, shape=(64, 64, 64), dtype="bfloat16"),
          "root_f32": dict(B=32, C=1, shape=(80, 80, 20), dtype="float32")}
V, MAP, K, BETA = 4, (64, 64), 64, 1.0


def _look_at(eye, focal):
    eye = torch.tensor(eye, dtype=torch.float64)
    fwd = -eye / eye.norm()
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
    right = right / right.norm()
    Rc = torch.stack([right, torch.linalg.cross(fwd, right), fwd])
    Kc = torch.tensor([[focal, 0.0, (MAP[1] - 1) / 2.0], [0.0, focal, (MAP[0] - 1) / 2.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return Kc @ torch.cat([Rc, (-Rc @ eye)[:, None]], 1)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _graphed(fn):
    """fn captured on a side stream after a warm-up: the replay runs its kernels alone, without the host side of the call"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        keep = fn()
    return lambda: (graph.replay(), keep)[1]


def time_shape(name, method, a, dev):
    s = SHAPES[name]
    B, C, shape, dtype = s["B"], s["C"], s["shape"], getattr(torch, s["dtype"])
    torch.manual_seed(0)
    sides = [2500.0, 2500.0, 2500.0 * shape[2] / shape[0]]
    pos = [-x / 2 for x in sides]
    rot = torch.linalg.qr(torch.randn(B, 3, 3, device=dev))[0].contiguous()
    cen = torch.zeros(B, 3, device=dev)
    P = torch.stack([_look_at([3500.0 * math.cos(1.57 * v + 0.3), 3500.0 * math.sin(1.57 * v + 0.3), 600.0], 75.0) for v in range(V)])
    rays = volproject.camera_rays(P[None].expand(B, V, 3, 4).to(dev))
    vol = torch.randn(B, C, *shape, device=dev).to(dtype).requires_grad_(True)
    g = torch.randn(B, V, C, *MAP, device=dev)
    with torch.no_grad():
        ranges = volproject.project_volume_cuboid(vol, rays, rot, cen, pos, sides, MAP, K, return_ranges=True)[1]
    hit = ranges[..., 0] < ranges[..., 1]
    u, v = torch.meshgrid(torch.arange(MAP[1], device=dev, dtype=torch.float32), torch.arange(MAP[0], device=dev, dtype=torch.float32), indexing="xy")
    pix = torch.stack([u, v, torch.ones_like(u)], -1)
    step = torch.tensor([x / (n - 1) for x, n in zip(sides, shape)], device=dev)
    pos_t, size = torch.tensor(pos, device=dev), torch.tensor([n - 1.0 for n in shape], device=dev)

    def torch_fwd():
        d = torch.einsum("bvij,hwj->bvhwi", rays[..., :3], pix)
        lam = ranges[..., :1] + (torch.arange(K, device=dev) + 0.5) * ((ranges[..., 1:] - ranges[..., :1]) / K)
        x = rays[:, :, None, None, None, :, 3] + lam[..., None] * d[..., None, :]
        c = cen[:, None, None, None, None]
        t = (torch.einsum("bia,bvhwki->bvhwka", rot, x - c) + (c - pos_t)) / step
        grid = (2 * t / size - 1).flip(-1).reshape(B, V * MAP[0], MAP[1], K, 3)
        smp = F.grid_sample(vol.float(), grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(B, C, V, *MAP, K)
        out = smp.mean(-1) if method == "mean" else smp.amax(-1) if method == "max" else (torch.softmax(BETA * smp, -1) * smp).sum(-1)
        return (out * hit[:, None]).transpose(1, 2)

    def backward_of(fwd):
        return lambda: torch.autograd.grad((fwd() * g).sum(), vol)

    new_fwd = lambda: volproject.project_volume_cuboid(vol, rays, rot, cen, pos, sides, MAP, K, method, beta=BETA)     # noqa: E731
    runs = {"new fwd": new_fwd, "new fwd+bwd": backward_of(new_fwd), "torch fwd": torch_fwd, "torch fwd+bwd": backward_of(torch_fwd)}
    with torch.no_grad():                                                     # the two compute the same thing: said once, before anything is timed
        agree = float((new_fwd() - torch_fwd()).abs().max())
    peak = {}
    for k, fn in runs.items():
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated(dev) - base
    runs["new fwd kernels"] = _graphed(new_fwd)
    runs["new fwd+bwd kernels"] = _graphed(backward_of(new_fwd))
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
    res = {"shape": "B%d C%d %s %s, %d maps %dx%d, K %d, %s" % (B, C, "x".join(map(str, shape)), s["dtype"], V, MAP[0], MAP[1], K, method),
           "volume_bytes": vol.numel() * vol.element_size(), "rays_that_hit": round(float(hit.float().mean()), 4), "max_abs_vs_torch": agree,
           "workspace_bytes": aggregation._capi.lib().mvhmr_project_volume_workspace_bytes(B, C, *shape)}
    for k, v in times.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
        res[k + "_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
        if k in peak:
            res[k + "_peak_bytes"] = int(peak[k])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--soak-ms", type=float, default=500.0)
    ap.add_argument("--shapes", default="heat_f32,heat_bf16,root_f32")
    ap.add_argument("--methods", default="mean,max,softmax")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_project_volume.py needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"reps": a.reps, "warmup": a.warmup, "soak_ms": a.soak_ms}
    for name in a.shapes.split(","):
        for method in a.methods.split(","):
            res["%s_%s" % (name, method)] = time_shape(name, method, a, dev)
            torch.cuda.empty_cache()
            print(json.dumps({"%s_%s" % (name, method): res["%s_%s" % (name, method)]}), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
