#!/usr/bin/env python3
"""Times sample_volume_cuboid against the torch composition it replaces, on the same inputs: R^T (x - c) + c built with
torch ops, normalised to [-1, 1], flipped to (z, y, x), then the 5-D grid_sample (bilinear, zeros, align_corners=True).  Two shapes: (a)
every point samples every channel, (b) the paired call of the volumetric cross-entropy, for which the composition samples J x J and takes
the diagonal.  Each forward alone and forward + backward w.r.t. the volume and the points.  One process, a soak, the candidates
alternated, device events; prints one JSON line with medians, spreads (ms) and the peak memory each candidate adds to its inputs.

    python scripts/time_sample_volume.py [--reps 7 --warmup 2 --out profiles/r16_sample_volume.json]
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
import torch.nn.functional as F  # noqa: E402

from multiviewhmr_amd import aggregation, volsample  # noqa: E402

SHAPES = {"a_full": dict(B=32, C=256, S=64, N=1024, paired=False), "b_paired": dict(B=32, C=17, S=64, N=17, paired=True)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def time_shape(name, a, dev):
    s = SHAPES[name]
    B, C, S, N, paired = s["B"], s["C"], s["S"], s["N"], s["paired"]
    torch.manual_seed(0)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=2500.0, device=dev)
    cub = gen.cuboid()
    pos, sides = [float(x) for x in cub.position], [float(x) for x in cub.sides]
    rot = torch.linalg.qr(torch.randn(B, 3, 3, device=dev))[0].contiguous()
    cen = (100.0 * torch.randn(B, 3, device=dev)).contiguous()
    # uniform over the cuboid grown by 2 % per side, placed as the volume is: about 94 % of the points fall inside, the rest just outside
    grid = (torch.rand(B, N, 3, device=dev) * 2 - 1) * (0.51 * 2500.0)
    pts = (torch.einsum("bia,bna->bni", rot, grid - cen[:, None]) + cen[:, None]).requires_grad_(True)
    vol = torch.randn(B, C, S, S, S, device=dev).requires_grad_(True)
    g = torch.randn((B, C) if paired else (B, C, N), device=dev)
    pos_t = torch.tensor(pos, device=dev)
    step = torch.tensor([x / (S - 1) for x in sides], device=dev)

    def torch_fwd():
        d = torch.einsum("bia,bni->bna", rot, pts - cen[:, None])
        t = (d + (cen[:, None] - pos_t)) / step
        grid = (2 * t / (S - 1) - 1).flip(-1)[:, None, None]
        out = F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, :, 0, 0]
        return torch.diagonal(out, dim1=1, dim2=2) if paired else out

    def backward_of(fwd):
        return lambda: torch.autograd.grad((fwd() * g).sum(), (vol, pts))

    new_fwd = lambda: volsample.sample_volume_cuboid(vol, pts, rot, cen, pos, sides, paired=paired)     # noqa: E731
    runs = {"new fwd": new_fwd, "new fwd+bwd": backward_of(new_fwd), "torch fwd": torch_fwd, "torch fwd+bwd": backward_of(torch_fwd)}
    with torch.no_grad():                                                     # the two compute the same thing: said once, before anything is timed
        agree = float((new_fwd() - torch_fwd()).abs().max())
        index = volsample.sample_volume_cuboid(vol, pts, rot, cen, pos, sides, paired=paired, return_index=True)[1]
        inside = float(((index >= 0) & (index <= S - 1)).all(-1).float().mean())
        sampled = float(((index > -1) & (index < S)).all(-1).float().mean())
    peak = {}
    for k, fn in runs.items():
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated(dev) - base
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
    res = {"shape": "B%d C%d %d^3 float32 N%d%s" % (B, C, S, N, " paired" if paired else ""), "volume_bytes": vol.numel() * vol.element_size(),
           "chunk_points": aggregation._capi.lib().mvhmr_sample_volume_chunk_points(), "max_abs_vs_torch": agree,
           "points_inside_the_cuboid": round(inside, 4), "points_sampled": round(sampled, 4)}
    for k, v in times.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
        res[k + "_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
        res[k + "_peak_bytes"] = int(peak[k])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--soak-ms", type=float, default=1000.0)
    ap.add_argument("--shapes", default="a_full,b_paired")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sample_volume.py needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"reps": a.reps, "warmup": a.warmup, "soak_ms": a.soak_ms}
    for name in a.shapes.split(","):
        res[name] = time_shape(name, a, dev)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
