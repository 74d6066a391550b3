#!/usr/bin/env python3
"""Times the volumetric soft-argmax against the torch composition it replaces, on the same inputs: softmax over the
flattened volume, then the product with the coordinates VolumeGenerator.coord_volumes materialises.  Candidates: the cuboid route, the
tensor route (both through the public functions and autograd) and the composition, each forward alone and forward + backward w.r.t. the
volume; the new ops' forward and backward also as direct op calls, for their effective bytes per second (one read of the volume forward;
one read and one write backward) beside the achievable copy rate.  One process, a soak, the candidates alternated, device events; prints
one JSON line with medians, spreads (ms) and the peak memory each candidate adds to its inputs.

    python scripts/time_soft_argmax.py [--reps 7 --warmup 2 --out profiles/r15_soft_argmax.json]
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

from multiviewhmr_amd import aggregation, softargmax  # noqa: E402

COPY_RATE = 6.3e12                                       # bytes / s: the achievable HBM copy rate of the MI355X
SHAPES = {"b32_f32": dict(B=32, J=17, S=64, dtype=torch.float32), "b32_bf16": dict(B=32, J=17, S=64, dtype=torch.bfloat16),
          "b1_f32": dict(B=1, J=17, S=64, dtype=torch.float32)}
BETA = 2.0


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def time_shape(name, a, dev):
    s = SHAPES[name]
    B, J, S, dtype = s["B"], s["J"], s["S"], s["dtype"]
    torch.manual_seed(0)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=2500.0, device=dev)
    cub = gen.cuboid()
    pos, sides = [float(x) for x in cub.position], [float(x) for x in cub.sides]
    rot = torch.linalg.qr(torch.randn(B, 3, 3, device=dev))[0].contiguous()
    cen = (100.0 * torch.randn(B, 3, device=dev)).contiguous()
    coords = gen.coord_volumes(rot, cen, dev)
    vol = torch.randn(B, J, S, S, S, device=dev).to(dtype).requires_grad_(True)
    g = torch.randn(B, J, 3, device=dev)
    flat = coords.view(B, -1, 3)
    ops = torch.ops.mvhmr

    def torch_fwd():
        return torch.bmm(torch.softmax(BETA * vol.flatten(2).float(), dim=-1), flat)

    def backward_of(fwd):
        return lambda: torch.autograd.grad((fwd() * g).sum(), vol)

    cub_fwd = lambda: softargmax.soft_argmax_3d_cuboid(vol, rot, cen, pos, sides, beta=BETA)           # noqa: E731
    ten_fwd = lambda: softargmax.soft_argmax_3d(vol, coords, beta=BETA)                                # noqa: E731
    with torch.no_grad():
        _, lse_c, mom_c = ops.soft_argmax3d_cuboid(vol, rot, cen, pos, sides, BETA)
        _, lse_t, mom_t = ops.soft_argmax3d(vol, coords, BETA)
    runs = {"cuboid fwd": cub_fwd, "cuboid fwd+bwd": backward_of(cub_fwd), "tensor fwd": ten_fwd, "tensor fwd+bwd": backward_of(ten_fwd),
            "torch fwd": torch_fwd, "torch fwd+bwd": backward_of(torch_fwd),
            "cuboid bwd op": lambda: ops.soft_argmax3d_cuboid_backward(vol, rot, cen, pos, sides, BETA, lse_c, mom_c, g, None),
            "tensor bwd op": lambda: ops.soft_argmax3d_backward(vol, coords, BETA, lse_t, mom_t, g, None)}
    # the three routes compute the same thing: said once per shape, before anything is timed
    with torch.no_grad():
        ref = torch_fwd()
        agree = {k: float((runs[k + " fwd"]() - ref).abs().max()) for k in ("cuboid", "tensor")}
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
    volume_bytes = vol.numel() * vol.element_size()
    res = {"shape": "B%d J%d %d^3 %s beta=%g" % (B, J, S, str(dtype)[6:], BETA), "volume_bytes": volume_bytes,
           "splits": aggregation._capi.lib().mvhmr_soft_argmax3d_splits(B, J, S ** 3), "max_abs_vs_torch": agree}
    for k, v in times.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
        res[k + "_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
        res[k + "_peak_bytes"] = int(peak[k])
    for route in ("cuboid", "tensor"):
        extra = coords.numel() * 4 if route == "tensor" else 0                # the tensor route also reads the coordinates, once per joint tile at most
        res[route + " fwd_bytes_per_s"] = round(volume_bytes / (res[route + " fwd_ms"] * 1e-3), 0)
        res[route + " bwd_bytes_per_s"] = round(2 * volume_bytes / (res[route + " bwd op_ms"] * 1e-3), 0)
        res[route + " fwd_share_of_copy_rate"] = round(res[route + " fwd_bytes_per_s"] / COPY_RATE, 4)
        res[route + " bwd_share_of_copy_rate"] = round(res[route + " bwd_bytes_per_s"] / COPY_RATE, 4)
        res[route + " coords_bytes_not_counted"] = extra
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--soak-ms", type=float, default=1000.0)
    ap.add_argument("--shapes", default="b32_f32,b32_bf16,b1_f32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_soft_argmax.py needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"reps": a.reps, "warmup": a.warmup, "soak_ms": a.soak_ms, "copy_rate_bytes_per_s": COPY_RATE}
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
