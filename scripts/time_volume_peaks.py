#!/usr/bin/env python3
"""Times volume_peaks against the torch recipe it replaces, on the same inputs:

    pooled = F.max_pool3d(v, 2r+1, 1, r); keep = (pooled == v) & (v > thr)
    scores, idx = torch.where(keep, v, -inf).flatten(2).topk(K)

Each forward alone and forward + backward of scores.sum().  One process, a soak, the candidates alternated; a sample is 20 back-to-back
calls between one pair of device events, divided by 20, so that the host's dispatch of one call hides under the card's work on the one
before (an eager figure still holds host time wherever the host is the slower of the two).  The new op's forward is also replayed from a
captured graph, which leaves the two kernels alone, and that time is set against one read of the volume at the 6.3 TB/s copy rate of
DESIGN.md 5.17.  Prints one JSON line with medians, spreads (ms) and the peak memory each candidate adds to
its inputs.  The volumes are standard normal: tie-free, one voxel in 27 a peak for radius 1 -- far denser than a trained heat volume.

    python scripts/time_volume_peaks.py [--reps 7 --warmup 2 --out profiles/r17_volume_peaks.json]
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

from multiviewhmr_amd import _capi, peaks  # noqa: E402

COPY_RATE = 6.3e12                                                              # bytes/s, the copy rate DESIGN.md 5.17 measures against
SHAPES = {
    "root_80x80x20": dict(B=32, J=1, vol=(80, 80, 20), dtype=torch.float32, K=10, r=1),
    "j17_64_f32": dict(B=32, J=17, vol=(64, 64, 64), dtype=torch.float32, K=4, r=1),
    "j17_64_bf16": dict(B=32, J=17, vol=(64, 64, 64), dtype=torch.bfloat16, K=4, r=1),
    "j17_64_f32_r3": dict(B=32, J=17, vol=(64, 64, 64), dtype=torch.float32, K=4, r=3),
}


def _timed(fn, calls):
    """ms per call over `calls` back-to-back calls between one pair of events: the host runs ahead of the card after the first call, so the
    figure is the card's time per call unless the host is the slower of the two"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def time_shape(name, a, dev):
    s = SHAPES[name]
    B, J, vol_shape, dtype, K, r = s["B"], s["J"], s["vol"], s["dtype"], s["K"], s["r"]
    torch.manual_seed(0)
    vol = torch.randn(B, J, *vol_shape, device=dev).to(dtype).requires_grad_(True)
    thr = 0.5
    ninf = torch.tensor(float("-inf"), device=dev, dtype=dtype)

    def torch_fwd():
        pooled = F.max_pool3d(vol, 2 * r + 1, 1, r)
        keep = (pooled == vol) & (vol > thr)
        return torch.where(keep, vol, ninf).flatten(2).topk(K)

    new_fwd = lambda: peaks.volume_peaks(vol, K, radius=r, threshold=thr)      # noqa: E731

    def backward_of(fwd):
        return lambda: torch.autograd.grad(fwd()[0].float().sum(), vol)

    with torch.no_grad():                                                     # the two compute the same thing on tie-free input: said once
        ns, ni = new_fwd()
        ts, ti = torch_fwd()
        agree = bool(torch.equal(ns, ts.float()) and torch.equal(ni.long(), ti))          # (16-bit normals tie: there the recipe's order is its own)
        same_scores = bool(torch.equal(ns, ts.float()))
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            new_fwd()
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph):
            new_fwd()
    runs = {"new fwd": torch.no_grad()(new_fwd), "new fwd+bwd": backward_of(new_fwd), "new fwd graph": graph.replay,
            "torch fwd": torch.no_grad()(torch_fwd), "torch fwd+bwd": backward_of(torch_fwd)}
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
            t = _timed(fn, a.calls)
            if i >= a.warmup:
                times[k].append(t)
    L = _capi.lib()
    volume_bytes = vol.numel() * vol.element_size()
    res = {"shape": "B%d J%d %s %s K%d r%d" % (B, J, "x".join(map(str, vol_shape)), str(dtype)[6:], K, r), "volume_bytes": volume_bytes,
           "workspace_bytes": int(L.mvhmr_volume_peaks_workspace_bytes(B, J, *vol_shape, K)), "equal_to_torch_recipe": agree, "scores_equal_to_torch_recipe": same_scores,
           "one_read_at_copy_rate_ms": round(volume_bytes / COPY_RATE * 1e3, 4)}
    for k, v in times.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
        res[k + "_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
        res[k + "_peak_bytes"] = int(peak[k])
    res["kernels_share_of_copy_rate"] = round(res["one_read_at_copy_rate_ms"] / res["new fwd graph_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20, help="calls between one pair of events")
    ap.add_argument("--soak-ms", type=float, default=1000.0)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_volume_peaks.py needs a HIP device")
    dev = torch.device("cuda:0")
    tile = (3 * __import__("ctypes").c_int32)()
    _capi.lib().mvhmr_volume_peaks_tile(tile)
    res = {"reps": a.reps, "warmup": a.warmup, "calls_per_sample": a.calls, "soak_ms": a.soak_ms, "tile": list(tile)}
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
