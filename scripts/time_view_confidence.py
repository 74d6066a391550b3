#!/usr/bin/env python3
"""Times per-pixel view confidence maps against the per-view weights call they generalise: forward, feature backward and
geometry backward (which also writes the gradient w.r.t. the weights / the maps) of
    weighted         mvhmr_unproject_*_weighted with all-ones view_weights, from --parent-lib (a build of the parent commit's library;
                     without it this build's own weighted call, whose kernels are the parent's instruction for instruction)
    confidence ones  mvhmr_unproject_*_confidence of this build with all-ones maps, no mask
    confidence half  the same with every map zero on its left half: the views are absent for the voxels that project there
on the same inputs, at BASELINE configs[1] and at the north-star shape.  All calls go through the C ABI with ctypes, are alternated in one
process after a warm-up, and are timed with device events; prints one JSON line with medians and spreads (ms).

    python scripts/time_view_confidence.py [--reps 7 --warmup 2 --method softmax --parent-lib PATH --out profiles/r11_view_confidence.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import ring_projections  # noqa: E402
from multiviewhmr_amd import _capi, aggregation  # noqa: E402

SHAPES = {"configs1": dict(B=8, S=32, C=256, V=4, HW=96), "north_star": dict(B=32, S=64, C=256, V=4, HW=96)}
VP, SZ = ctypes.c_void_p, ctypes.c_size_t
LEGS = ("forward", "backward", "backward_geometry")


def _bind(L):
    dp = ctypes.POINTER(_capi.Desc)
    sigs = {"forward_weighted": [dp, VP, VP, VP, VP, VP, VP, VP, SZ, VP], "backward_weighted": [dp, VP, VP, VP, VP, VP, VP, VP, VP, SZ, VP],
            "backward_geometry_weighted": [dp, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP, SZ, VP],
            "forward_confidence": [dp, VP, VP, VP, VP, VP, ctypes.c_int, VP, VP, SZ, VP],
            "backward_confidence": [dp, VP, VP, VP, VP, VP, VP, ctypes.c_int, VP, VP, SZ, VP],
            "backward_geometry_confidence": [dp, VP, VP, VP, VP, VP, VP, ctypes.c_int, VP, VP, VP, VP, SZ, VP]}
    for name, args in sigs.items():
        if hasattr(L, "mvhmr_unproject_" + name):
            getattr(L, "mvhmr_unproject_" + name).argtypes, getattr(L, "mvhmr_unproject_" + name).restype = args, ctypes.c_int
            q = getattr(L, "mvhmr_unproject_%s_workspace_bytes" % name)
            q.argtypes, q.restype = [dp], SZ
    L.mvhmr_last_error.restype = ctypes.c_char_p
    return L


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def time_shape(name, a, dev, parent, this):
    s = SHAPES[name]
    B, S, C, V, HW = s["B"], s["S"], s["C"], s["V"], s["HW"]
    torch.manual_seed(0)
    f = torch.randn(B, V, C, HW, HW, device=dev)
    p = torch.from_numpy(ring_projections(B, V, (HW, HW), seed=0)).to(dev)
    ax = torch.linspace(-1000.0, 1000.0, S, device=dev)
    c = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)[None].expand(B, S, S, S, 3).contiguous()
    g = torch.randn(B, C, S, S, S, device=dev)
    out, grad = torch.empty(B, C, S, S, S, device=dev), torch.empty_like(f)
    gp, gc = torch.empty(B, V, 3, 4, device=dev), torch.empty(B, S, S, S, 3, device=dev)
    w, gw = torch.ones(B, V, device=dev), torch.empty(B, V, device=dev)
    ones, gk = torch.ones(B, V, HW, HW, device=dev), torch.empty(B, V, HW, HW, device=dev)
    half = ones.clone()
    half[..., :HW // 2] = 0
    d = aggregation._make_desc(f, (S, S, S), _capi.AGG[a.method], torch.float32, _capi.LAYOUT_BVCHW, _capi.VARIANT["gather"])
    ref = ctypes.byref(d)
    stream = VP(torch.cuda.current_stream(dev).cuda_stream)
    need = max(getattr(L_, "mvhmr_unproject_%s_%s_workspace_bytes" % (leg, tag))(ref) for L_, tag in ((parent, "weighted"), (this, "confidence")) for leg in LEGS)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ptr = lambda t: VP(t.data_ptr())  # noqa: E731

    def check(L, rc):
        if rc != _capi.OK:
            raise RuntimeError(L.mvhmr_last_error().decode())

    runs = {
        "weighted fwd": lambda: check(parent, parent.mvhmr_unproject_forward_weighted(ref, ptr(f), ptr(p), ptr(c), None, ptr(w), ptr(out), ptr(ws), need, stream)),
        "weighted bwd_features": lambda: check(parent, parent.mvhmr_unproject_backward_weighted(ref, ptr(g), ptr(f), ptr(p), ptr(c), None, ptr(w), ptr(grad), ptr(ws),
                                                                                                need, stream)),
        "weighted bwd_geometry": lambda: check(parent, parent.mvhmr_unproject_backward_geometry_weighted(ref, ptr(g), ptr(f), ptr(p), ptr(c), None, ptr(w), ptr(gp),
                                                                                                         ptr(gc), ptr(gw), ptr(ws), need, stream)),
    }
    for tag, k in (("confidence ones", ones), ("confidence half", half)):
        runs[tag + " fwd"] = lambda k=k: check(this, this.mvhmr_unproject_forward_confidence(ref, ptr(f), ptr(p), ptr(c), None, ptr(k), 0, ptr(out), ptr(ws), need,
                                                                                             stream))
        runs[tag + " bwd_features"] = lambda k=k: check(this, this.mvhmr_unproject_backward_confidence(ref, ptr(g), ptr(f), ptr(p), ptr(c), None, ptr(k), 0, ptr(grad),
                                                                                                       ptr(ws), need, stream))
        runs[tag + " bwd_geometry"] = lambda k=k: check(this, this.mvhmr_unproject_backward_geometry_confidence(ref, ptr(g), ptr(f), ptr(p), ptr(c), None, ptr(k), 0,
                                                                                                                ptr(gp), ptr(gc), ptr(gk), ptr(ws), need, stream))
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
    ap.add_argument("--shapes", default="configs1,north_star")
    ap.add_argument("--parent-lib", default=None, help="libmvhmr_unproject.so built from the parent commit (default: this build's weighted call)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_view_confidence.py needs a HIP device")
    dev = torch.device("cuda:0")
    this = _bind(ctypes.CDLL(_capi.LIB_PATH))
    parent = _bind(ctypes.CDLL(os.path.abspath(a.parent_lib))) if a.parent_lib else this
    res = {"weighted_from": "parent library" if a.parent_lib else "this build", "reps": a.reps, "warmup": a.warmup}
    res.update({name: time_shape(name, a, dev, parent, this) for name in a.shapes.split(",")})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
