#!/usr/bin/env python3
"""Generate tests/golden/viewweights_*.npz by RUNNING the reference on duplicated views.

An integer weight k on view v is the reference's unprojection on a sample that holds view v k times: sum adds it k times, mean counts it
k times, softmax gives it k equal terms.  That anchors unprojection(view_weights=...) to the reference, which has no
weights of its own in the aggregate.  Per case and per aggregation method (sum, mean, softmax) the reference runs sample by sample on
the duplicated views; the feature gradients of a view's copies are added up.  A sample whose weights are all zero has no views at all:
the reference's zero-initialised volume and zero gradients.

Only ever run where the reference is mounted (it never travels); it is imported unmodified, as tests/golden/make_golden.py does, whose
synthetic geometry this script reuses.  Each file holds inputs AND expected outputs, float32:
    features, proj, coords, weights (integers 0 ... 3 as float32), grad_out -> out_<method>, gfeat_<method>

Usage:  python tests/golden/make_golden_viewweights.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg  # noqa: E402  (imports the reference; writes nothing on import)

METHODS = ("sum", "mean", "softmax")


def run_case(name, features, proj, coords, weights, seed):
    B, V, C = features.shape[:3]
    vol = coords.shape[1:4]
    grad_out = torch.randn(B, C, *vol, generator=torch.Generator().manual_seed(seed + 1000))
    rec = dict(features=features, proj=proj, coords=coords, weights=weights.astype(np.float32), grad_out=grad_out.numpy())
    for method in METHODS:
        out = np.zeros((B, C) + tuple(vol), np.float32)
        gfeat = np.zeros_like(features)
        for b in range(B):
            dup = [v for v in range(V) for _ in range(int(weights[b, v]))]
            if not dup:
                continue
            f = torch.from_numpy(features[b:b + 1, dup]).requires_grad_(True)
            o = mg.ref_agg.unprojection(f, torch.from_numpy(proj[b:b + 1, dup]), torch.from_numpy(coords[b:b + 1]), aggregation_method=method)
            (o * grad_out[b:b + 1]).sum().backward()
            out[b] = o.detach().numpy()[0]
            for k, v in enumerate(dup):
                gfeat[b, v] += f.grad.numpy()[0, k]
        rec["out_" + method], rec["gfeat_" + method] = out, gfeat
    path = os.path.join(HERE, "viewweights_%s.npz" % name)
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


def problem(B, V, C, H, W, vol, seed):
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((B, V, C, H, W)).astype(np.float32)
    proj = np.stack([mg.feature_level_projections(mg.ring_cameras(V, 5000.0, 1500.0, 1145.0, 1000.0, rng, jitter=0.05), (150, 150, 850, 850),
                                                  (4 * H, 4 * W), (H, W)) for _ in range(B)])
    coords = np.stack([mg.cuboid_coords(vol, 2500.0, theta=0.2 * b) for b in range(B)])
    return feats, proj, coords


def main():
    # V = 4 (the vector-view instances): every weight 0 ... 3, an all-zero sample, a single-view sample; sum_v k_v <= 8
    f, p, c = problem(4, 4, 5, 20, 20, (6, 5, 7), seed=41)
    w = np.array([[1, 2, 0, 3], [0, 0, 0, 0], [0, 0, 2, 0], [3, 1, 2, 2]])
    run_case("v4c5", f, p, c, w, seed=41)
    # run-time view count (3 views), non-square maps
    f, p, c = problem(3, 3, 6, 16, 24, (5, 6, 4), seed=42)
    w = np.array([[2, 3, 1], [0, 1, 0], [0, 0, 0]])
    run_case("v3c6_nonsquare", f, p, c, w, seed=42)
    # 12 views, non-square maps
    f, p, c = problem(3, 12, 4, 12, 16, (4, 4, 5), seed=43)
    w = np.array([[1, 0, 0, 2, 0, 1, 0, 0, 3, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0], [0] * 12])
    run_case("v12c4_nonsquare", f, p, c, w, seed=43)


if __name__ == "__main__":
    main()
