#!/usr/bin/env python3
"""Generate tests/golden/visibility_*.npz by RUNNING the reference on the seeing views of every voxel.

On the voxels whose set of seeing views is S, unprojection(visible_only=True) must equal the reference run on the views
S alone: there every view of the call sees the voxel, so none of them contributes the zero of quirk Q2.  That anchors the feature to the
reference, which has no visibility of its own.  Per case, per aggregation method, per sample and per distinct pattern S the reference
runs on views S; its output is taken on the voxels with that pattern, grad_out restricted to those voxels is back-propagated, and the
feature gradients of all patterns are added up.  A voxel no view sees keeps the zero-initialised volume and zero gradients.

The pattern of a voxel comes from the fp32 positions of the forward (tests/geomgrad_oracle.sample_cells) and the rule
    z > 0  and  0 <= ix <= Wf - 1  and  0 <= iy <= Hf - 1
Every case is checked to keep each voxel-view at least 1e-3 px away from a map edge (so no position is a matter of rounding and nothing
has to be left out of a comparison), the first two to populate every count 0 ... V, the third to hold voxel-views behind a camera.

Only ever run where the reference is mounted (it never travels); it is imported unmodified, as tests/golden/make_golden.py does, whose
synthetic geometry this script reuses.  Each file holds inputs AND expected outputs:
    features, proj, coords, grad_out (float32), bits (int32, bit v = view v sees the voxel) -> out_<method>, gfeat_<method> (float32)

Usage:  python tests/golden/make_golden_visibility.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                                   # tests/: geomgrad_oracle
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))                  # the repository root: the oracle package geomgrad_oracle imports

import numpy as np
import torch

import make_golden as mg  # noqa: E402  (imports the reference; writes nothing on import)
from geomgrad_oracle import sample_cells  # noqa: E402

METHODS = ("sum", "mean", "max", "softmax")


def problem(B, V, C, H, W, vol, seed, side):
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((B, V, C, H, W)).astype(np.float32)
    proj = np.stack([mg.feature_level_projections(mg.ring_cameras(V, 5000.0, 1500.0, 1145.0, 1000.0, rng, jitter=0.05), (150, 150, 850, 850),
                                                  (4 * H, 4 * W), (H, W)) for _ in range(B)])
    coords = np.stack([mg.cuboid_coords(vol, side, theta=0.2 * b) for b in range(B)])
    return feats, proj, coords


def seen_views(proj, coords, H, W):
    """-> (seen (B, V, N) bool by the rule, near (B, V, N) bool: within 1e-3 px of a map edge in front of the camera, behind (B, V, N) bool)"""
    B, V = proj.shape[:2]
    N = int(np.prod(coords.shape[1:4]))
    seen, near, behind = (np.zeros((B, V, N), bool) for _ in range(3))
    for b in range(B):
        pts = torch.from_numpy(coords[b].reshape(-1, 3))
        for v in range(V):
            _, _, z, ix, iy = sample_cells(torch.from_numpy(proj[b, v]), pts, H, W)
            seen[b, v] = ((z > 0) & (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)).numpy()
            d = torch.stack([ix.abs(), (ix - (W - 1)).abs(), iy.abs(), (iy - (H - 1)).abs()]).min(0).values
            near[b, v] = ((d < 1e-3) & (z > 0)).numpy()
            behind[b, v] = (~(z > 0)).numpy()
    return seen, near, behind


def run_case(name, features, proj, coords, seed, every_count, want_behind):
    B, V, C, H, W = features.shape
    vol = tuple(coords.shape[1:4])
    N = int(np.prod(vol))
    seen, near, behind = seen_views(proj, coords, H, W)
    assert not near.any(), "%s: %d voxel-views within 1e-3 px of a map edge" % (name, near.sum())
    counts = np.bincount(seen.sum(1).ravel(), minlength=V + 1)
    assert not every_count or (counts > 0).all(), "%s: counts %s" % (name, counts.tolist())
    assert not want_behind or behind.any(), "%s: no voxel-view behind a camera" % name
    codes = (seen.astype(np.int64) << np.arange(V, dtype=np.int64)[None, :, None]).sum(1)            # (B, N)
    grad_out = torch.randn(B, C, *vol, generator=torch.Generator().manual_seed(seed + 1000))
    rec = dict(features=features, proj=proj, coords=coords, grad_out=grad_out.numpy(), bits=codes.astype(np.int32).reshape((B,) + vol))
    patterns = 0
    for method in METHODS:
        out = np.zeros((B, C, N), np.float32)
        gfeat = np.zeros_like(features)
        for b in range(B):
            for code in np.unique(codes[b]):
                if code == 0:
                    continue
                patterns += 1
                views = [v for v in range(V) if code >> v & 1]
                sel = torch.from_numpy(codes[b] == code)
                f = torch.from_numpy(features[b:b + 1, views]).requires_grad_(True)
                o = mg.ref_agg.unprojection(f, torch.from_numpy(proj[b:b + 1, views]), torch.from_numpy(coords[b:b + 1]), aggregation_method=method)
                o = o.reshape(C, N)
                (o[:, sel] * grad_out[b].reshape(C, N)[:, sel]).sum().backward()
                out[b][:, sel.numpy()] = o.detach().numpy()[:, sel.numpy()]
                gfeat[b, views] += f.grad.numpy()[0]
        rec["out_" + method], rec["gfeat_" + method] = out.reshape((B, C) + vol), gfeat
    path = os.path.join(HERE, "visibility_%s.npz" % name)
    np.savez_compressed(path, **rec)
    print("wrote %s, %d bytes: seen %.3f, behind %.3f, counts %s, %d pattern runs" % (path, os.path.getsize(path), seen.mean(), behind.mean(),
                                                                                      counts.tolist(), patterns))
    assert os.path.getsize(path) < 500 * 1000


def main():
    # V = 4 (the vector-view instances) and V = 3 (run-time view count, non-square maps): a 4 m cuboid, every count 0 ... V
    f, p, c = problem(3, 4, 5, 20, 20, (6, 5, 7), 51, 4000.0)
    run_case("v4c5", f, p, c, 51, every_count=True, want_behind=False)
    f, p, c = problem(2, 3, 6, 16, 24, (5, 6, 4), 52, 4000.0)
    run_case("v3c6_nonsquare", f, p, c, 52, every_count=True, want_behind=False)
    # V = 8, a 10 m cuboid that reaches behind the cameras
    f, p, c = problem(2, 8, 4, 12, 16, (4, 4, 5), 53, 10000.0)
    run_case("v8c4_behind", f, p, c, 53, every_count=False, want_behind=True)


if __name__ == "__main__":
    main()
