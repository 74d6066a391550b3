#!/usr/bin/env python3
"""Generate tests/golden/shared_*.npz by RUNNING the reference on features[idx] and proj[idx].

unprojection(features, proj, coords, method, feature_index=idx) is, by definition, the reference's
unprojection(features[idx], proj[idx], coords): M volumes from B feature samples.  Here torch indexing materialises the duplicated inputs,
the reference runs on them, and its own autograd sends grad_out back through the indexing: grad_features[b] and grad_proj[b] come out as the
sums over the volumes that name b (zeros for a sample no volume names), grad_coords per volume.  Every voxel is compared: nothing is left out.

Three cases:
    b3m5v4c5            index [1, 0, 1, 1, 0]: sample 2 is unused
    b2m4v3c6_nonsquare  index [1, 1, 0, 1]: unsorted, a non-square map
    b1m3v8c4_behind     one sample named three times, a cuboid that reaches behind the cameras

Only ever run where the reference is mounted (it never travels); it is imported unmodified, as tests/golden/make_golden.py does.  Each file
holds inputs AND expected outputs:
    features (B,V,C,H,W), proj (B,V,3,4), coords (M,X,Y,Z,3), index (M,) int32, grad_out (M,C,X,Y,Z)
        -> out_<method> (M,C,X,Y,Z), gfeat_<method> (B,V,C,H,W), gproj_<method> (B,V,3,4), gcoords_<method> (M,X,Y,Z,3)   (float32)

Usage:  python tests/golden/make_golden_shared.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg  # noqa: E402  (imports the reference; writes nothing on import)

METHODS = ("softmax", "sum", "mean", "max")


def problem(B, V, C, H, W, vol, index, seed, side):
    """B feature samples under their own camera rings, one cuboid per VOLUME (its own rotation and pivot)"""
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((B, V, C, H, W)).astype(np.float32)
    proj = np.stack([mg.feature_level_projections(mg.ring_cameras(V, 5000.0, 1500.0, 1145.0, 1000.0, rng, jitter=0.05), (150, 150, 850, 850),
                                                  (4 * H, 4 * W), (H, W)) for _ in range(B)])
    coords = np.stack([mg.cuboid_coords(vol, side, center=(60.0 * m, -40.0 * m, 25.0 * m), theta=0.2 * m + 0.1) for m in range(len(index))])
    return feats, proj.astype(np.float32), coords.astype(np.float32)


def run_case(name, features, proj, coords, index, seed, want_behind=False):
    B, V, C, H, W = features.shape
    M = len(index)
    vol = tuple(coords.shape[1:4])
    idx = torch.tensor(index, dtype=torch.long)
    assert coords.shape[0] == M and 0 <= min(index) and max(index) < B
    if want_behind:
        z = np.einsum("mvj,mnj->mvn", proj[index][:, :, 2, :3].astype(np.float64), coords.reshape(M, -1, 3).astype(np.float64)) + proj[index][:, :, 2, 3:4]
        assert (z <= 0).mean() > 0.02, (z <= 0).mean()
    grad_out = torch.randn(M, C, *vol, generator=torch.Generator().manual_seed(seed + 1000))
    rec = dict(features=features, proj=proj, coords=coords, index=np.asarray(index, np.int32), grad_out=grad_out.numpy())
    for method in METHODS:
        f = torch.from_numpy(features).requires_grad_(True)
        P = torch.from_numpy(proj).requires_grad_(True)
        X = torch.from_numpy(coords).requires_grad_(True)
        out = mg.ref_agg.unprojection(f[idx], P[idx], X, aggregation_method=method)
        assert tuple(out.shape) == (M, C) + vol
        out.backward(grad_out)
        rec["out_" + method] = out.detach().numpy()
        rec["gfeat_" + method] = f.grad.numpy()
        rec["gproj_" + method] = P.grad.numpy()
        rec["gcoords_" + method] = X.grad.numpy()
        for b in set(range(B)) - set(index):
            assert not f.grad[b].any() and not P.grad[b].any()
    path = os.path.join(HERE, "shared_%s.npz" % name)
    np.savez_compressed(path, **rec)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 500 * 1000


def main():
    index = [1, 0, 1, 1, 0]
    run_case("b3m5v4c5", *problem(3, 4, 5, 16, 16, (6, 5, 7), index, 61, 4000.0), index, 61)
    index = [1, 1, 0, 1]
    run_case("b2m4v3c6_nonsquare", *problem(2, 3, 6, 16, 24, (5, 6, 4), index, 62, 4000.0), index, 62)
    index = [0, 0, 0]
    run_case("b1m3v8c4_behind", *problem(1, 8, 4, 12, 16, (4, 4, 5), index, 63, 10000.0), index, 63, want_behind=True)


if __name__ == "__main__":
    main()
