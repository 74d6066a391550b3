#!/usr/bin/env python3
"""Generate tests/golden/geomgrad_<case>.npz by RUNNING the reference's unprojection with proj_matricies and coord_volumes requiring
grad: the geometric gradients autograd gives through its graph (matmul, perspective divide, normalisation, F.grid_sample, masking,
the cross-view aggregate).

Run it only where the reference code base is importable, like make_golden.py (whose synthetic cameras and cuboids it reuses;
importing it imports the reference).  CPU only.  Each file holds the inputs and, per aggregation mode, gproj_<mode> (B,V,3,4), gcoords_<mode> (B,X,Y,Z,3) and
gfeat_<mode>.

Usage:  python tests/golden/make_golden_geomgrad.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (imports the reference)


def run_case(name, features, proj, coords, seed):
    g = torch.Generator().manual_seed(seed + 2000)
    B, V, C = features.shape[:3]
    grad_out = torch.randn(B, C, *coords.shape[1:4], generator=g)
    rec = dict(features=features, proj=proj, coords=coords, grad_out=grad_out.numpy())
    for mode in mg.MODES:
        f = torch.from_numpy(features).clone().requires_grad_(True)
        P = torch.from_numpy(proj).clone().requires_grad_(True)
        Cv = torch.from_numpy(coords).clone().requires_grad_(True)
        out = mg.ref_agg.unprojection(f, P, Cv, aggregation_method=mode)
        (out * grad_out).sum().backward()
        rec["gproj_" + mode] = P.grad.numpy()
        rec["gcoords_" + mode] = Cv.grad.numpy()
        rec["gfeat_" + mode] = f.grad.numpy()
    path = os.path.join(HERE, "geomgrad_%s.npz" % name)
    np.savez_compressed(path, **rec)
    print("wrote", path)


def main():
    rng = np.random.default_rng(11)

    def feats(B, V, C, H, W, seed, scale=1.0):
        gen = torch.Generator().manual_seed(seed)
        return (torch.randn(B, V, C, H, W, generator=gen) * scale).numpy()

    # non-square maps (Q1: dix/du = (Wf - 1) / Hf, diy/dw = (Hf - 1) / Wf), 3 views, odd volume extents, voxels outside the frame
    cams = mg.ring_cameras(3, 4800.0, 1400.0, 1145.0, 1000.0, rng, jitter=0.05)
    P = mg.feature_level_projections(cams, (100, 180, 900, 820), (96, 120), (14, 22))
    coords = np.stack([mg.cuboid_coords((5, 3, 7), 3600.0, center=(30.0, -50.0, 80.0), theta=1.1),
                       mg.cuboid_coords((5, 3, 7), 2400.0, theta=0.3)])
    run_case("nonsquare_v3c5", feats(2, 3, 5, 14, 22, 21), np.stack([P, P[::-1].copy()]), coords, 21)

    # camera inside the cuboid: voxels behind it (z <= 0 -> no gradient) and a frustum that misses part of the grid, 4 views
    cams = mg.ring_cameras(4, 900.0, 200.0, 700.0, 1000.0, rng)
    P = mg.feature_level_projections(cams, (200, 200, 800, 800), (64, 80), (12, 18))
    run_case("adversarial_v4c6", feats(1, 4, 6, 12, 18, 22, scale=2.0), P[None], mg.cuboid_coords((6, 5, 4), 2500.0)[None], 22)


if __name__ == "__main__":
    main()
