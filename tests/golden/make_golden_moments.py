#!/usr/bin/env python3
"""Generate tests/golden/moments_*.npz by RUNNING the reference once per view.

The reference has no cross-view variance, but it has every ingredient: the per-view sample volume of view v is the reference's own
    unprojection(features[:, v:v+1], proj_matricies[:, v:v+1], coord_volumes, aggregation_method='sum')
(one view: the sum IS the sample, quirks included -- a view behind the camera or outside the map gives its zero).  The V volumes are
combined in float64, per voxel and channel, over the participating views S:

    mu = sum_S s_v / |S|          var = sum_S (s_v - mu)^2 / |S|          (|S| = 0: both 0)

once with S = every view (the plain call) and once with S = the views that see the voxel (visible_only=True), read from the `bits` of the
matching visibility golden -- the same stitching by pattern as tests/golden/make_golden_visibility.py, whose three geometries (and inputs)
this script reuses, so the files are no larger than those.  Gradients are not recorded: the oracle takes them from autograd on the same
float64 restatement, and the reference's own backward of a single-view `sum` adds nothing to that.

Only ever run where the reference is mounted (it never travels); it is imported unmodified, as tests/golden/make_golden.py does.  Each
file holds inputs AND expected outputs:
    features, proj, coords (float32), bits (int32) -> samples (V volumes, float32), mean_plain, var_plain, mean_visible, var_visible (float64)

Usage:  python tests/golden/make_golden_moments.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg  # noqa: E402  (imports the reference; writes nothing on import)

CASES = ("v4c5", "v3c6_nonsquare", "v8c4_behind")


def combine(S, part):
    """S (V, B, C, N) float64, part (V, B, N) bool -> (mu, var), each (B, C, N)"""
    m = part[:, :, None, :]
    n = np.maximum(part.sum(0), 1)[:, None, :].astype(np.float64)
    mu = np.where(m, S, 0.0).sum(0) / n
    var = np.where(m, (S - mu[None]) ** 2, 0.0).sum(0) / n
    return mu, var


def run_case(name):
    d = np.load(os.path.join(HERE, "visibility_%s.npz" % name))
    features, proj, coords, bits = d["features"], d["proj"], d["coords"], d["bits"]
    B, V, C, H, W = features.shape
    vol = tuple(coords.shape[1:4])
    N = int(np.prod(vol))
    samples = []
    for v in range(V):
        with torch.no_grad():
            o = mg.ref_agg.unprojection(torch.from_numpy(features[:, v:v + 1]), torch.from_numpy(proj[:, v:v + 1]), torch.from_numpy(coords),
                                        aggregation_method="sum")
        samples.append(o.numpy().reshape(B, C, N))
    S32 = np.stack(samples)                                                     # (V, B, C, N) float32, the reference's own
    S = S32.astype(np.float64)
    seen = np.stack([(bits.reshape(B, N) >> v & 1).astype(bool) for v in range(V)])
    rec = dict(features=features, proj=proj, coords=coords, bits=bits, samples=S32.reshape((V, B, C) + vol))
    for tag, part in (("plain", np.ones((V, B, N), bool)), ("visible", seen)):
        mu, var = combine(S, part)
        rec["mean_" + tag], rec["var_" + tag] = mu.reshape((B, C) + vol), var.reshape((B, C) + vol)
    path = os.path.join(HERE, "moments_%s.npz" % name)
    np.savez_compressed(path, **rec)
    counts = np.bincount(seen.sum(0).ravel(), minlength=V + 1)
    print("wrote %s, %d bytes (the visibility golden: %d): seeing counts %s, max var plain %.3g visible %.3g"
          % (path, os.path.getsize(path), os.path.getsize(os.path.join(HERE, "visibility_%s.npz" % name)), counts.tolist(),
             rec["var_plain"].max(), rec["var_visible"].max()))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "visibility_%s.npz" % name))


if __name__ == "__main__":
    for case in CASES:
        run_case(case)
