#!/usr/bin/env python3
"""Generate tests/golden/confidence_*.npz by RUNNING the reference on the seeing views of every voxel, each view repeated k_v times.

View v carries the CONSTANT confidence map k_v in {1, 2, 3}.  Where view v sees a voxel (the rule of DESIGN.md 5.10: its bilinear footprint
lies wholly inside the map) the map samples to k_v up to rounding; where none of its taps lies inside the map (z <= 0, ix <= -1, ix >= Wf,
iy <= -1 or iy >= Hf) it samples to exactly 0 and the view is absent.  A voxel is CLEAN when every view is one or the other.  On a clean
voxel whose seeing views are S, unprojection(view_confidence=...) must equal the reference run on the views of S with view
v present k_v times: sum adds k_v s_v, mean divides by sum k_v, softmax weighs e^{s_v} by k_v.  That anchors the feature to the reference,
which has no confidence of its own.  Per case, per method, per sample and per distinct pattern S among the clean voxels the reference
runs on the repeated views; its output is taken on the clean voxels with that pattern, grad_out -- zeroed on every other voxel, so the
feature gradients compare too -- is back-propagated, and the gradients of a view's copies and of all patterns are added up.

The rigs are those of make_golden_visibility.py (problem(...) with seeds 51 / 52 / 53).  Asserted here: clean voxels are at least 70 % of
every sample's voxels, and every seeing count 0 ... V occurs among the clean voxels of the first two cases.

Only ever run where the reference is mounted (it never travels); it is imported unmodified, as tests/golden/make_golden.py does.  Each file
holds inputs AND expected outputs:
    features, proj, coords, grad_out, confidence (float32), clean (bool, (B,X,Y,Z)) -> out_<method>, gfeat_<method> (float32)

Usage:  python tests/golden/make_golden_confidence.py
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
from make_golden_visibility import problem  # noqa: E402

METHODS = ("sum", "mean", "softmax")


def classify(proj, coords, H, W):
    """-> (seen (B, V, N) bool by the rule of 5.10, outside (B, V, N) bool: no tap inside the map)"""
    B, V = proj.shape[:2]
    N = int(np.prod(coords.shape[1:4]))
    seen, outside = np.zeros((B, V, N), bool), np.zeros((B, V, N), bool)
    for b in range(B):
        pts = torch.from_numpy(coords[b].reshape(-1, 3))
        for v in range(V):
            with np.errstate(all="ignore"):
                _, _, z, ix, iy = sample_cells(torch.from_numpy(proj[b, v]), pts, H, W)
            seen[b, v] = ((z > 0) & (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)).numpy()
            outside[b, v] = (~(z > 0) | (ix <= -1) | (ix >= W) | (iy <= -1) | (iy >= H)).numpy()
    return seen, outside


def run_case(name, features, proj, coords, seed, every_count):
    B, V, C, H, W = features.shape
    vol = tuple(coords.shape[1:4])
    N = int(np.prod(vol))
    seen, outside = classify(proj, coords, H, W)
    clean = (seen | outside).all(1)                                          # (B, N)
    share = clean.mean(1)
    assert (share >= 0.70).all(), "%s: clean share %s" % (name, share.tolist())
    counts = np.bincount(seen.sum(1)[clean], minlength=V + 1)
    assert not every_count or (counts > 0).all(), "%s: counts %s" % (name, counts.tolist())
    k = np.random.default_rng(seed + 2000).integers(1, 4, size=(B, V))        # the constant maps, 1 ... 3
    conf = np.broadcast_to(k[:, :, None, None].astype(np.float32), (B, V, H, W)).copy()
    codes = (seen.astype(np.int64) << np.arange(V, dtype=np.int64)[None, :, None]).sum(1)            # (B, N)
    grad_out = torch.randn(B, C, *vol, generator=torch.Generator().manual_seed(seed + 1000))
    grad_out = grad_out * torch.from_numpy(clean).reshape((B, 1) + vol)
    rec = dict(features=features, proj=proj, coords=coords, grad_out=grad_out.numpy(), confidence=conf, clean=clean.reshape((B,) + vol))
    patterns = set()
    for method in METHODS:
        out = np.zeros((B, C, N), np.float32)
        gfeat = np.zeros_like(features)
        for b in range(B):
            for code in np.unique(codes[b][clean[b]]):
                if code == 0:
                    continue
                patterns.add((b, int(code)))
                views = [v for v in range(V) if code >> v & 1 for _ in range(k[b, v])]          # view v, k_v times
                sel = torch.from_numpy((codes[b] == code) & clean[b])
                f = torch.from_numpy(features[b:b + 1, views]).requires_grad_(True)
                o = mg.ref_agg.unprojection(f, torch.from_numpy(proj[b:b + 1, views]), torch.from_numpy(coords[b:b + 1]), aggregation_method=method)
                o = o.reshape(C, N)
                (o[:, sel] * grad_out[b].reshape(C, N)[:, sel]).sum().backward()
                out[b][:, sel.numpy()] = o.detach().numpy()[:, sel.numpy()]
                np.add.at(gfeat[b], views, f.grad.numpy()[0])
        rec["out_" + method], rec["gfeat_" + method] = out.reshape((B, C) + vol), gfeat
    path = os.path.join(HERE, "confidence_%s.npz" % name)
    np.savez_compressed(path, **rec)
    print("wrote %s, %d bytes: clean share %.3f-%.3f, counts among clean %s, %d patterns" % (path, os.path.getsize(path), share.min(), share.max(),
                                                                                             counts.tolist(), len(patterns)))
    assert os.path.getsize(path) < 500 * 1000


def main():
    f, p, c = problem(3, 4, 5, 20, 20, (6, 5, 7), 51, 4000.0)
    run_case("v4c5", f, p, c, 51, every_count=True)
    f, p, c = problem(2, 3, 6, 16, 24, (5, 6, 4), 52, 4000.0)
    run_case("v3c6_nonsquare", f, p, c, 52, every_count=True)
    f, p, c = problem(2, 8, 4, 12, 16, (4, 4, 5), 53, 10000.0)
    run_case("v8c4_behind", f, p, c, 53, every_count=False)


if __name__ == "__main__":
    main()
