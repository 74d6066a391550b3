"""CPU oracle of shared feature maps (unprojection(feature_index=...)).

TEST INFRASTRUCTURE ONLY.  No new arithmetic: the existing oracles (oracle.cport for the volume and the feature gradient,
geomgrad_oracle.geometry_grad for the geometry gradients) run on features[idx] and proj[idx], and np.add.at sums the per-volume gradients of
the features and the projections over the index.  An entry outside [0, B) is "no sample": a zero volume that contributes to no gradient."""
import numpy as np

from geomgrad_oracle import geometry_grad
from oracle import cport


def shared_unprojection(features, proj, coords, index, grad_out, method, geometry=True):
    """features (B,V,C,H,W), proj (B,V,3,4), coords (M,X,Y,Z,3), index (M,), grad_out (M,C,X,Y,Z) -> dict of out (M,C,X,Y,Z), grad_features
    (B,V,C,H,W), and with `geometry` grad_proj (B,V,3,4) and grad_coords (M,X,Y,Z,3): float64 numpy"""
    features, proj, coords, grad_out = (np.asarray(x) for x in (features, proj, coords, grad_out))
    index = np.asarray(index, dtype=np.int64)
    B, M = features.shape[0], len(index)
    ok = np.nonzero((index >= 0) & (index < B))[0]
    idx = index[ok]
    out = np.zeros((M,) + grad_out.shape[1:], np.float64)
    r = dict(out=out, grad_features=np.zeros(features.shape, np.float64))
    if geometry:
        r["grad_proj"] = np.zeros(proj.shape, np.float64)
        r["grad_coords"] = np.zeros(coords.shape, np.float64)
    if not len(ok):
        return r
    f, p, c, g = features[idx], proj[idx], coords[ok], grad_out[ok]
    out[ok] = cport.forward(f, p, c, method)
    np.add.at(r["grad_features"], idx, np.asarray(cport.backward(g, f, p, c, method), np.float64))
    if geometry:
        gp, gc = geometry_grad(f, p, c, g, method)
        np.add.at(r["grad_proj"], idx, gp)
        r["grad_coords"][ok] = gc
    return r
