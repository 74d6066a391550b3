"""CPU oracle of the geometric gradients of unprojection (mvhmr_unproject_backward_geometry): dL/d proj_matricies and
dL/d coord_volumes for a given grad_out.

TEST INFRASTRUCTURE ONLY.  The sample positions ix, iy are computed in fp32 with exactly the forward's rounding (the FMA chain of
oracle.reference_loop_torch._project, IEEE divides, quirk Q1), so the oracle and the kernels pick the same bilinear cells even where
the ill-conditioned projection puts a voxel next to a cell boundary.  Everything downstream is float64: tap values (zero outside the
map), ds/dix and ds/diy, the aggregate's gradient, the chain rule through the perspective divide, and the sums over channels,
views and voxels.  GPU and oracle then differ only by the kernels' fp32 sums."""
import numpy as np
import torch

from oracle.reference_loop_torch import _project


def sample_cells(P, pts, H, W):
    """fp32 (a, b, z, ix, iy) of the (N,3) fp32 points under the (3,4) fp32 matrix P, in the forward's rounding order"""
    h = _project(pts, P)
    a, b, z = h[:, 0], h[:, 1], h[:, 2]
    u, w = a / z, b / z
    gx = 2.0 * (u / float(H) - 0.5)                   # Q1: x normalised by Hf, y by Wf
    gy = 2.0 * (w / float(W) - 0.5)
    ix = ((gx + 1.0) * 0.5) * float(W - 1)
    iy = ((gy + 1.0) * 0.5) * float(H - 1)
    return a, b, z, ix, iy


def _agg_grad(S, g, method):
    """dL/ds (V, C, N) for the stacked samples S and grad_out g (C, N), float64 -- autograd of aggregation.py:71-83"""
    V = S.shape[0]
    if method == "sum":
        return g[None].expand_as(S).clone()
    if method == "mean":
        return (g / V)[None].expand_as(S).clone()
    if method == "max":
        am = torch.from_numpy(np.argmax(S.numpy(), axis=0))          # first arg-max, as torch.max(dim)
        return torch.where(torch.arange(V)[:, None, None] == am[None], g[None], torch.zeros_like(S))
    if method == "softmax":
        p = torch.softmax(S, dim=0)
        out = (p * S).sum(0)
        return g[None] * p * (1.0 + S - out[None])
    raise ValueError(method)


def geometry_grad(features, proj, coords, grad_out, method):
    """features (B,V,C,H,W), proj (B,V,3,4), coords (B,X,Y,Z,3), grad_out (B,C,X,Y,Z): numpy or torch, any float dtype (features and
    grad_out are used as given, upcast; proj and coords as fp32).  -> (grad_proj (B,V,3,4), grad_coords (B,X,Y,Z,3)) float64 numpy"""
    f = torch.as_tensor(np.asarray(features, dtype=np.float64) if not torch.is_tensor(features) else features.double())
    P32 = torch.as_tensor(np.asarray(proj, dtype=np.float32) if not torch.is_tensor(proj) else proj.float())
    X32 = torch.as_tensor(np.asarray(coords, dtype=np.float32) if not torch.is_tensor(coords) else coords.float())
    G = torch.as_tensor(np.asarray(grad_out, dtype=np.float64) if not torch.is_tensor(grad_out) else grad_out.double())
    B, V, C, H, W = f.shape
    vol = tuple(X32.shape[1:4])
    N = int(np.prod(vol))
    gp = torch.zeros(B, V, 3, 4, dtype=torch.float64)
    gc = torch.zeros(B, N, 3, dtype=torch.float64)
    for b in range(B):
        pts = X32[b].reshape(-1, 3)
        Xh = torch.cat([pts.double(), torch.ones(N, 1, dtype=torch.float64)], 1)
        g = G[b].reshape(C, N)
        S, DX, DY, geo = [], [], [], []
        for v in range(V):
            a, bb, z, ix, iy = sample_cells(P32[b, v], pts, H, W)
            ix64, iy64 = ix.double(), iy.double()
            valid = (z > 0) & (ix >= -1) & (ix < W) & (iy >= -1) & (iy < H)
            x0 = torch.where(valid, torch.floor(ix64), torch.zeros_like(ix64))
            y0 = torch.where(valid, torch.floor(iy64), torch.zeros_like(iy64))
            tx, ty = torch.where(valid, ix64 - x0, 0.0), torch.where(valid, iy64 - y0, 0.0)
            fp = torch.nn.functional.pad(f[b, v], (1, 1, 1, 1))           # a tap outside the map has the value 0
            xi, yi = x0.long() + 1, y0.long() + 1
            f00, f01 = fp[:, yi, xi], fp[:, yi, xi + 1]
            f10, f11 = fp[:, yi + 1, xi], fp[:, yi + 1, xi + 1]
            s = f00 * (1 - tx) * (1 - ty) + f01 * tx * (1 - ty) + f10 * (1 - tx) * ty + f11 * tx * ty
            dx = (1 - ty) * (f01 - f00) + ty * (f11 - f10)
            dy = (1 - tx) * (f10 - f00) + tx * (f11 - f01)
            m = valid.double()[None]
            S.append(s * m); DX.append(dx * m); DY.append(dy * m)
            geo.append((a.double(), bb.double(), z.double(), valid))
        ds = _agg_grad(torch.stack(S), g, method)
        for v in range(V):
            a, bb, z, valid = geo[v]
            gx = (ds[v] * DX[v]).sum(0)
            gy = (ds[v] * DY[v]).sum(0)
            du = gx * (W - 1) / H
            dw = gy * (H - 1) / W
            zs = torch.where(valid, z, torch.ones_like(z))
            u, w = a / zs, bb / zs
            dh = torch.stack([du / zs, dw / zs, -(du * u + dw * w) / zs], 1)
            dh = torch.where(valid[:, None], dh, torch.zeros_like(dh))
            P64 = P32[b, v].double()
            gc[b] += dh @ P64[:, :3]
            gp[b, v] = dh.T @ Xh
    return gp.numpy(), gc.reshape((B,) + vol + (3,)).numpy()
