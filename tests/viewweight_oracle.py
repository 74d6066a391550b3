"""CPU oracle of the un-projection under per-view confidence weights (unprojection(view_weights=...), mvhmr_unproject_*_weighted;
DESIGN.md 5.9): the volume and its gradients w.r.t. features, weights, proj_matricies and coord_volumes for a given grad_out.

TEST INFRASTRUCTURE ONLY.  As in geomgrad_oracle.py the sample positions are computed in fp32 with exactly the forward's rounding
(geomgrad_oracle.sample_cells), so oracle and kernels pick the same bilinear cells and no comparison has to leave out any voxel, view or
sample; everything downstream is float64.  Per sample b the present views are P = { v : (no mask or mask[b,v]) and w[b,v] > 0 }; with
s_v the per-view sample (zero where z <= 0 or the taps leave the map; such zeros take part) and W = sum_P w_v

    sum      out = sum_P w_v s_v                                           ds_v = g w_v              dw_v = g s_v
    mean     out = sum_P w_v s_v / W                                       ds_v = g w_v / W          dw_v = g (s_v - out) / W
    softmax  out = sum_P p_v s_v,  p_v = w_v e^{s_v} / sum_P w_u e^{s_u}    ds_v = g p_v (1 + s_v - out)   dw_v = g (p_v / w_v)(s_v - out)

`out`, grad_features and grad_weights come from float64 autograd through the `out` column; grad_proj and grad_coords from the ds_v
column (weighted_agg_grad, the weighted form of geomgrad_oracle._agg_grad) through geomgrad_oracle's chain rule.  Absent views are never
touched (their features and projections may hold anything) and get zero gradients; a sample without present views gives zeros."""
import numpy as np
import torch

from geomgrad_oracle import sample_cells

METHODS = ("sum", "mean", "softmax")


def weighted_out(S, w, method):
    """the `out` column: S (P, C, N) float64 samples of the present views, w (P,) float64 weights > 0 -> (C, N)"""
    ww = w[:, None, None]
    if method == "sum":
        return (ww * S).sum(0)
    if method == "mean":
        return (ww * S).sum(0) / w.sum()
    if method == "softmax":
        e = ww * torch.exp(S - S.max(0, keepdim=True).values)
        return (e * S).sum(0) / e.sum(0)
    raise ValueError(method)


def weighted_agg_grad(S, w, g, method):
    """the ds_v and dw_v columns: -> (dL/dS (P, C, N), per-voxel-and-channel contributions to dL/dw (P, C, N)), float64"""
    ww = w[:, None, None]
    out = weighted_out(S, w, method)[None]
    if method == "sum":
        return g[None] * ww.expand_as(S), g[None] * S
    if method == "mean":
        W = w.sum()
        return g[None] * (ww / W).expand_as(S), g[None] * (S - out) / W
    if method == "softmax":
        e = torch.exp(S - S.max(0, keepdim=True).values)
        q = e / (ww * e).sum(0, keepdim=True)                 # p_v / w_v
        return g[None] * ww * q * (1.0 + S - out), g[None] * q * (S - out)
    raise ValueError(method)


def _as(x, dtype):
    return torch.as_tensor(np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=dtype))


def present_views(weights, mask=None):
    """(B, V) bool numpy: mask (None: all) and weight > 0 -- zero, negative and NaN weights are absent"""
    w = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights, dtype=np.float64)
    p = w > 0
    if mask is not None:
        p &= np.asarray(mask.detach().cpu() if torch.is_tensor(mask) else mask) != 0
    return p


def weighted_unprojection(features, proj, coords, weights, grad_out, method, mask=None, geometry=True):
    """features (B,V,C,H,W), proj (B,V,3,4), coords (B,X,Y,Z,3), weights (B,V), grad_out (B,C,X,Y,Z), mask (B,V) or None: numpy or torch
    (features, weights and grad_out used as given, upcast; proj and coords as fp32).
    -> dict of float64 numpy: out (B,C,X,Y,Z), grad_features (B,V,C,H,W), grad_weights (B,V), and with geometry grad_proj (B,V,3,4),
    grad_coords (B,X,Y,Z,3)"""
    f_all = _as(features, np.float64)
    P32, X32 = _as(proj, np.float32), _as(coords, np.float32)
    w_all, G = _as(weights, np.float64), _as(grad_out, np.float64)
    B, V, C, H, W = f_all.shape
    vol = tuple(X32.shape[1:4])
    N = int(np.prod(vol))
    present = present_views(w_all, mask)
    res = dict(out=torch.zeros(B, C, N, dtype=torch.float64), grad_features=torch.zeros(B, V, C, H, W, dtype=torch.float64),
               grad_weights=torch.zeros(B, V, dtype=torch.float64), grad_proj=torch.zeros(B, V, 3, 4, dtype=torch.float64),
               grad_coords=torch.zeros(B, N, 3, dtype=torch.float64))
    for b in range(B):
        views = [int(v) for v in np.nonzero(present[b])[0]]
        if not views:
            continue
        pts = X32[b].reshape(-1, 3)
        Xh = torch.cat([pts.double(), torch.ones(N, 1, dtype=torch.float64)], 1)
        g = G[b].reshape(C, N)
        f = f_all[b, views].clone().requires_grad_(True)
        w = w_all[b, views].clone().requires_grad_(True)
        S, DX, DY, geo = [], [], [], []
        for k, v in enumerate(views):
            a, bb, z, ix, iy = sample_cells(P32[b, v], pts, H, W)
            ix64, iy64 = ix.double(), iy.double()
            valid = (z > 0) & (ix >= -1) & (ix < W) & (iy >= -1) & (iy < H)
            x0 = torch.where(valid, torch.floor(ix64), torch.zeros_like(ix64))
            y0 = torch.where(valid, torch.floor(iy64), torch.zeros_like(iy64))
            tx, ty = torch.where(valid, ix64 - x0, 0.0), torch.where(valid, iy64 - y0, 0.0)
            fp = torch.nn.functional.pad(f[k], (1, 1, 1, 1))              # a tap outside the map has the value 0
            xi, yi = x0.long() + 1, y0.long() + 1
            f00, f01 = fp[:, yi, xi], fp[:, yi, xi + 1]
            f10, f11 = fp[:, yi + 1, xi], fp[:, yi + 1, xi + 1]
            m = valid.double()[None]
            S.append((f00 * (1 - tx) * (1 - ty) + f01 * tx * (1 - ty) + f10 * (1 - tx) * ty + f11 * tx * ty) * m)
            DX.append((((1 - ty) * (f01 - f00) + ty * (f11 - f10)) * m).detach())
            DY.append((((1 - tx) * (f10 - f00) + tx * (f11 - f01)) * m).detach())
            geo.append((a.double(), bb.double(), z.double(), valid))
        S = torch.stack(S)
        out = weighted_out(S, w, method)
        gf, gw = torch.autograd.grad((out * g).sum(), (f, w))
        res["out"][b] = out.detach()
        res["grad_features"][b, views] = gf
        res["grad_weights"][b, views] = gw
        if not geometry:
            continue
        ds, _ = weighted_agg_grad(S.detach(), w.detach(), g, method)
        for k, v in enumerate(views):
            a, bb, z, valid = geo[k]
            du = (ds[k] * DX[k]).sum(0) * (W - 1) / H
            dw = (ds[k] * DY[k]).sum(0) * (H - 1) / W
            zs = torch.where(valid, z, torch.ones_like(z))
            u, ww = a / zs, bb / zs
            dh = torch.stack([du / zs, dw / zs, -(du * u + dw * ww) / zs], 1)
            dh = torch.where(valid[:, None], dh, torch.zeros_like(dh))
            res["grad_coords"][b] += dh @ P32[b, v].double()[:, :3]
            res["grad_proj"][b, v] = dh.T @ Xh
    res["out"] = res["out"].reshape((B, C) + vol)
    res["grad_coords"] = res["grad_coords"].reshape((B,) + vol + (3,))
    if not geometry:
        del res["grad_proj"], res["grad_coords"]
    return {k: t.numpy() for k, t in res.items()}
