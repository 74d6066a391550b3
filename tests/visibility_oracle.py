"""CPU oracle of visibility-aware aggregation (unprojection(visible_only=True), mvhmr_unproject_*_visible): the volume, the
bitmask of seeing views and the gradients w.r.t. features, proj_matricies and coord_volumes for a given grad_out.

TEST INFRASTRUCTURE ONLY.  As in geomgrad_oracle.py the sample positions are computed in fp32 with exactly the forward's rounding
(geomgrad_oracle.sample_cells), so oracle and kernels decide "seen" from the same ix, iy, z; everything downstream is float64.  View v
SEES voxel n iff

    z > 0  and  0 <= ix <= Wf - 1  and  0 <= iy <= Hf - 1          (both ends inclusive; NaN anywhere is not seen)

and S(b, n) is the set of present views (mask (B, V) or None) that see n.  With s_v the bilinear sample of a seeing view (its footprint
lies wholly inside the map)

    sum      out = sum_S s_v                       ds_v = g
    mean     out = sum_S s_v / |S|                 ds_v = g / |S|
    max      out = max_S s_v                       ds_v = g for the first arg-max in view order
    softmax  out = sum_S p_v s_v, p over S         ds_v = g p_v (1 + s_v - out)

|S| = 0: out = 0 and every gradient of the voxel is 0; ds_v = 0 for v outside S.  S is piecewise constant in the geometry: grad_proj and
grad_coords are geomgrad_oracle's chain rule over v in S.  `edge_voxels` marks the voxels a comparison may leave out: one of their
(present) views lies within `eps` px of a map edge or has |z| < eps * max |z| in float64, where fp32 and float64 may disagree about S."""
import numpy as np
import torch

from geomgrad_oracle import sample_cells

METHODS = ("sum", "mean", "max", "softmax")


def _as(x, dtype):
    return torch.as_tensor(np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=dtype))


def seen_views(proj, coords, H, W, mask=None):
    """(B, V, N) bool numpy: view v is present and sees voxel n, decided in fp32 exactly as the kernels do"""
    P32, X32 = _as(proj, np.float32), _as(coords, np.float32)
    B, V = P32.shape[:2]
    N = int(np.prod(X32.shape[1:4]))
    seen = np.zeros((B, V, N), bool)
    for b in range(B):
        pts = X32[b].reshape(-1, 3)
        for v in range(V):
            if mask is not None and not bool(np.asarray(mask)[b, v]):
                continue
            with np.errstate(all="ignore"):
                _, _, z, ix, iy = sample_cells(P32[b, v], pts, H, W)
            seen[b, v] = ((z > 0) & (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)).numpy()
    return seen


def visibility_bits(proj, coords, H, W, mask=None):
    """(B, X, Y, Z) int32 numpy: bit v = view v is present and sees the voxel (what view_visibility returns)"""
    seen = seen_views(proj, coords, H, W, mask)
    V = seen.shape[1]
    bits = (seen.astype(np.int64) << np.arange(V, dtype=np.int64)[None, :, None]).sum(1).astype(np.int32)
    return bits.reshape(tuple(coords.shape[:4]))


def edge_voxels(proj, coords, H, W, eps=1e-3, mask=None):
    """(B, N) bool numpy: some present view of the voxel lies within eps px of a map edge, or has |z| < eps * max |z|, in float64"""
    P = np.asarray(_as(proj, np.float32), np.float64)
    X = np.asarray(_as(coords, np.float32), np.float64)
    B, V = P.shape[:2]
    pts = X.reshape(B, -1, 3)
    hom = np.concatenate([pts, np.ones(pts.shape[:2] + (1,))], -1)
    r = np.einsum("bvij,bnj->bvni", P, hom)
    z = r[..., 2]
    with np.errstate(all="ignore"):
        ix = r[..., 0] / z / H * (W - 1)
        iy = r[..., 1] / z / W * (H - 1)
        near = np.minimum.reduce([np.abs(ix), np.abs(ix - (W - 1)), np.abs(iy), np.abs(iy - (H - 1))]) < eps
        near &= z > 0                                                # behind the camera the position means nothing
    near |= np.abs(z) < eps * np.abs(z).max()
    if mask is not None:
        near &= (np.asarray(mask) != 0)[:, :, None]
    return near.any(1)


def seen_out(S, seen, method):
    """the `out` column: S (V, C, N) float64 samples (anything where not seen), seen (V, N) bool -> (C, N); |S| = 0 gives 0"""
    m = seen[:, None, :]
    cnt = seen.sum(0)
    if method in ("sum", "mean"):
        r = torch.where(m, S, torch.zeros_like(S)).sum(0)
        return r / cnt.clamp(min=1) if method == "mean" else r
    Sm = torch.where(m, S, torch.full_like(S, -float("inf")))
    mx = Sm.max(0).values
    mx = torch.where(cnt > 0, mx, torch.zeros_like(mx))
    if method == "max":
        return mx
    if method == "softmax":
        e = torch.where(m, torch.exp(torch.where(m, S, torch.zeros_like(S)) - mx[None]), torch.zeros_like(S))
        den = e.sum(0)
        return (e * torch.where(m, S, torch.zeros_like(S))).sum(0) / torch.where(cnt > 0, den, torch.ones_like(den))
    raise ValueError(method)


def seen_agg_grad(S, seen, g, method):
    """the ds_v column: dL/dS (V, C, N) float64, exact zeros outside S"""
    V = S.shape[0]
    m = seen[:, None, :]
    cnt = seen.sum(0).clamp(min=1).double()
    zero = torch.zeros_like(S)
    if method == "sum":
        return torch.where(m, g[None].expand_as(S), zero)
    if method == "mean":
        return torch.where(m, (g / cnt)[None].expand_as(S), zero)
    Sm = torch.where(m, S, torch.full_like(S, -float("inf")))
    if method == "max":
        am = torch.from_numpy(np.argmax(Sm.numpy(), axis=0))          # first arg-max in view order, as torch.max(dim)
        return torch.where((torch.arange(V)[:, None, None] == am[None]) & m, g[None].expand_as(S), zero)
    if method == "softmax":
        out = seen_out(S, seen, method)
        mx = torch.where(seen.any(0), Sm.max(0).values, torch.zeros_like(out))
        Sz = torch.where(m, S, zero)
        e = torch.where(m, torch.exp(Sz - mx[None]), zero)
        den = e.sum(0)
        p = e / torch.where(den > 0, den, torch.ones_like(den))[None]
        return torch.where(m, g[None] * p * (1.0 + Sz - out[None]), zero)
    raise ValueError(method)


def visible_unprojection(features, proj, coords, grad_out, method, mask=None, geometry=True):
    """features (B,V,C,H,W), proj (B,V,3,4), coords (B,X,Y,Z,3), grad_out (B,C,X,Y,Z), mask (B,V) or None: numpy or torch (features and
    grad_out used as given, upcast; proj and coords as fp32).
    -> dict of numpy: out (B,C,X,Y,Z), grad_features (B,V,C,H,W), bits (B,X,Y,Z) int32, seen (B,V,N) bool, and with geometry grad_proj
    (B,V,3,4), grad_coords (B,X,Y,Z,3); floats are float64"""
    f_all = _as(features, np.float64)
    P32, X32 = _as(proj, np.float32), _as(coords, np.float32)
    G = _as(grad_out, np.float64)
    B, V, C, H, W = f_all.shape
    vol = tuple(X32.shape[1:4])
    N = int(np.prod(vol))
    seen_all = seen_views(P32, X32, H, W, mask)
    res = dict(out=torch.zeros(B, C, N, dtype=torch.float64), grad_features=torch.zeros(B, V, C, H, W, dtype=torch.float64),
               grad_proj=torch.zeros(B, V, 3, 4, dtype=torch.float64), grad_coords=torch.zeros(B, N, 3, dtype=torch.float64))
    for b in range(B):
        pts = X32[b].reshape(-1, 3)
        Xh = torch.cat([pts.double(), torch.ones(N, 1, dtype=torch.float64)], 1)
        g = G[b].reshape(C, N)
        f = f_all[b].clone().requires_grad_(True)
        seen = torch.from_numpy(seen_all[b])
        S, DX, DY, geo = [], [], [], []
        for v in range(V):
            with np.errstate(all="ignore"):
                a, bb, z, ix, iy = sample_cells(P32[b, v], pts, H, W)
            sv = seen[v]
            ix64 = torch.where(sv, ix.double(), torch.zeros_like(ix, dtype=torch.float64))
            iy64 = torch.where(sv, iy.double(), torch.zeros_like(iy, dtype=torch.float64))
            x0, y0 = torch.floor(ix64), torch.floor(iy64)
            tx, ty = ix64 - x0, iy64 - y0
            fp = torch.nn.functional.pad(f[v], (1, 1, 1, 1))               # a tap outside the map has the value 0 (ix == Wf - 1: weight 0 too)
            xi, yi = x0.long() + 1, y0.long() + 1
            f00, f01 = fp[:, yi, xi], fp[:, yi, xi + 1]
            f10, f11 = fp[:, yi + 1, xi], fp[:, yi + 1, xi + 1]
            m = sv[None]                                                 # selected, not multiplied: what an unseen view would tap may hold anything
            zero = torch.zeros((), dtype=torch.float64)
            S.append(torch.where(m, f00 * (1 - tx) * (1 - ty) + f01 * tx * (1 - ty) + f10 * (1 - tx) * ty + f11 * tx * ty, zero))
            DX.append(torch.where(m, (1 - ty) * (f01 - f00) + ty * (f11 - f10), zero).detach())
            DY.append(torch.where(m, (1 - tx) * (f10 - f00) + tx * (f11 - f01), zero).detach())
            geo.append((a.double(), bb.double(), z.double()))
        S = torch.stack(S)
        out = seen_out(S, seen, method)
        (gf,) = torch.autograd.grad((out * g).sum(), (f,))
        res["out"][b] = out.detach()
        res["grad_features"][b] = gf
        if not geometry:
            continue
        ds = seen_agg_grad(S.detach(), seen, g, method)
        for v in range(V):
            a, bb, z = geo[v]
            sv = seen[v]
            du = (ds[v] * DX[v]).sum(0) * (W - 1) / H
            dw = (ds[v] * DY[v]).sum(0) * (H - 1) / W
            zs = torch.where(sv, z, torch.ones_like(z))
            u, ww = torch.where(sv, a, torch.zeros_like(a)) / zs, torch.where(sv, bb, torch.zeros_like(bb)) / zs
            dh = torch.stack([du / zs, dw / zs, -(du * u + dw * ww) / zs], 1)
            dh = torch.where(sv[:, None], dh, torch.zeros_like(dh))
            res["grad_coords"][b] += dh @ P32[b, v].double()[:, :3]
            res["grad_proj"][b, v] = dh.T @ Xh
    res["out"] = res["out"].reshape((B, C) + vol)
    res["grad_coords"] = res["grad_coords"].reshape((B,) + vol + (3,))
    if not geometry:
        del res["grad_proj"], res["grad_coords"]
    res = {k: t.numpy() for k, t in res.items()}
    res["seen"] = seen_all
    res["bits"] = (seen_all.astype(np.int64) << np.arange(V, dtype=np.int64)[None, :, None]).sum(1).astype(np.int32).reshape((B,) + vol)
    return res
