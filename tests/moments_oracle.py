"""CPU oracle of the cross-view variance aggregates (unprojection(..., 'var' | 'meanvar'), mvhmr_unproject_*_moments): the
volume and the gradients w.r.t. features, proj_matricies and coord_volumes for a given grad_out.

TEST INFRASTRUCTURE ONLY.  Built on the machinery of the existing oracles: the sample positions are computed in fp32 with exactly the
forward's rounding (geomgrad_oracle.sample_cells), so oracle and kernels pick the same bilinear cells and decide "seen" from the same
ix, iy, z (visibility_oracle.seen_views); everything downstream is float64.  With S the participating views of one (voxel, channel),
n = |S| and s_v the per-view bilinear samples (zero padding: a view behind the camera or outside the map has the sample 0):

    mu  = sum_S s_v / n            var = sum_S (s_v - mu)^2 / n         (population variance; n = 0 gives 0 for both)

    'var'     -> (B, C, X, Y, Z)  = var
    'meanvar' -> (B, 2C, X, Y, Z) = cat([mu, var], 1)

S: every view (plain call); the present views of the sample (mask (B, V)); with `visible` the present views that see the voxel.  The
gradient of the aggregate is NOT a formula here: it is torch.autograd on this float64 restatement (w.r.t. the features, and w.r.t. the
samples -- the ds_v that drive geomgrad_oracle's chain rule through the perspective divide).  S is piecewise constant in the geometry."""
import numpy as np
import torch

from geomgrad_oracle import sample_cells
from visibility_oracle import _as, seen_views

METHODS = ("var", "meanvar")


def moments(S, part):
    """S (V, C, N) float64 samples, part (V, N) bool -> (mu, var), each (C, N); views outside `part` are selected away, not multiplied"""
    m = part[:, None, :]
    n = part.sum(0).clamp(min=1).double()
    zero = torch.zeros((), dtype=torch.float64)
    mu = torch.where(m, S, zero).sum(0) / n
    var = torch.where(m, (S - mu[None]) ** 2, zero).sum(0) / n
    return mu, var


def participating(proj, coords, H, W, mask=None, visible=False):
    """(B, V, N) bool numpy: view v takes part for voxel n"""
    B, V = np.asarray(proj).shape[:2]
    N = int(np.prod(np.asarray(coords).shape[1:4]))
    if visible:
        return seen_views(proj, coords, H, W, mask)
    part = np.ones((B, V, N), bool)
    if mask is not None:
        part &= (np.asarray(mask) != 0)[:, :, None]
    return part


def moments_unprojection(features, proj, coords, grad_out, method, mask=None, visible=False, geometry=True):
    """features (B,V,C,H,W), proj (B,V,3,4), coords (B,X,Y,Z,3), grad_out (B,C or 2C,X,Y,Z) or None, mask (B,V) or None: numpy or torch
    (features and grad_out used as given, upcast; proj and coords as fp32).
    -> dict of numpy: out (B,C|2C,X,Y,Z), mean and var (B,C,X,Y,Z), part (B,V,N) bool, count (B,N), samples_max = max |s_v| over the
    participating samples, dev_max = max |s_v - mu| over them, and with grad_out grad_features (B,V,C,H,W), tap_count (B,V,H,W) = taps of
    non-zero weight of participating voxel-views meeting in each pixel, and with geometry grad_proj (B,V,3,4), grad_coords (B,X,Y,Z,3);
    floats are float64"""
    assert method in METHODS, method
    f_all = _as(features, np.float64)
    P32, X32 = _as(proj, np.float32), _as(coords, np.float32)
    B, V, C, H, W = f_all.shape
    vol = tuple(X32.shape[1:4])
    N = int(np.prod(vol))
    halves = 2 if method == "meanvar" else 1
    G = None if grad_out is None else _as(grad_out, np.float64).reshape(B, halves * C, N)
    part_all = participating(P32, X32, H, W, mask, visible)
    res = dict(mean=torch.zeros(B, C, N, dtype=torch.float64), var=torch.zeros(B, C, N, dtype=torch.float64),
               grad_features=torch.zeros(B, V, C, H, W, dtype=torch.float64), grad_proj=torch.zeros(B, V, 3, 4, dtype=torch.float64),
               grad_coords=torch.zeros(B, N, 3, dtype=torch.float64))
    tap_count = np.zeros((B, V, H * W), np.int64)
    samples_max = dev_max = 0.0
    for b in range(B):
        pts = X32[b].reshape(-1, 3)
        Xh = torch.cat([pts.double(), torch.ones(N, 1, dtype=torch.float64)], 1)
        f = f_all[b].clone().requires_grad_(True)
        part = torch.from_numpy(part_all[b])
        S, DX, DY, geo = [], [], [], []
        for v in range(V):
            with np.errstate(all="ignore"):
                a, bb, z, ix, iy = sample_cells(P32[b, v], pts, H, W)
            valid = (z > 0) & (ix >= -1) & (ix < W) & (iy >= -1) & (iy < H) & part[v]      # (NaN compares false)
            ix64 = torch.where(valid, ix.double(), torch.zeros_like(ix, dtype=torch.float64))
            iy64 = torch.where(valid, iy.double(), torch.zeros_like(iy, dtype=torch.float64))
            x0, y0 = torch.floor(ix64), torch.floor(iy64)
            tx, ty = ix64 - x0, iy64 - y0
            fp = torch.nn.functional.pad(f[v], (1, 1, 1, 1))               # a tap outside the map has the value 0
            xi, yi = x0.long() + 1, y0.long() + 1
            f00, f01 = fp[:, yi, xi], fp[:, yi, xi + 1]
            f10, f11 = fp[:, yi + 1, xi], fp[:, yi + 1, xi + 1]
            m = valid[None]
            zero = torch.zeros((), dtype=torch.float64)
            S.append(torch.where(m, f00 * (1 - tx) * (1 - ty) + f01 * tx * (1 - ty) + f10 * (1 - tx) * ty + f11 * tx * ty, zero))
            DX.append(torch.where(m, (1 - ty) * (f01 - f00) + ty * (f11 - f10), zero).detach())
            DY.append(torch.where(m, (1 - tx) * (f10 - f00) + tx * (f11 - f01), zero).detach())
            geo.append((a.double(), bb.double(), z.double(), valid))
            if G is not None:
                for wt, px, py in (((1 - tx) * (1 - ty), x0, y0), (tx * (1 - ty), x0 + 1, y0), ((1 - tx) * ty, x0, y0 + 1), (tx * ty, x0 + 1, y0 + 1)):
                    ok = valid & (wt > 0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
                    tap_count[b, v] += np.bincount((py[ok].long() * W + px[ok].long()).numpy(), minlength=H * W)
        S = torch.stack(S)
        mu, var = moments(S, part)
        res["mean"][b], res["var"][b] = mu.detach(), var.detach()
        Sd = S.detach()
        pm = part[:, None, :].expand_as(Sd)
        if pm.any():
            samples_max = max(samples_max, float(Sd[pm].abs().max()))
            dev_max = max(dev_max, float((Sd - mu.detach()[None])[pm].abs().max()))
        if G is None:
            continue
        out = torch.cat([mu, var]) if halves == 2 else var
        gf, ds = torch.autograd.grad((out * G[b]).sum(), (f, S))
        res["grad_features"][b] = gf
        if not geometry:
            continue
        for v in range(V):
            a, bb, z, valid = geo[v]
            du = (ds[v] * DX[v]).sum(0) * (W - 1) / H
            dw = (ds[v] * DY[v]).sum(0) * (H - 1) / W
            zs = torch.where(valid, z, torch.ones_like(z))
            u, ww = torch.where(valid, a, torch.zeros_like(a)) / zs, torch.where(valid, bb, torch.zeros_like(bb)) / zs
            dh = torch.stack([du / zs, dw / zs, -(du * u + dw * ww) / zs], 1)
            dh = torch.where(valid[:, None], dh, torch.zeros_like(dh))
            res["grad_coords"][b] += dh @ P32[b, v].double()[:, :3]
            res["grad_proj"][b, v] = dh.T @ Xh
    res["mean"] = res["mean"].reshape((B, C) + vol)
    res["var"] = res["var"].reshape((B, C) + vol)
    res["out"] = torch.cat([res["mean"], res["var"]], 1) if halves == 2 else res["var"]
    res["grad_coords"] = res["grad_coords"].reshape((B,) + vol + (3,))
    if G is None:
        del res["grad_features"]
    if G is None or not geometry:
        del res["grad_proj"], res["grad_coords"]
    res = {k: t.numpy() for k, t in res.items()}
    res.update(part=part_all, count=part_all.sum(1), samples_max=samples_max, dev_max=dev_max)
    if G is not None:
        res["tap_count"] = tap_count.reshape(B, V, H, W)
    return res


# ---------------------------------------------------------------------------------------------- the exact lattice rig (tests/lattice_rig.py)
def lattice_moments(features, proj, coords, grad_out, method, view_mask=None, visible_only=False):
    """float64 numpy restatement on the lattice rig's own tap tables (lattice_rig.taps64), for problems on which every fp32 operation of
    the pinned order is exact wherever n is a power of two.
    -> dict: out (B,C|2C,X,Y,Z), grad_features (B,V,C,H,W) (autograd, float64), count (B,X,Y,Z) = n per voxel, compared (B,X,Y,Z) bool = n
    is 0 or a power of two, fwd_budget = the largest sum_S d_v^2 / quantum of a compared element (d_v and mu in units of the finest bit of
    any participating weight over n), bwd_budget = the largest sum |ds w| / quantum of a gradient element.  grad_out is used as given:
    zero it where `compared` is false first."""
    import lattice_rig
    F = np.float64
    f = np.asarray(features, F)
    B, V, C, H, W = f.shape
    vol = tuple(coords.shape[1:4])
    N = int(np.prod(vol))
    halves = 2 if method == "meanvar" else 1
    out = np.zeros((B, halves * C, N), F)
    gf = np.zeros((B, V, C, H * W), F)
    count = np.zeros((B, N), np.int64)
    fwd_budget = bwd_budget = 0.0
    g_all = None if grad_out is None else np.asarray(grad_out, F).reshape(B, halves * C, N)
    for b in range(B):
        pts = coords[b].reshape(-1, 3)
        T, P = [], []
        for v in range(V):
            t = lattice_rig.taps64(proj[b, v], pts, H, W)
            seen = (t["z"] > 0) & (t["ix"] >= 0) & (t["ix"] <= W - 1) & (t["iy"] >= 0) & (t["iy"] <= H - 1)
            present = np.ones(N, bool)
            if view_mask is not None:
                present &= bool(np.asarray(view_mask)[b, v])
            if visible_only:
                present &= seen
            T.append(t); P.append(present)
        P = np.stack(P)
        n = P.sum(0)
        count[b] = n
        ft = torch.from_numpy(f[b].reshape(V, C, H * W).copy()).requires_grad_(True)
        S = torch.stack([sum(ft[v][:, torch.from_numpy(T[v]["off"][k])] * torch.from_numpy(T[v]["w"][k])[None] for k in range(4)) for v in range(V)])
        mu, var = moments(S, torch.from_numpy(P))
        o = torch.cat([mu, var]) if halves == 2 else var
        out[b] = o.detach().numpy()
        # forward budget: every sample is a multiple of q_s = the finest bit of any participating weight (features are whole); mu and d_v are
        # multiples of q_s / n, d_v^2 of (q_s / n)^2: the sums stay exact while sum d_v^2 / (q_s / n)^2 < 2^24 (n a power of two)
        qs = np.full(N, np.inf)
        for v in range(V):
            qs = np.minimum(qs, np.where(P[v], lattice_rig.lowbit(T[v]["w"]).min(0), np.inf))
        qs = np.where(np.isfinite(qs), np.minimum(qs, 1.0), 1.0)
        cmp_ = (n & (n - 1)) == 0
        d = np.where(P[:, None], S.detach().numpy() - mu.detach().numpy()[None], 0.0)
        unit = qs / np.maximum(n, 1)
        with np.errstate(invalid="ignore"):
            fb = (d ** 2).sum(0) / (unit ** 2)[None]
        if cmp_.any():
            fwd_budget = max(fwd_budget, float(fb[:, cmp_].max()), float((np.abs(np.where(P[:, None], S.detach().numpy(), 0.0)).sum(0) / qs[None])[:, cmp_].max()))
        if g_all is None:
            continue
        (g_f, ds) = torch.autograd.grad((o * torch.from_numpy(g_all[b])).sum(), (ft, S))
        gf[b] = g_f.numpy()
        # backward budget: ds_v is a multiple of unit / n (g whole, 2 g_v d_v / n + g_m / n), every scatter term ds * w of that times the
        # weight's finest bit
        dsn = np.abs(ds.numpy())
        for v in range(V):
            t = T[v]
            q_el = np.full(H * W, np.inf)
            mag = np.zeros((C, H * W), F)
            for k in range(4):
                live = t["ok"][k] & (t["w"][k] > 0) & P[v] & cmp_          # (grad_out is zero at the voxels that are not compared)
                lb = np.where(live, unit / np.maximum(n, 1) * lattice_rig.lowbit(t["w"][k]), np.inf)
                np.minimum.at(q_el, t["off"][k], lb)
                for c in range(C):
                    mag[c] += np.bincount(t["off"][k], weights=np.where(live, dsn[v, c] * t["w"][k], 0.0), minlength=H * W)
            with np.errstate(invalid="ignore"):
                bwd_budget = max(bwd_budget, float(np.where(np.isfinite(q_el)[None], mag / q_el[None], 0.0).max()))
    compared = ((count & (count - 1)) == 0).reshape((B,) + vol)
    return dict(out=out.reshape((B, halves * C) + vol), grad_features=gf.reshape(B, V, C, H, W), count=count.reshape((B,) + vol),
                compared=compared, fwd_budget=fwd_budget, bwd_budget=bwd_budget)
