"""CPU oracle of per-pixel view confidence (unprojection(view_confidence=...), mvhmr_unproject_*_confidence): the volume and
the gradients w.r.t. features, the confidence maps, proj_matricies and coord_volumes for a given grad_out.

TEST INFRASTRUCTURE ONLY.  As in geomgrad_oracle.py the sample positions are computed in fp32 with exactly the forward's rounding
(geomgrad_oracle.sample_cells); everything downstream is float64 torch.  For voxel n and view v, s_v is the bilinear sample of the view's
features and c_v the bilinear sample of its confidence map with the same taps and weights (a tap outside the map has the value 0).  The
present set is

    S(b, n) = { v : mask[b, v] (if given) and c_v > 0 [and v sees n by the rule of visibility_oracle, if visible] }

so a sample that is zero, negative or NaN (a NaN pixel under a tap of non-zero weight), a view behind the camera or wholly outside the map,
is absent.  With W = sum_S c_v

    sum      out = sum_S c_v s_v
    mean     out = sum_S c_v s_v / W
    softmax  out = sum_S p_v s_v,  p_v = c_v e^(s_v - m) / sum_S c_u e^(s_u - m),  m = max_S s

(One difference of measure zero: the kernels multiply every tap inside the map by its weight, so a NaN pixel under a tap of weight EXACTLY 0
-- ix or iy a whole number -- also makes c_v NaN and the view absent there, while this oracle counts a NaN pixel only under a tap of
non-zero weight.  The tests' positions are never whole numbers.)  An empty S gives 0.

grad_features and grad_confidence are autograd's through that graph; ds_v and sum_channels dc_v are autograd's too (gradients w.r.t. the
stacked samples), and grad_proj / grad_coords are geomgrad_oracle's chain rule over v in S in float64 with one more
term per view, (sum_channels dc_v) * grad c_v(ix, iy)."""
import numpy as np
import torch

from geomgrad_oracle import sample_cells

METHODS = ("sum", "mean", "softmax")


def _as(x, dtype):
    return torch.as_tensor(np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=dtype))


def _taps(img, xi, yi):
    """img (..., H + 2, W + 2) zero-padded by one pixel; -> the four taps at (yi, xi), (yi, xi + 1), (yi + 1, xi), (yi + 1, xi + 1)"""
    return img[..., yi, xi], img[..., yi, xi + 1], img[..., yi + 1, xi], img[..., yi + 1, xi + 1]


def aggregate(S, c, present, method):
    """S (V, C, N) samples, c (V, N) confidences, present (V, N) bool -> (C, N) float64; values outside `present` are selected away"""
    m = present[:, None, :]
    zero = torch.zeros((), dtype=torch.float64)
    Sz = torch.where(m, S, zero)
    cz = torch.where(present, c, zero)[:, None, :]
    any_ = present.any(0)
    if method == "sum":
        return (cz * Sz).sum(0)
    if method == "mean":
        W = cz.sum(0)
        return (cz * Sz).sum(0) / torch.where(any_[None], W, torch.ones_like(W))
    if method == "softmax":
        mx = torch.where(m, S, torch.full_like(S, -float("inf"))).max(0).values.detach()
        mx = torch.where(any_[None].expand_as(mx), mx, torch.zeros_like(mx))
        e = cz * torch.where(m, torch.exp(Sz - mx[None]), zero)
        den = e.sum(0)
        return (e * Sz).sum(0) / torch.where(any_[None].expand_as(den), den, torch.ones_like(den))
    raise ValueError(method)


def conf_unprojection(features, proj, coords, conf, grad_out, method, mask=None, visible=False, geometry=True):
    """features (B,V,C,H,W), proj (B,V,3,4), coords (B,X,Y,Z,3), conf (B,V,H,W), grad_out (B,C,X,Y,Z), mask (B,V) or None: numpy or torch
    (features, conf and grad_out used as given, upcast; proj and coords as fp32).
    -> dict of numpy: out (B,C,X,Y,Z), grad_features (B,V,C,H,W), grad_confidence (B,V,H,W), present (B,V,N) bool, csample (B,V,N), and with
    geometry grad_proj (B,V,3,4), grad_coords (B,X,Y,Z,3); floats are float64"""
    f_all, c_all = _as(features, np.float64), _as(conf, np.float64)
    P32, X32 = _as(proj, np.float32), _as(coords, np.float32)
    G = _as(grad_out, np.float64)
    B, V, C, H, W = f_all.shape
    vol = tuple(X32.shape[1:4])
    N = int(np.prod(vol))
    res = dict(out=torch.zeros(B, C, N, dtype=torch.float64), grad_features=torch.zeros(B, V, C, H, W, dtype=torch.float64),
               grad_confidence=torch.zeros(B, V, H, W, dtype=torch.float64), grad_proj=torch.zeros(B, V, 3, 4, dtype=torch.float64),
               grad_coords=torch.zeros(B, N, 3, dtype=torch.float64))
    present_all = np.zeros((B, V, N), bool)
    csample = np.zeros((B, V, N))
    zero = torch.zeros((), dtype=torch.float64)
    for b in range(B):
        pts = X32[b].reshape(-1, 3)
        Xh = torch.cat([pts.double(), torch.ones(N, 1, dtype=torch.float64)], 1)
        g = G[b].reshape(C, N)
        f = f_all[b].clone().requires_grad_(True)
        cnan = torch.isnan(c_all[b])
        cm = torch.where(cnan, zero, c_all[b]).clone().requires_grad_(True)       # NaN pixels: absent wherever a tap touches them (below)
        S, Cs, DX, DY, DCX, DCY, geo, pres = [], [], [], [], [], [], [], []
        for v in range(V):
            with np.errstate(all="ignore"):
                a, bb, z, ix, iy = sample_cells(P32[b, v], pts, H, W)
            valid = (z > 0) & (ix > -1) & (ix < W) & (iy > -1) & (iy < H)         # some tap inside the map (make_taps)
            ix64 = torch.where(valid, ix.double(), zero)
            iy64 = torch.where(valid, iy.double(), zero)
            x0, y0 = torch.floor(ix64), torch.floor(iy64)
            tx, ty = ix64 - x0, iy64 - y0
            xi, yi = x0.long() + 1, y0.long() + 1
            w00, w01, w10, w11 = (1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty
            c00, c01, c10, c11 = _taps(torch.nn.functional.pad(cm[v], (1, 1, 1, 1)), xi, yi)
            n00, n01, n10, n11 = _taps(torch.nn.functional.pad(cnan[v].double(), (1, 1, 1, 1)), xi, yi)
            touched = (n00 * w00 + n01 * w01 + n10 * w10 + n11 * w11) > 0
            cv = c00 * w00 + c01 * w01 + c10 * w10 + c11 * w11
            p = valid & ~touched & (cv.detach() > 0)
            if mask is not None:
                p = p & bool(np.asarray(mask)[b, v])
            if visible:
                p = p & (z > 0) & (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
            f00, f01, f10, f11 = _taps(torch.nn.functional.pad(f[v], (1, 1, 1, 1)), xi, yi)
            m = p[None]                                                           # selected, not multiplied: an absent view's taps may hold anything
            S.append(torch.where(m, f00 * w00 + f01 * w01 + f10 * w10 + f11 * w11, zero))
            Cs.append(torch.where(p, cv, zero))
            DX.append(torch.where(m, (1 - ty) * (f01 - f00) + ty * (f11 - f10), zero).detach())
            DY.append(torch.where(m, (1 - tx) * (f10 - f00) + tx * (f11 - f01), zero).detach())
            DCX.append(torch.where(p, (1 - ty) * (c01 - c00) + ty * (c11 - c10), zero).detach())
            DCY.append(torch.where(p, (1 - tx) * (c10 - c00) + tx * (c11 - c01), zero).detach())
            geo.append((a.double(), bb.double(), z.double()))
            pres.append(p)
        S, Cs, present = torch.stack(S), torch.stack(Cs), torch.stack(pres)
        out = aggregate(S, Cs, present, method)
        gf, gc, ds, dc = torch.autograd.grad((out * g).sum(), (f, cm, S, Cs), allow_unused=True)
        res["out"][b] = out.detach()
        res["grad_features"][b] = gf if gf is not None else 0.0
        res["grad_confidence"][b] = gc if gc is not None else 0.0
        present_all[b] = present.numpy()
        csample[b] = Cs.detach().numpy()
        if not geometry:
            continue
        ds = torch.where(present[:, None, :], ds if ds is not None else torch.zeros_like(S), zero)
        dc = torch.where(present, dc if dc is not None else torch.zeros_like(Cs), zero)
        for v in range(V):
            a, bb, z = geo[v]
            sv = present[v]
            du = ((ds[v] * DX[v]).sum(0) + dc[v] * DCX[v]) * (W - 1) / H
            dw = ((ds[v] * DY[v]).sum(0) + dc[v] * DCY[v]) * (H - 1) / W
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
    res["present"], res["csample"] = present_all, csample
    return res
