"""CPU oracle of the lens-distortion-aware un-projection (unprojection(lens=), mvhmr_unproject_*_lens): the volume and the
gradients w.r.t. features, proj_matricies and coord_volumes for a given grad_out.

TEST INFRASTRUCTURE ONLY.  The sample positions are built from geomgrad_oracle.sample_cells' building blocks (the fp32 FMA chain of
oracle.reference_loop_torch._project, IEEE divides, quirk Q1) with the lens step between the divides and the grid normalisation restated in
numpy float32, one separately rounded operation per step in the order the header pins (`lens_step32`), so oracle and kernels pick the same
bilinear cell.  A view whose five coefficients are zero skips the step.  Everything downstream is float64, laid out as
geomgrad_oracle.geometry_grad lays it out (with zero coefficients the geometry gradients are that oracle's bit for bit): tap values, ds/dix
and ds/diy, the aggregate and its gradient (geomgrad_oracle._agg_grad), the chain rule through the perspective divide.  The 2x2 Jacobian of the
lens step comes from torch.autograd on a float64 restatement of the lens FUNCTION (`lens_fn64`), not from a formula."""
import numpy as np
import torch

from geomgrad_oracle import _agg_grad
from oracle.reference_loop_torch import _project

F32 = np.float32


def _as(x, dtype):
    return torch.from_numpy(np.array(x.detach().cpu() if torch.is_tensor(x) else x, dtype=dtype))        # (a copy: the rigs' arrays are read-only)


def is_plain(L):
    """all five coefficients are +0.0 or -0.0 (NaN is not)"""
    return bool(np.all(np.asarray(L, F32)[4:9] == 0))


def lens_step32(L, u, v):
    """the pinned lens step on float32 numpy arrays u, v under one record L (10 float32) -> dict of every intermediate (float32) and `ok`
    (r2 <= r2max; NaN compares false).  numpy rounds every elementwise operation separately: no FMA"""
    L = np.asarray(L, F32)
    fx, fy, cx, cy, k1, k2, p1, p2, k3, r2max = (F32(x) for x in L)
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    two, one = F32(2), F32(1)
    with np.errstate(all="ignore"):
        xn = (u - cx) / fx
        yn = (v - cy) / fy
        xx, yy, xy = xn * xn, yn * yn, xn * yn
        r2 = xx + yy
        ok = r2 <= r2max
        rad = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = (xn * rad + (two * p1) * xy) + p2 * (r2 + two * xx)
        yd = (yn * rad + p1 * (r2 + two * yy)) + (two * p2) * xy
        ud = fx * xd + cx
        vd = fy * yd + cy
    out = dict(xn=xn, yn=yn, xx=xx, yy=yy, xy=xy, r2=r2, rad=rad, xd=xd, yd=yd, ud=ud, vd=vd, ok=ok)
    assert all(a.dtype == F32 for k, a in out.items() if k != "ok")
    return out


def lens_step64(L, u, v):
    """the same steps in float64 (for the exact rig's precondition: every intermediate must be identical)"""
    L = np.asarray(L, np.float64)
    fx, fy, cx, cy, k1, k2, p1, p2, k3, r2max = L
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        xn = (u - cx) / fx
        yn = (v - cy) / fy
        xx, yy, xy = xn * xn, yn * yn, xn * yn
        r2 = xx + yy
        ok = r2 <= r2max
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = (xn * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx)
        yd = (yn * rad + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy
        ud = fx * xd + cx
        vd = fy * yd + cy
    return dict(xn=xn, yn=yn, xx=xx, yy=yy, xy=xy, r2=r2, rad=rad, xd=xd, yd=yd, ud=ud, vd=vd, ok=ok)


def lens_fn64(L, u, v):
    """the lens FUNCTION on float64 torch tensors (differentiable): what torch.autograd takes the Jacobian of"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (float(x) for x in np.asarray(L, np.float64)[:9])
    xn, yn = (u - cx) / fx, (v - cy) / fy
    r2 = xn * xn + yn * yn
    rad = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = xn * rad + 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)
    yd = yn * rad + p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn
    return fx * xd + cx, fy * yd + cy


def lens_pull_back(L, u, v, du, dv):
    """(d/du', d/dv') -> (d/du, d/dv) at the float64 points (u, v): a vector-Jacobian product by torch.autograd (elementwise independent)"""
    uu, vv = u.detach().clone().requires_grad_(True), v.detach().clone().requires_grad_(True)
    ud, vd = lens_fn64(L, uu, vv)
    gu, gv = torch.autograd.grad((ud * du).sum() + (vd * dv).sum(), (uu, vv))
    return gu, gv


def lens_cells(P, L, pts, H, W):
    """fp32 torch (a, b, z, ix, iy, ok) of the (N,3) fp32 points under the (3,4) fp32 matrix P and the lens record L, in the kernels'
    rounding order: sample_cells with the lens step between the divides and Q1; ok = inside the fold-back guard (all True for a plain view)"""
    h = _project(pts, P)
    a, b, z = h[:, 0], h[:, 1], h[:, 2]
    u, w = a / z, b / z
    ok = torch.ones_like(z, dtype=torch.bool)
    if not is_plain(L):
        st = lens_step32(L, u.numpy(), w.numpy())
        u, w, ok = torch.from_numpy(st["ud"]), torch.from_numpy(st["vd"]), torch.from_numpy(st["ok"])
    gx = 2.0 * (u / float(H) - 0.5)                   # Q1: x normalised by Hf, y by Wf
    gy = 2.0 * (w / float(W) - 0.5)
    ix = ((gx + 1.0) * 0.5) * float(W - 1)
    iy = ((gy + 1.0) * 0.5) * float(H - 1)
    return a, b, z, ix, iy, ok


def _agg_out(S, method):
    """the aggregate of the stacked samples S (V, C, N), float64 (aggregation.py:71-83)"""
    if method == "sum":
        return S.sum(0)
    if method == "mean":
        return S.mean(0)
    if method == "max":
        return S.max(0).values
    if method == "softmax":
        return (torch.softmax(S, dim=0) * S).sum(0)
    raise ValueError(method)


def lens_unprojection(features, proj, coords, lens, grad_out, method, geometry=True):
    """features (B,V,C,H,W), proj (B,V,3,4), coords (B,X,Y,Z,3), lens (B,V,10), grad_out (B,C,X,Y,Z): numpy or torch (features and grad_out
    used as given, upcast; proj, coords and lens as fp32).
    -> dict of float64 numpy: out (B,C,X,Y,Z), grad_features (B,V,C,H,W), with geometry grad_proj (B,V,3,4), grad_coords (B,X,Y,Z,3); and
    bool numpy live (B,V,N): z > 0, inside the guard and a tap inside the map; guarded (B,V,N): z > 0 and outside the guard"""
    f_all = _as(features, np.float64)
    P32, X32, L32 = _as(proj, np.float32), _as(coords, np.float32), np.asarray(_as(lens, np.float32))
    G = _as(grad_out, np.float64)
    B, V, C, H, W = f_all.shape
    vol = tuple(X32.shape[1:4])
    N = int(np.prod(vol))
    out = torch.zeros(B, C, N, dtype=torch.float64)
    gf_all = torch.zeros(B, V, C, H, W, dtype=torch.float64)
    gp = torch.zeros(B, V, 3, 4, dtype=torch.float64)
    gc = torch.zeros(B, N, 3, dtype=torch.float64)
    live = np.zeros((B, V, N), bool)
    guarded = np.zeros((B, V, N), bool)
    for b in range(B):
        pts = X32[b].reshape(-1, 3)
        Xh = torch.cat([pts.double(), torch.ones(N, 1, dtype=torch.float64)], 1)
        g = G[b].reshape(C, N)
        f = f_all[b].clone().requires_grad_(True)
        S, DX, DY, geo = [], [], [], []
        for v in range(V):
            with np.errstate(all="ignore"):
                a, bb, z, ix, iy, ok = lens_cells(P32[b, v], L32[b, v], pts, H, W)
            ix64, iy64 = ix.double(), iy.double()
            valid = (z > 0) & ok & (ix >= -1) & (ix < W) & (iy >= -1) & (iy < H)
            live[b, v] = ((z > 0) & ok & (ix > -1) & (ix < W) & (iy > -1) & (iy < H)).numpy()
            guarded[b, v] = ((z > 0) & ~ok).numpy()
            x0 = torch.where(valid, torch.floor(ix64), torch.zeros_like(ix64))
            y0 = torch.where(valid, torch.floor(iy64), torch.zeros_like(iy64))
            tx, ty = torch.where(valid, ix64 - x0, 0.0), torch.where(valid, iy64 - y0, 0.0)
            fp = torch.nn.functional.pad(f[v], (1, 1, 1, 1))              # a tap outside the map has the value 0
            xi, yi = x0.long() + 1, y0.long() + 1
            f00, f01 = fp[:, yi, xi], fp[:, yi, xi + 1]
            f10, f11 = fp[:, yi + 1, xi], fp[:, yi + 1, xi + 1]
            s = f00 * (1 - tx) * (1 - ty) + f01 * tx * (1 - ty) + f10 * (1 - tx) * ty + f11 * tx * ty
            dx = (1 - ty) * (f01 - f00) + ty * (f11 - f10)
            dy = (1 - tx) * (f10 - f00) + tx * (f11 - f01)
            m = valid.double()[None]
            S.append(s * m); DX.append((dx * m).detach()); DY.append((dy * m).detach())
            geo.append((a.double(), bb.double(), z.double(), valid))
        S = torch.stack(S)
        o = _agg_out(S, method)
        (gf,) = torch.autograd.grad((o * g).sum(), (f,))
        out[b] = o.detach()
        gf_all[b] = gf
        if not geometry:
            continue
        ds = _agg_grad(S.detach(), g, method)
        for v in range(V):
            a, bb, z, valid = geo[v]
            gx = (ds[v] * DX[v]).sum(0)
            gy = (ds[v] * DY[v]).sum(0)
            du = gx * (W - 1) / H
            dw = gy * (H - 1) / W
            zs = torch.where(valid, z, torch.ones_like(z))
            u, w = a / zs, bb / zs
            if not is_plain(L32[b, v]):
                # (d/du', d/dv') -> (d/du, d/dv) through the lens; evaluated at a harmless point where the view takes no part
                uq, wq = torch.where(valid, u, torch.zeros_like(u)), torch.where(valid, w, torch.zeros_like(w))
                du, dw = lens_pull_back(L32[b, v], uq, wq, torch.where(valid, du, torch.zeros_like(du)), torch.where(valid, dw, torch.zeros_like(dw)))
            dh = torch.stack([du / zs, dw / zs, -(du * u + dw * w) / zs], 1)
            dh = torch.where(valid[:, None], dh, torch.zeros_like(dh))
            P64 = P32[b, v].double()
            gc[b] += dh @ P64[:, :3]
            gp[b, v] = dh.T @ Xh
    res = dict(out=out.reshape((B, C) + vol).numpy(), grad_features=gf_all.numpy(), live=live, guarded=guarded)
    if geometry:
        res.update(grad_proj=gp.numpy(), grad_coords=gc.reshape((B,) + vol + (3,)).numpy())
    return res


# ------------------------------------------------------------------------------------------------------------- rigs
def ring_rig(B, V, C, H, W, vol, seed, dists, focal=1145.0, radius=5000.0, side=2500.0, theta=0.3):
    """cameras on a ring around a cuboid (test_unproject_gpu._ring_problem's geometry) WITH lens coefficients: dists[(b * V + v) % len(dists)]
    is the (k1, k2, p1, p2, k3) of camera (b, v) (None: a pin-hole camera).  The projections and the lens records come from the package's own
    helpers, as a caller builds them.  -> features (B,V,C,H,W), proj (B,V,3,4), coords (B,X,Y,Z,3), lens (B,V,10): numpy fp32"""
    from multiviewhmr_amd import aggregation, multiview
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((B, V, C, H, W), dtype=np.float32)
    cameras = [[None] * B for _ in range(V)]
    for b in range(B):
        for v in range(V):
            az = 2 * np.pi * v / V + 0.3 + 0.1 * b
            eye = np.array([radius * np.cos(az), radius * np.sin(az), 0.3 * radius])
            fwd = -eye / np.linalg.norm(eye)
            right = np.cross(fwd, [0, 0, 1.0]); right /= np.linalg.norm(right)
            R = np.stack([right, np.cross(fwd, right), fwd])
            cam = multiview.Camera(R, -R @ eye, [[focal, 0, 512], [0, focal, 512], [0, 0, 1]], dist=dists[(b * V + v) % len(dists)])
            cam.update_after_crop((150, 150, 850, 850))
            cameras[v][b] = cam
    proj = aggregation.feature_level_projections(cameras, (700, 700), (H, W))
    lens = aggregation.feature_level_lens(cameras, (700, 700), (H, W))
    X, Y, Z = vol
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).astype(np.float64)
    pts = -side / 2 + g * (side / np.maximum(np.array([X, Y, Z]) - 1, 1))
    ct, st = np.cos(theta), np.sin(theta)
    pts = pts @ np.array([[ct, -st, 0], [st, ct, 0], [0, 0, 1.0]]).T
    coords = np.broadcast_to(pts.astype(np.float32), (B,) + pts.shape).copy()
    return feats, proj, coords, lens


BARREL = (-0.2, 0.05, 0.0, 0.0, 0.0)
TANGENTIAL = (0.0, 0.0, 0.01, -0.008, 0.0)
FULL = (-0.18, 0.04, 0.006, -0.004, 0.01)
LENSES = {"barrel": (BARREL,), "tangential": (TANGENTIAL,), "full": (FULL,), "mixed": (FULL, None, BARREL)}


def raw_positions(P, L, pts, H, W):
    """fp32 torch (z, ix, iy, ok): lens_cells, for the fold-back tests -- ix, iy are where the raw polynomial lands, whatever the guard says"""
    _, _, z, ix, iy, ok = lens_cells(P, L, pts, H, W)
    return z, ix, iy, ok


def foldback_rig(B=1, V=2, C=8, H=18, W=26, vol=(5, 5, 4), seed=7):
    """a wide-angle rig under strong barrel distortion (k1 = -0.3: r2max = 1 / 0.9): cameras close to a large cuboid, so that the far voxels
    lie past the guard while the raw polynomial, no longer monotonic there, folds them back into the frame.  Folded rays land inside the disc
    the live ones cover (r rad(r^2) peaks at the guard), so the map is finer than the parity rigs': 468 pixels for 100 voxels leave pixels
    that ONLY a folded ray would tap, which the GPU test poisons"""
    return ring_rig(B, V, C, H, W, vol, seed, ((-0.3, 0.0, 0.0, 0.0, 0.0),), focal=300.0, radius=2400.0, side=4200.0)


# ------------------------------------------------------------------------------------------------------------- the exact rig
EXACT = dict(B=2, V=4, C=6, H=8, W=4, vol=(4, 4, 3), seed=71, fmax=8, gmax=4, half_steps=False, depths=(2,))


def exact_rig():
    """tests/lattice_rig.py geometry with power-of-two maps, so that Q1's divisions are exact after the lens as well: u is a whole number and
    v a multiple of 1/2 (row scales H / q in {2, 4} and W / q in {1, 2}, depths 1 and 2, whole offsets).  fx = 2, fy = 1, cx = 4, cy = 2 make
    xn and yn multiples of 1/2, and with only k1 = +-2^-j non-zero every intermediate of the lens step has a handful of bits: u' is a multiple
    of 2^-(j+2), ix and iy of 3 / 2^(j+5) and 7 / 2^(j+5).  Views take k1 = -1/4, +1/4, -1/8 and 0 (a plain view) in turn.
    -> features, proj, coords, grad_out, lens: numpy fp32"""
    import lattice_rig
    feats, proj, coords, grad = lattice_rig.lattice_problem(**EXACT)
    B, V = EXACT["B"], EXACT["V"]
    from multiviewhmr_amd import aggregation
    lens = np.zeros((B, V, 10), F32)
    k1s = (-0.25, 0.25, -0.125, 0.0)
    for b in range(B):
        for v in range(V):
            k1 = k1s[(b + v) % 4]
            lens[b, v] = (2.0, 1.0, 4.0, 2.0, k1, 0, 0, 0, 0, aggregation.lens_r2max(k1, 0.0, 0.0))
    return feats, proj, coords, grad, lens
