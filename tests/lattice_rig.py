"""The exact lattice rig: un-projection problems on which every fp32 operation of the kernels is exact, and their float64 oracle.

TEST INFRASTRUCTURE ONLY (a plain helper module; tests/test_lattice_cpu.py checks its premise, tests/test_lattice_gpu.py uses it).

Construction.  coords[b, i, j, k] = (i, j, k).  View v of sample b reads two volume axes (a0, a1), taken in rotation
over (0,1), (1,2), (2,0), (0,2) starting at b, so one brick's z-run is a point, a row or a column of the map depending on the view:

    row 0 = (H / q0) * (e_a0 | t0)        row 1 = (W / q1) * (e_a1 | t1)        row 2 = (0, 0, 0 | d)

q = the power of two >= (extent of that axis - 1), d in {1, 2, 4} (with V > 2 one view has d = -1, behind the camera, and one d = 0),
t in [-q/4, q/4].  Quirk Q1 divides u by Hf, hence H in row 0: u / Hf = (c + t) / (q d) exactly, ix = that * (W - 1) exactly, and the
bilinear weights are multiples of 1 / (q d): every product and every partial sum of the forward and of the scatter is a dyadic number
of few bits, so `sum`, `max` and power-of-two `mean` do not depend on the order of the additions (or of float atomics) and the fp32
result has the bits of the float64 one.  `budget` verifies that from the tap tables: sum |terms| / quantum < 2^24 per compared element.

One departure from whole-number t: with t whole, ix lies in (W - 1, W) only when q > W - 1 (0 < c + t - q d < q d / (W - 1) has no
whole solution otherwise), which none of the map sizes the kernels' routes need satisfies.  Views with d = 1 therefore draw t from the
half-integers half of the time; the weights are then multiples of 1 / (2 q d), just as exact, and c + t = q + 1/2 lands between the last
column and the edge of the zero padding.

The depths are not drawn freely from {1, 2, 4} either: the views take turns of six, four with d = 1 (only they can reach the last pixel
and the band behind it; their t aims at the edge conditions, edge_offset) and two with d drawn from `depths` = (2, 4) and a random t.

Features are whole numbers in [-fmax, fmax] (exact in fp16 / bf16), grad_out whole numbers in [-gmax, gmax].  The oracle is numpy
float64 throughout (oracle/unproject_np.py's steps, plus the options of README "Per-sample view masks" ... "Shared feature maps"); its
result is cast once to the storage type.  For `max` the oracle reports the voxels whose two largest samples tie; `grad_for` zeroes
grad_out there so the tie rule cannot matter.

The geometry gradients (proj_matricies, coord_volumes, the cuboid's rotations / centers) have rigs (GEO_RIGS: power-of-two maps), an
oracle (geo_oracle) and a budget (geo_budget) of their own: the section "the geometry path" below."""
import functools

import numpy as np

PAIRS = ((0, 1), (1, 2), (2, 0), (0, 2))
LIMIT = float(2 ** 24)


def _pow2_ge(n):
    p = 1
    while p < n:
        p *= 2
    return p


EDGE_ROLES = ("hi", "lo", "top", "zero")


def edge_feasible(role, extent, span, half_steps=True):
    """can a d = 1 view put a voxel of an axis of `extent` voxels onto this edge condition of a map `span` pixels across?
    hi: strictly between the last pixel and the padding's edge (c + t = q + 1/2, and half a lattice step is less than a pixel);
    lo: the same before pixel 0 (c + t = -1/2); top: exactly the last pixel (c + t = q); zero: exactly pixel 0."""
    q = _pow2_ge(extent - 1)
    reach = q - (extent - 1)
    if role == "hi":
        return half_steps and reach + 0.5 <= q / 4 and 2 * q > span - 1
    if role == "lo":
        return half_steps and q >= 2 and 2 * q > span - 1
    if role == "top":
        return reach <= q // 4
    return True


def edge_offset(role, extent):
    """the offset t with which a d = 1 view puts a voxel of an axis of `extent` voxels onto the edge condition `role` (c + t as in
    edge_feasible; the caller has checked that the role is feasible, so |t| <= q / 4 where the issue's range matters)"""
    q = _pow2_ge(extent - 1)
    reach = q - (extent - 1)                                        # the least t with which the last voxel reaches c + t = q
    if role == "hi":
        return reach + 0.5                                          # the last voxel lands on q + 1/2: between the last pixel and the padding's edge
    if role == "lo":
        return -0.5                                                 # voxel 0 lands on -1/2: between the padding's edge and pixel 0
    if role == "top":
        # a voxel exactly on the last pixel: the last one with t = reach.  Where extent - 1 is a power of two (reach = 0) and t = 1 is
        # within q / 4 (q >= 4), t = 1 puts the last voxel but one there and the last one a whole step past it, outside the map
        return float(reach if reach or q < 4 else 1)
    # zero: a voxel exactly on pixel 0.  t = 0 puts voxel 0 there; with q >= 8 (so that -1 is within q / 4) t = -1 puts voxel 1 there
    # and voxel 0 outside the map on the low side as well
    return -1.0 if q >= 8 else 0.0


def lattice_problem(B, V, C, H, W, vol, seed, fmax=8, gmax=4, half_steps=True, M=None, depths=(2, 4), coords=None):
    """-> features (B,V,C,H,W), proj (B,V,3,4), coords (M or B,X,Y,Z,3), grad_out (M or B,C,X,Y,Z): numpy fp32.
    coords: the voxel centres to use instead of (i, j, k) -- whole numbers that stay within [0, extent - 1] on every axis, so that the
    offsets aimed at the map's edges keep their meaning (the cuboid rigs hand in a quarter turn of the lattice about its centre)"""
    rng = np.random.default_rng(seed)
    vol = tuple(int(x) for x in vol)
    n_vol = B if M is None else M
    feats = rng.integers(-fmax, fmax + 1, (B, V, C, H, W)).astype(np.float32)
    grad = rng.integers(-gmax, gmax + 1, (n_vol, C) + vol).astype(np.float32)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in vol], indexing="ij"), -1).astype(np.float32)
    if coords is None:
        coords = np.broadcast_to(grid, (n_vol,) + grid.shape).copy()
    else:
        coords = np.ascontiguousarray(coords, np.float32)
        assert coords.shape == (n_vol,) + grid.shape and (coords == np.round(coords)).all()
        assert (coords >= 0).all() and (coords <= np.array(vol, np.float32) - 1).all(), "coordinates leave the lattice's reach"
    proj = np.zeros((B, V, 3, 4), np.float32)
    # The views take turns of six: four with d = 1 whose offsets aim at the map's edges, then two with d in {2, 4} and a random whole t.
    # Each row takes the scarcest edge condition of `unmet` that its volume axis can reach (edge_feasible), so every condition some axis
    # can reach is met as soon as the rig has the views for it.
    unmet = {0: list(EDGE_ROLES), 1: list(EDGE_ROLES)}
    late = [k for k in range(B * V) if k % 6 == 5]
    dead0 = 4 if B * V >= 6 else V - 1
    dead1 = next((k for k in late if k // V != dead0 // V), late[0] if late else V - 2)
    for b in range(B):
        for v in range(V):
            k = b * V + v
            aimed = k % 6 < 4
            d = 1.0 if aimed else float(rng.choice(depths))
            if V > 2 and k == dead0:
                d = -1.0                                            # behind the camera: the sample is exactly zero
            elif V > 2 and k == dead1:
                d = 0.0
            for row, (axis, size) in enumerate(zip(PAIRS[(v + b) % 4], (H, W))):
                q = _pow2_ge(vol[axis] - 1)
                span = (W, H)[row]                                  # quirk Q1: row 0 lands on ix, scaled by W - 1
                t = float(rng.integers(-(q // 4), q // 4 + 1))
                # the scarcest unmet condition this axis can reach (fewest axes reach it); hi / top need d = 1, lo / zero any depth in front
                can = [r for r in unmet[row] if d > 0 and (d == 1.0 or r in ("lo", "zero")) and edge_feasible(r, vol[axis], span, half_steps)]
                if can:
                    role = min(can, key=lambda r: sum(edge_feasible(r, e, span, half_steps) for e in vol))
                    unmet[row].remove(role)
                    t = edge_offset(role, vol[axis])
                elif aimed and d == 1.0 and half_steps and q >= 8:
                    t = float(rng.choice([-1.5, -0.5, 0.5]))
                proj[b, v, row, axis] = size / q
                proj[b, v, row, 3] = size / q * t
            proj[b, v, 2, 3] = d
    return feats, proj, coords, grad


# ------------------------------------------------------------------------------------------------------------- float64 oracle
def taps64(proj_bv, pts, H, W):
    """oracle/unproject_np.tap_table in float64 -> dict(off (4,N), w (4,N), ok (4,N), ix, iy, z (N,), inside (N,))"""
    F = np.float64
    P = proj_bv.astype(F)
    hom = np.concatenate([pts.astype(F), np.ones((len(pts), 1), F)], axis=1)
    a, b, z = (hom * P[0]).sum(1), (hom * P[1]).sum(1), (hom * P[2]).sum(1)
    invalid = z <= 0
    zs = np.where(z == 0, F(1), z)
    u, v = a / zs, b / zs
    gx = F(2) * (u / F(H) - F(0.5))
    gy = F(2) * (v / F(W) - F(0.5))
    ix = ((gx + F(1)) / F(2)) * F(W - 1)
    iy = ((gy + F(1)) / F(2)) * F(H - 1)
    inside = (ix > -1) & (ix < W) & (iy > -1) & (iy < H) & ~invalid
    ixc, iyc = np.where(inside, ix, F(0)), np.where(inside, iy, F(0))
    x0f, y0f = np.floor(ixc), np.floor(iyc)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    wx1, wy1 = ixc - x0f, iyc - y0f
    wx0, wy0 = (x0f + 1) - ixc, (y0f + 1) - iyc
    xs = np.stack([x0, x0 + 1, x0, x0 + 1])
    ys = np.stack([y0, y0, y0 + 1, y0 + 1])
    ws = np.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1])
    ok = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H) & inside[None]
    return dict(off=np.where(ok, ys * W + xs, 0), w=np.where(ok, ws, F(0)), ok=ok, ix=ix, iy=iy, z=z, inside=inside)


def lowbit(x):
    """the value of the lowest set bit of each float64 (inf for 0): the coarsest power of two every multiple of which x is"""
    x = np.abs(np.asarray(x, np.float64))
    m, e = np.frexp(x)
    mi = np.ldexp(m, 53).astype(np.int64)
    lb = (mi & -mi).astype(np.float64)
    return np.where(x == 0, np.inf, np.ldexp(lb, e - 53))


def _scatter(off, val, size):
    return np.bincount(off.ravel(), weights=val.ravel(), minlength=size)


def oracle(features, proj, coords, grad_out, method, view_mask=None, view_weights=None, visible_only=False, view_confidence=None,
           feature_index=None, want_side_grads=False):
    """float64 un-projection with the options' definitions restated from the README:
      view_mask       a masked view is absent; `max` over no view is 0
      view_weights    present = mask and w > 0; sum is sum w_v s_v
      visible_only    present also needs z > 0, 0 <= ix <= W - 1, 0 <= iy <= H - 1
      view_confidence c_v = the map sampled with the features' taps; present also needs c_v > 0; sum is sum c_v s_v
      feature_index   volume m reads sample idx[m]; an entry outside [0, B) is a zero volume without gradients
    -> dict: out (M,C,X,Y,Z), grad_features (B,V,C,H,W), tied (M,C,X,Y,Z) bool (`max`: the two largest present samples are equal),
       visibility (M,X,Y,Z) int32, bwd_abs (B,V,C,H,W) = sum |ds w| per gradient element, tap_count (B,V,H,W), ds_max (B,V,C), fwd_budget / bwd_budget (the largest sum |terms| / quantum of any element), stats (tap coverage),
       and with want_side_grads grad_weights (B,V) / grad_confidence (B,V,H,W) and side_budget.  grad_out is used as given (zero it at `tied`
       first for `max`: see grad_for)."""
    F = np.float64
    f = np.asarray(features, F)
    B, V, C, H, W = f.shape
    vol = tuple(coords.shape[1:4])
    N = int(np.prod(vol))
    idx = np.arange(B) if feature_index is None else np.asarray(feature_index)
    M = len(idx)
    out = np.zeros((M, C, N), F)
    tied = np.zeros((M, C, N), bool)
    gf = np.zeros((B, V, C, H * W), F)
    gw = np.zeros((B, V), F)
    gc = np.zeros((B, V, H * W), F)
    bits = np.zeros((M, N), np.int64)
    g_all = None if grad_out is None else np.asarray(grad_out, F).reshape(M, C, N)
    tap_count = np.zeros((B, V, H * W), np.int64)          # taps of non-zero weight meeting in each pixel; max |ds| per (sample, view, channel)
    ds_max = np.zeros((B, V, C), F)
    bq = np.full((B, V, H * W), np.inf)                    # backward: quantum and magnitude per feature-gradient element
    bm = np.zeros((B, V, C, H * W), F)
    fwd_budget = side_budget = 0.0
    st = dict(voxel_views=0, live=0, live_taps=0, frac_taps=0, behind=0, ix0=0, ixW=0, ix_lo=0, ix_hi=0, iy0=0, iyH=0, iy_lo=0, iy_hi=0)
    for m in range(M):
        b = int(idx[m])
        if b < 0 or b >= B:
            continue
        pts = coords[m].reshape(-1, 3)
        T, S, A, P = [], [], [], []
        for v in range(V):
            t = taps64(proj[b, v], pts, H, W)
            planes = f[b, v].reshape(C, H * W)
            s = sum(planes[:, t["off"][k]] * t["w"][k][None] for k in range(4))
            seen = (t["z"] > 0) & (t["ix"] >= 0) & (t["ix"] <= W - 1) & (t["iy"] >= 0) & (t["iy"] <= H - 1)
            present = np.ones(N, bool)
            a = np.ones(N, F)
            if view_mask is not None:
                present &= bool(np.asarray(view_mask)[b, v])
            if view_weights is not None:
                present &= bool(view_weights[b, v] > 0)
                a = a * F(view_weights[b, v])
            if view_confidence is not None:
                cmap = np.asarray(view_confidence, F)[b, v].reshape(H * W)
                a = sum(cmap[t["off"][k]] * t["w"][k] for k in range(4))
                side_budget = max(side_budget, float((sum(np.abs(cmap[t["off"][k]] * t["w"][k]) for k in range(4))
                                                      / np.minimum(lowbit(t["w"]).min(0), 1.0) * 2).max()))   # maps are multiples of 1/2
                present &= a > 0
            if visible_only:
                present &= seen
            bits[m] |= (seen & (True if view_mask is None else bool(np.asarray(view_mask)[b, v]))).astype(np.int64) << v
            T.append(t); S.append(s); A.append(np.where(present, a, 0.0)); P.append(present)
            zpos = t["z"] > 0
            st["voxel_views"] += N
            st["live"] += int(t["inside"].sum())
            st["behind"] += int((t["z"] < 0).sum())
            livet = t["ok"] & (t["w"] > 0)
            st["live_taps"] += int(livet.sum())
            st["frac_taps"] += int((livet & (t["w"] < 1)).sum())
            for key, cond in (("ix0", t["ix"] == 0), ("ixW", t["ix"] == W - 1), ("ix_lo", (t["ix"] > -1) & (t["ix"] < 0)),
                              ("ix_hi", (t["ix"] > W - 1) & (t["ix"] < W)), ("iy0", t["iy"] == 0), ("iyH", t["iy"] == H - 1),
                              ("iy_lo", (t["iy"] > -1) & (t["iy"] < 0)), ("iy_hi", (t["iy"] > H - 1) & (t["iy"] < H))):
                st[key] += int((cond & t["inside"] & zpos).sum())
        S, A, P = np.stack(S), np.stack(A), np.stack(P)           # (V,C,N), (V,N), (V,N)
        # forward budget: every term a_v * f * w against the finest bit of any a_v * w (f is whole)
        qn = np.full(N, np.inf)
        mag = np.zeros((C, N), F)
        for v in range(V):
            t = T[v]
            qn = np.minimum(qn, np.where(P[v], (lowbit(A[v])[None] * lowbit(t["w"])).min(0), np.inf))
            planes = np.abs(f[b, v].reshape(C, H * W))
            mag += A[v][None] * sum(planes[:, t["off"][k]] * t["w"][k][None] for k in range(4))
        with np.errstate(invalid="ignore"):
            fwd_budget = max(fwd_budget, float(np.where(np.isfinite(qn)[None], mag / qn[None], 0.0).max()))
        if method == "sum":
            out[m] = (A[:, None] * S).sum(0)
            dS = np.broadcast_to(A[:, None], S.shape)              # ds_v / g
        elif method == "mean":
            assert view_mask is None and view_weights is None and view_confidence is None and not visible_only and V & (V - 1) == 0
            out[m] = (S.sum(0).astype(np.float32) / np.float32(V)).astype(F)      # the exact sum, then ONE fp32 division as the kernel does
            dS = np.full(S.shape, 1.0 / V)
        elif method == "max":
            assert view_weights is None and view_confidence is None
            Sm = np.where(P[:, None], S, -np.inf)
            srt = np.sort(Sm, axis=0)
            any_ = P.any(0)
            out[m] = np.where(any_[None], srt[-1], 0.0)
            if V > 1:
                tied[m] = (srt[-1] == srt[-2]) & any_[None]
            dS = ((np.arange(V)[:, None, None] == Sm.argmax(0)[None]) & P[:, None]).astype(F)
        else:
            raise ValueError(method)
        if g_all is None:
            continue
        g = g_all[m]
        for v in range(V):
            t = T[v]
            ds = g * dS[v]                                           # (C,N)
            coef = np.abs(dS[v]).max(0) if dS[v].ndim == 2 else np.abs(dS[v])
            ds_max[b, v] = np.maximum(ds_max[b, v], np.abs(ds).max(1))
            for k in range(4):
                tap_count[b, v] += np.bincount(t["off"][k][t["w"][k] > 0], minlength=H * W)
                for c in range(C):
                    gf[b, v, c] += _scatter(t["off"][k], ds[c] * t["w"][k], H * W)
                    bm[b, v, c] += _scatter(t["off"][k], np.abs(ds[c] * t["w"][k]), H * W)
                lb = np.where(t["ok"][k] & (coef > 0), lowbit(coef) * lowbit(t["w"][k]), np.inf)
                np.minimum.at(bq[b, v], t["off"][k], lb)
            if want_side_grads and method == "sum":
                gs = (g * S[v]).sum(0) * P[v]                        # sum over channels of g * s_v, per voxel
                gw[b, v] += gs.sum()
                for k in range(4):
                    gc[b, v] += _scatter(t["off"][k], gs * t["w"][k], H * W)
                # their own budgets: the per-voxel terms g * f * w, summed over channels, taps and voxels
                fin = lowbit(t["w"]).min(0)
                q_side = fin[np.isfinite(fin)].min() if np.isfinite(fin).any() else 1.0
                planes = np.abs(f[b, v].reshape(C, H * W))
                vox = (np.abs(g) * sum(planes[:, t["off"][k]] * t["w"][k][None] for k in range(4))).sum(0) * P[v]
                pix = sum(_scatter(t["off"][k], vox * t["w"][k], H * W) for k in range(4))
                side_budget = max(side_budget, float(vox.sum() / q_side), float(pix.max() / (q_side * q_side)))
    with np.errstate(invalid="ignore"):
        bwd_budget = float(np.where(np.isfinite(bq)[:, :, None], bm / bq[:, :, None], 0.0).max()) if g_all is not None else 0.0
    res = dict(out=out.reshape((M, C) + vol), grad_features=gf.reshape(B, V, C, H, W), tied=tied.reshape((M, C) + vol),
               visibility=bits.astype(np.int32).reshape((M,) + vol), fwd_budget=fwd_budget, bwd_budget=bwd_budget, stats=st,
               bwd_abs=bm.reshape(B, V, C, H, W), tap_count=tap_count.reshape(B, V, H, W), ds_max=ds_max)
    if want_side_grads:
        res.update(grad_weights=gw, grad_confidence=gc.reshape(B, V, H, W), side_budget=side_budget)
    return res


def assert_budget(res, what=""):
    """the exactness budget of the module docstring; a rig that breaks it is a test-authoring error, not a kernel finding"""
    for key in ("fwd_budget", "bwd_budget", "side_budget"):
        assert res.get(key, 0.0) < LIMIT, "lattice rig %s breaks its exactness budget: %s = %g >= 2^24" % (what, key, res[key])


# ------------------------------------------------------------------------------------------------------------- the rigs
_G = dict(C=5, H=13, W=9, vol=(9, 7, 34))                       # gather forward, scatter backward: V = 3 / C % 4 != 0 keep it off the plane kernel
_BK = dict(B=3, C=8, H=12, W=10, vol=(8, 8, 32))                # one 8 x 8 x 32 brick per sample, windows fit
RIGS = {
    "gather_v3": dict(B=4, V=3, seed=11, **_G),
    "gather_cl": dict(B=4, V=3, C=8, H=13, W=9, vol=(9, 7, 34), seed=17),             # channels-last features need C % 4 == 0
    "gather_v1": dict(B=4, V=1, seed=12, **_G),
    "gather_v2": dict(B=4, V=2, seed=13, **_G),
    "gather_v4": dict(B=3, V=4, seed=14, **_G),
    "gather_v8": dict(B=2, V=8, seed=15, **_G),
    "gather_v12": dict(B=2, V=12, seed=16, **_G),
    "brick_v2": dict(V=2, seed=21, **_BK),
    "brick_v4": dict(V=4, seed=22, **_BK),
    "brick_v8": dict(V=8, seed=23, **_BK),
    "brick_v3": dict(V=3, seed=24, **dict(_BK, B=4)),
    "brick_v6": dict(V=6, seed=25, **_BK),
    "brick_ragged": dict(B=3, V=4, C=8, H=12, W=10, vol=(9, 7, 34), seed=26),
    "brick_c4": dict(B=3, V=4, C=4, H=12, W=10, vol=(8, 8, 32), seed=27),
    "brick_c6": dict(B=3, V=4, C=6, H=12, W=10, vol=(8, 8, 32), seed=28),
    "brick_c9": dict(B=3, V=4, C=9, H=12, W=10, vol=(8, 8, 32), seed=29),
    # windows overflow LDS: the out-of-line path.  That the kernel takes it is not observable: one brick per sample is too few for AUTO to
    # ask the device gate, so the gate is queried on `auto_gather` (the same maps, bricks that cover no more of them) and answers gather;
    # that this rig's windows overflow too is inferred from that, not measured.
    "brick_slow": dict(B=3, V=4, C=8, H=320, W=320, vol=(8, 8, 32), seed=30),
    "ws_v3": dict(B=16, V=3, C=4, H=32, W=24, vol=(32, 32, 32), seed=31, gmax=2),              # 256 bricks: k_fwd_ws
    "ws_v4": dict(B=16, V=4, C=4, H=32, W=24, vol=(32, 32, 32), seed=32, gmax=2),
    "auto_brick": dict(B=3, V=4, C=8, H=48, W=40, vol=(64, 64, 32), seed=33, gmax=1, depths=(2,)),          # the gate picks the bricks
    "auto_gather": dict(B=3, V=4, C=8, H=320, W=320, vol=(32, 64, 64), seed=34),       # every brick overflows: the gate picks gather
    "quad_c8": dict(B=4, V=3, C=8, H=5, W=3, vol=(4, 4, 8), seed=41),
    "quad_c512": dict(B=4, V=3, C=512, H=5, W=3, vol=(4, 4, 8), seed=42),
    "band_h124_w5": dict(B=4, V=2, C=6, H=124, W=5, vol=(8, 8, 32), seed=43),
    "band_h125_w5": dict(B=4, V=2, C=6, H=125, W=5, vol=(8, 8, 32), seed=44),
    "band_h124_w33": dict(B=4, V=2, C=6, H=124, W=33, vol=(8, 8, 32), seed=45),
    "band_h125_w33": dict(B=4, V=2, C=6, H=125, W=33, vol=(8, 8, 32), seed=46),
    "plane_v2": dict(B=3, V=2, C=8, H=12, W=12, vol=(16, 16, 16), seed=51),            # the shipped configuration's backward: the plane kernel
    "plane_v4": dict(B=3, V=4, C=8, H=12, W=12, vol=(16, 16, 16), seed=52),
    "plane_v8": dict(B=3, V=8, C=8, H=12, W=12, vol=(16, 16, 16), seed=53),
    "options": dict(B=4, V=3, seed=61, **_G),                                          # the option routes (gather family)
    "options_conf": dict(B=4, V=3, C=5, H=13, W=9, vol=(8, 8, 8), seed=63, gmax=2, depths=(2,)),   # view_confidence: c_v has the weights' bits again
    "side_grads": dict(B=4, V=3, C=4, H=6, W=5, vol=(4, 4, 8), seed=62, fmax=4, gmax=2),   # grad_weights / grad_confidence: their own budget
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """the rig's arrays (shared, read-only)"""
    arrs = lattice_problem(**(RIGS.get(name) or OPTION_RIGS[name]))
    for a in arrs:
        a.setflags(write=False)
    return arrs


@functools.lru_cache(maxsize=None)
def reference(name, method):
    """-> (out float64, grad_out fp32 as the test must feed it, grad_features float64, the oracle's dict); budget asserted"""
    feats, proj, coords, grad = problem(name)
    if method == "max":
        tied = oracle(feats, proj, coords, None, "max")["tied"]
        grad = np.where(tied, np.float32(0), grad)
    res = oracle(feats, proj, coords, grad, method)
    assert_budget(res, "%s %s" % (name, method))
    for a in (res["out"], res["grad_features"], grad):
        a.setflags(write=False)
    return res["out"], grad, res["grad_features"], res


# ------------------------------------------------------------------------------------------------------------- the option routes
def _option_inputs(name):
    cfg = RIGS.get(name) or OPTION_RIGS.get(name) or GEO_RIGS[name]
    B, V, H, W = cfg["B"], cfg["V"], cfg["H"], cfg["W"]
    rng = np.random.default_rng(cfg["seed"] + 1000)
    mask = np.ones((B, V), np.uint8)
    mask[1] = 0
    mask[1, 1] = 1                                                   # sample 0 full, sample 1 a single view, sample 2 empty
    mask[2] = 0
    weights = rng.choice(np.array([0, 0.5, 1, 2], np.float32), (B, V))
    weights[0] = (1, 0.5, 2)[:V] if V >= 3 else 1
    conf = rng.choice(np.array([0, 0, 0.5, 1, 2], np.float32), (B, V, H, W))
    return mask, weights, conf


def option_cases():
    """(tag, rig, method, the keyword arguments of the option) for every option route the GPU file runs"""
    mask, weights, conf = _option_inputs("options")
    _, w_small, c_small = _option_inputs("side_grads")
    cases = []
    for method in ("sum", "max"):
        cases.append(("mask " + method, "options", method, dict(view_mask=mask)))
        cases.append(("visible " + method, "options", method, dict(visible_only=True)))
        cases.append(("visible+mask " + method, "options", method, dict(visible_only=True, view_mask=mask)))
        cases.append(("shared " + method, "options_shared", method, dict(feature_index=np.array([1, 1, 3, 7, 0], np.int32))))   # 1 twice, 2 never, 7 out of range
    cases.append(("weights sum", "options", "sum", dict(view_weights=weights)))
    cases.append(("confidence sum", "options_conf", "sum", dict(view_confidence=_option_inputs("options_conf")[2])))
    cases.append(("weights side sum", "side_grads", "sum", dict(view_weights=w_small, want_side_grads=True)))
    cases.append(("confidence side sum", "side_grads", "sum", dict(view_confidence=c_small, want_side_grads=True)))
    return cases


OPTION_RIGS = {"options_shared": dict(RIGS["options"], M=5)}           # M volumes over B samples: only the shared oracle reads it


@functools.lru_cache(maxsize=None)
def option_reference(tag):
    """the oracle's dict for one option case, with `grad_out` as the test must feed it (zeroed at ties for `max`); budget asserted"""
    _, name, method, kw = next(c for c in option_cases() if c[0] == tag)
    feats, proj, coords, grad = problem(name)
    if method == "max":
        grad = np.where(oracle(feats, proj, coords, None, "max", **kw)["tied"], np.float32(0), grad)
    res = oracle(feats, proj, coords, grad, method, **kw)
    assert_budget(res, tag)
    res["grad_out"] = grad
    return res


# ------------------------------------------------------------------------------------------------------------- the geometry path
# Gradients w.r.t. proj_matricies, coord_volumes and the cuboid's rotations / centers (DESIGN.md 5.5a "geometry").  The chain of
# csrc/unproject_geom_bwd.hip multiplies by kx = (W - 1) / H and ky = (H - 1) / W, which are dyadic only when H and W are powers of two:
# the geometry rigs (GEO_RIGS) are lattice problems on such maps.  ix == -1 cannot lie on the lattice: ix = (c + t) (W - 1) / (q d), and
# (c + t) = -q d / (W - 1) is no multiple of 1/2 for W - 1 = 3, 7, 15; the kept boundary has a test of its own off the lattice.
def geotaps64(proj_bv, pts, planes, H, W):
    """One view's samples and their derivatives in float64, restated from the head of csrc/unproject_geom_bwd.hip: a view takes part
    where z > 0 and -1 <= ix < W, -1 <= iy < H (ix == -1 / iy == -1 are KEPT); a tap outside the map has the VALUE 0.
    planes (K, H * W) -> dict: s (K,N), tdx / tdy (2,K,N) = the two terms of ds/dix resp. ds/diy, adx / ady (K,N) = those derivatives with
    every tap value replaced by its magnitude, u, w, z (1 where the view is behind), depth, ix, iy, valid, seen (N,)"""
    F = np.float64
    P = proj_bv.astype(F)
    K = len(planes)
    hom = np.concatenate([pts.astype(F), np.ones((len(pts), 1), F)], axis=1)
    a, b, z = (hom * P[0]).sum(1), (hom * P[1]).sum(1), (hom * P[2]).sum(1)
    front = z > 0
    zs = np.where(front, z, F(1))
    u, w = a / zs, b / zs
    ix = ((F(2) * (u / F(H) - F(0.5)) + F(1)) / F(2)) * F(W - 1)          # quirk Q1: x normalised by H, y by W
    iy = ((F(2) * (w / F(W) - F(0.5)) + F(1)) / F(2)) * F(H - 1)
    valid = front & (ix >= -1) & (ix < W) & (iy >= -1) & (iy < H)
    x0, y0 = np.where(valid, np.floor(ix), F(0)), np.where(valid, np.floor(iy), F(0))
    tx, ty = np.where(valid, ix - x0, F(0)), np.where(valid, iy - y0, F(0))
    pad = np.zeros((K, H + 2, W + 2), F)                                # one ring of zeros: x0 = -1 ... W - 1 and x0 + 1 all index it
    pad[:, 1:-1, 1:-1] = np.asarray(planes, F).reshape(K, H, W)
    xi, yi = x0.astype(np.int64) + 1, y0.astype(np.int64) + 1
    f00, f01, f10, f11 = pad[:, yi, xi], pad[:, yi, xi + 1], pad[:, yi + 1, xi], pad[:, yi + 1, xi + 1]
    m = valid[None].astype(F)
    s = (f00 * (1 - tx) * (1 - ty) + f01 * tx * (1 - ty) + f10 * (1 - tx) * ty + f11 * tx * ty) * m
    tdx = np.stack([(1 - ty) * (f01 - f00), ty * (f11 - f10)]) * m
    tdy = np.stack([(1 - tx) * (f10 - f00), tx * (f11 - f01)]) * m
    adx = ((1 - ty) * (np.abs(f01) + np.abs(f00)) + ty * (np.abs(f11) + np.abs(f10))) * m      # sum |terms| of ds/dix, for derived bounds
    ady = ((1 - tx) * (np.abs(f10) + np.abs(f00)) + tx * (np.abs(f11) + np.abs(f01))) * m
    seen = front & (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
    return dict(s=s, tdx=tdx, tdy=tdy, adx=adx, ady=ady, u=u, w=w, z=zs, depth=z, ix=ix, iy=iy, valid=valid, seen=seen)


class _Budget:
    """sum |terms| / quantum of every sum the chain takes, quantum = the lowest set bit of any term (lowbit); `worst` keeps the largest"""
    def __init__(self):
        self.worst = 0.0

    def sum(self, terms, axis=0):
        terms = np.asarray(terms, np.float64)
        if terms.shape[axis] == 0:
            return terms.sum(axis)
        q = lowbit(terms).min(axis)
        with np.errstate(invalid="ignore"):
            r = np.where(np.isfinite(q), np.abs(terms).sum(axis) / q, 0.0)
        if r.size:
            self.worst = max(self.worst, float(r.max()))
        return terms.sum(axis)

    def value(self, x):
        return self.sum(np.asarray(x, np.float64)[None])


GEO_STATS = ("voxel_views", "live", "behind", "z0", "ix0", "ixW", "ix_lo", "ix_hi", "iy0", "iyH", "iy_lo", "iy_hi")


def geo_oracle(features, proj, coords, grad_out, method, view_mask=None, view_weights=None, visible_only=False, view_confidence=None,
               feature_index=None, pose=None, want=("proj", "coords"), ds=None):
    """float64 geometry gradients of un-projection, the same inputs and options as `oracle`:
        Gx_v = sum_c ds_vc ds_vc/dix (+ under view_confidence sum_c g_c s_vc dc_v/dix: the sampled confidence moves with the voxel too)
        du = Gx kx, dw = Gy ky (kx = (W - 1) / H, ky = (H - 1) / W), dh_v = (du / z, dw / z, -(du u + dw w) / z), 0 where the view is absent
        grad_coords[m, n] = sum_v P_v[:, :3]^T dh_v        grad_proj[b, v] = sum over the volumes m naming b, and n, of dh_v (X, 1)^T
    pose = (rotations (M,3,3), centers (M,3), offsets d (M,N,3)) with coords = R d + c:  grad_rot = sum_n gX (x) d,  grad_center =
    (I - R^T) sum_n gX  (dX/dc = I - R).
    ds_vc is the aggregate's gradient as in `oracle` (sum: the view's coefficient times g; power-of-two mean: g / V; max: g at the first
    largest present sample -- zero grad_out at the returned `tied` first, see geo_reference).  want: which of grad_proj / grad_coords the caller compares;
    method 'given' takes the aggregate's gradient from the caller instead: ds (M,V,C,N) float64, zero where a view does not take part
    (the cross-view moments, whose ds depends on the other views' samples: tests/test_moments_cpu.py).
    geo_budget covers the chain ds dx -> Gx kx -> / z -> u -> P or X -> sum_n of those alone (plus the pose sums when pose is given).
    -> dict: grad_proj (B,V,3,4), grad_coords (M,X,Y,Z,3), grad_rot (M,3,3), grad_center (M,3) [pose], geo_budget, stats, tied (M,C,X,Y,Z)"""
    F = np.float64
    f = np.asarray(features, F)
    B, V, C, H, W = f.shape
    vol = tuple(coords.shape[1:4])
    N = int(np.prod(vol))
    idx = np.arange(B) if feature_index is None else np.asarray(feature_index)
    M = len(idx)
    g_all = None if method == "given" else np.asarray(grad_out, F).reshape(M, C, N)
    kx, ky = F(W - 1) / F(H), F(H - 1) / F(W)
    chain, bc, bp, bpose = _Budget(), _Budget(), _Budget(), _Budget()
    gcoords = np.zeros((M, N, 3), F)
    tied = np.zeros((M, C, N), bool)
    proj_terms = {(b, v): [] for b in range(B) for v in range(V)}
    st = dict.fromkeys(GEO_STATS, 0)
    for m in range(M):
        b = int(idx[m])
        if b < 0 or b >= B:
            continue
        pts = np.asarray(coords[m], F).reshape(-1, 3)
        Xh = np.concatenate([pts, np.ones((N, 1), F)], axis=1)
        g = None if g_all is None else g_all[m]
        T, S, A, P = [], [], [], []
        for v in range(V):
            planes = f[b, v].reshape(C, H * W)
            if view_confidence is not None:
                planes = np.concatenate([planes, np.asarray(view_confidence, F)[b, v].reshape(1, H * W)])
            t = geotaps64(proj[b, v], pts, planes, H, W)
            present = np.ones(N, bool)
            a = np.ones(N, F)
            if view_mask is not None:
                present &= bool(np.asarray(view_mask)[b, v])
            if view_weights is not None:
                present &= bool(view_weights[b, v] > 0)
                a = a * F(view_weights[b, v])
            if view_confidence is not None:
                a = t["s"][C]
                present &= a > 0
            if visible_only:
                present &= t["seen"]
            T.append(t); S.append(t["s"][:C]); A.append(np.where(present, a, 0.0)); P.append(present)
            live = t["valid"]
            st["voxel_views"] += N
            st["live"] += int(live.sum())
            st["behind"] += int((t["depth"] < 0).sum())
            st["z0"] += int((t["depth"] == 0).sum())
            for key, cond in (("ix0", t["ix"] == 0), ("ixW", t["ix"] == W - 1), ("ix_lo", (t["ix"] > -1) & (t["ix"] < 0)),
                              ("ix_hi", (t["ix"] > W - 1) & (t["ix"] < W)), ("iy0", t["iy"] == 0), ("iyH", t["iy"] == H - 1),
                              ("iy_lo", (t["iy"] > -1) & (t["iy"] < 0)), ("iy_hi", (t["iy"] > H - 1) & (t["iy"] < H))):
                st[key] += int((cond & live).sum())
        S, A, P = np.stack(S), np.stack(A), np.stack(P)
        if method == "sum":
            dS = np.broadcast_to(A[:, None], S.shape)
        elif method == "mean":
            assert view_mask is None and view_weights is None and view_confidence is None and not visible_only and V & (V - 1) == 0
            dS = np.full(S.shape, 1.0 / V)
        elif method == "max":
            assert view_weights is None and view_confidence is None
            Sm = np.where(P[:, None], S, -np.inf)
            dS = ((np.arange(V)[:, None, None] == Sm.argmax(0)[None]) & P[:, None]).astype(F)
            # a tie the geometry gradients can see: the largest sample is shared, and one of the sharing views takes part in the voxel.
            # (Two views that both miss the map share the sample 0, but whichever of them is given ds has ds/dix = ds/diy = 0.)
            top = (Sm == Sm.max(0)[None]) & P[:, None]
            live = np.stack([t["valid"] for t in T])
            tied[m] = (top.sum(0) >= 2) & (top & live[:, None]).any(0)
        elif method != "given":
            raise ValueError(method)
        coord_terms = []
        for v in range(V):
            t = T[v]
            dsv = g * dS[v] if method != "given" else chain.value(np.asarray(ds, F)[m, v])      # (C,N)
            tx_, ty_ = dsv[None] * t["tdx"][:, :C], dsv[None] * t["tdy"][:, :C]  # (2,C,N): every term of Gx / Gy
            tx_, ty_ = tx_.reshape(2 * C, N), ty_.reshape(2 * C, N)
            if view_confidence is not None:                                      # out = sum_v c_v s_v: d/dix of c_v as well
                dc = np.where(P[v], (g * S[v]).sum(0), 0.0)
                chain.sum(g * S[v])
                tx_ = np.concatenate([tx_, dc[None] * t["tdx"][:, C]])
                ty_ = np.concatenate([ty_, dc[None] * t["tdy"][:, C]])
            Gx, Gy = chain.sum(tx_), chain.sum(ty_)
            du, dw = chain.value(Gx * kx), chain.value(Gy * ky)
            z = t["z"]
            d0, d1 = chain.value(du / z), chain.value(dw / z)
            d2 = -chain.value(chain.sum(np.stack([chain.value(du * t["u"]), chain.value(dw * t["w"])])) / z)
            dh = np.stack([d0, d1, d2], 1) * (t["valid"] & P[v])[:, None]        # (N,3)
            P64 = np.asarray(proj[b, v], F)
            coord_terms.append(dh[:, :, None] * P64[None, :, :3])               # (N, r, k)
            proj_terms[(b, v)].append(dh[:, :, None] * Xh[:, None, :])           # (N, r, 4)
        gcoords[m] = bc.sum(np.concatenate(coord_terms, axis=1), axis=1)         # sum over (v, r)
    gproj = np.zeros((B, V, 3, 4), F)
    for (b, v), terms in proj_terms.items():
        if terms:
            gproj[b, v] = bp.sum(np.concatenate(terms, axis=0), axis=0)
    res = dict(grad_proj=gproj, grad_coords=gcoords.reshape((M,) + vol + (3,)), stats=st, tied=tied.reshape((M, C) + vol), chain_budget=chain.worst,
               coords_budget=bc.worst, proj_budget=bp.worst)
    budget = max([chain.worst] + ([bc.worst] if "coords" in want or pose is not None else []) + ([bp.worst] if "proj" in want else []))
    if pose is not None:
        rot, cen, d = (np.asarray(x, F) for x in pose)
        grot, gcen = np.zeros((M, 3, 3), F), np.zeros((M, 3), F)
        for m in range(M):
            grot[m] = bpose.sum(gcoords[m][:, :, None] * d[m][:, None, :])       # sum_n gX[r] d[k]
            Sg = bpose.sum(gcoords[m])
            gcen[m] = bpose.sum(np.concatenate([Sg[None], -(rot[m] * Sg[:, None])]))   # S_g[k] - sum_r R[r][k] S_g[r]
        res.update(grad_rot=grot, grad_center=gcen, pose_budget=bpose.worst)
        budget = max(budget, bpose.worst)
    res["geo_budget"] = budget
    return res


def assert_geo_budget(res, what=""):
    assert res["geo_budget"] < LIMIT, "geometry rig %s breaks its exactness budget: geo_budget = %g >= 2^24" % (what, res["geo_budget"])


_GEO = dict(H=8, W=8, vol=(5, 4, 7), fmax=4, gmax=2)                 # 140 voxels: 5 tiles of 32, the last with 12
GEO_RIGS = {
    "geo_v1": dict(_GEO, B=2, V=1, C=4, vol=(5, 4, 6), seed=71),                       # one view, 4 tiles with a 24-voxel tail
    "geo_v3": dict(_GEO, B=2, V=3, C=5, H=8, W=4, seed=72),                            # CPL = 4, C % 4 != 0, non-square, dead views d = -1 and 0
    "geo_v4": dict(_GEO, B=2, V=4, C=8, vol=(5, 5, 9), seed=73),                       # 8 tiles; the power-of-two mean
    "geo_v5": dict(_GEO, B=2, V=5, C=6, seed=74),                                      # first CPL = 2 instance
    "geo_v8": dict(_GEO, B=2, V=8, C=6, seed=75),                                      # last CPL = 2 instance; mean
    "geo_v9": dict(_GEO, B=2, V=9, C=3, seed=76),                                      # first CPL = 1 instance
    "geo_v16": dict(_GEO, B=1, V=16, C=3, seed=77),                                    # kMaxViews
    "geo_c260": dict(_GEO, B=2, V=3, C=260, vol=(3, 4, 5), fmax=2, gmax=1, seed=78),   # second 256-channel group, idle lanes
    "geo_h16": dict(_GEO, B=2, V=2, C=4, H=16, W=8, vol=(9, 5, 9), seed=79),           # q = 8 axis, H != W
    # grad_coords alone (its budget is per voxel and does not grow with N): the part == nullptr launch
    "geo_coords_big": dict(_GEO, B=2, V=3, C=5, vol=(9, 7, 34), seed=80, want=("coords",)),
    # 272 tiles per sample: k_geom_reduce's 256-thread stride takes a second trip.  grad_out is zero except at `sparse` seeded voxels
    # (voxel 0, the last one and one of tile 256 among them); with (8, 8, 160) or more seeded voxels grad_proj's budget does not hold
    "geo_many_tiles": dict(_GEO, B=1, V=2, C=4, vol=(16, 17, 32), fmax=2, gmax=1, seed=81, sparse=32),
    # the cuboid route: sample 0 unrotated, the others a quarter turn of the 5^3 lattice about its centre (about z, about x)
    "geo_pose": dict(_GEO, B=3, V=3, C=5, vol=(5, 5, 5), seed=82, pose=True),
    # the option routes
    "geo_options": dict(_GEO, B=4, V=3, C=5, seed=83),
    "geo_options_shared": dict(_GEO, B=4, V=3, C=5, seed=83, M=5),
    "geo_conf": dict(_GEO, B=4, V=3, C=5, vol=(3, 4, 5), fmax=2, gmax=1, depths=(2,), seed=84),    # c_v carries the weights' bits again
}
_QUARTER = (np.eye(3), np.array([[0., -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[1., 0, 0], [0, 0, -1], [0, 1, 0]]))


@functools.lru_cache(maxsize=None)
def geo_problem(name):
    """-> (features, proj, coords, grad_out, extras): the rig's arrays (shared, read-only); extras holds `want`, and for the cuboid rig
    rotations (B,3,3), centers (B,3), offsets d (B,N,3), position, sides"""
    cfg = dict(GEO_RIGS[name])
    extras = dict(want=cfg.pop("want", ("proj", "coords")))
    sparse, pose = cfg.pop("sparse", None), cfg.pop("pose", False)
    vol = cfg["vol"]
    if pose:
        B = cfg["B"]
        grid = np.stack(np.meshgrid(*[np.arange(s) for s in vol], indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        cen = np.tile((np.array(vol, np.float64) - 1) / 2, (B, 1))
        assert (cen == np.round(cen)).all() and len(set(vol)) == 1, "a quarter turn must map the lattice onto itself"
        rot = np.stack([_QUARTER[b % 3] for b in range(B)])
        d = grid[None] - cen[:, None]
        cfg["coords"] = (np.einsum("brk,bnk->bnr", rot, d) + cen[:, None]).reshape((B,) + tuple(vol) + (3,))
        extras.update(rotations=rot.astype(np.float32), centers=cen.astype(np.float32), d=d, position=(0.0, 0.0, 0.0),
                      sides=tuple(float(s - 1) for s in vol))
    feats, proj, coords, grad = lattice_problem(**cfg)
    if sparse:
        N = int(np.prod(vol))
        rng = np.random.default_rng(cfg["seed"] + 500)
        keep = np.zeros(N, bool)
        keep[rng.choice(N, sparse - 3, replace=False)] = True
        keep[[0, N - 1, 256 * 32 + 5]] = True                       # voxel 0, the last voxel, one in tile 256
        grad = grad * keep.reshape(vol)[None, None]
        extras["seeded"] = keep.reshape(vol)
    for a in (feats, proj, coords, grad):
        a.setflags(write=False)
    return feats, proj, coords, grad, extras


def _geo_pose_arg(extras):
    return (extras["rotations"], extras["centers"], extras["d"]) if "rotations" in extras else None


@functools.lru_cache(maxsize=None)
def geo_reference(name, method):
    """-> (grad_out fp32 as the test must feed it (zeroed at ties for `max`), the geometry oracle's dict, the tie fraction); budget asserted"""
    feats, proj, coords, grad, extras = geo_problem(name)
    ties = 0.0
    if method == "max":
        tied = geo_oracle(feats, proj, coords, np.zeros_like(grad), "max")["tied"]
        ties = float(tied.mean())
        grad = np.where(tied, np.float32(0), grad)
    res = geo_oracle(feats, proj, coords, grad, method, pose=_geo_pose_arg(extras), want=extras["want"])
    assert_geo_budget(res, "%s %s" % (name, method))
    grad.setflags(write=False)
    return grad, res, ties


def geo_option_cases():
    """(tag, rig, method, the keyword arguments of the option) for every option route of the geometry tests"""
    mask, weights, _ = _option_inputs("geo_options")
    conf = _option_inputs("geo_conf")[2]
    cases = []
    for method in ("sum", "max"):
        cases.append(("mask " + method, "geo_options", method, dict(view_mask=mask)))
        cases.append(("visible " + method, "geo_options", method, dict(visible_only=True)))
        cases.append(("visible+mask " + method, "geo_options", method, dict(visible_only=True, view_mask=mask)))
        cases.append(("shared " + method, "geo_options_shared", method, dict(feature_index=np.array([1, 1, 3, 7, 0], np.int32))))
    cases.append(("weights sum", "geo_options", "sum", dict(view_weights=weights)))
    cases.append(("confidence sum", "geo_conf", "sum", dict(view_confidence=conf)))
    return cases


@functools.lru_cache(maxsize=None)
def geo_option_reference(tag):
    """the geometry oracle's dict for one option case, with `grad_out` as the test must feed it; budget asserted"""
    _, name, method, kw = next(c for c in geo_option_cases() if c[0] == tag)
    feats, proj, coords, grad, _ = geo_problem(name)
    if method == "max":
        grad = np.where(geo_oracle(feats, proj, coords, np.zeros_like(grad), "max", **kw)["tied"], np.float32(0), grad)
    res = geo_oracle(feats, proj, coords, grad, method, **kw)
    assert_geo_budget(res, "geometry option " + tag)
    if "view_weights" in kw:                                         # grad_weights comes out of the same kernel: the feature oracle's value
        side = oracle(feats, proj, coords, grad, method, want_side_grads=True, **kw)
        assert_budget(side, "geometry option " + tag)
        res["grad_weights"] = side["grad_weights"]
    res["grad_out"] = grad
    return res
