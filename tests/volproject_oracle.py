"""Oracle of the ray-march of volumes into camera-view maps: the contract at the top of volume_project.hip restated in numpy,
operation for operation in float32 (fma emulated as volsample_oracle does) or, with dtype=np.float64, the same formulas in float64; the
reductions and the volume gradient in float64 downstream of the fp32 sample indices and tap weights; the exponent of the fixed-point
accumulator; the error bounds the GPU tests hold the kernels to; and the rigs.  numpy only: the CPU tests import it without a device.

Shapes: v (B, C, X*Y*Z) volume values as float64; rays (B, V, 3, 4) = [D | o]; maps (B, V, C, Hm, Wm); ranges (B, V, Hm, Wm, 2); per-ray
quantities (B, V, Hm, Wm); per-sample ones carry a trailing K.  Pixel (u, v) = (column, row).
"""
import numpy as np

import volsample_oracle as vo
from volsample_oracle import EPS, STORE, TAPS, f32, fma32, gamma

METHODS = ("mean", "max", "softmax")
GROUP, UNROLL = 8, 4        # channels per block and per loop trip (volume_project.hip: kPvGroup, kPvUnroll)
MAX_SAMPLES = 1024
POISON = 0x7FFFFFFF
EXP_ULPS = 3.0              # expf and logf: the 3 ulp OpenCL grants exp and log, which the device library is built to (1 ulp = 2 EPS)


def _fma(a, b, c, T):
    if T is np.float32:
        return fma32(a, b, c)
    return np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)


def camera_rays(P):
    """float64 [D | o] of projections (..., 3, 4) = [M | p4]: D = M^-1, o = -M^-1 p4"""
    P = np.asarray(P, np.float64)
    D = np.linalg.inv(P[..., :3])
    return np.concatenate([D, -(D @ P[..., 3:])], -1)


# ---- the contract: geometry
def origin_index(rays, rot, centers, position, sides, shape, T=np.float32, true_steps=False):
    """t_o (B, V, 3): volume_sample's index of the point o"""
    o = np.asarray(rays)[..., 3]
    if T is np.float32:
        return vo.index_fp32(o, rot, centers, position, sides, shape)
    R, c = np.asarray(rot, np.float64), np.asarray(centers, np.float64)[:, None, :]
    st = vo.steps(sides, shape, np.float64) if true_steps else vo.steps(sides, shape).astype(np.float64)
    y = np.asarray(o, np.float64) - c
    return (np.einsum("bia,bvi->bva", R, y) + (c - np.asarray(position, np.float64))) / st


def ray_geometry(rays, rot, centers, position, sides, shape, map_shape, min_depth=0.0, max_depth=np.inf, T=np.float32, true_steps=False):
    """dict: to (B,V,1,1,3), e (B,V,Hm,Wm,3), lin, lout (B,V,Hm,Wm) -- (0, 0) for a miss --, hit"""
    rays, R = np.asarray(rays, T), np.asarray(rot, T)
    Hm, Wm = map_shape
    st = vo.steps(sides, shape, np.float64).astype(T) if true_steps else vo.steps(sides, shape).astype(T)
    to = origin_index(rays, rot, centers, position, sides, shape, T, true_steps).astype(T)[:, :, None, None, :]
    u, v = np.arange(Wm, dtype=T)[None, :], np.arange(Hm, dtype=T)[:, None]
    Dm = rays[..., :3][:, :, None, None]                                        # (B,V,1,1,3,3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = [_fma(Dm[..., i, 1], v, _fma(Dm[..., i, 0], u, Dm[..., i, 2], T), T) for i in range(3)]
        Rb = R[:, None, None, None]                                             # (B,1,1,1,3,3)
        r = [_fma(Rb[..., 2, a], d[2], _fma(Rb[..., 1, a], d[1], (Rb[..., 0, a] * d[0]).astype(T), T), T) for a in range(3)]
        e = np.stack([(r[a] / st[a]).astype(T) for a in range(3)], -1)
        ok = np.ones(e.shape[:-1], bool)
        lin, lout = np.full(ok.shape, T(min_depth)), np.full(ok.shape, T(max_depth))
        for a in range(3):
            ea, ta, hi = e[..., a], np.broadcast_to(to[..., a], ok.shape), T(shape[a] - 1)
            zero = ea == 0
            l0, l1 = ((T(0) - ta) / ea).astype(T), ((hi - ta) / ea).astype(T)
            less = l0 < l1
            near, far = np.where(less, l0, l1), np.where(less, l1, l0)
            ok &= np.where(zero, (ta >= 0) & (ta <= hi), ~(np.isnan(l0) | np.isnan(l1)))
            lin = np.where(~zero & (near > lin), near, lin)
            lout = np.where(~zero & (far < lout), far, lout)
        hit = ok & (lin < lout) & (lin > -np.inf) & (lout < np.inf)
    zero = T(0)
    return {"to": to, "e": e, "lin": np.where(hit, lin, zero).astype(T), "lout": np.where(hit, lout, zero).astype(T), "hit": hit}


def sample_indices(geo, ranges, K, T=np.float32):
    """t (B,V,Hm,Wm,K,3) of the K samples of every ray from (lin, lout) = ranges (the kernel's own, or the oracle's)"""
    lin, lout = np.asarray(ranges[..., 0], T), np.asarray(ranges[..., 1], T)
    with np.errstate(invalid="ignore", over="ignore"):
        h = ((lout - lin) / T(K)).astype(T)
        k = np.arange(K, dtype=T) + T(0.5)
        lam = _fma(k, h[..., None], lin[..., None], T)                           # (B,V,Hm,Wm,K)
        return np.stack([_fma(lam, geo["e"][..., None, a], geo["to"][..., None, a], T) for a in range(3)], -1).astype(T)


def taps(t, shape, T=np.float32):
    """volume_sample's taps of indices t (..., 3): dict of live (...), w (..., 8) in T, use (..., 8): inside and of nonzero weight, vox (..., 8)"""
    t, S = np.asarray(t, T), np.asarray(shape)
    with np.errstate(invalid="ignore"):
        live = ((t > -1) & (t < S.astype(T))).all(-1)
    ts = np.where(live[..., None], t, T(0))
    fl = np.floor(ts)
    wa = np.stack([((fl + T(1)) - ts).astype(T), (ts - fl).astype(T)], -1)       # (..., 3, 2)
    idx = fl.astype(np.int64)[..., None, :] + TAPS
    inside = ((idx >= 0) & (idx < S)).all(-1) & live[..., None]
    w = ((wa[..., 0, :][..., TAPS[:, 0]] * wa[..., 1, :][..., TAPS[:, 1]]).astype(T) * wa[..., 2, :][..., TAPS[:, 2]]).astype(T)
    vox = np.where(inside, (idx[..., 0] * shape[1] + idx[..., 1]) * shape[2] + idx[..., 2], 0)
    return {"live": live, "w": w, "use": inside & (w != 0), "vox": vox}


def _gather(v, tp):
    """tap values (B,V,C,Hm,Wm,K,8) of v (B,C,Vox)"""
    B, C, _ = v.shape
    vox = tp["vox"]
    flat = vox.reshape(B, 1, -1)
    return np.take_along_axis(v, np.broadcast_to(flat, (B, C, flat.shape[2])), 2).reshape((B, C) + vox.shape[1:]).swapaxes(1, 2)


def samples(v, tp, T=np.float64):
    """s (B,V,C,Hm,Wm,K) and mag = sum |w v| over the taps that count.  T = float32: the kernel's fma chain, bit for bit"""
    vals = _gather(np.asarray(v, np.float64), tp)
    use, w = tp["use"][:, :, None], tp["w"][:, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.where(use, w.astype(np.float64) * np.where(use, vals, 0.0), 0.0)
        if T is np.float32:
            acc = np.zeros(terms.shape[:-1], np.float32)
            for j in range(8):
                acc = np.where(use[..., j], fma32(np.broadcast_to(w[..., j], acc.shape), np.where(use[..., j], vals[..., j], 0.0), acc), acc)
            return acc, np.abs(terms).sum(-1)
        return terms.sum(-1), np.abs(terms).sum(-1)


def reduce_fp32(s, hit, method, K):
    """maps (B,V,C,Hm,Wm) fp32 and the arg-k from the fp32 samples, by the contract's 'mean' and 'max' (softmax has no bit-exact oracle: expf)"""
    s = f32(s)
    h = hit[:, :, None]
    if method == "mean":
        acc = np.zeros(s.shape[:-1], np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(K):
                acc = (acc + s[..., k]).astype(np.float32)
            return np.where(h, (acc / np.float32(K)).astype(np.float32), np.float32(0)), None
    m, arg = s[..., 0].copy(), np.zeros(s.shape[:-1], np.int32)
    for k in range(1, K):
        with np.errstate(invalid="ignore"):
            take = s[..., k] > m
        m, arg = np.where(take, s[..., k], m), np.where(take, k, arg)
    return np.where(h, m, np.float32(0)), np.where(h, arg, 0)


# ---- float64 downstream of the samples
def forward(s, hit, method, beta=1.0, arg=None):
    """out (B,V,C,Hm,Wm) float64 from samples s (..., K); softmax also p (..., K) and lse.  max takes the maximum (arg only names the
    gradient's k)"""
    h = hit[:, :, None]
    res = {}
    with np.errstate(invalid="ignore", over="ignore"):
        if method == "mean":
            out = s.mean(-1)
        elif method == "max":
            out = s.max(-1)
        else:
            z = beta * s
            m = z.max(-1, keepdims=True)
            ex = np.exp(z - m)
            S = ex.sum(-1, keepdims=True)
            res["p"], res["lse"] = ex / S, np.where(h, (m + np.log(S))[..., 0], 0.0)
            out = (res["p"] * s).sum(-1)
    res["out"] = np.where(h, out, 0.0)
    return res


def backward(tp, s, hit, g, method, n_vox, beta=1.0, arg=None, fw=None):
    """grad_v (B,C,Vox) float64 by np.add.at over every live tap of every hit ray; ds (B,V,C,Hm,Wm,K); mag_v = sum |w ds|; count (B,Vox) the
    taps a voxel receives (per channel)"""
    g = np.asarray(g, np.float64)[..., None]
    K = s.shape[-1]
    h = hit[:, :, None, :, :, None]
    if method == "mean":
        ds = np.broadcast_to(g / K, s.shape)
    elif method == "max":
        ds = np.where(np.arange(K) == arg[..., None], g, 0.0)
    else:
        ds = g * fw["p"] * (1.0 + beta * (s - fw["out"][..., None]))
    ds = np.where(h, ds, 0.0)
    B, V, C = s.shape[:3]
    grad_v, mag_v, count = np.zeros((B, C, n_vox)), np.zeros((B, C, n_vox)), np.zeros((B, n_vox), np.int64)
    use = tp["use"] & hit[..., None, None]                                       # (B,V,Hm,Wm,K,8)
    w = np.where(use, tp["w"].astype(np.float64), 0.0)
    for b in range(B):
        vox = tp["vox"][b].reshape(-1)
        np.add.at(count[b], vox, use[b].reshape(-1).astype(np.int64))
        for c in range(C):
            contrib = (w[b] * ds[b, :, c][..., None]).reshape(-1)               # (V,Hm,Wm,K,8)
            np.add.at(grad_v[b, c], vox, contrib)
            np.add.at(mag_v[b, c], vox, np.abs(contrib))
    return {"grad_v": grad_v, "mag_v": mag_v, "count": count, "ds": ds}


# ---- the exponent of the fixed-point accumulator (k_pv3d_exponent; DESIGN.md 5.7's scheme)
def log2_ceil(n):
    return int(n - 1).bit_length() if n > 1 else 0


def exponents(g, v, method, K, n_rays_samples, beta=1.0):
    """E (B, C) from grad_maps g (B,V,C,Hm,Wm) and volume values v (B,C,Vox) as the kernels see them (fp32): N * bound * 2^E < 2^62"""
    g, v = f32(g), f32(v)
    B, C = v.shape[:2]
    E = np.zeros((B, C), np.int64)
    for b in range(B):
        for c in range(C):
            gm = np.abs(g[b, :, c]).astype(np.float64)
            gmax = np.inf if not np.isfinite(gm).all() else gm.max()
            fm = np.abs(v[b, c]).astype(np.float64)
            fmax = 0.0 if method != "softmax" else (np.inf if not np.isfinite(fm).all() else fm.max())
            if not np.isfinite(gmax) or not np.isfinite(fmax):
                E[b, c] = POISON
                continue
            bound = gmax / K if method == "mean" else gmax if method == "max" else gmax * (1.0 + 2.0 * float(np.abs(np.float32(beta))) * fmax)
            if bound == 0.0:
                continue
            if not bound < 3.4028234663852886e38:
                E[b, c] = POISON
                continue
            E[b, c] = 62 - log2_ceil(n_rays_samples) - np.frexp(bound)[1]
    return E


# ---- bounds: first order in EPS, counted from the code
def sample_error(mag):
    """the oracle shares the kernel's index and weight bits: only the 8-term fma chain is left"""
    return gamma(8) * mag


def bound_forward(s, mag, hit, method, beta=1.0, fw=None):
    """|maps - oracle| (B,V,C,Hm,Wm).  mean: the samples' errors, K - 1 adds and the division over sum |s_k|.  max: the largest sample
    error.  softmax: weight k is off by a factor 1 + theta with theta <= K (1 + 2 EXP_ULPS + 4 A) EPS, A = max |beta s| -- per step of the
    recurrence an fmul, an expf and an argument whose two z and whose difference are rounded (4 A EPS) -- so the weighted mean moves by
    2 theta sum p |s|; the sums add gamma(K + 2) of it; and a sample's own error enters through p_k (1 + |beta| |s_k - out|)"""
    K = s.shape[-1]
    es = sample_error(mag)
    if method == "mean":
        b = (es.sum(-1) + gamma(K) * np.abs(s).sum(-1)) / K * (1.0 + gamma(K))
    elif method == "max":
        b = es.max(-1)
    else:
        A = np.abs(beta * s).max(-1)
        theta = K * (1.0 + 2.0 * EXP_ULPS + 4.0 * A) * EPS
        p, out = fw["p"], fw["out"][..., None]
        b = (p * (1.0 + abs(beta) * np.abs(s - out)) * es).sum(-1) + (2.0 * theta + gamma(K + 2)) * (p * np.abs(s)).sum(-1)
    return np.where(hit[:, :, None], b, 0.0)


def ds_error(s, mag, hit, g, method, beta=1.0, fw=None, e_out=None):
    """(relative roundings r, absolute error) of ds_k before the tap's fmul.  mean: fdiv.  max: exact.  softmax: p_k = expf(z_k - lse) with
    lse off by e_lse = theta + gamma(K) + 2 EXP_ULPS EPS |ln S| + EPS |lse| + |beta| max e_s, z and the difference rounded (EPS (A + |z - lse|)),
    the expf, the sample's own error through beta; then two fmul, the fma and the fsub (4), and (s_k - out) off by e_s + e_out"""
    K = s.shape[-1]
    if method == "mean":
        return 1, np.zeros(s.shape)
    if method == "max":
        return 0, np.zeros(s.shape)
    es = sample_error(mag)
    g = np.abs(np.asarray(g, np.float64))[..., None]
    A = np.abs(beta * s).max(-1, keepdims=True)
    theta = K * (1.0 + 2.0 * EXP_ULPS + 4.0 * A) * EPS
    lse = fw["lse"][..., None]
    ln_s = np.abs(lse - (beta * s).max(-1, keepdims=True))
    e_lse = theta + gamma(K) + 2.0 * EXP_ULPS * EPS * ln_s + EPS * np.abs(lse) + abs(beta) * es.max(-1, keepdims=True)
    th_b = e_lse + abs(beta) * es + EPS * (A + np.abs(beta * s - lse)) + 2.0 * EXP_ULPS * EPS
    fac = np.abs(1.0 + beta * (s - fw["out"][..., None]))
    err = g * fw["p"] * ((th_b + gamma(4)) * fac + abs(beta) * (es + e_out[..., None]))
    return 0, np.where(hit[:, :, None, :, :, None], err, 0.0)


def bound_grad_volumes(tp, bw, hit, E, r, ds_err, store="float32"):
    """|grad_volumes - oracle| (B,C,Vox): per tap gamma(r + 1) |w ds| (ds's roundings and the fmul), w times ds's absolute error, and half a
    quantum 2^-E of the fixed point; then the conversion's rounding to fp32 and the storage type's"""
    u, floor = STORE[store]
    B, C, n_vox = bw["grad_v"].shape
    extra = np.zeros((B, C, n_vox))
    use = tp["use"] & hit[..., None, None]
    w = np.where(use, tp["w"].astype(np.float64), 0.0)
    for b in range(B):
        vox = tp["vox"][b].reshape(-1)
        for c in range(C):
            np.add.at(extra[b, c], vox, (w[b] * ds_err[b, :, c][..., None]).reshape(-1))
    quantum = np.where(E == POISON, 0.0, np.ldexp(1.0, -np.where(E == POISON, 0, E).astype(np.int64)))[:, :, None]
    inner = gamma(r + 1) * bw["mag_v"] + extra + 0.5 * quantum * bw["count"][:, None, :]
    return inner + (EPS + u) * (np.abs(bw["grad_v"]) + inner) + floor


# ---- rigs
def look_at(eye, target, focal, map_shape):
    """P (3,4) float64 of a pinhole at `eye` looking at `target` (up = world z), focal length in pixels, principal point the map's centre"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    Rc = np.stack([right, down, fwd])
    Hm, Wm = map_shape
    Kc = np.array([[focal, 0.0, (Wm - 1) / 2.0], [0.0, focal, (Hm - 1) / 2.0], [0.0, 0.0, 1.0]])
    return Kc @ np.concatenate([Rc, (-Rc @ eye)[:, None]], 1)


def rot_z(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def issue_rig():
    """the issue's rig: a 5x6x7 volume on a cuboid rotated 0.7 rad about z around the origin, a 6x9 map, K = 8, the camera at
    (3000, 500, 400) looking at the origin with focal length 6"""
    shape, map_shape = (5, 6, 7), (6, 9)
    rng = np.random.default_rng(3)
    sides = [2000.0, 2000.0, 2000.0]
    return {"shape": shape, "map_shape": map_shape, "K": 8, "sides": sides, "position": [-1000.0, -1000.0, -1000.0],
            "rot": rot_z(0.7)[None], "centers": np.zeros((1, 3)), "P": look_at([3000.0, 500.0, 400.0], [0.0, 0.0, 0.0], 6.0, map_shape)[None, None],
            "v": rng.normal(size=(1, 2, int(np.prod(shape)))), "g": rng.normal(size=(1, 1, 2) + map_shape)}


def general_problem(seed, B, C, V, shape, map_shape, focal=None):
    """generic rotations, a cuboid of about 2 m sides 3 to 13 m from the origin (volsample_oracle.general_problem), V cameras 2.5 to 4 m from its
    centre looking near it; the focal length chosen so that rays near the map's edge miss; fp32 inputs"""
    pr = vo.general_problem(seed, B, C, shape, 1)
    rng = np.random.default_rng(seed + 1000)
    Hm, Wm = map_shape
    focal = focal or 0.5 * max(Hm, Wm, 2)
    P = np.zeros((B, V, 3, 4))
    mid = vo.world_points(np.broadcast_to((np.asarray(shape) - 1) / 2.0, (B, 1, 3)), pr["rot"], pr["centers"], pr["position"], pr["sides"], shape)[:, 0]
    for b in range(B):
        for v in range(V):
            direction = rng.normal(size=3)
            direction /= np.linalg.norm(direction)
            P[b, v] = look_at(mid[b] + direction * rng.uniform(2500.0, 4000.0), mid[b] + rng.uniform(-200, 200, 3), focal, map_shape)
    pr["rays"] = camera_rays(P).astype(np.float32)
    pr["P"] = P
    pr["g"] = rng.normal(size=(B, V, C) + tuple(map_shape))
    return pr


def exact_rig(seed, B, C, V, shape, map_shape, K):
    """Every fp32 operation of the contract is exact here (K a power of two): step = 1/2, position and centers multiples of 1/8, rotations signed
    permutations, the camera of view v four voxels in front of face v % 3 of the index box with t_o a multiple of 1/2, and index-space
    directions e = (1, (u - u0) / 4, (v - v0) / 4) (permuted) with u0, v0 the map's centre pixel -- so for maps up to 5 x 5 every e_a is 0 or
    a power of two and every slab division is exact; volume values and grad_maps small integers (grad_maps multiples of K, so g / K is one)."""
    assert K & (K - 1) == 0 and max(map_shape) <= 5
    rng = np.random.default_rng(seed)
    step = 0.5
    sides = [step * (s - 1) for s in shape]
    position = (rng.integers(-64, 64, 3) / 8.0).tolist()
    centers = rng.integers(-256, 256, (B, 3)) / 8.0
    rot = np.stack([vo.SIGNED_PERMUTATIONS[(seed + b) % len(vo.SIGNED_PERMUTATIONS)] for b in range(B)])
    Hm, Wm = map_shape
    u0, v0 = (Wm - 1) // 2, (Hm - 1) // 2
    rays, to_all, E_all = np.zeros((B, V, 3, 4)), np.zeros((B, V, 3)), np.zeros((B, V, 3, 3))
    for v in range(V):
        a = v % 3
        others = [x for x in range(3) if x != a]
        sign = 1.0 if v % 2 == 0 else -1.0
        to = np.array([np.floor((s - 1) / 2.0) + 0.5 if s > 2 else 0.5 for s in shape])
        to[a] = -4.0 if sign > 0 else shape[a] - 1 + 4.0
        E0 = np.zeros((3, 3))                                                    # e = E0 (u, v, 1)
        E0[a] = [0.0, 0.0, sign]
        E0[others[0]] = [0.25, 0.0, -0.25 * u0]
        E0[others[1]] = [0.0, 0.25, -0.25 * v0]
        to_all[:, v], E_all[:, v] = to, E0
        for b in range(B):
            rays[b, v, :, :3] = rot[b] @ (step * E0)
            rays[b, v, :, 3] = vo.world_points(to[None, None], rot[b:b + 1], centers[b:b + 1], position, sides, shape)[0, 0]
    v = rng.integers(-2, 3, (B, C, int(np.prod(shape)))).astype(np.float64)
    g = (rng.integers(-1, 2, (B, V, C) + tuple(map_shape)) * K).astype(np.float64)
    return {"position": position, "sides": sides, "centers": centers, "rot": rot, "rays": rays, "v": v, "g": g, "to": to_all, "E0": E_all, "step": step}


def full(pr, shape, map_shape, K, method, beta=1.0, ranges=None, min_depth=0.0, max_depth=np.inf, g=None, store="float32"):
    """the whole oracle on a problem dict: the fp32 geometry (its ranges, or the kernel's own), fp32 sample indices and weights, float64
    samples, maps and gradient, with every bound"""
    geo = ray_geometry(pr["rays"], pr["rot"], pr["centers"], pr["position"], pr["sides"], shape, map_shape, min_depth, max_depth)
    own = np.stack([geo["lin"], geo["lout"]], -1)
    ranges = own if ranges is None else np.asarray(ranges, np.float32)
    hit = ranges[..., 0] < ranges[..., 1]
    tp = taps(sample_indices(geo, ranges, K), shape)
    s, mag = samples(pr["v"], tp)
    res = {"geo": geo, "ranges": own, "hit": hit, "tp": tp, "s": s, "mag": mag}
    arg = None
    if method == "max":
        s32, _ = samples(pr["v"], tp, np.float32)
        res["maps32"], arg = reduce_fp32(s32, hit, "max", K)
    elif method == "mean":
        s32, _ = samples(pr["v"], tp, np.float32)
        res["maps32"], _ = reduce_fp32(s32, hit, "mean", K)
    fw = forward(s, hit, method, beta)
    res.update(fw=fw, out=fw["out"], arg=arg, e_out=bound_forward(s, mag, hit, method, beta, fw))
    g = pr["g"] if g is None else g
    if g is not None:
        n_vox = int(np.prod(shape))
        bw = backward(tp, s, hit, g, method, n_vox, beta, arg, fw)
        E = exponents(g, pr["v"], method, K, pr["rays"].shape[1] * map_shape[0] * map_shape[1] * K, beta)
        r, ds_err = ds_error(s, mag, hit, g, method, beta, fw, res["e_out"])
        res.update(bw=bw, E=E, grad_v=bw["grad_v"], e_grad=bound_grad_volumes(tp, bw, hit, E, r, ds_err, store))
    return res
