"""float64 oracle of the volumetric soft-argmax, a numpy restatement of the kernels' fp32 reduction order, the error
bounds the tests hold both to, and the exact rig.  numpy only: the CPU tests import it without a device.

Shapes: v (B, J, N) volume values as floats (whatever the storage dtype held), u (B, N, 3) accumulation-frame coordinates (the caller's
coord_volumes on the tensor route, cuboid_offsets() on the cuboid route), g (B, J, 3) = d/d keypoint, gl (B, J) = d/d logsumexp.
"""
import math

import numpy as np

LOG2E = 1.4426950408889634
EPS = 2.0 ** -24          # unit roundoff of fp32
EPS_EXP = 2.0 * 2.0 ** -23  # exp2: the instruction's documented 1 ulp, doubled (the one constant that does not come from the code)
TINY = 2.0 ** -126        # fp32's smallest normal: the exp2 instruction flushes a smaller weight to zero (an absolute error of the weight, before
#                           normalisation by D >= 1 in the forward, after it in the backward)
THREADS, WAVE = 256, 64


# ---- sizes: Python mirrors of sa3d_splits and of the vector width the launcher picks (16-byte vectors, else scalar)
def splits(batch, joints, voxels):
    tiles = batch * (joints // 4 + ((joints & 2) >> 1) + (joints & 1))
    if tiles >= 2048:
        return 1
    return max(1, min(-(-2048 // tiles), voxels // 2048))


def vector_width(voxels, itemsize):
    vec = 16 // itemsize
    return vec if voxels % vec == 0 else 1


# ---- coordinates
def cuboid_offsets(position, sides, shape, centers, dtype=np.float32):
    """d[b, n] = (position + step * index) - center[b], n = (i*Y + j)*Z + k.  float32: cuboid_offset's roundings (step = fl32(sides / (S-1))
    from float64, fl32 product, fl32 sum, fl32 difference) -- the contract; float64: the unrounded recipe, for finite differences."""
    X, Y, Z = shape
    f = dtype
    step = [f(float(sides[a]) / (shape[a] - 1)) if shape[a] > 1 else f(0) for a in range(3)]
    axes = [f(position[a]) + step[a] * np.arange(shape[a]).astype(f) for a in range(3)]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(1, X * Y * Z, 3).astype(f)
    return (grid - np.asarray(centers).astype(f)[:, None, :]).astype(f)


def world_coords(offsets, rot, centers):
    """float64 world points R d + c of the offsets: what the tensor route is handed when both routes are compared"""
    return np.einsum("brc,bnc->bnr", np.asarray(rot, np.float64), np.asarray(offsets, np.float64)) + np.asarray(centers, np.float64)[:, None, :]


# ---- the float64 oracle
def forward(v, u, beta, rot=None, centers=None):
    """-> dict(p (B,J,N), L (B,J), mu (B,J,3), kp (B,J,3)).  A slice with NaN, +inf or nothing but -inf is NaN throughout."""
    v, u = np.asarray(v, np.float64), np.asarray(u, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = beta * v
        m = t.max(-1, keepdims=True)
        bad = np.isnan(t).any(-1, keepdims=True) | ~np.isfinite(m)
        e = np.exp(t - np.where(bad, 0.0, m))
        D = e.sum(-1, keepdims=True)
        p = np.where(bad, np.nan, e / D)
        L = np.where(bad, np.nan, m + np.log(D))[..., 0]
        mu = np.einsum("bjn,bnc->bjc", np.where(bad, 0.0, p), u)
        mu = np.where(bad, np.nan, mu)
    kp = mu if rot is None else np.einsum("brc,bjc->bjr", np.asarray(rot, np.float64), mu) + np.asarray(centers, np.float64)[:, None, :]
    return {"p": p, "L": L, "mu": mu, "kp": kp}


def backward(v, u, beta, g=None, gl=None, rot=None):
    """-> dict(grad_v (B,J,N), grad_coords (B,N,3), grad_rot (B,3,3), grad_center (B,3)); the last two only with rot"""
    f = forward(v, u, beta)
    B, J, N = f["p"].shape
    g = np.zeros((B, J, 3)) if g is None else np.asarray(g, np.float64)
    gl = np.zeros((B, J)) if gl is None else np.asarray(gl, np.float64)
    h = g if rot is None else np.einsum("brc,bjr->bjc", np.asarray(rot, np.float64), g)          # R^T g
    dev = np.asarray(u, np.float64)[:, None, :, :] - f["mu"][:, :, None, :]
    out = {"grad_v": beta * f["p"] * (np.einsum("bjc,bjnc->bjn", h, dev) + gl[..., None]),
           "grad_coords": np.einsum("bjn,bjc->bnc", f["p"], g), "h": h}
    if rot is not None:
        out["grad_rot"] = np.einsum("bjr,bjc->brc", g, f["mu"])
        out["grad_center"] = (g - h).sum(1)
    return out


# ---- the kernels' reduction order in fp32 (soft_argmax3d.hip's header comment, operation for operation; exp2 is numpy's, not the card's)
def _f32(x):
    return np.asarray(x, np.float32)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)     # (double rounding: rare, not on the exact rig)


def _safe(m):
    return np.where(np.isneginf(m), np.float32(0), m)


def _merge(A, B):
    """records as (m, D, a): arrays (...,), (...,), (..., 3)"""
    m = np.fmax(A[0], B[0])
    ms = _safe(m)
    sA, sB = np.exp2(A[0] - ms), np.exp2(B[0] - ms)
    return m, A[1] * sA + B[1] * sB, A[2] * sA[..., None] + B[2] * sB[..., None]


def _butterfly(rec):
    """xor butterflies 1..32 inside every wave of 64 along the leading axis"""
    lanes = np.arange(rec[0].shape[0])
    for off in (1, 2, 4, 8, 16, 32):
        rec = _merge(rec, tuple(x[lanes ^ off] for x in rec))
    return rec


def _identity(n):
    return _f32(np.full(n, -np.inf)), _f32(np.zeros(n)), _f32(np.zeros((n, 3)))


def _block(t, u, first, last, vec):
    """one block: chunks [first, last) of one slice; t (N,) fp32 scaled values, u (N, 3) fp32 -> its record"""
    m, D, a = _identity(THREADS)
    for base in range(first, last, THREADS):
        c = base + np.arange(THREADS)
        live = c < last
        idx = np.where(live, c, first)[:, None] * vec + np.arange(vec)
        tc = t[idx]
        tm = _f32(np.full(THREADS, -np.inf))
        for e in range(vec):
            tm = np.fmax(tm, tc[:, e])
        mn = np.fmax(m, tm)
        ms = _safe(mn)
        sc = np.exp2(m - ms)
        Dn, an = D * sc, a * sc[:, None]
        for e in range(vec):
            p = np.exp2(tc[:, e] - ms)
            Dn = Dn + p
            an = _fma(p[:, None], u[idx[:, e]], an)
        m, D, a = np.where(live, mn, m), np.where(live, Dn, D), np.where(live[:, None], an, a)
    m, D, a = _butterfly((m, D, a))
    rec = (m[0], D[0], a[0])
    for w in range(1, THREADS // WAVE):
        rec = _merge(rec, (m[w * WAVE], D[w * WAVE], a[w * WAVE]))
    return rec


def emulate_fp32(v, u, beta, itemsize=4, rot=None, centers=None):
    """The kernels' mu, L and keypoints as fp32 arrays, by their documented order.  v (B,J,N): the stored values; u (B,N,3) fp32."""
    v, u = _f32(v), _f32(u)
    B, J, N = v.shape
    vec, S = vector_width(N, itemsize), splits(B, J, N)
    C = N // vec
    Cs = -(-C // S)
    c2 = np.float32(beta * LOG2E)
    mu, L = np.empty((B, J, 3), np.float32), np.empty((B, J), np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for b in range(B):
            for j in range(J):
                t = c2 * v[b, j]
                recs = [_block(t, u[b], s * Cs, min(s * Cs + Cs, C), vec) for s in range(S)]
                m, D, a = _identity(WAVE)
                for s0 in range(0, S, WAVE):                               # lane l merges records l, l + 64, ... in order
                    part = recs[s0:s0 + WAVE]
                    k = len(part)
                    other = tuple(np.concatenate([_f32(np.stack([r[i] for r in part])), x[k:]]) for i, x in enumerate(_identity(WAVE)))
                    m, D, a = _merge((m, D, a), other)
                m, D, a = (x[0] for x in _butterfly((m, D, a)))
                if D == 0:
                    mu[b, j], L[b, j] = np.nan, np.nan
                else:
                    mu[b, j] = a / D
                    L[b, j] = (m + np.log2(D)) * np.float32(math.log(2.0))
    kp = mu
    if rot is not None:
        R, c = _f32(rot), _f32(centers)
        kp = np.empty_like(mu)
        for r in range(3):
            acc = R[:, None, r, 0] * mu[..., 0]
            acc = _fma(R[:, None, r, 1], mu[..., 1], acc)
            acc = _fma(R[:, None, r, 2], mu[..., 2], acc)
            kp[..., r] = acc + c[:, None, r]
    return {"mu": mu, "L": L, "kp": kp}


# ---- the bounds (derivation: DESIGN.md 5.17).  All first order in 2^-24, per component, from float64 oracle quantities.
def counts(batch, joints, voxels, itemsize):
    """(cnt, n_exp): roundings on the longest path of one term into a / D, and exp2 evaluations that scale it"""
    vec, S = vector_width(voxels, itemsize), splits(batch, joints, voxels)
    chunks = -(-(-(-(voxels // vec) // S)) // THREADS)                 # chunks one lane walks
    depth = 6 + 3 + (-(-S // WAVE)) + 6                                # lane butterfly, waves, strided records, record butterfly
    return chunks * vec + chunks + 3 * depth, 1 + chunks + depth


def eps_p(beta, v, batch, joints, voxels, itemsize):
    """relative error of one softmax weight before normalisation, summed over the exp2 evaluations that touch it: the instruction's
    error plus the argument's (two roundings in fl(c2 v), one in the difference: 2^-22 max|t| in log2 units, times ln 2)"""
    finite = np.abs(np.asarray(v, np.float64)[np.isfinite(v)])
    vmax = float(finite.max()) if finite.size else 0.0
    return counts(batch, joints, voxels, itemsize)[1] * (EPS_EXP + 2.0 ** -22 * abs(beta) * vmax)


def moment_bound(v, u, beta, itemsize=4):
    """(B, J, 3) bound on |mu - oracle|: summation + (argument rounding + exp2)"""
    f = forward(v, u, beta)
    B, J, N = f["p"].shape
    cnt, _ = counts(B, J, N, itemsize)
    u = np.asarray(u, np.float64)
    pu = np.einsum("bjn,bnc->bjc", f["p"], np.abs(u))
    pdev = np.einsum("bjn,bjnc->bjc", f["p"], np.abs(u[:, None] - f["mu"][:, :, None, :]))
    flushed = N * TINY * np.abs(u[:, None] - f["mu"][:, :, None, :]).max(2)
    return 2 * (cnt + 2) * EPS * pu + eps_p(beta, v, B, J, N, itemsize) * pdev + flushed


def keypoint_bound(v, u, beta, rot, centers, itemsize=4):
    """the moment bound through |R|, plus the affine map's four roundings"""
    f = forward(v, u, beta, rot, centers)
    R = np.abs(np.asarray(rot, np.float64))
    mb = moment_bound(v, u, beta, itemsize)
    return np.einsum("brc,bjc->bjr", R, mb) + 4 * EPS * (np.einsum("brc,bjc->bjr", R, np.abs(f["mu"])) + np.abs(f["kp"]))


def lse_bound(v, u, beta, itemsize=4):
    """(B, J): the relative error of D (summation and weights), the roundings of (m + log2 D) ln 2, log2's own 2 ulp"""
    f = forward(v, u, beta)
    B, J, N = f["p"].shape
    cnt, _ = counts(B, J, N, itemsize)
    return cnt * EPS + eps_p(beta, v, B, J, N, itemsize) + 6 * EPS * np.abs(f["L"]) + 2.0 ** -21 + N * TINY


def grad_bounds(v, u, beta, g=None, gl=None, rot=None, itemsize=4, store_eps=0.0):
    """bounds on the four gradients, as dict like backward()'s.  store_eps: the relative rounding of grad_volumes' storage dtype"""
    f = forward(v, u, beta)
    bw = backward(v, u, beta, g, gl, rot)
    B, J, N = f["p"].shape
    g = np.zeros((B, J, 3)) if g is None else np.asarray(g, np.float64)
    gl = np.zeros((B, J)) if gl is None else np.asarray(gl, np.float64)
    h, u = np.abs(bw["h"]), np.asarray(u, np.float64)
    mb, lb = moment_bound(v, u, beta, itemsize), lse_bound(v, u, beta, itemsize)
    # p = exp2(fl(c2 v) - fl(L log2e)): the weight's own error, L's, and the two roundings of L log2e
    ep = (eps_p(beta, v, B, J, N, itemsize) + lb + 4 * EPS * np.abs(f["L"]))[..., None]
    dev = np.abs(u[:, None] - f["mu"][:, :, None, :])
    inner = np.abs(np.einsum("bjc,bjnc->bjn", bw["h"], u[:, None] - f["mu"][:, :, None, :]) + gl[..., None])
    hdev = np.einsum("bjc,bjnc->bjn", h, dev) + np.abs(gl)[..., None]
    hmu = np.einsum("bjc,bjc->bj", h, mb)[..., None] + 2 * EPS * np.einsum("bjc,bjnc->bjn", h, np.abs(u[:, None]) + np.abs(f["mu"][:, :, None, :]))
    gv = abs(beta) * ((f["p"] * (ep + 4 * EPS) + TINY) * inner + f["p"] * (hmu + 6 * EPS * hdev))
    gv = gv + store_eps * np.abs(bw["grad_v"])
    out = {"grad_v": gv, "grad_coords": np.einsum("bjn,bjc->bnc", f["p"] * (ep + (J + 1) * EPS) + TINY, np.abs(g))}
    if rot is not None:
        out["grad_rot"] = np.einsum("bjr,bjc->brc", np.abs(g), mb + (J + 1) * EPS * np.abs(f["mu"]))
        out["grad_center"] = (J + 5) * EPS * (np.abs(g) + np.einsum("brc,bjr->bjc", np.abs(np.asarray(rot, np.float64)), np.abs(g))).sum(1)
    return out


# ---- the exact rig: every fp32 operation of the kernels is exact on it, so they must equal the float64 oracle cast once to fp32
def signed_permutations(rng, batch):
    R = np.zeros((batch, 3, 3), np.float32)
    for b in range(batch):
        R[b, np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
    return R


def exact_rig(seed, batch, joints, shape, on=16, level=0.0, off=-1e30):
    """volumes in {level, off} with K = `on` (a power of two <= 256, <= N) voxels at `level` per slice; dyadic geometry (multiples of 2^-3
    below 2^12); rotations signed permutations; g, gl dyadic.  With beta > 0: exp2 is exactly 1 or 0 and every partial sum is exact."""
    rng = np.random.RandomState(seed)
    X, Y, Z = shape
    N = X * Y * Z
    K = min(on, 1 << int(math.log2(N)))
    v = np.full((batch, joints, N), off, np.float32)
    for b in range(batch):
        for j in range(joints):
            v[b, j, rng.choice(N, K, replace=False)] = level
    dy = lambda *s: (rng.randint(-2 ** 10, 2 ** 10, size=s) / 8.0)                       # noqa: E731  multiples of 2^-3, |x| < 2^7
    step = rng.randint(1, 33, size=3) / 8.0
    rig = {"v": v, "K": K, "shape": shape, "position": dy(3), "sides": step * (np.array(shape) - 1), "centers": dy(batch, 3).astype(np.float32),
           "rot": signed_permutations(rng, batch), "coords": dy(batch, N, 3).astype(np.float32),
           "g": (rng.randint(-8, 9, size=(batch, joints, 3)) / 4.0).astype(np.float32),
           "gl": (rng.randint(-8, 9, size=(batch, joints)) / 4.0).astype(np.float32)}
    rig["offsets"] = cuboid_offsets(rig["position"], rig["sides"], shape, rig["centers"])
    return rig
