"""Oracle of the trilinear volume sampling at world points: the contract's fp32 index and weights restated in numpy,
operation for operation; everything downstream of them in float64; a numpy emulation of the volume gradient's (voxel, point) order and
chunking; the error bounds the GPU tests hold the kernels to; and the exact rig.  numpy only: the CPU tests import it without a device.

Shapes: v (B, C, V) volume values as float64 (whatever the storage type held), V = X*Y*Z, flat voxel (i*Y + j)*Z + k; points (B, N, 3);
t (B, N, 3) fp32, the continuous voxel index; g = d/d samples, (B, C, N) or, paired, (B, C) with N == C.
"""
import numpy as np

EPS = 2.0 ** -24            # unit roundoff of fp32
CHUNK = 256                 # mvhmr_sample_volume_chunk_points(): the tests hold the library to this value
GROUP, UNROLL = 32, 4       # channels per block and per loop trip of the forward (volume_sample.hip: kVsGroup, kVsUnroll)
# unit roundoff of a storage type and the absolute floor of its subnormals, by the name of the torch dtype
STORE = {"float32": (0.0, 0.0), "float16": (2.0 ** -11, 2.0 ** -25), "bfloat16": (2.0 ** -8, 0.0)}
TAPS = np.array([[k >> 2, (k >> 1) & 1, k & 1] for k in range(8)])


def f32(x):
    return np.asarray(x, np.float32)


def fma32(a, b, c):
    """fp32 fma(a, b, c), correctly rounded: a * b is exact in float64, the sum is rounded to odd there (its exact TwoSum error picks the odd
    neighbour) and rounds once more to fp32 (Boldo & Melquiond 2008) -- the plain float64 sum can double-round"""
    p, c = f32(a).astype(np.float64) * f32(b).astype(np.float64), f32(c).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bp = s - p
        e = (p - (s - bp)) + (c - bp)
        odd = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(odd, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def steps(sides, shape, dtype=np.float32):
    """step_a = fl32(sides_a / (S_a - 1)), the quotient in float64 as coords_from_cuboid takes it"""
    return np.array([dtype(float(sides[a]) / (shape[a] - 1)) for a in range(3)], dtype)


# ---- the contract in fp32
def index_fp32(points, rot, centers, position, sides, shape):
    """t (B, N, 3) fp32: y = x - c; d_a = fma(R[2][a], y2, fma(R[1][a], y1, R[0][a] * y0)); t_a = ((d_a + (c_a - p_a)) / step_a)"""
    x, R, c = f32(points), f32(rot), f32(centers)[:, None, :]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        y = x - c
        d = np.stack([fma32(R[:, None, 2, a], y[..., 2], fma32(R[:, None, 1, a], y[..., 1], R[:, None, 0, a] * y[..., 0])) for a in range(3)], -1)
        o = c - f32(position)
        return ((d + o) / steps(sides, shape)).astype(np.float32)


def taps(t, shape):
    """dict: live (B,N) -- -1 < t < S on every axis; wa (B,N,3,2) fp32 per-axis weights (w0, w1); w (B,N,8) fp32 tap weights in the order
    dx*4 + dy*2 + dz; inside (B,N,8) the tap lies in the grid; vox (B,N,8) its flat voxel (0 where outside).  A dead point has no tap inside."""
    t = f32(t)
    S = np.asarray(shape)
    with np.errstate(invalid="ignore"):
        live = ((t > -1) & (t < S.astype(np.float32))).all(-1)
    ts = np.where(live[..., None], t, np.float32(0))
    fl = np.floor(ts)
    w1 = ts - fl
    w0 = (fl + np.float32(1)) - ts
    wa = np.stack([w0, w1], -1).astype(np.float32)
    i0 = fl.astype(np.int64)
    idx = i0[..., None, :] + TAPS                                                   # (B,N,8,3)
    inside = ((idx >= 0) & (idx < S)).all(-1) & live[..., None]
    w = ((wa[..., 0, :][..., TAPS[:, 0]] * wa[..., 1, :][..., TAPS[:, 1]]).astype(np.float32) * wa[..., 2, :][..., TAPS[:, 2]]).astype(np.float32)
    vox = np.where(inside, (idx[..., 0] * shape[1] + idx[..., 1]) * shape[2] + idx[..., 2], 0)
    return {"live": live, "wa": wa, "w": w, "inside": inside, "vox": vox}


# ---- float64 downstream of the fp32 index and weights
def _gather(v, vox, paired):
    """tap values (B,C,N,8), or paired (B,N,8): channel n at point n"""
    B, C, V = v.shape
    if paired:
        return np.take_along_axis(v, vox.reshape(B, C, 8), 2)
    return np.take_along_axis(v[:, :, None, :], np.broadcast_to(vox[:, None], (B, C) + vox.shape[1:]), 3)


def forward(v, t, shape, paired=False):
    """-> samples (B,C,N) / (B,C) float64 and mag = sum |w v| over the taps that count (for the bound).  A tap counts when it lies inside
    the grid and its weight is not exactly zero: then, and only then, its value is read (a -inf beside a node stays out)."""
    tp = taps(t, shape)
    use = tp["inside"] & (tp["w"] != 0)
    vals = _gather(np.asarray(v, np.float64), tp["vox"], paired)
    w, use = (tp["w"].astype(np.float64), use) if paired else (tp["w"].astype(np.float64)[:, None], use[:, None])
    with np.errstate(invalid="ignore"):
        terms = np.where(use, w * np.where(use, vals, 0.0), 0.0)
    return terms.sum(-1), np.abs(terms).sum(-1)


def backward(v, t, points, rot, centers, sides, shape, g, paired=False):
    """-> dict of float64: grad_v (B,C,V); q, u (B,N,3); grad_points (B,N,3); grad_rot (B,3,3); grad_center (B,3); and the magnitudes the bounds need.
    q follows grid_sample: taps outside the grid count as value 0 (zero-weight taps inside it are read), the cell is floor(t)."""
    v, g = np.asarray(v, np.float64), np.asarray(g, np.float64)
    B, C, V = v.shape
    tp = taps(t, shape)
    N = tp["live"].shape[1]
    gn = g[:, :, None] if paired else g                                            # paired: (B,N,1) against taps (B,N,8)
    # volume gradient
    use = tp["inside"] & (tp["w"] != 0)
    w64 = np.where(use, tp["w"].astype(np.float64), 0.0)
    grad_v, mag_v, count = np.zeros((B, C, V)), np.zeros((B, C, V)), np.zeros((B, V), np.int64)
    for b in range(B):
        for n in range(N):
            for k in np.nonzero(use[b, n])[0]:
                if paired:
                    grad_v[b, n, tp["vox"][b, n, k]] += w64[b, n, k] * g[b, n]
                    mag_v[b, n, tp["vox"][b, n, k]] += abs(w64[b, n, k] * g[b, n])
                else:
                    grad_v[b, :, tp["vox"][b, n, k]] += w64[b, n, k] * g[b, :, n]
                    mag_v[b, :, tp["vox"][b, n, k]] += np.abs(w64[b, n, k] * g[b, :, n])
                count[b, tp["vox"][b, n, k]] += 1
    # dL/dt
    vals = np.where(tp["inside"] if paired else tp["inside"][:, None], _gather(v, tp["vox"], paired), 0.0)        # (B,[C,]N,8)
    wa = tp["wa"].astype(np.float64)
    q, mag_q = np.zeros((B, N, 3)), np.zeros((B, N, 3))
    for a in range(3):
        others = [x for x in range(3) if x != a]
        s, m = 0.0, 0.0
        for k in range(8):
            d = TAPS[k]
            pair = wa[:, :, others[0], d[others[0]]] * wa[:, :, others[1], d[others[1]]]
            pair = pair if paired else pair[:, None]
            s = s + (1.0 if d[a] else -1.0) * pair * vals[..., k]
            m = m + pair * np.abs(vals[..., k])
        if paired:
            q[..., a], mag_q[..., a] = g * s, np.abs(g) * m
        else:
            q[..., a], mag_q[..., a] = (g * s).sum(1), (np.abs(g) * m).sum(1)
    live = tp["live"][..., None]
    q, mag_q = np.where(live, q, 0.0), np.where(live, mag_q, 0.0)
    st = steps(sides, shape).astype(np.float64)
    u = q / st
    R, c = np.asarray(rot, np.float64), np.asarray(centers, np.float64)
    y = np.where(live, np.asarray(f32(points), np.float64) - c[:, None, :], 0.0)
    Ru = np.einsum("bia,bna->bni", R, u)
    return {"grad_v": grad_v, "mag_v": mag_v, "count": count, "q": q, "mag_q": mag_q, "u": u, "y": y, "live": tp["live"], "grad_points": Ru,
            "grad_rot": np.einsum("bni,bna->bia", y, u), "grad_center": (u - Ru).sum(1)}


# ---- the volume gradient's order and chunking in fp32 (volume_sample.hip's header, operation for operation)
def emulate_grad_volumes(t, g, shape, channels, paired=False, chunk=CHUNK, store=np.float32):
    """per chunk of `chunk` points: the live taps in ascending (voxel, point), per (voxel, channel) acc = fmul(w, g) then fma(w, g, acc), the
    owner stores store(fadd(stored, acc)).  `store` rounds an fp32 array to the storage type and back (identity for fp32)."""
    tp = taps(t, shape)
    B, N = tp["live"].shape
    V = int(np.prod(shape))
    g = f32(g)
    out = np.zeros((B, channels, V), np.float32)
    use = tp["inside"] & (tp["w"] != 0)
    for b in range(B):
        if paired:
            for n in range(N):
                for k in np.nonzero(use[b, n])[0]:
                    out[b, n, tp["vox"][b, n, k]] = store(f32(0) + tp["w"][b, n, k] * g[b, n])
            continue
        for first in range(0, N, chunk):
            entries = sorted((int(tp["vox"][b, n, k]), n, k) for n in range(first, min(first + chunk, N)) for k in np.nonzero(use[b, n])[0])
            i = 0
            while i < len(entries):
                vox, n, k = entries[i]
                acc = tp["w"][b, n, k] * g[b, :, n]
                i += 1
                while i < len(entries) and entries[i][0] == vox:
                    _, n, k = entries[i]
                    acc = fma32(np.broadcast_to(tp["w"][b, n, k], acc.shape), g[b, :, n], acc)
                    i += 1
                out[b, :, vox] = store((out[b, :, vox] + acc).astype(np.float32))
    return out


# ---- bounds: first order in EPS by counting the roundings of the code, written as gamma_k = k EPS / (1 - k EPS)
def gamma(k):
    k = np.asarray(k, np.float64)
    return k * EPS / (1.0 - k * EPS)


def bound_forward(mag):
    """the oracle shares the kernel's weight bits, so only the chain is left: every term passes through at most 8 fma roundings"""
    return gamma(8) * mag


def bound_grad_volumes(mag_v, count, n_points, store="float32", chunk=CHUNK):
    """a voxel with m contributions in K <= min(m, chunks) chunks: every term passes through at most m chain roundings and K adds to the
    stored value; a 16-bit grad_volumes also rounds the running value (<= sum |w g|) once per chunk that touches the voxel"""
    u, floor = STORE[store]
    m = count[:, None, :].astype(np.float64)
    K = np.minimum(m, -(-n_points // chunk))
    return (gamma(m + K) + K * u * (1.0 + gamma(m + K))) * mag_v + K * floor


def bound_u(bw, sides, shape, channels):
    """per term: fsub(v_hi, v_lo) (1, relative to |v_hi| + |v_lo|), the pair weight's fmul (1), the 4-term chain (4), the fma over the
    channels (C), the division by step (1)"""
    return gamma(7 + channels) * bw["mag_q"] / np.abs(steps(sides, shape).astype(np.float64))


def bound_geometry(bw, rot, sides, shape, channels):
    """-> bounds of grad_points, grad_rot, grad_center from bound_u: R u is a 3-term chain; grad_rot rounds y once and chains the live
    points; grad_center rounds (R u)_a, the difference, and the running sum over the live points"""
    eu = bound_u(bw, sides, shape, channels)
    aR, au, ay = np.abs(np.asarray(rot, np.float64)), np.abs(bw["u"]), np.abs(bw["y"])
    e_Ru = np.einsum("bia,bna->bni", aR, eu) + gamma(3) * np.einsum("bia,bna->bni", aR, au)
    n_live = bw["live"].sum(1).astype(np.float64)
    e_rot = np.einsum("bni,bna->bia", ay, eu) + gamma(n_live + 1)[:, None, None] * np.einsum("bni,bna->bia", ay, au)
    diff = np.abs(bw["u"] - bw["grad_points"])
    e_cen = (eu + e_Ru).sum(1) + gamma(n_live + 1)[:, None] * diff.sum(1)
    return e_Ru, e_rot, e_cen


def bound_roundtrip_index(coords, centers, position, sides, shape):
    """(B, N, 3) bound on |t - (i, j, k)| when the points are mvhmr_build_coord_volumes' own fp32 coordinates.  Roundings, each relative to
    M = the largest magnitude of a sample (coordinates, centre, corner) plus the cuboid's extent: the grid point (2), the offset (1), R d + c
    (3 + 1, seen through |R^T|: a factor sqrt 3), the sample's y, R^T y, o, sum and quotient (1 + 3 + 1 + 1 + 1), R^T R - I for an fp32 R
    (3): 20 in all, divided by the step"""
    B = coords.shape[0]
    M = np.array([max(np.abs(coords[b]).max(), np.abs(centers[b]).max(), np.abs(np.asarray(position)).max()) + float(np.sum(sides)) for b in range(B)])
    dt = 20.0 * EPS * M[:, None, None] / np.abs(steps(sides, shape).astype(np.float64))
    return np.broadcast_to(dt, (B, int(np.prod(shape)), 3))


# ---- inputs
SIGNED_PERMUTATIONS = [np.array(m, np.float64) for m in (
    [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[0, 0, 1], [1, 0, 0], [0, 1, 0]], [[-1, 0, 0], [0, 0, 1], [0, 1, 0]])]


def point_indices(rng, shape, n, fractions=None):
    """n continuous voxel indices (n, 3) that cover, in one tensor, the issue's point sets as far as n allows: index 0 first (the caller
    duplicates it), 40 identical points, exact nodes, t = S - 1, half-in cells on both sides, t <= -1 and t >= S, a NaN point, the rest interior.
    fractions: None = any fraction, else the denominator the fractional parts are multiples of (the exact rig: 4)."""
    S = np.asarray(shape, np.float64)

    def frac(size):
        return rng.random(size) if fractions is None else rng.integers(0, fractions, size) / fractions

    def interior(m):
        return rng.integers(0, np.maximum(S - 1, 1).astype(np.int64), (m, 3)) + frac((m, 3))

    rows = [interior(1)]
    if n >= 60:
        rows.append(np.repeat(interior(1), 40, 0))
    if n >= 12:
        rows += [rng.integers(0, S.astype(np.int64), (2, 3)).astype(np.float64),                                # nodes: f = 0
                 np.stack([S - 1, np.array([S[0] - 1, 0.5, 0.25])]),                            # t = S - 1 exactly
                 np.array([[-0.5, 0.5, 0.25], [0.25, -0.75, -0.25]]) + 0.0,                     # -1 < t < 0
                 np.stack([S - 0.5, np.array([0.5, S[1] - 0.25, 0.75])]),                       # S - 1 < t < S
                 np.array([[-1.0, 0.5, 0.5], [0.5, 0.5, -2.25]]),                               # t <= -1
                 np.stack([np.array([0.5, S[1], 0.5]), S + 1.5]),                               # t >= S
                 np.full((1, 3), np.nan)]                                                       # a NaN point
    have = sum(len(r) for r in rows)
    assert have <= n, (have, n)
    rows.append(interior(n - have))
    return np.concatenate(rows)[:n]


def world_points(tt, rot, centers, position, sides, shape):
    """float64 world points R (position + step * t - c) + c of indices tt (B, N, 3)"""
    grid = np.asarray(position, np.float64) + steps(sides, shape).astype(np.float64) * tt
    c = np.asarray(centers, np.float64)[:, None, :]
    return np.einsum("bia,bna->bni", np.asarray(rot, np.float64), grid - c) + c


def exact_rig(seed, B, C, shape, N, paired=False, duplicate=None):
    """Every fp32 operation of the contract is exact here: step = 1/2, position and centers multiples of 1/8, rotations signed permutations,
    fractional parts multiples of 1/4, volume values and grad_samples small integers.  duplicate = (src, dst): point dst repeats point src."""
    rng = np.random.default_rng(seed)
    step = 0.5
    sides = [step * (s - 1) for s in shape]
    position = (rng.integers(-64, 64, 3) / 8.0).tolist()
    centers = rng.integers(-256, 256, (B, 3)) / 8.0
    rot = np.stack([SIGNED_PERMUTATIONS[(seed + b) % len(SIGNED_PERMUTATIONS)] for b in range(B)])
    tt = np.stack([point_indices(rng, shape, N, fractions=4) for _ in range(B)])
    if duplicate:
        tt[:, duplicate[1]] = tt[:, duplicate[0]]
    points = world_points(tt, rot, centers, position, sides, shape)
    v = rng.integers(-2, 3, (B, C, int(np.prod(shape)))).astype(np.float64)
    g = rng.integers(-1, 2, (B, C) if paired else (B, C, N)).astype(np.float64)
    return {"position": position, "sides": sides, "centers": centers, "rot": rot, "tt": tt, "points": points, "v": v, "g": g, "step": step}


def assert_rig_premises(rig, shape):
    """the premises that make every fp32 operation exact, asserted on the rig's own data"""
    assert rig["step"] == 0.5 and all(s * 2 == n - 1 for s, n in zip(rig["sides"], shape))
    for x in (rig["position"], rig["centers"], rig["points"]):
        x = np.asarray(x, np.float64)
        x = x[~np.isnan(x)]                                                        # (the NaN point)
        assert np.array_equal(x * 8, np.round(x * 8)) and np.abs(x).max() < 2 ** 12
    assert np.array_equal(rig["tt"] * 4, np.round(rig["tt"] * 4), equal_nan=True)
    for R in rig["rot"]:
        assert np.array_equal(np.abs(R).sum(0), np.ones(3)) and np.array_equal(np.abs(R).sum(1), np.ones(3)) and set(np.unique(R)) <= {-1.0, 0.0, 1.0}
    for x in (rig["v"], rig["g"]):
        assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 2


def assert_exact_sums(bw):
    """... and of the sums over the points: sum |y| |u| and sum |u - R u|, in units of 2^-6, stay below 2^24, so no partial sum rounds"""
    assert np.einsum("bni,bna->bia", np.abs(bw["y"]), np.abs(bw["u"])).max() * 64 < 2 ** 24
    assert np.abs(bw["u"]).sum(1).max() * 2 * 64 < 2 ** 24
    assert bw["mag_v"].max() * 64 < 2 ** 24 and bw["mag_q"].max() * 64 < 2 ** 24


def general_problem(seed, B, C, shape, N, paired=False, duplicate=None, offset=3000.0):
    """generic rotations, a cuboid of 2 m sides, centers `offset` .. `offset` + 10000 mm from the origin on every axis; fp32 inputs"""
    rng = np.random.default_rng(seed)
    rot = []
    for _ in range(B):
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        th = rng.uniform(0.2, 2.5)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        rot.append(np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K)
    rot = np.stack(rot).astype(np.float32)
    centers = (rng.uniform(offset, offset + 10000.0, (B, 3)) * rng.choice([-1.0, 1.0], (B, 3))).astype(np.float32)
    sides = [2000.0, 1800.0, 2200.0]
    position = (centers[0].astype(np.float64) - np.array(sides) / 2 + rng.uniform(-50, 50, 3)).tolist()
    centers[1:] = centers[0] + rng.uniform(-100, 100, (B - 1, 3)).astype(np.float32)
    tt = np.stack([point_indices(rng, shape, N) for _ in range(B)])
    if duplicate:
        tt[:, duplicate[1]] = tt[:, duplicate[0]]
    points = world_points(tt, rot, centers, position, sides, shape).astype(np.float32)
    if duplicate:
        points[:, duplicate[1]] = points[:, duplicate[0]]
    v = rng.normal(size=(B, C, int(np.prod(shape))))
    g = rng.normal(size=(B, C) if paired else (B, C, N))
    return {"position": position, "sides": sides, "centers": centers, "rot": rot, "tt": tt, "points": points, "v": v, "g": g}
