"""Numpy restatement of volume_peaks (multiviewhmr_amd/peaks.py): the semantics, not the kernel.

Voxel n of slice (b, j) is a peak iff no value of its clipped box [i-r, i+r] x [j-r, j+r] x [k-r, k+r] is NaN, v_n >= every value of the
box (outside counts as -inf; equal values do not suppress each other; -0 == +0) and v_n > threshold, strictly.  The K outputs are the peaks
by value descending, ties by ascending flat index; missing slots hold score -inf, index -1, position 0.  The box maximum is taken by
(2r+1)^3 shifted maxima with NaN poisoning, the order by np.lexsort((index, -score)).  Also here: the fp32 cuboid recipe for the positions
(every operation rounded once, the fused ones emulated exactly) and the float64 gradients.
"""
import numpy as np

U = 2.0 ** -24                                            # unit roundoff of fp32


def peak_mask(v, radius, threshold=None):
    """bool array shaped like v (..., X, Y, Z): which voxels are peaks.  v: float array (16-bit storage widened by the caller)."""
    v = np.asarray(v)
    r = int(radius)
    thr = -np.inf if threshold is None else np.float32(threshold)
    nan = np.isnan(v)
    lead = [(0, 0)] * (v.ndim - 3)
    w = np.pad(np.where(nan, -np.inf, v), lead + [(r, r)] * 3, constant_values=-np.inf)
    p = np.pad(nan, lead + [(r, r)] * 3, constant_values=False)
    X, Y, Z = v.shape[-3:]
    best = np.full(v.shape, -np.inf, w.dtype)
    poisoned = np.zeros(v.shape, bool)
    for dx in range(2 * r + 1):
        for dy in range(2 * r + 1):
            for dz in range(2 * r + 1):
                sl = (Ellipsis, slice(dx, dx + X), slice(dy, dy + Y), slice(dz, dz + Z))
                best = np.maximum(best, w[sl])
                poisoned |= p[sl]
    with np.errstate(invalid="ignore"):
        return ~poisoned & (v >= best) & (v > thr)


def volume_peaks(v, k, radius=1, threshold=None):
    """(scores (B, J, k) float32, index (B, J, k) int32) of volumes v (B, J, X, Y, Z)"""
    v = np.asarray(v)
    B, J = v.shape[:2]
    mask = peak_mask(v, radius, threshold).reshape(B, J, -1)
    flat = v.reshape(B, J, -1)
    scores = np.full((B, J, k), -np.inf, np.float32)
    index = np.full((B, J, k), -1, np.int32)
    for b in range(B):
        for j in range(J):
            idx = np.nonzero(mask[b, j])[0]
            val = flat[b, j, idx].astype(np.float64)
            order = np.lexsort((idx, -val))[:k]
            scores[b, j, :len(order)] = val[order]
            index[b, j, :len(order)] = idx[order]
    return scores, index


def grad_volumes(index, grad_scores, voxels):
    """float64 (B, J, voxels): grad_scores scattered to index, nothing from the missing slots"""
    B, J, K = index.shape
    g = np.zeros((B, J, voxels), np.float64)
    for b in range(B):
        for j in range(J):
            present = index[b, j] >= 0
            g[b, j, index[b, j, present]] = np.asarray(grad_scores, np.float64)[b, j, present]
    return g


# ---- the cuboid recipe in fp32 (device_common.h::cuboid_offset, voxel_xyz), evaluated at chosen indices only
def _fma32(a, b, c):
    """fl32(a * b + c) with one rounding: the product is exact in float64, the sum is rounded to odd there (two-sum tells which way the
    true value lies), and round-to-odd at 53 bits followed by round-to-nearest at 24 is correct rounding"""
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where((e != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def offsets(index, position, sides, shape, centers):
    """fp32 d = (position + step * (i, j, k)) - center[b] at index (B, J, K) (any value for a missing slot) -> (B, J, K, 3) float32"""
    X, Y, Z = shape
    f = np.float32
    n = np.maximum(np.asarray(index, np.int64), 0)
    ijk = np.stack([n // (Y * Z), (n // Z) % Y, n % Z], -1).astype(f)
    step = np.array([f(float(sides[a]) / (shape[a] - 1)) if shape[a] > 1 else f(0) for a in range(3)], f)
    grid = (np.asarray(position, np.float64).astype(f) + (step * ijk).astype(f)).astype(f)
    return (grid - np.asarray(centers, f)[:, None, None, :]).astype(f)


def positions(index, position, sides, shape, rot, centers):
    """(B, J, K, 3) float32 world positions: fl32(fma(R2, dz, fma(R1, dy, fl32(R0 * dx))) + c) per row of rot; 0 for a missing slot"""
    f = np.float32
    d = offsets(index, position, sides, shape, centers)
    R = np.asarray(rot, f)[:, None, None, :, :]
    acc = (R[..., 0].astype(np.float64) * d[..., 0:1].astype(np.float64)).astype(f)
    acc = _fma32(R[..., 1], d[..., 1:2], acc)
    acc = _fma32(R[..., 2], d[..., 2:3], acc)
    x = (acc + np.asarray(centers, f)[:, None, None, :]).astype(f)
    return np.where((np.asarray(index) >= 0)[..., None], x, f(0))


def pose_grads(index, grad_positions, position, sides, shape, rot, centers):
    """float64 (grad_rot (B, 3, 3), grad_center (B, 3)) of sum(grad_positions * positions) over the present slots, with the fp32 offsets the
    kernels recompute (they are inputs of the sums, not results), and a bound on what fp32 sums of n = J*K terms in slot order may differ:
    grad_rot[r][c] is n fused steps, each one rounding of a partial sum bounded by sum |g_r d_c|; grad_center[c] adds t = g_c - h_c with h
    three fused steps over R^T g (3 U sum_i |R_ic g_i|), one rounding for the difference, and n for the running sum"""
    d = offsets(index, position, sides, shape, centers).astype(np.float64)
    g = np.asarray(grad_positions, np.float64) * (np.asarray(index) >= 0)[..., None]
    R = np.asarray(rot, np.float64)
    B, J, K = index.shape
    n = J * K
    grad_rot = np.einsum("bjkr,bjkc->brc", g, d)
    bound_rot = 1.01 * n * U * np.einsum("bjkr,bjkc->brc", np.abs(g), np.abs(d))
    h = np.einsum("bic,bjki->bjkc", R, g)
    t = g - h
    grad_center = t.sum((1, 2))
    habs = np.einsum("bic,bjki->bjkc", np.abs(R), np.abs(g))
    bound_center = 1.01 * ((3 * U * habs + U * np.abs(t)).sum((1, 2)) + n * U * (np.abs(t) + 3 * U * habs).sum((1, 2)))
    return grad_rot, grad_center, bound_rot, bound_center
