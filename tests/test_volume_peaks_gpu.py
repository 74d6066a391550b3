"""volume_peaks on the card against tests/peaks_oracle.py.  Scores, indices, positions and grad_volumes involve no rounding, so every one of
those comparisons is exact (bound 0); only the pose gradients, which are fp32 sums, have a bound, counted from the code."""
import ctypes

import numpy as np
import pytest
import torch

import peaks_oracle as po
from conftest import record_err
from multiviewhmr_amd import _capi, aggregation, peaks, softargmax
from test_unproject_gpu import _ring_problem

pytestmark = pytest.mark.gpu

INF = float("inf")


def _tile():
    t = (ctypes.c_int32 * 3)()
    _capi.lib().mvhmr_volume_peaks_tile(t)
    return tuple(t)


TX, TY, TZ = _tile()                                       # the strip of one block: planes of one X run, Y tile, Z tile
MAX_K = peaks.MAX_K
# (B, J, volume): the minimum; odd extents inside one strip; Y and Z on both sides of one and two tile edges; X across the run edge
BASE = [(1, 1, (1, 1, 1)), (2, 3, (3, 5, 7))]
EDGE_Y = [(1, 2, (3, y, 5)) for y in (TY - 1, TY, TY + 1, 2 * TY + 1)]
EDGE_Z = [(1, 2, (3, 4, z)) for z in (TZ - 1, TZ, TZ + 1, 2 * TZ + 1)]
EDGE_X = [(1, 2, (TX + 1, 3, 5))]
SHAPES = BASE + EDGE_Y + EDGE_Z + EDGE_X
HALF_SHAPES = [BASE[1], EDGE_Y[3], EDGE_Z[2]]


def _id(s):
    return "b%dj%d_%s" % (s[0], s[1], "x".join(map(str, s[2])))


def _exact(name, got, want):
    """equal as numbers, NaN in the same places; anything else is an error above the bound 0"""
    got, want = np.asarray(got), np.asarray(want)
    err = 0.0
    if got.shape != want.shape:
        err = float("inf")
    elif not np.array_equal(got, want, equal_nan=True):
        with np.errstate(invalid="ignore"):
            d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        d = np.where(np.isnan(got) & np.isnan(want), 0.0, np.where(np.isnan(d), np.inf, d))
        err = float(d.max()) or float("inf")
    print("%s: max-abs %.3e" % (name, err))
    record_err(name, err, 0.0)


def _stored(v, dtype):
    """float32 numpy of the values a volume of `dtype` holds"""
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dtype).float().numpy()


def _boundary(extent, tile):
    """indices on the faces of an axis and on both sides of every tile edge inside it"""
    return sorted({0, extent - 1} | {e for t in range(tile, extent, tile) for e in (t - 1, t)})


def _content(kind, seed, B, J, shape):
    """float32 (B, J, X, Y, Z).  levels: 8 values, so nearly every comparison is a tie.  planted: distinct small noise and the SAME large value
    on the corners, edges, faces and on both sides of every tile edge (neighbours in the box suppress no one: a plateau; far ones sit in
    other strips, so the merge breaks the tie).  special: levels with NaN, +-inf and +-0 strewn in.  few: -inf but for two voxels."""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    if kind == "levels":
        return rng.integers(0, 8, (B, J, X, Y, Z)).astype(np.float32)
    if kind == "planted":
        v = (rng.permutation(B * J * X * Y * Z).reshape(B, J, X, Y, Z) / np.float32(B * J * X * Y * Z)).astype(np.float32)
        for x in _boundary(X, TX):
            for y in _boundary(Y, TY):
                for z in _boundary(Z, TZ):
                    v[:, :, x, y, z] = 5.0
        v[0, 0, X // 2, Y // 2, Z // 2] = 7.0
        return v
    if kind == "special":
        v = rng.integers(-2, 3, (B, J, X, Y, Z)).astype(np.float32)
        flat = v.reshape(-1)
        for value in (np.nan, INF, -INF, -0.0):
            flat[rng.integers(0, flat.size, max(1, flat.size // 40))] = value
        return v
    assert kind == "few"
    v = np.full((B, J, X, Y, Z), -INF, np.float32)
    v.reshape(B, J, -1)[:, :, [0, (X * Y * Z) // 2]] = np.float32([1.5, -2.0])
    return v


def _run(gpu, v, dtype, k, radius, threshold):
    vol = torch.from_numpy(np.ascontiguousarray(v)).to(dtype).to(gpu)
    scores, index = peaks.volume_peaks(vol, k, radius=radius, threshold=threshold)
    assert scores.dtype == torch.float32 and index.dtype == torch.int32 and tuple(scores.shape) == tuple(index.shape) == v.shape[:2] + (k,)
    return scores.cpu().numpy(), index.cpu().numpy()


def _check(gpu, tag, v, dtype, k, radius, threshold=None):
    v = _stored(v, dtype)
    want_s, want_i = po.volume_peaks(v, k, radius, threshold)
    got_s, got_i = _run(gpu, v, dtype, k, radius, threshold)
    _exact(tag + " index", got_i, want_i)
    _exact(tag + " scores", got_s, want_s)
    assert np.array_equal(np.signbit(got_s), np.signbit(want_s)), tag                           # the stored bits: -0 comes back as -0


# ------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_forward_fp32_every_radius_and_content(case, gpu):
    B, J, shape = case
    for radius in (0, 1, 2, 3):
        for n, kind in enumerate(("levels", "planted", "special", "few")):
            v = _content(kind, 100 + n, B, J, shape)
            _check(gpu, "pk %s r%d %s" % (_id(case), radius, kind), v, torch.float32, 7, radius)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("case", HALF_SHAPES, ids=_id)
def test_forward_16_bit_storage(case, dtype, gpu):
    B, J, shape = case
    for radius, kind in ((1, "levels"), (2, "planted"), (3, "special"), (0, "few")):
        _check(gpu, "pk %s %s r%d %s" % (_id(case), str(dtype)[6:], radius, kind), _content(kind, 110, B, J, shape), dtype, 9, radius)


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_ring_filling_and_wrapping_along_x(radius, gpu):
    """X = 1, 2, 2r and 2r + 2: fewer planes than the ring holds, exactly as many as the halo, and enough to shift it out once"""
    for X in (1, 2, 2 * radius, 2 * radius + 2):
        for kind in ("levels", "planted"):
            _check(gpu, "pk ring x%d r%d %s" % (X, radius, kind), _content(kind, 120 + X, 2, 2, (X, 5, 6)), torch.float32, 6, radius)


@pytest.mark.parametrize("radius", [1, 3])
def test_forward_64_cubed(radius, gpu):
    v = _content("levels", 130, 2, 2, (64, 64, 64))
    v += _content("planted", 131, 2, 2, (64, 64, 64)) * (v == 7)                                # ties at the top, some of them on the edges
    _check(gpu, "pk 64^3 r%d" % radius, v, torch.float32, 16, radius)


def test_more_slices_than_a_grid_axis_holds(gpu):
    _check(gpu, "pk 65537 slices", _content("levels", 140, 65537, 1, (2, 2, 2)), torch.float32, 3, 1)


@pytest.mark.parametrize("k", [1, 8, MAX_K])
def test_constant_volume_every_voxel_a_peak(k, gpu):
    """the dense worst case: more peaks per plane than any list holds, all of them equal"""
    shape = (TX + 2, TY + 3, TZ + 5)
    for radius in (0, 2):
        _check(gpu, "pk constant k%d r%d" % (k, radius), np.full((1, 2) + shape, 0.25, np.float32), torch.float32, k, radius)


def test_rising_volume_refills_the_lists(gpu):
    """values that rise with the index: every plane's peaks beat everything the block has kept (radius 0: every voxel is a peak)"""
    shape = (TX + 2, TY + 3, TZ + 5)
    v = np.arange(int(np.prod(shape)), dtype=np.float32).reshape((1, 1) + shape)
    _check(gpu, "pk rising r0", v, torch.float32, MAX_K, 0)
    _check(gpu, "pk rising r1", v, torch.float32, 5, 1)


def test_threshold_is_strict(gpu):
    v = _content("planted", 150, 2, 2, (5, TY + 2, 9))
    for thr in (5.0, 0.5, 7.0, -INF, INF):
        _check(gpu, "pk threshold %r" % thr, v, torch.float32, 12, 1, threshold=thr)
    got_s, got_i = _run(gpu, v, torch.float32, 12, 1, 5.0)
    assert got_i[0, 0, 0] >= 0 and got_s[0, 0, 0] == 7.0 and (got_i[0, 0, 1:] == -1).all()      # the planted 5s are not above 5
    assert (got_i[1] == -1).all() and np.isneginf(got_s[1]).all()


def test_non_contiguous_input_and_raw_c_route(gpu):
    B, J, shape, k, radius, thr = 2, 3, (4, TY + 1, 9), 10, 2, 1.0
    v = _content("levels", 160, B, J, shape)
    vol = torch.from_numpy(v).to(gpu)
    want_s, want_i = peaks.volume_peaks(vol, k, radius=radius, threshold=thr)
    view = vol.transpose(3, 4).contiguous().transpose(3, 4)
    assert not view.is_contiguous()
    got_s, got_i = peaks.volume_peaks(view, k, radius=radius, threshold=thr)
    assert torch.equal(got_s, want_s) and torch.equal(got_i, want_i)
    L = _capi.lib()
    need = L.mvhmr_volume_peaks_workspace_bytes(B, J, *shape, k)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    raw_s, raw_i = torch.empty(B, J, k, device=gpu), torch.empty(B, J, k, dtype=torch.int32, device=gpu)
    rc = L.mvhmr_volume_peaks(vol.data_ptr(), _capi.F32, B, J, *shape, k, radius, thr, None, None, None, None, raw_s.data_ptr(), raw_i.data_ptr(), None,
                              ws.data_ptr(), need, aggregation._stream(gpu))
    assert rc == _capi.OK, L.mvhmr_last_error()
    torch.cuda.synchronize()
    assert torch.equal(raw_s, want_s) and torch.equal(raw_i, want_i)


# ------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda d: str(d)[6:])
def test_grad_volumes_is_the_scatter(dtype, gpu):
    B, J, shape, k = 2, 3, (3, TY + 1, 7), 6
    N = int(np.prod(shape))
    g = np.random.default_rng(170).standard_normal((B, J, k)).astype(np.float32)
    for kind in ("levels", "few"):
        v = _stored(_content(kind, 171, B, J, shape), dtype)
        runs = []
        for _ in range(2):
            vol = torch.from_numpy(v).to(dtype).to(gpu).requires_grad_(True)
            scores, index = peaks.volume_peaks(vol, k, radius=1)
            (scores.masked_fill(index < 0, 0) * torch.from_numpy(g).to(gpu)).sum().backward()   # -inf * g of a missing slot must not reach the sum
            assert vol.grad.dtype == dtype and vol.grad.shape == vol.shape
            runs.append(vol.grad)
        assert torch.equal(runs[0], runs[1])
        index = index.cpu().numpy()
        want = torch.from_numpy(po.grad_volumes(index, g, N).astype(np.float32)).to(dtype).float().numpy()
        _exact("pk grad_volumes %s %s" % (kind, str(dtype)[6:]), runs[0].float().cpu().numpy().reshape(B, J, N), want)
        assert int(torch.count_nonzero(runs[0])) <= int((index >= 0).sum())
        if kind == "few":
            assert (index[..., 2:] == -1).all() and int(torch.count_nonzero(runs[0])) == int(np.count_nonzero(g[..., :2]))
    # a gradient that reaches a missing slot directly is dropped
    vol = torch.from_numpy(v).to(dtype).to(gpu).requires_grad_(True)
    scores, index = peaks.volume_peaks(vol, k, radius=1)
    scores.backward(torch.ones_like(scores))
    assert int(torch.count_nonzero(vol.grad)) == 2 * B * J


# ------------------------------------------------------------------------------------ positions
def _pose(seed, B):
    rng = np.random.default_rng(seed)
    rot = np.linalg.qr(rng.standard_normal((B, 3, 3)))[0].astype(np.float32)
    return rot, rng.uniform(-100, 100, (B, 3)).astype(np.float32)


def test_positions_carry_the_coordinate_volumes_bits(gpu):
    B, J, S, k = 2, 2, 12, 5
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=2500.0, device=gpu)
    cub = gen.cuboid()
    rot, cen = _pose(180, B)
    v = _content("levels", 181, B, J, (S, S, S))
    v[1, 1] = -INF
    v[1, 1, 3, 4, 5] = 1.0                                                                      # one peak, k - 1 missing slots
    vol, r, c = torch.from_numpy(v).to(gpu), torch.from_numpy(rot).to(gpu).requires_grad_(True), torch.from_numpy(cen).to(gpu).requires_grad_(True)
    scores, index, positions = gen.peaks(vol, r, c, k, radius=1)
    plain_s, plain_i = peaks.volume_peaks(vol, k, radius=1)
    assert torch.equal(scores, plain_s) and torch.equal(index, plain_i) and tuple(positions.shape) == (B, J, k, 3)
    coords = gen.coord_volumes(r.detach(), c.detach(), gpu).view(B, 1, S ** 3, 3).expand(B, J, S ** 3, 3)      # mvhmr_build_coord_volumes
    gathered = torch.gather(coords, 2, index.clamp(min=0).long()[..., None].expand(B, J, k, 3)) * (index >= 0)[..., None]
    _exact("pk positions vs coord volumes", positions.detach().cpu().numpy(), gathered.cpu().numpy())
    index_np = index.cpu().numpy()
    assert (index_np[1, 1, 1:] == -1).all() and (positions[1, 1, 1:] == 0).all()
    _exact("pk positions vs recipe", positions.detach().cpu().numpy(), po.positions(index_np, cub.position, cub.sides, (S, S, S), rot, cen))

    g = np.random.default_rng(182).standard_normal((B, J, k, 3)).astype(np.float32)
    grads = []
    for _ in range(2):
        r.grad = c.grad = None
        _, _, positions = gen.peaks(vol, r, c, k, radius=1)
        (positions * torch.from_numpy(g).to(gpu)).sum().backward()
        grads.append((r.grad.clone(), c.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    gr, gc, bound_r, bound_c = po.pose_grads(index_np, g, cub.position, cub.sides, (S, S, S), rot, cen)
    for name, got, ref, bound in (("rot", grads[0][0], gr, bound_r), ("center", grads[0][1], gc, bound_c)):
        err = np.abs(got.double().cpu().numpy() - ref)
        share = err / np.maximum(bound, 1e-300)
        i = np.unravel_index(int(np.argmax(share)), share.shape)
        print("pk grad_%s: max-abs %.3e, largest share of the bound %.3f" % (name, float(err.max()), float(share[i])))
        record_err("pk grad_" + name, float(err[i]), float(bound[i]))


# ------------------------------------------------------------------------------------ composition
def _chain(gen, cub, S, f, p, heat, rot, cen, k):
    scores, index, positions = gen.peaks(heat, rot, cen, k, radius=1, threshold=0.0)
    centers, fi, valid = peaks.peak_proposals(scores, index, positions)
    rots = rot.repeat_interleave(heat.shape[1] * k, 0)
    fine = aggregation.unprojection_cuboid(f, p, rots, centers, cub.position, cub.sides, (S, S, S), "softmax", feature_index=fi)
    keypoints = softargmax.soft_argmax_3d_cuboid(fine, rots, centers, cub.position, cub.sides, beta=2.0)
    return scores, index, centers, fi, valid, rots, fine, keypoints


def test_proposals_feed_one_volume_per_peak_and_capture_in_a_graph(gpu):
    B, V, C, H, W, S, k = 2, 3, 4, 16, 12, 8, 3
    feats, proj, _ = _ring_problem(B, V, C, H, W, (S, S, S), seed=190)
    f, p = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=2500.0, device=gpu)
    cub = gen.cuboid()
    rot, cen = (torch.from_numpy(x).to(gpu) for x in _pose(191, B))
    heat = torch.from_numpy(_content("levels", 192, B, 1, (S, S, S))).to(gpu) - 6.5              # sample 0: many peaks above 0 ...
    heat[1] = -1.0
    heat[1, 0, 2, 3, 4] = 2.0                                                                    # ... sample 1: one, and two missing slots
    scores, index, centers, fi, valid, rots, fine, keypoints = _chain(gen, cub, S, f, p, heat, rot, cen, k)
    assert fi.dtype == torch.int32 and fi.tolist() == [0, 0, 0, 1, -1, -1] and valid.tolist() == [True] * 4 + [False] * 2
    m = valid.nonzero().flatten()
    plain = aggregation.unprojection_cuboid(f[fi[m].long()], p[fi[m].long()], rots[m], centers[m], cub.position, cub.sides, (S, S, S), "softmax",
                                            variant="gather")
    assert tuple(fine.shape) == (B * k, C, S, S, S) and torch.equal(fine[m], plain)
    assert torch.count_nonzero(fine[~valid]) == 0
    assert tuple(keypoints.shape) == (B * k, C, 3) and torch.isfinite(keypoints[m]).all()

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _chain(gen, cub, S, f, p, heat, rot, cen, k)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _chain(gen, cub, S, f, p, heat, rot, cen, k)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, (scores, index, centers, fi, valid, rots, fine, keypoints)):
        assert torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    heat[1, 0, 5, 5, 5] = 3.0                                                                    # a second peak in sample 1: the replay follows
    graph.replay()
    torch.cuda.synchronize()
    assert captured[3].tolist() == [0, 0, 0, 1, 1, -1] and float(captured[0][1, 0, 0]) == 3.0
