"""volume_peaks without a GPU: the numpy oracle against the torch recipe and against first principles, the Python front end's argument
checks, fake-tensor shapes, the C ABI's refusals (against the cross-compiled library) and peak_proposals on CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import peaks_oracle as po
from multiviewhmr_amd import _capi, aggregation, peaks

INF = float("inf")


def _torch_recipe(v, k, r, thr):
    """the recipe the op replaces, valid where no two values of a slice are equal"""
    t = torch.from_numpy(v)
    pooled = F.max_pool3d(t, 2 * r + 1, 1, r) if r else t
    keep = (pooled == t) & (t > thr)
    n = t[0, 0].numel()
    scores, idx = torch.where(keep, t, torch.full_like(t, -INF)).flatten(2).topk(min(k, n))
    idx = torch.where(scores > -INF, idx, torch.full_like(idx, -1))
    pad = k - scores.shape[-1]
    return F.pad(scores, (0, pad), value=-INF).numpy(), F.pad(idx, (0, pad), value=-1).numpy().astype(np.int32)


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (2, 9, 4)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_oracle_equals_torch_recipe_on_tie_free_inputs(shape, radius):
    """a random permutation of distinct values per slice: nothing is left undefined, so every slot must agree (radius 2 and 3 exceed an
    extent of (2, 9, 4), every radius > 0 exceeds (1, 1, 1))"""
    rng = np.random.default_rng(radius * 100 + shape[1])
    n = shape[0] * shape[1] * shape[2]
    v = np.stack([rng.permutation(n) for _ in range(6)]).reshape(2, 3, *shape).astype(np.float32) - n // 2
    for k, thr in ((1, -INF), (4, -INF), (n + 3, -INF), (5, 0.0), (5, float(v.max()))):
        want_s, want_i = _torch_recipe(v, k, radius, thr)
        got_s, got_i = po.volume_peaks(v, k, radius, None if thr == -INF else thr)
        assert np.array_equal(got_s, want_s) and np.array_equal(got_i, want_i), (k, thr)


def test_oracle_plateau_order_and_padding():
    v = np.zeros((1, 1, 2, 3, 4), np.float32)
    s, i = po.volume_peaks(v, 30, 1)
    assert np.array_equal(i[0, 0, :24], np.arange(24)) and (i[0, 0, 24:] == -1).all()          # a plateau is all peaks, in index order
    assert (s[0, 0, :24] == 0).all() and np.isneginf(s[0, 0, 24:]).all()
    v[0, 0, 1, 2, 3] = 1                                                                       # suppresses its 2x2x2 clipped box, and is first
    s, i = po.volume_peaks(v, 30, 1)
    box = {(x * 3 + y) * 4 + z for x in (0, 1) for y in (1, 2) for z in (2, 3)}
    assert i[0, 0, 0] == 23 and s[0, 0, 0] == 1
    assert list(i[0, 0, 1:17]) == [n for n in range(24) if n not in box] and (i[0, 0, 17:] == -1).all()


def test_oracle_nan_poisons_exactly_its_boxes():
    v = np.arange(5 * 5 * 5, dtype=np.float32).reshape(1, 1, 5, 5, 5) * 0                      # constant: every voxel a peak but the poisoned
    v[0, 0, 2, 2, 0] = np.nan
    for r in (0, 1, 2):
        mask = po.peak_mask(v, r)[0, 0]
        want = np.ones((5, 5, 5), bool)
        want[max(2 - r, 0):2 + r + 1, max(2 - r, 0):2 + r + 1, 0:r + 1] = False
        assert np.array_equal(mask, want), r


def test_oracle_infinities_threshold_and_zeros():
    v = np.full((1, 1, 1, 1, 6), -INF, np.float32)
    s, i = po.volume_peaks(v, 3, 1)
    assert (i == -1).all() and np.isneginf(s).all()                                            # -inf is never a peak, whatever the threshold
    v[0, 0, 0, 0, 4] = INF
    s, i = po.volume_peaks(v, 3, 1)
    assert list(i[0, 0]) == [4, -1, -1] and s[0, 0, 0] == INF                                  # +inf is one
    v = np.array([3, 1, 2, 0, 2, 1, 3], np.float32).reshape(1, 1, 1, 1, 7)
    assert list(po.volume_peaks(v, 4, 1)[1][0, 0]) == [0, 6, 2, 4]                             # value descending, ties by ascending index
    assert list(po.volume_peaks(v, 4, 2)[1][0, 0]) == [0, 6, -1, -1]                           # radius 2: both 2s have a 3 in their box
    assert list(po.volume_peaks(v, 4, 1, threshold=2.0)[1][0, 0]) == [0, 6, -1, -1]            # strictly above the threshold
    assert list(po.volume_peaks(v, 4, 1, threshold=3.0)[1][0, 0]) == [-1] * 4
    z = np.array([0.0, -0.0, 0.0, -1.0], np.float32).reshape(1, 1, 1, 1, 4)
    s, i = po.volume_peaks(z, 4, 1)
    assert list(i[0, 0]) == [0, 1, 2, -1]                                                      # -0 and +0 are equal: neither suppresses the other
    assert np.signbit(s[0, 0, 1]) and not np.signbit(s[0, 0, 0])                               # and the stored bits come back


def test_oracle_single_rounding_fma():
    a, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)                              # a*b = 1 + 2^-11 + 2^-24: a tie of fp32 ...
    assert po._fma32(a, b, np.float32(2.0 ** -60)) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)  # ... that the tiny addend must break upward
    assert po._fma32(a, b, np.float32(-2.0 ** -60)) == np.float32(1 + 2.0 ** -11)
    assert po._fma32(a, b, np.float32(0)) == np.float32(1 + 2.0 ** -11)                        # the tie itself goes to even


def test_oracle_positions_and_pose_gradients():
    rng = np.random.default_rng(5)
    shape, B = (3, 5, 7), 2
    rot = np.linalg.qr(rng.standard_normal((B, 3, 3)))[0].astype(np.float32)
    cen = rng.standard_normal((B, 3)).astype(np.float32)
    pos, sides = [-1.0, -0.5, 0.25], [2.0, 1.0, 3.0]
    index = rng.integers(0, 105, (B, 2, 4)).astype(np.int32)
    index[1, 0, 3] = -1
    x = po.positions(index, pos, sides, shape, rot, cen)
    n = np.maximum(index, 0)
    ijk = np.stack([n // 35, (n // 7) % 5, n % 7], -1)
    grid = np.asarray(pos) + np.asarray(sides) / (np.asarray(shape) - 1) * ijk
    want = np.einsum("brc,bjkc->bjkr", rot.astype(np.float64), grid - cen[:, None, None]) + cen[:, None, None]
    want[1, 0, 3] = 0
    assert np.abs(x - want).max() < 1e-5 and (x[1, 0, 3] == 0).all()
    g = rng.standard_normal(index.shape + (3,))
    gr, gc, br, bc = po.pose_grads(index, g, pos, sides, shape, rot, cen)
    R = torch.tensor(rot, dtype=torch.float64, requires_grad=True)
    c = torch.tensor(cen, dtype=torch.float64, requires_grad=True)
    d = torch.from_numpy(po.offsets(index, pos, sides, shape, cen).astype(np.float64) + cen[:, None, None].astype(np.float64)) - c[:, None, None]
    xt = torch.einsum("brc,bjkc->bjkr", R, d) + c[:, None, None]
    (xt * torch.from_numpy(g * (index >= 0)[..., None])).sum().backward()
    assert np.allclose(gr, R.grad.numpy(), atol=1e-12) and np.allclose(gc, c.grad.numpy(), atol=1e-12)
    assert (br >= 0).all() and (bc >= 0).all() and br.max() < 1e-4 and bc.max() < 1e-4


def test_oracle_grad_volumes_skips_missing_slots():
    index = np.array([[[3, 0, -1]]], np.int32)
    g = po.grad_volumes(index, np.array([[[2.0, 5.0, 7.0]]]), 6)
    assert list(g[0, 0]) == [5.0, 0, 0, 2.0, 0, 0]


# ---- the Python front end
def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype)


def test_argument_validation():
    v, rot, cen, pos, sides = _meta(2, 3, 3, 5, 7), _meta(2, 3, 3), _meta(2, 3), [0, 0, 0], [1, 1, 1]
    for bad in (0, 129, -1, 2.0, True, None, "4"):
        with pytest.raises(ValueError, match="k must be"):
            peaks.volume_peaks(v, bad)
        with pytest.raises(ValueError, match="k must be"):
            peaks.volume_peaks_cuboid(v, rot, cen, pos, sides, bad)
    for bad in (-1, 4, 1.0, False, None):
        with pytest.raises(ValueError, match="radius must be"):
            peaks.volume_peaks(v, 4, radius=bad)
    for bad in (float("nan"), np.float32("nan"), "0.5", True, np.bool_(True), torch.tensor(0.5)):
        with pytest.raises(ValueError, match="threshold"):
            peaks.volume_peaks(v, 4, threshold=bad)
    for good in (0.5, 1, np.float32(0.3), np.float64(0.3), np.int64(2), -INF):                  # thresholds out of a numpy config are numbers too
        peaks.volume_peaks(v, 4, threshold=good)
    for dt in (torch.float64, torch.int32):
        with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
            peaks.volume_peaks(_meta(2, 3, 3, 5, 7, dtype=dt), 4)
    with pytest.raises(TypeError):
        peaks.volume_peaks(np.zeros((2, 3, 3, 5, 7), np.float32), 4)
    for bad in (_meta(2, 3, 5, 7), _meta(2, 0, 3, 5, 7), _meta(2, 3, 0, 5, 7)):
        with pytest.raises(ValueError):
            peaks.volume_peaks(bad, 4)
    with pytest.raises(ValueError, match="rotations must be"):
        peaks.volume_peaks_cuboid(v, _meta(3, 3, 3), cen, pos, sides, 4)
    with pytest.raises(ValueError, match="centers must be"):
        peaks.volume_peaks_cuboid(v, rot, _meta(2, 4), pos, sides, 4)
    with pytest.raises(ValueError, match="sides takes 3 finite"):
        peaks.volume_peaks_cuboid(v, rot, cen, pos, [1, 1], 4)
    cpu = torch.zeros(2, 3, 3, 5, 7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        peaks.volume_peaks(cpu, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        peaks.volume_peaks_cuboid(cpu, torch.zeros(2, 3, 3), torch.zeros(2, 3), pos, sides, 4)


def test_fake_shapes_and_dtypes():
    rot, cen, pos, sides = _meta(2, 3, 3), _meta(2, 3), [0, 0, 0], [1, 1, 1]
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        v = _meta(2, 3, 3, 5, 7, dtype=dt)
        s, i = peaks.volume_peaks(v, 9, radius=0, threshold=0.5)
        assert tuple(s.shape) == tuple(i.shape) == (2, 3, 9) and s.dtype == torch.float32 and i.dtype == torch.int32
        s, i, x = peaks.volume_peaks_cuboid(v, rot, cen, pos, sides, 128, radius=3)
        assert tuple(s.shape) == tuple(i.shape) == (2, 3, 128) and tuple(x.shape) == (2, 3, 128, 3)
        assert s.dtype == x.dtype == torch.float32 and i.dtype == torch.int32
        gv = torch.ops.mvhmr.volume_peaks_backward(i, s, [2, 3, 3, 5, 7], dt)
        assert tuple(gv.shape) == (2, 3, 3, 5, 7) and gv.dtype == dt
        gr, gc = torch.ops.mvhmr.volume_peaks_backward_pose(i, x, rot, cen, pos, sides, [3, 5, 7])
        assert tuple(gr.shape) == (2, 3, 3) and tuple(gc.shape) == (2, 3)
    gen = aggregation.VolumeGenerator.__new__(aggregation.VolumeGenerator)
    assert callable(gen.peaks)


def test_backward_graph_holds_the_two_backward_ops():
    """forward + backward of the cuboid op through AOT autograd on meta tensors: a scatter for the scores, a pose kernel for the positions"""
    from functorch.compile import make_boxed_func
    from torch._functorch.aot_autograd import aot_function
    graphs = {}

    def keep(name):
        def compiler(gm, _):
            graphs[name] = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
            return make_boxed_func(gm)
        return compiler

    def fn(v, rot, cen):
        s, i, x = peaks.volume_peaks_cuboid(v, rot, cen, [0, 0, 0], [1, 1, 1], 4)
        return s.sum() + x.sum()

    args = [torch.empty(s, device="meta").requires_grad_(True) for s in ((2, 3, 3, 5, 7), (2, 3, 3), (2, 3))]
    aot_function(fn, fw_compiler=keep("fw"), bw_compiler=keep("bw"))(*args).backward()
    assert sum("volume_peaks_cuboid" in t for t in graphs["fw"]) == 1
    assert sum("volume_peaks_backward.default" in t for t in graphs["bw"]) == 1 and sum("volume_peaks_backward_pose" in t for t in graphs["bw"]) == 1


def test_peak_proposals_on_cpu_tensors():
    index = torch.tensor([[[5, -1], [0, 2]], [[-1, -1], [7, -1]]], dtype=torch.int32)
    scores = torch.where(index >= 0, torch.ones(2, 2, 2), torch.full((2, 2, 2), -INF))
    positions = torch.arange(24, dtype=torch.float32).view(2, 2, 2, 3).requires_grad_(True)
    centers, fi, valid = peaks.peak_proposals(scores, index, positions)
    assert tuple(centers.shape) == (8, 3) and fi.dtype == torch.int32 and valid.dtype == torch.bool
    assert fi.tolist() == [0, -1, 0, 0, -1, -1, 1, -1] and valid.tolist() == [True, False, True, True, False, False, True, False]
    assert torch.equal(centers, positions.detach().view(8, 3))
    centers.sum().backward()
    assert torch.equal(positions.grad, torch.ones_like(positions))
    with pytest.raises(ValueError):
        peaks.peak_proposals(scores, index, positions[..., :2])
    with pytest.raises(TypeError):
        peaks.peak_proposals(scores, index.numpy(), positions)


# ---- the C ABI's host answers
def test_c_layer_constants_and_refusals():
    L = _capi.lib()
    tile = (ctypes.c_int32 * 3)()
    L.mvhmr_volume_peaks_tile(tile)
    TX, TY, TZ = tile
    assert min(TX, TY, TZ) >= 1 and L.mvhmr_volume_peaks_max_k() == peaks.MAX_K
    blocks = lambda x, y, z: -(-x // TX) * -(-y // TY) * -(-z // TZ)                               # noqa: E731
    for sizes in ((2, 3, 3, 5, 7, 4), (1, 1, TX + 1, 2 * TY + 1, TZ, 128), (32, 17, 64, 64, 64, 4)):
        B, J, X, Y, Z, K = sizes
        assert L.mvhmr_volume_peaks_workspace_bytes(*sizes) == B * J * blocks(X, Y, Z) * K * 8     # K keys per block, whatever the volume holds
    assert L.mvhmr_volume_peaks_workspace_bytes(2, 3, 3, 5, 7, 129) == 0 and L.mvhmr_volume_peaks_workspace_bytes(0, 3, 3, 5, 7, 4) == 0

    d3 = (ctypes.c_double * 3)
    pos, sides = d3(0, 0, 0), d3(1, 1, 1)
    p = ctypes.c_void_p(256)                                                                   # never dereferenced: every call below is refused first
    need = L.mvhmr_volume_peaks_workspace_bytes(2, 3, 3, 5, 7, 4)
    INVALID, UNSUPPORTED, WORKSPACE = _capi.ERR_INVALID_ARGUMENT, _capi.ERR_UNSUPPORTED, _capi.ERR_WORKSPACE

    def fwd(volumes=p, dtype=_capi.F32, sizes=(2, 3, 3, 5, 7, 4), radius=1, thr=-INF, rot=p, center=p, position=pos, side=sides, scores=p, index=p,
            positions=p, ws=p, ws_bytes=need):
        return L.mvhmr_volume_peaks(volumes, dtype, *sizes, radius, thr, rot, center, position, side, scores, index, positions, ws, ws_bytes, None)

    def bwd(dtype=_capi.F32, index=p, g=p, sizes=(2, 3, 3, 5, 7, 4), gv=p):
        return L.mvhmr_volume_peaks_backward(dtype, index, g, *sizes, gv, None)

    def pose(index=p, g=p, rot=p, center=p, position=pos, side=sides, sizes=(2, 3, 3, 5, 7, 4), gr=p, gc=p):
        return L.mvhmr_volume_peaks_backward_pose(index, g, rot, center, position, side, *sizes, gr, gc, None)

    for kw in (dict(volumes=None), dict(scores=None), dict(index=None), dict(rot=None), dict(center=None), dict(position=None), dict(side=None),
               dict(radius=-1), dict(radius=4), dict(thr=float("nan"))):
        assert fwd(**kw) == INVALID, kw
    bad_sizes = [(0, 3, 3, 5, 7, 4), (2, 0, 3, 5, 7, 4), (2, 3, 0, 5, 7, 4), (2, 3, 3, 0, 7, 4), (2, 3, 3, 5, 0, 4), (2, 3, 3, 5, 7, 0), (2, 3, 3, 5, 7, 129),
                 (2, 3, 2048, 2048, 512, 4), (1 << 16, 1 << 16, 3, 5, 7, 4), (2, 3, 1 << 21, 1 << 21, 1 << 22, 4), (2, 3, 1 << 30, 1 << 30, 1 << 30, 4)]
    for sizes in bad_sizes:
        assert fwd(sizes=sizes) == INVALID and bwd(sizes=sizes) == INVALID and pose(sizes=sizes) == INVALID, sizes
    # the order of the checks: an argument error wins over the dtype, the dtype over the workspace
    assert fwd(dtype=7, radius=4, ws=None) == INVALID and fwd(dtype=7, ws=None) == UNSUPPORTED and fwd(dtype=-1) == UNSUPPORTED
    assert bwd(dtype=3) == UNSUPPORTED and bwd(dtype=3, index=None) == INVALID
    # more blocks than one launch holds (2^24 - 1 of 256 threads) is refused by name, before the workspace is looked at
    assert fwd(sizes=(1 << 15, 1 << 9, 3, 5, 7, 4), ws=None) == UNSUPPORTED and b"split the batch" in L.mvhmr_last_error()
    assert fwd(sizes=(1 << 15, 1 << 9, 3, 5, 7, 4), dtype=7) == UNSUPPORTED and b"dtype" in L.mvhmr_last_error()
    # null pointers come first: the pose gradient names a missing cuboid pointer even when a size is wrong as well
    assert pose(rot=None, sizes=(0, 3, 3, 5, 7, 4)) == INVALID and b"non-null" in L.mvhmr_last_error()
    for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws=ctypes.c_void_p(264)), dict(ws_bytes=0)):
        assert fwd(**kw) == WORKSPACE and b"workspace" in L.mvhmr_last_error(), kw
    # without positions the cuboid is not looked at
    assert fwd(positions=None, rot=None, center=None, position=None, side=None, ws=None) == WORKSPACE
    for kw in (dict(index=None), dict(g=None), dict(gv=None)):
        assert bwd(**kw) == INVALID, kw
    for kw in (dict(index=None), dict(g=None), dict(rot=None), dict(center=None), dict(position=None), dict(side=None), dict(gr=None, gc=None)):
        assert pose(**kw) == INVALID, kw
