"""Ray-marching volumes into camera-view maps on the MI355X (multiviewhmr_amd/volproject.py, volume_project.hip): the geometry to bits, bit
equality with the float64 oracle on the exact rig, general inputs within the derived bounds (tests/volproject_oracle.py),
agreement with sample_volume_cuboid, the special values, bitwise reproducibility, graph capture, the raw C ABI and the refusals.  Every
error is asserted through conftest.record_err, which also keeps it.  No ray is left out of any comparison: the oracle takes the kernel's
own ranges."""
import ctypes

import numpy as np
import pytest
import torch

import volproject_oracle as po
import volsample_oracle as vo
from conftest import record_err
from multiviewhmr_amd import _capi, aggregation, volproject, volsample

pytestmark = pytest.mark.gpu

# (B, C, V, volume, map, K): the minimum; odd extents, two views, a 5 x 9 map (two pixel tiles, both with a tail) at K = 1, 3, 8
BASE = [(1, 1, 1, (2, 2, 2), (1, 1), 1)] + [(2, 3, 2, (3, 5, 7), (5, 9), k) for k in (1, 3, 8)]
# one channel count on each side of the unroll boundary (po.UNROLL = 4 channels per loop trip) and of the channel-group boundary
# (po.GROUP = 8 channels per block, forward and backward)
EDGES = [(1, c, 1, (3, 5, 7), (5, 9), 3) for c in (po.UNROLL - 1, po.UNROLL, po.UNROLL + 1, po.GROUP - 1, po.GROUP, po.GROUP + 1)]
CASES = [(s, torch.float32) for s in BASE + EDGES] + [(s, dt) for s in (BASE[0], BASE[2]) for dt in (torch.float16, torch.bfloat16)]
IDS = ["b%dc%dv%d_%s_%dx%d_k%d_%s" % (s[0], s[1], s[2], "x".join(map(str, s[3])), s[4][0], s[4][1], s[5], str(dt)[6:]) for s, dt in CASES]
# the exact rig needs K a power of two and maps up to 5 x 5
EXACT = [((1, 1, 1, (2, 2, 2), (1, 1), 1), torch.float32), ((2, 3, 2, (3, 5, 7), (5, 5), 8), torch.float32), ((1, 9, 3, (3, 5, 7), (5, 4), 2), torch.float32),
         ((2, 3, 2, (3, 5, 7), (5, 5), 8), torch.float16), ((2, 3, 2, (3, 5, 7), (5, 5), 8), torch.bfloat16)]
EXACT_IDS = ["b%dc%dv%d_%s_%dx%d_k%d_%s" % (s[0], s[1], s[2], "x".join(map(str, s[3])), s[4][0], s[4][1], s[5], str(dt)[6:]) for s, dt in EXACT]
BETA = -1.5


def _t(x, gpu, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype))).to(gpu)


def _stored(v, dtype):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dtype).double().numpy()


def _hold(name, got, ref, bound):
    """|got - ref| <= bound elementwise; the element with the largest share of its bound is the one recorded"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(ref))
    err = np.abs(got - ref)
    assert not np.isnan(err).any(), name
    share = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    i = np.unravel_index(int(np.argmax(share)), share.shape) if share.ndim else ()
    print("%s: max-abs %.3e, largest share of the bound %.3f" % (name, float(err.max()), float(share[i])))
    record_err(name, float(err[i]), float(bound[i]))


def _exact(name, got, want):
    """equal as fp32 numbers, NaN in the same places (the sign of a zero is not told apart); anything else is an error above the bound 0"""
    got, want = np.asarray(got), np.asarray(want)
    err = 0.0
    if not np.array_equal(got, want, equal_nan=True):
        with np.errstate(invalid="ignore"):
            d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        d = np.where(np.isnan(got) & np.isnan(want), 0.0, np.where(np.isnan(d), np.inf, d))
        err = float(d.max()) or float("inf")
    print("%s: max-abs %.3e" % (name, err))
    record_err(name, err, 0.0)


def _run(gpu, pr, shape, ms, K, method, dtype=torch.float32, grad=True, g=None, **kw):
    """forward (+ backward) through the public function -> dict of numpy results"""
    B, C = pr["v"].shape[:2]
    vol = torch.from_numpy(np.ascontiguousarray(pr["v"])).to(dtype).view(B, C, *shape).to(gpu).requires_grad_(grad)
    maps, ranges = volproject.project_volume_cuboid(vol, _t(pr["rays"], gpu), _t(pr["rot"], gpu), _t(pr["centers"], gpu), pr["position"], pr["sides"], ms, K,
                                                    method, return_ranges=True, **kw)
    V = pr["rays"].shape[1]
    assert maps.dtype == ranges.dtype == torch.float32 and tuple(maps.shape) == (B, V, C) + tuple(ms) and tuple(ranges.shape) == (B, V) + tuple(ms) + (2,)
    res = {"maps": maps.detach().cpu().numpy(), "ranges": ranges.detach().cpu().numpy(), "grad_v": None}
    if grad:
        (maps * _t(pr["g"] if g is None else g, gpu)).sum().backward()
        assert vol.grad.dtype == dtype
        res["grad_v"] = vol.grad.detach().float().cpu().numpy().reshape(B, C, -1)
    return res


def _problem(case, dtype, seed):
    B, C, V, shape, ms, K = case
    pr = po.general_problem(seed, B, C, V, shape, ms)
    pr["v"], pr["g"] = _stored(pr["v"], dtype), pr["g"].astype(np.float32).astype(np.float64)
    return pr


def test_the_library_groups_channels_as_the_tests_assume():
    """EDGES straddles the kernel's own channel group and unroll, not a copy of them"""
    L = _capi.lib()
    group = (ctypes.c_int32 * 2)()
    L.mvhmr_project_volume_channel_group(group)
    assert tuple(group) == (po.GROUP, po.UNROLL) and L.mvhmr_project_volume_max_samples() == po.MAX_SAMPLES


# ------------------------------------------------------------------------------------ geometry: bits
def _special_rays():
    """index = world (identity rotation, step 1, corner 0) on a 3 x 5 x 7 volume; one ray per row: (o, d, what)"""
    n = np.nan
    return [([-4, 1, 1], [1, 0, 0], "parallel to two axes, inside their slabs"), ([-4, 1, 1], [1, -0.0, 0.0], "minus zero"),
            ([-4, 4.5, 1], [1, 0, 0], "parallel, outside the y slab"), ([-4, 4, 6], [1, 0, 0], "parallel, on the slab faces"),
            ([1, 1, 1], [1, 0.25, 0], "camera inside the cuboid"), ([4, 1, 1], [1, 0, 0], "cuboid behind the camera"),
            ([-4, 1, 1], [1, 0.5, 0.25], "oblique hit"), ([-4, 1, 1], [1, 3, 0], "oblique miss"), ([-4, 1, 1], [n, 0, 0], "NaN direction"),
            ([-4, n, 1], [1, 0, 0], "NaN origin"), ([1, 1, 1], [0, 0, 0], "no direction"), ([-1, 2, 3], [1, 0, 0], "through nodes")]


@pytest.mark.parametrize("depth", [(0.0, np.inf), (0.25, 4.5), (4.5, 5.5)], ids=["open", "near_far", "cut"])
def test_special_rays_are_clipped_as_the_contract_says(depth, gpu):
    """rays that miss, rays parallel to an axis inside and outside the slab, the camera inside the cuboid (lin = min_depth), the cuboid
    behind the camera, a max_depth that cuts the segment, NaN in rays: ranges equal the fp32 oracle bit for bit, and hits / misses are the
    ones the rules name"""
    shape, ms, K = (3, 5, 7), (1, 1), 3
    rows = _special_rays()
    B = len(rows)
    rays = np.zeros((B, 1, 3, 4), np.float32)
    for b, (o, d, _) in enumerate(rows):
        rays[b, 0, :, 2], rays[b, 0, :, 3] = d, o
    rng = np.random.default_rng(4)
    pr = {"rays": rays, "rot": np.broadcast_to(np.eye(3), (B, 3, 3)).copy(), "centers": np.zeros((B, 3)), "position": [0.0, 0.0, 0.0], "sides": [2.0, 4.0, 6.0],
          "v": rng.normal(size=(B, 2, 105)).astype(np.float32).astype(np.float64), "g": np.ones((B, 1, 2, 1, 1))}
    got = _run(gpu, pr, shape, ms, K, "mean", min_depth=depth[0], max_depth=depth[1])
    ref = po.full(pr, shape, ms, K, "mean", min_depth=depth[0], max_depth=depth[1])
    _exact("pv special rays %s: ranges" % (depth,), got["ranges"], ref["ranges"])
    hit = got["ranges"][..., 0] < got["ranges"][..., 1]
    if depth == (0.0, np.inf):
        want = [True, True, False, True, True, False, True, False, False, False, False, True]
        assert hit[:, 0, 0, 0].tolist() == want
        assert got["ranges"][0, 0, 0, 0].tolist() == [4.0, 6.0] and got["ranges"][4, 0, 0, 0].tolist() == [0.0, 1.0]
    if depth == (0.25, 4.5):
        assert got["ranges"][4, 0, 0, 0].tolist() == [0.25, 1.0] and got["ranges"][0, 0, 0, 0].tolist() == [4.0, 4.5]
    assert (got["ranges"][~hit] == 0).all()
    ref = po.full(pr, shape, ms, K, "mean", ranges=got["ranges"], min_depth=depth[0], max_depth=depth[1])
    _hold("pv special rays %s: maps" % (depth,), got["maps"], ref["out"], ref["e_out"])
    _hold("pv special rays %s: grad_volumes" % (depth,), got["grad_v"], ref["grad_v"], ref["e_grad"])
    miss = ~hit[:, 0, 0, 0]
    record_err("pv special rays %s: maps of misses" % (depth,), float(np.abs(got["maps"][miss]).max()), 0.0)
    record_err("pv special rays %s: gradient of misses" % (depth,), float(np.abs(got["grad_v"][miss]).max()), 0.0)


def test_the_origin_index_carries_the_bits_of_sample_volume_cuboid(gpu):
    """t_o, from which every ray of a view starts, is sample_volume_cuboid's index of the point o: the oracle's fp32 t_o (to which the
    ranges test above holds the kernel) equals the index the sampling op returns for o"""
    B, C, V, shape, ms, K = BASE[2]
    pr = po.general_problem(31, B, C, V, shape, ms)
    vol = torch.zeros(B, C, *shape, device=gpu)
    o = _t(pr["rays"][..., 3], gpu)
    _, idx = volsample.sample_volume_cuboid(vol, o, _t(pr["rot"], gpu), _t(pr["centers"], gpu), pr["position"], pr["sides"], return_index=True)
    _exact("pv origin index", idx.cpu().numpy(), po.origin_index(pr["rays"], pr["rot"], pr["centers"], pr["position"], pr["sides"], shape))


# ------------------------------------------------------------------------------------ the exact rig: bits
@pytest.mark.parametrize("method", ["mean", "max"])
@pytest.mark.parametrize("case", EXACT, ids=EXACT_IDS)
def test_exact_rig_is_bit_equal_to_the_float64_oracle(case, method, gpu):
    (B, C, V, shape, ms, K), dtype = case
    rig = po.exact_rig(21, B, C, V, shape, ms, K)
    assert np.array_equal(_stored(rig["v"], dtype), rig["v"])
    got = _run(gpu, rig, shape, ms, K, method, dtype)
    tag = "pv exact rig %s %s " % (EXACT_IDS[EXACT.index(case)], method)
    g64 = po.ray_geometry(rig["rays"], rig["rot"], rig["centers"], rig["position"], rig["sides"], shape, ms, T=np.float64)
    assert g64["hit"].any()
    r64 = np.stack([g64["lin"], g64["lout"]], -1)
    _exact(tag + "ranges", got["ranges"], r64.astype(np.float32))
    assert np.array_equal(r64.astype(np.float32).astype(np.float64), r64)
    tp = po.taps(po.sample_indices(g64, r64, K, np.float64), shape, np.float64)
    s, _ = po.samples(rig["v"], tp)
    fw = po.forward(s, g64["hit"], method)
    arg = np.where(g64["hit"][:, :, None], s.argmax(-1), 0) if method == "max" else None      # argmax: the first of equal maxima
    bw = po.backward(tp, s, g64["hit"], rig["g"], method, int(np.prod(shape)), 1.0, arg, fw)
    for x in (fw["out"], bw["grad_v"]):                                          # the oracle's values ARE fp32 numbers
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    _exact(tag + "maps", got["maps"], fw["out"].astype(np.float32))
    _exact(tag + "grad_volumes", got["grad_v"], torch.from_numpy(bw["grad_v"].astype(np.float32)).to(dtype).float().numpy())
    assert (bw["grad_v"] != 0).any() and (ms == (1, 1) or bw["count"].max() > 1)   # rays collide on voxels


# ------------------------------------------------------------------------------------ general inputs: the bounds
@pytest.mark.parametrize("method", po.METHODS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_general_inputs_stay_within_the_bounds(case, method, gpu):
    """coordinates 3 to 13 m from the origin in millimetres, generic rotations and cameras.  ranges must be the contract's bit for bit; maps
    and grad_volumes are held to the float64 oracle on the kernel's own ranges; 'mean' and 'max' maps also equal the contract's fp32 chain
    bit for bit"""
    (B, C, V, shape, ms, K), dtype = case
    pr = _problem((B, C, V, shape, ms, K), dtype, 60 + B + C + K)
    got = _run(gpu, pr, shape, ms, K, method, dtype, beta=BETA)
    tag = "pv general %s %s " % (IDS[CASES.index(case)], method)
    ref = po.full(pr, shape, ms, K, method, BETA, ranges=got["ranges"], store=str(dtype)[6:])
    _exact(tag + "ranges", got["ranges"], ref["ranges"])
    if ms != (1, 1):
        assert ref["hit"].any() and not ref["hit"].all()                         # rays that miss are there
    _hold(tag + "maps", got["maps"], ref["out"], ref["e_out"])
    if method != "softmax":
        _exact(tag + "maps against the fp32 chain", got["maps"], ref["maps32"])
    _hold(tag + "grad_volumes", got["grad_v"], ref["grad_v"], ref["e_grad"])


def test_a_non_contiguous_volume_gives_the_same_bits(gpu):
    B, C, V, shape, ms, K = BASE[2]
    pr = _problem(BASE[2], torch.float32, 70)
    want = _run(gpu, pr, shape, ms, K, "softmax", beta=BETA)
    base = torch.from_numpy(pr["v"].astype(np.float32)).view(B, C, *shape).to(gpu)
    wide = torch.zeros(B, C, shape[0], shape[1], 2 * shape[2], device=gpu)
    wide[..., ::2] = base
    vol = wide[..., ::2].requires_grad_(True)
    assert not vol.is_contiguous()
    maps = volproject.project_volume_cuboid(vol, _t(pr["rays"], gpu), _t(pr["rot"], gpu), _t(pr["centers"], gpu), pr["position"], pr["sides"], ms, K, "softmax",
                                            beta=BETA)
    gv, = torch.autograd.grad((maps * _t(pr["g"], gpu)).sum(), vol)
    assert np.array_equal(maps.detach().cpu().numpy().view(np.uint32), want["maps"].view(np.uint32))
    assert np.array_equal(gv.reshape(B, C, -1).cpu().numpy().view(np.uint32), want["grad_v"].view(np.uint32))


def test_two_passes_of_channels_give_the_bits_of_one_channel_at_a_time(gpu):
    """a volume whose single channel fills more than half of the accumulator's 2^30 bytes: two channels take two passes (the second with
    c_first = 1 and an accumulator row that is not the channel's index).  The exponent of a (b, c) reads its own rows only, so each
    channel's gradient must carry the bits it has when it is projected alone, in one pass"""
    shape, ms, K, V = (512, 512, 257), (5, 9), 3, 2
    n_vox = shape[0] * shape[1] * shape[2]
    L = _capi.lib()
    one = L.mvhmr_project_volume_workspace_bytes(1, 1, *shape)
    assert one > 2 ** 29 and L.mvhmr_project_volume_workspace_bytes(1, 2, *shape) == one        # one channel per pass, whatever C
    pr = po.general_problem(73, 1, 2, V, (3, 5, 7), ms)
    rays, rot, cen, g = _t(pr["rays"], gpu), _t(pr["rot"], gpu), _t(pr["centers"], gpu), _t(pr["g"], gpu)
    torch.manual_seed(3)
    vol = torch.randn(1, 2, *shape, device=gpu).to(torch.bfloat16).requires_grad_(True)
    for method in ("mean", "softmax"):
        maps = volproject.project_volume_cuboid(vol, rays, rot, cen, pr["position"], pr["sides"], ms, K, method, beta=BETA)
        both, = torch.autograd.grad((maps * g).sum(), vol)
        assert int((both[0, 0] != 0).sum()) > 0 and int((both[0, 1] != 0).sum()) > 0 and bool(torch.isfinite(both).all())
        for c in range(2):
            alone = vol.detach()[:, c:c + 1].clone().requires_grad_(True)
            m1 = volproject.project_volume_cuboid(alone, rays, rot, cen, pr["position"], pr["sides"], ms, K, method, beta=BETA)
            g1, = torch.autograd.grad((m1 * g[:, :, c:c + 1]).sum(), alone)
            assert torch.equal(m1[:, :, 0], maps[:, :, c]) and torch.equal(g1[0, 0].view(torch.int16), both[0, c].view(torch.int16)), (method, c)
            del alone, m1, g1
        del maps, both
    assert n_vox * 8 > 2 ** 29


# ------------------------------------------------------------------------------------ against existing code
def test_mean_is_the_mean_of_sample_volume_cuboid_along_the_rays(gpu):
    """the points o + lambda_k d rebuilt in float64 from the kernel's ranges, sampled by sample_volume_cuboid and averaged in float64.  The
    points pass through fp32 and the sampling op's own index, so the index of a sample may differ from the march's by the roundings of
    volsample_oracle.bound_roundtrip_index -- counted once for the rebuilt point and once for the march's origin and direction, which pass
    through the same operations --, and that moves a sample by at most the index error times the largest step between neighbouring voxels"""
    B, C, V, shape, ms, K = BASE[3]
    pr = _problem(BASE[3], torch.float32, 75)
    got = _run(gpu, pr, shape, ms, K, "mean", grad=False)
    rays = pr["rays"].astype(np.float64)
    lin, lout = got["ranges"][..., 0].astype(np.float64), got["ranges"][..., 1].astype(np.float64)
    hit = lin < lout
    u, v = np.meshgrid(np.arange(ms[1], dtype=np.float64), np.arange(ms[0], dtype=np.float64))
    d = np.einsum("bvij,hwj->bvhwi", rays[..., :3], np.stack([u, v, np.ones_like(u)], -1))
    lam = lin[..., None] + (np.arange(K) + 0.5) * ((lout - lin) / K)[..., None]
    x = rays[:, :, None, None, None, :, 3] + lam[..., None] * d[..., None, :]    # (B,V,Hm,Wm,K,3)
    vol = torch.from_numpy(pr["v"].astype(np.float32)).view(B, C, *shape).to(gpu)
    s = volsample.sample_volume_cuboid(vol, _t(x.reshape(B, -1, 3), gpu), _t(pr["rot"], gpu), _t(pr["centers"], gpu), pr["position"], pr["sides"])
    s = s.double().cpu().numpy().reshape((B, C, V) + tuple(ms) + (K,)).swapaxes(1, 2)
    mean = np.where(hit[:, :, None], s.mean(-1), 0.0)
    ref = po.full(pr, shape, ms, K, "mean", ranges=got["ranges"], g=None)
    dt = vo.bound_roundtrip_index(x.reshape(B, -1, 3), pr["centers"], pr["position"], pr["sides"], shape)[:, 0].sum(-1).max()
    slack = 2.0 * np.abs(pr["v"]).max() * 2.0 * dt + vo.gamma(8) * np.abs(pr["v"]).max()      # 2 dt: the point's roundings, and the march's own
    _hold("pv against sample_volume_cuboid: mean", got["maps"], mean, ref["e_out"] + slack)
    assert hit.any() and np.abs(mean).max() > 0


def test_volume_generator_project_is_the_free_function_on_its_cuboid(gpu):
    S, B, C, V, ms, K = 4, 2, 3, 2, (5, 9), 3
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=2500.0, device=gpu)
    cub = gen.cuboid()
    pr = po.general_problem(92, B, C, V, (S, S, S), ms)
    look = np.stack([[po.look_at([3000.0 + 200 * v, 500.0 * (b + 1), 400.0], [0.0, 0.0, 0.0], 6.0, ms) for v in range(V)] for b in range(B)])
    vol = torch.from_numpy(pr["v"].astype(np.float32)).view(B, C, S, S, S).to(gpu)
    rays = volproject.camera_rays(torch.from_numpy(look).to(gpu))
    rot, cen = _t(pr["rot"], gpu), torch.zeros(B, 3, device=gpu)
    a, ra = gen.project(vol, rays, rot, cen, ms, K, "max", return_ranges=True)
    b, rb = volproject.project_volume_cuboid(vol, rays, rot, cen, cub.position, cub.sides, ms, K, "max", return_ranges=True)
    assert torch.equal(a, b) and torch.equal(ra, rb) and a.abs().max() > 0 and (ra[..., 0] < ra[..., 1]).any()


# ------------------------------------------------------------------------------------ special values
def test_a_view_that_misses_gives_exact_zeros_and_no_gradient(gpu):
    """a view turned away from the cuboid: its maps and ranges are exactly 0, a gradient that arrives for it alone leaves grad_volumes exactly
    0, and the other view's maps carry the bits they have without it"""
    B, C, V, shape, ms, K = BASE[2]
    pr = _problem(BASE[2], torch.float32, 77)
    away = dict(pr, rays=pr["rays"].copy())
    away["rays"][:, 1, :, :3] *= -1.0                                            # view 1 looks the other way: the cuboid lies behind it
    g = pr["g"].copy()
    g[:, 0] = 0.0                                                                # only the view that misses carries a gradient
    for method in po.METHODS:
        full = _run(gpu, away, shape, ms, K, method, beta=BETA, g=g)
        part = _run(gpu, dict(pr, rays=pr["rays"][:, :1]), shape, ms, K, method, beta=BETA, grad=False)
        record_err("pv miss %s: maps" % method, float(np.abs(full["maps"][:, 1]).max()), 0.0)
        record_err("pv miss %s: ranges" % method, float(np.abs(full["ranges"][:, 1]).max()), 0.0)
        record_err("pv miss %s: grad_volumes" % method, float(np.abs(full["grad_v"]).max()), 0.0)
        assert np.array_equal(full["maps"][:, :1].view(np.uint32), part["maps"].view(np.uint32)) and np.abs(part["maps"]).max() > 0


def test_max_ties_take_the_lowest_k(gpu):
    """a volume constant along x under rays parallel to x: the K samples of a ray are equal bit for bit, so the gradient lands on the taps
    of sample 0 alone"""
    shape, ms, K = (5, 3, 4), (1, 1), 4
    rig = po.exact_rig(9, 1, 2, 1, shape, ms, K)                                  # view 0 marches along +x from t_x = -4; e = (1, 0, 0)
    plane = np.random.default_rng(1).integers(-2, 3, (1, 2, 1, 3, 4)).astype(np.float64)
    rig["v"] = np.broadcast_to(plane, (1, 2) + shape).reshape(1, 2, -1).copy()
    rig["g"] = np.full((1, 1, 2, 1, 1), 3.0)
    got = _run(gpu, rig, shape, ms, K, "max")
    assert got["ranges"][0, 0, 0, 0].tolist() == [4.0, 8.0]                       # samples at t_x = 0.5, 1.5, 2.5, 3.5
    g = got["grad_v"].reshape(1, 2, *shape)
    record_err("pv max ties: gradient outside sample 0", float(np.abs(g[:, :, 2:]).max()), 0.0)
    assert np.abs(g[:, :, :2]).max() > 0 and np.array_equal(g.sum((2, 3, 4)), np.full((1, 2), 3.0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
def test_a_sample_on_a_node_between_minus_infinity_returns_the_node(dtype, gpu):
    shape, ms, K = (3, 5, 7), (1, 1), 1
    rig = po.exact_rig(5, 1, 2, 1, shape, ms, K)
    to = np.array([-4.0, 2.0, 3.0])                                              # lin = 4, lout = 6, the one sample at t = (1, 2, 3)
    rig["rays"][0, 0, :, 3] = vo.world_points(to[None, None], rig["rot"], rig["centers"], rig["position"], rig["sides"], shape)[0, 0]
    vol = torch.full((1, 2) + shape, -float("inf"), dtype=dtype, device=gpu)
    vol[0, 0, 1, 2, 3], vol[0, 1, 1, 2, 3] = 0.75, -1.5
    for method in ("mean", "max"):
        maps = volproject.project_volume_cuboid(vol, _t(rig["rays"], gpu), _t(rig["rot"], gpu), _t(rig["centers"], gpu), rig["position"], rig["sides"], ms, K,
                                                method)
        _exact("pv special: -inf neighbours %s %s" % (method, str(dtype)[6:]), maps.cpu().numpy(), np.array([[[[[0.75]], [[-1.5]]]]], np.float32))


def test_a_non_finite_grad_row_poisons_its_row_alone(gpu):
    B, C, V, shape, ms, K = BASE[2]
    pr = _problem(BASE[2], torch.float32, 79)
    for method in po.METHODS:
        clean = _run(gpu, pr, shape, ms, K, method, beta=BETA)
        g = pr["g"].copy()
        hit = clean["ranges"][..., 0] < clean["ranges"][..., 1]
        where = np.argwhere(~hit[1, 0])
        g[(1, 0, 2) + (tuple(where[0]) if len(where) else (0, 0))] = np.inf       # even under a ray that misses: the row's maximum sees it
        g[0, 1, 0, 2, 3] = np.nan
        bad = _run(gpu, pr, shape, ms, K, method, beta=BETA, g=g)["grad_v"]
        assert np.isnan(bad[1, 2]).all() and np.isnan(bad[0, 0]).all()
        keep = np.ones((B, C), bool)
        keep[1, 2] = keep[0, 0] = False
        assert np.array_equal(bad[keep].view(np.uint32), clean["grad_v"][keep].view(np.uint32)), method


# ------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("deterministic", [False, True])
def test_two_runs_are_bitwise_identical(deterministic, gpu):
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(deterministic)
    try:
        for case, dtype in ((BASE[3], torch.float32), (EDGES[5], torch.float32), (BASE[2], torch.bfloat16)):
            B, C, V, shape, ms, K = case
            pr = _problem(case, dtype, 80)
            for method in po.METHODS:
                a, b = (_run(gpu, pr, shape, ms, K, method, dtype, beta=BETA) for _ in range(2))
                for key in a:
                    assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), (method, key)
    finally:
        torch.use_deterministic_algorithms(prev)


def test_permuting_the_channels_permutes_maps_and_gradient_bitwise(gpu):
    case = EDGES[5]                                                              # 9 channels: two groups
    B, C, V, shape, ms, K = case
    pr = _problem(case, torch.float32, 81)
    perm = np.array([3, 0, 8, 1, 2, 7, 4, 6, 5])
    for method in po.METHODS:
        a = _run(gpu, pr, shape, ms, K, method, beta=BETA)
        b = _run(gpu, dict(pr, v=pr["v"][:, perm], g=pr["g"][:, :, perm]), shape, ms, K, method, beta=BETA)
        assert np.array_equal(a["maps"][:, :, perm].view(np.uint32), b["maps"].view(np.uint32)), method
        assert np.array_equal(a["grad_v"][:, perm].view(np.uint32), b["grad_v"].view(np.uint32)), method


# ------------------------------------------------------------------------------------ graphs, the raw ABI, refusals
def test_graph_capture_and_replay_match_eager(gpu):
    """forward + backward of all three methods captured into one HIP graph on a single stream; the replay on new volume values equals
    eager bit for bit"""
    B, C, V, shape, ms, K = BASE[3]
    pr = _problem(BASE[3], torch.float32, 95)
    vol = torch.from_numpy(pr["v"].astype(np.float32)).view(B, C, *shape).to(gpu).requires_grad_(True)
    rays, rot, cen, g = _t(pr["rays"], gpu), _t(pr["rot"], gpu), _t(pr["centers"], gpu), _t(pr["g"], gpu)
    pos, sides = list(pr["position"]), list(pr["sides"])

    def step():
        outs = []
        for method in po.METHODS:
            maps, ranges = volproject.project_volume_cuboid(vol, rays, rot, cen, pos, sides, ms, K, method, beta=BETA, return_ranges=True)
            outs += [maps, ranges, torch.autograd.grad((maps * g).sum(), vol)[0]]
        return outs

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = step()
    with torch.no_grad():
        vol.copy_(torch.randn_like(vol))                 # new values, same buffers
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    torch.cuda.synchronize()
    for a, b in zip(captured, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_raw_c_abi_call_equals_the_op(gpu):
    """the C ABI through ctypes alone: forward and backward give the op's bits; a null and an undersized workspace are refused and launch
    nothing"""
    L = _capi.lib()
    B, C, V, shape, ms, K = BASE[3]
    pr = _problem(BASE[3], torch.float32, 96)
    ref = _run(gpu, pr, shape, ms, K, "softmax", beta=BETA)
    vol = torch.from_numpy(pr["v"].astype(np.float32)).view(B, C, *shape).to(gpu)
    rays, rot, cen, g = _t(pr["rays"], gpu), _t(pr["rot"], gpu), _t(pr["centers"], gpu), _t(pr["g"], gpu)
    d3 = ctypes.c_double * 3
    pos, sides, stream = d3(*pr["position"]), d3(*pr["sides"]), aggregation._stream(gpu)
    maps, aux = torch.full((B, V, C) + ms, 7.0, device=gpu), torch.full((B, V, C) + ms, 7.0, device=gpu)
    ranges = torch.full((B, V) + ms + (2,), 7.0, device=gpu)
    place = (vol.data_ptr(), _capi.F32, rays.data_ptr(), rot.data_ptr(), cen.data_ptr(), pos, sides, B, V, C) + shape + ms + (K, 2, BETA, 0.0, float("inf"))
    assert L.mvhmr_project_volume_forward(*place, maps.data_ptr(), ranges.data_ptr(), aux.data_ptr(), stream) == _capi.OK
    need = L.mvhmr_project_volume_workspace_bytes(B, C, *shape)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    gv = torch.full_like(vol, 7.0)                                               # the call writes every element itself
    tail = (g.data_ptr(), maps.data_ptr(), aux.data_ptr(), gv.data_ptr())
    assert L.mvhmr_project_volume_backward_volumes(*place, *tail, ws.data_ptr(), need, stream) == _capi.OK
    torch.cuda.synchronize()
    for name, t in (("maps", maps), ("ranges", ranges), ("grad_v", gv.view(B, C, -1))):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), ref[name].view(np.uint32)), name
    before = gv.clone()
    assert L.mvhmr_project_volume_backward_volumes(*place, *tail, ws.data_ptr(), need - 1, stream) == _capi.ERR_WORKSPACE
    assert b"workspace" in L.mvhmr_last_error()
    assert L.mvhmr_project_volume_backward_volumes(*place, *tail, None, need, stream) == _capi.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(before, gv)


def test_geometry_that_requires_grad_is_refused(gpu):
    B, C, V, shape, ms, K = BASE[2]
    pr = _problem(BASE[2], torch.float32, 97)
    vol = torch.zeros(B, C, *shape, device=gpu, requires_grad=True)
    for which in range(3):
        args = [_t(pr["rays"], gpu), _t(pr["rot"], gpu), _t(pr["centers"], gpu)]
        args[which].requires_grad_(True)
        with pytest.raises(ValueError, match="requires grad"):
            volproject.project_volume_cuboid(vol, *args, pr["position"], pr["sides"], ms, K)
    with pytest.raises(ValueError, match="method"):
        volproject.project_volume_cuboid(vol, _t(pr["rays"], gpu), _t(pr["rot"], gpu), _t(pr["centers"], gpu), pr["position"], pr["sides"], ms, K, "sum")
    with pytest.raises(RuntimeError):
        volproject.project_volume_cuboid(vol, _t(pr["rays"], gpu).cpu(), _t(pr["rot"], gpu), _t(pr["centers"], gpu), pr["position"], pr["sides"], ms, K)
