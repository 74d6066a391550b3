"""Ray-marching volumes into camera-view maps without a device (multiviewhmr_amd/volproject.py, tests/volproject_oracle.py):
the numpy oracle held to the torch recipe in float64, its fp32 restatement held to its float64 self, camera_rays, the exponent arithmetic
of the fixed-point accumulator, refusals of the Python and the C layer, fake-tensor shapes and traced graphs, and the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import volproject_oracle as po
from multiviewhmr_amd import _capi, aggregation, volproject

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mvhmr_unproject.h")


# ---- the oracle against the torch recipe: points o + lambda_k d, 5-D grid_sample, reduce
def _recipe(rig, method, beta):
    """maps (1,V,C,Hm,Wm) and grad_volumes from torch alone, in float64, on the oracle's float64 ranges"""
    shape, (Hm, Wm), K = rig["shape"], rig["map_shape"], rig["K"]
    rays = po.camera_rays(rig["P"])
    geo = po.ray_geometry(rays, rig["rot"], rig["centers"], rig["position"], rig["sides"], shape, (Hm, Wm), T=np.float64, true_steps=True)
    hit = torch.from_numpy(geo["hit"])
    lin, lout = torch.from_numpy(geo["lin"]), torch.from_numpy(geo["lout"])
    D, o = torch.from_numpy(rays[..., :3]), torch.from_numpy(rays[..., 3])
    u, v = torch.meshgrid(torch.arange(Wm, dtype=torch.float64), torch.arange(Hm, dtype=torch.float64), indexing="xy")
    pix = torch.stack([u, v, torch.ones_like(u)], -1)                             # (Hm,Wm,3)
    d = torch.einsum("bvij,hwj->bvhwi", D, pix)
    lam = lin[..., None] + (torch.arange(K, dtype=torch.float64) + 0.5) * ((lout - lin) / K)[..., None]
    x = o[:, :, None, None, None, :] + lam[..., None] * d[..., None, :]           # (B,V,Hm,Wm,K,3) world points
    R, c = torch.from_numpy(rig["rot"]), torch.from_numpy(rig["centers"])
    step = torch.tensor([rig["sides"][a] / (shape[a] - 1) for a in range(3)], dtype=torch.float64)
    t = (torch.einsum("bia,bvhwki->bvhwka", R, x - c[:, None, None, None, None]) + (c[:, None, None, None, None] - torch.tensor(rig["position"]))) / step
    grid = (2.0 * t / (torch.tensor(shape, dtype=torch.float64) - 1.0) - 1.0).flip(-1)   # (z, y, x) order
    vol = torch.from_numpy(rig["v"]).view(1, -1, *shape).requires_grad_(True)
    B, V = x.shape[:2]
    s = F.grid_sample(vol, grid.reshape(B, V * Hm, Wm, K, 3), mode="bilinear", padding_mode="zeros", align_corners=True)
    s = s.view(B, -1, V, Hm, Wm, K).transpose(1, 2)                               # (B,V,C,Hm,Wm,K)
    out = s.mean(-1) if method == "mean" else s.max(-1).values if method == "max" else (torch.softmax(beta * s, -1) * s).sum(-1)
    out = torch.where(hit[:, :, None], out, torch.zeros_like(out))
    (out * torch.from_numpy(rig["g"])).sum().backward()
    return out.detach().numpy(), vol.grad.reshape(rig["v"].shape).numpy(), geo


@pytest.mark.parametrize("method", po.METHODS)
def test_float64_oracle_equals_the_torch_recipe(method):
    rig = po.issue_rig()
    shape, ms, K, beta = rig["shape"], rig["map_shape"], rig["K"], 1.7
    want, want_grad, geo = _recipe(rig, method, beta)
    n_hit = int(geo["hit"].sum())
    print("rays that hit: %d of %d" % (n_hit, geo["hit"].size))
    # hits and misses are both exercised.  The issue counts 30 hits on its rig but does not give the cuboid's sides; the 2 m cube centred on
    # the origin used here gives 29
    assert n_hit == 29 and geo["hit"].size == 54
    ranges = np.stack([geo["lin"], geo["lout"]], -1)
    tp = po.taps(po.sample_indices(geo, ranges, K, np.float64), shape, np.float64)
    s, _ = po.samples(rig["v"], tp)
    fw = po.forward(s, geo["hit"], method, beta)
    arg = s.argmax(-1) if method == "max" else None
    bw = po.backward(tp, s, geo["hit"], rig["g"], method, int(np.prod(shape)), beta, arg, fw)
    assert np.abs(fw["out"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.abs(bw["grad_v"] - want_grad).max() <= 1e-12 * max(1.0, np.abs(want_grad).max())
    assert np.abs(want[geo["hit"][:, :, None].repeat(want.shape[2], 2)]).min() > 0 and (want_grad != 0).any()


def test_pixels_are_column_row_and_lambda_is_the_depth():
    """P [o + lambda D (u, v, 1); 1] = lambda (u, v, 1), through the package's camera_rays and the oracle's alike"""
    rig = po.issue_rig()
    P = torch.from_numpy(rig["P"])
    rays = volproject.camera_rays(P)
    assert rays.dtype == torch.float32 and tuple(rays.shape) == (1, 1, 3, 4)
    assert np.allclose(rays.double().numpy(), po.camera_rays(rig["P"]), rtol=1e-6, atol=1e-9)
    r = po.camera_rays(rig["P"])[0, 0]
    for (u, v, lam) in ((0.0, 0.0, 1.0), (8.0, 5.0, 2500.0), (3.0, 2.0, 3100.0)):
        x = r[:, 3] + lam * r[:, :3] @ np.array([u, v, 1.0])
        assert np.allclose(rig["P"][0, 0] @ np.append(x, 1.0), lam * np.array([u, v, 1.0]), rtol=1e-9, atol=1e-6)
    with pytest.raises(ValueError):
        volproject.camera_rays(torch.zeros(2, 3, 4))


# ---- the fp32 restatement
def test_fp32_contract_stays_close_to_its_float64_self_and_marks_the_same_rays():
    rig = po.issue_rig()
    shape, ms = rig["shape"], rig["map_shape"]
    rays = po.camera_rays(rig["P"]).astype(np.float32)
    a = po.ray_geometry(rays, rig["rot"].astype(np.float32), rig["centers"], rig["position"], rig["sides"], shape, ms)
    b = po.ray_geometry(rays, rig["rot"].astype(np.float32), rig["centers"], rig["position"], rig["sides"], shape, ms, T=np.float64)
    assert a["lin"].dtype == np.float32 and np.array_equal(a["hit"], b["hit"])
    assert np.allclose(a["lin"], b["lin"], rtol=1e-4, atol=1e-2) and np.allclose(a["lout"], b["lout"], rtol=1e-4, atol=1e-2)
    assert (a["lin"][~a["hit"]] == 0).all() and (a["lout"][~a["hit"]] == 0).all()


def test_clip_rules_axis_parallel_depth_limits_and_nan():
    shape, ms = (3, 5, 7), (1, 1)
    eye = np.eye(3)[None]
    place = dict(rot=eye, centers=np.zeros((1, 3)), position=[0.0, 0.0, 0.0], sides=[2.0, 4.0, 6.0], shape=shape, map_shape=ms)   # step 1: index = world

    def ranges(o, d, **kw):
        rays = np.zeros((1, 1, 3, 4), np.float32)
        rays[0, 0, :, 2], rays[0, 0, :, 3] = d, o
        geo = po.ray_geometry(rays, **place, **kw)
        return float(geo["lin"][0, 0, 0, 0]), float(geo["lout"][0, 0, 0, 0]), bool(geo["hit"][0, 0, 0, 0])

    assert ranges([-4, 1, 1], [1, 0, 0]) == (4.0, 6.0, True)                      # parallel to y and z, inside their slabs
    assert ranges([-4, 1, 1], [1, -0.0, 0]) == (4.0, 6.0, True)                   # -0 is a zero too
    assert ranges([-4, 4.5, 1], [1, 0, 0]) == (0.0, 0.0, False)                   # ... outside the y slab
    assert ranges([-4, 4, 1], [1, 0, 0])[2]                                      # on the slab's face: inside
    assert ranges([1, 1, 1], [1, 0, 0]) == (0.0, 1.0, True)                       # the camera inside the cuboid: lin = min_depth
    assert ranges([1, 1, 1], [1, 0, 0], min_depth=0.25) == (0.25, 1.0, True)
    assert ranges([4, 1, 1], [1, 0, 0]) == (0.0, 0.0, False)                      # the cuboid behind the camera
    assert ranges([-4, 1, 1], [1, 0, 0], max_depth=5.0) == (4.0, 5.0, True)       # max_depth cuts the segment
    assert ranges([-4, 1, 1], [1, 0, 0], max_depth=4.0) == (0.0, 0.0, False)      # ... to nothing
    assert ranges([-4, 1, 1], [np.nan, 0, 0]) == (0.0, 0.0, False)
    assert ranges([-4, np.nan, 1], [1, 0, 0]) == (0.0, 0.0, False)
    assert ranges([1, 1, 1], [0, 0, 0]) == (0.0, 0.0, False)                      # no direction: lout stays infinite


def test_exact_rig_premises_hold():
    for (B, C, V, shape, ms, K) in ((1, 1, 1, (2, 2, 2), (1, 1), 1), (2, 3, 2, (3, 5, 7), (5, 5), 8)):
        rig = po.exact_rig(7, B, C, V, shape, ms, K)
        geo = po.ray_geometry(rig["rays"], rig["rot"], rig["centers"], rig["position"], rig["sides"], shape, ms)
        g64 = po.ray_geometry(rig["rays"], rig["rot"], rig["centers"], rig["position"], rig["sides"], shape, ms, T=np.float64)
        assert geo["hit"].any() and np.array_equal(geo["hit"], g64["hit"])
        for key in ("to", "e", "lin", "lout"):
            assert np.array_equal(geo[key].astype(np.float64), g64[key]), key     # every fp32 operation was exact
        assert np.array_equal(geo["to"][:, :, 0, 0], rig["to"])
        ranges = np.stack([geo["lin"], geo["lout"]], -1)
        t32, t64 = po.sample_indices(geo, ranges, K), po.sample_indices(g64, ranges.astype(np.float64), K, np.float64)
        assert np.array_equal(t32.astype(np.float64), t64)
        tp32, tp64 = po.taps(t32, shape), po.taps(t64, shape, np.float64)
        assert np.array_equal(tp32["w"].astype(np.float64), tp64["w"])
        s32, _ = po.samples(rig["v"], tp32, np.float32)
        s64, _ = po.samples(rig["v"], tp64)
        assert np.array_equal(s32.astype(np.float64), s64)


# ---- the exponent of the fixed-point accumulator
def test_exponent_leaves_two_bits_and_poisons_non_finite_rows():
    rng = np.random.default_rng(0)
    B, V, C, ms, K, n_vox = 2, 2, 3, (5, 9), 3, 105
    N = V * ms[0] * ms[1] * K
    for method in po.METHODS:
        for scale in (1e-30, 1.0, 3e7, 1e30):
            g = (rng.normal(size=(B, V, C) + ms) * scale).astype(np.float32)
            v = rng.normal(size=(B, C, n_vox)).astype(np.float32) * 5
            g[1, :, 2] = 0.0
            g[0, 1, 1, 2, 3] = np.inf
            E = po.exponents(g, v, method, K, N, beta=-2.5)
            assert E[0, 1] == po.POISON and E[1, 2] == 0
            for b, c in ((0, 0), (0, 2), (1, 0), (1, 1)):
                gm, F = float(np.abs(g[b, :, c]).max()), float(np.abs(v[b, c]).max())
                bound = gm / K if method == "mean" else gm if method == "max" else gm * (1 + 2 * 2.5 * F)
                total = N * bound * 2.0 ** int(E[b, c])
                assert 2.0 ** 60 / 2 <= total < 2.0 ** 62, (method, scale, total)
    v = np.ones((1, 1, 8), np.float32)
    v[0, 0, 3] = np.nan
    g = np.ones((1, 1, 1, 2, 2), np.float32)
    assert po.exponents(g, v, "softmax", 4, 16)[0, 0] == po.POISON and po.exponents(g, v, "mean", 4, 16)[0, 0] != po.POISON
    assert po.exponents(g * np.float32(3e38), np.full((1, 1, 8), 3e38, np.float32), "softmax", 4, 16)[0, 0] == po.POISON   # the bound overflows fp32


def test_workspace_is_the_tables_and_one_pass_of_channels_within_a_gibibyte():
    L = _capi.lib()
    assert L.mvhmr_project_volume_max_samples() == po.MAX_SAMPLES == volproject.MAX_SAMPLES
    tables = lambda B, C: -(-B * C * 12 // 256) * 256
    assert L.mvhmr_project_volume_workspace_bytes(2, 3, 3, 5, 7) == tables(2, 3) + 2 * 3 * 105 * 8
    big = L.mvhmr_project_volume_workspace_bytes(32, 17, 64, 64, 64)             # 64 MiB per channel: 15 of 17 fit beside the tables
    assert big == tables(32, 17) + 15 * 32 * 64 ** 3 * 8 and big <= 2 ** 30
    assert L.mvhmr_project_volume_workspace_bytes(32, 1, 256, 256, 256) == tables(32, 1) + 32 * 256 ** 3 * 8      # one channel needs more: granted
    assert L.mvhmr_project_volume_workspace_bytes(0, 3, 3, 5, 7) == 0 and L.mvhmr_project_volume_workspace_bytes(2, 3, 1, 5, 7) == 0


# ---- refusals
def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype)


def test_python_refusals():
    v, rays, rot, cen = _meta(2, 5, 3, 5, 7), _meta(2, 4, 3, 4), _meta(2, 3, 3), _meta(2, 3)
    pos, sides = [0, 0, 0], [1, 1, 1]
    f = volproject.project_volume_cuboid
    with pytest.raises(ValueError, match="method"):
        f(v, rays, rot, cen, pos, sides, (6, 9), 8, "sum")
    for n in (0, 1025, 2.0, True):
        with pytest.raises(ValueError, match="n_samples"):
            f(v, rays, rot, cen, pos, sides, (6, 9), n)
    with pytest.raises(ValueError, match="2\\^31"):
        f(v, rays, rot, cen, pos, sides, (1 << 10, 1 << 10), 1024)
    for bad in (_meta(2, 5, 1, 5, 7), _meta(2, 5, 3, 1, 7), _meta(2, 5, 3, 5, 1)):
        with pytest.raises(ValueError, match="extent"):
            f(bad, rays, rot, cen, pos, sides, (6, 9), 8)
    with pytest.raises(ValueError):
        f(_meta(2, 0, 3, 5, 7), rays, rot, cen, pos, sides, (6, 9), 8)
    with pytest.raises(ValueError):
        f(_meta(5, 3, 5, 7), rays, rot, cen, pos, sides, (6, 9), 8)
    with pytest.raises(TypeError):
        f(_meta(2, 5, 3, 5, 7, dtype=torch.float64), rays, rot, cen, pos, sides, (6, 9), 8)
    with pytest.raises(TypeError):
        f(v, None, rot, cen, pos, sides, (6, 9), 8)
    for kw in (dict(rays=_meta(2, 4, 4, 3)), dict(rays=_meta(3, 4, 3, 4)), dict(rot=_meta(2, 3)), dict(cen=_meta(3, 3))):
        a = dict(dict(rays=rays, rot=rot, cen=cen), **kw)
        with pytest.raises(ValueError, match="must be"):
            f(v, a["rays"], a["rot"], a["cen"], pos, sides, (6, 9), 8)
    for kw in (dict(beta=0.0), dict(beta=float("nan")), dict(beta=1e-60), dict(beta=float("inf"))):
        with pytest.raises(ValueError, match="beta"):
            f(v, rays, rot, cen, pos, sides, (6, 9), 8, "softmax", **kw)
    for kw in (dict(min_depth=float("nan")), dict(min_depth=float("-inf")), dict(max_depth=float("nan")), dict(max_depth="far")):
        with pytest.raises(ValueError, match="depth"):
            f(v, rays, rot, cen, pos, sides, (6, 9), 8, **kw)
    for bad_map in ((6,), 9, (6, -1)):
        with pytest.raises(ValueError, match="map_shape"):
            f(v, rays, rot, cen, pos, sides, bad_map, 8)
    with pytest.raises(ValueError, match="3 finite"):
        f(v, rays, rot, cen, [0, 0], sides, (6, 9), 8)
    # differentiable w.r.t. volumes only
    for which in range(3):
        args = [_meta(2, 4, 3, 4), _meta(2, 3, 3), _meta(2, 3)]
        args[which].requires_grad_(True)
        with pytest.raises(ValueError, match="requires grad"):
            f(v, *args, pos, sides, (6, 9), 8)
    # no fallback: CPU tensors raise
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(torch.zeros(2, 5, 3, 5, 7), torch.zeros(2, 4, 3, 4), torch.zeros(2, 3, 3), torch.zeros(2, 3), pos, sides, (6, 9), 8)


def test_empty_maps_return_without_a_launch():
    v, rot, cen = _meta(2, 5, 3, 5, 7), _meta(2, 3, 3), _meta(2, 3)
    for rays, ms, want in ((_meta(2, 4, 3, 4), (0, 9), (2, 4, 5, 0, 9)), (_meta(2, 4, 3, 4), (6, 0), (2, 4, 5, 6, 0)), (_meta(2, 0, 3, 4), (6, 9), (2, 0, 5, 6, 9))):
        maps, ranges = volproject.project_volume_cuboid(v, rays, rot, cen, [0, 0, 0], [1, 1, 1], ms, 8, return_ranges=True)
        assert tuple(maps.shape) == want and tuple(ranges.shape) == (2, want[1], ms[0], ms[1], 2) and maps.dtype == ranges.dtype == torch.float32


def test_c_layer_refusals():
    L = _capi.lib()
    d3 = (ctypes.c_double * 3)
    pos, sides = d3(0, 0, 0), d3(1, 1, 1)
    p = ctypes.c_void_p(256)                                                     # never dereferenced: every call below is refused first
    INVALID, WORKSPACE = _capi.ERR_INVALID_ARGUMENT, _capi.ERR_WORKSPACE
    good = (2, 4, 5, 3, 5, 7, 6, 9, 8)                                           # B, V, C, X, Y, Z, Hm, Wm, K
    need = L.mvhmr_project_volume_workspace_bytes(2, 5, 3, 5, 7)

    def fwd(volumes=p, dtype=_capi.F32, rays=p, rot=p, center=p, position=pos, side=sides, sizes=good, method=0, beta=1.0, dmin=0.0, dmax=float("inf"),
            maps=p, ranges=p, aux=p):
        return L.mvhmr_project_volume_forward(volumes, dtype, rays, rot, center, position, side, *sizes, method, beta, dmin, dmax, maps, ranges, aux, None)

    def bwd(volumes=p, dtype=_capi.F32, rays=p, rot=p, center=p, sizes=good, method=0, beta=1.0, dmin=0.0, dmax=float("inf"), g=p, maps=p, aux=p, gv=p,
            ws=p, ws_bytes=need):
        return L.mvhmr_project_volume_backward_volumes(volumes, dtype, rays, rot, center, pos, sides, *sizes, method, beta, dmin, dmax, g, maps, aux, gv,
                                                       ws, ws_bytes, None)

    for kw in (dict(volumes=None), dict(rays=None), dict(rot=None), dict(center=None), dict(position=None), dict(side=None), dict(maps=None),
               dict(ranges=None), dict(dtype=7), dict(dtype=-1), dict(method=3), dict(method=-1), dict(method=1, aux=None), dict(method=2, aux=None),
               dict(method=2, beta=0.0), dict(method=2, beta=float("nan")), dict(dmin=float("nan")), dict(dmin=float("-inf")), dict(dmax=float("nan"))):
        assert fwd(**kw) == INVALID, kw
    assert fwd(method=0, aux=None, volumes=None) == INVALID                      # (mean needs no aux: refused for the volume alone)
    bad_sizes = [(0,) + good[1:], (2, 0) + good[2:], (2, 4, 0) + good[3:], (2, 4, 5, 1, 5, 7, 6, 9, 8), (2, 4, 5, 3, 1, 7, 6, 9, 8), (2, 4, 5, 3, 5, 1, 6, 9, 8),
                 (2, 4, 5, 3, 5, 7, 0, 9, 8), (2, 4, 5, 3, 5, 7, 6, 0, 8), (2, 4, 5, 3, 5, 7, 6, 9, 0), (2, 4, 5, 3, 5, 7, 6, 9, 1025),
                 (2, 4, 5, 2048, 2048, 512, 6, 9, 8), (2, 4, 5, 3, 5, 7, 1 << 10, 1 << 10, 1024), (1 << 12, 1 << 10, 1 << 10, 3, 5, 7, 6, 9, 8)]
    for sizes in bad_sizes:
        assert fwd(sizes=sizes) == INVALID and bwd(sizes=sizes) == INVALID, sizes
    assert fwd(sizes=bad_sizes[9]) == INVALID and b"n_samples must be 1 .. 1024" in L.mvhmr_last_error()
    for kw in (dict(volumes=None), dict(rays=None), dict(g=None), dict(gv=None), dict(dtype=3), dict(method=1, aux=None), dict(method=2, maps=None)):
        assert bwd(**kw) == INVALID, kw
    for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws=ctypes.c_void_p(264)), dict(ws_bytes=0)):
        assert bwd(**kw) == WORKSPACE, kw
        assert b"workspace" in L.mvhmr_last_error()


# ---- tracing
def test_fake_shapes_and_one_node_under_fake_tensor_mode():
    pos, sides = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        v, rays, rot, cen = _meta(2, 5, 3, 5, 7, dtype=dt), _meta(2, 4, 3, 4), _meta(2, 3, 3), _meta(2, 3)
        for m, method in enumerate(po.METHODS):
            maps, ranges = volproject.project_volume_cuboid(v, rays, rot, cen, pos, sides, (6, 9), 8, method, return_ranges=True)
            assert (tuple(maps.shape), maps.dtype, tuple(ranges.shape), ranges.dtype) == ((2, 4, 5, 6, 9), torch.float32, (2, 4, 6, 9, 2), torch.float32)
            _, _, aux = torch.ops.mvhmr.project_volume_cuboid(v, rays, rot, cen, pos, sides, 6, 9, 8, m, 1.0, 0.0, float("inf"))
            assert (aux.numel(), aux.dtype) == ((0, torch.float32), (2 * 4 * 5 * 6 * 9, torch.int32), (2 * 4 * 5 * 6 * 9, torch.float32))[m]
            gv = torch.ops.mvhmr.project_volume_backward_volumes(v, rays, rot, cen, pos, sides, 6, 9, 8, m, 1.0, 0.0, float("inf"), maps, maps, aux)
            assert tuple(gv.shape) == tuple(v.shape) and gv.dtype == dt
    from torch.fx.experimental.proxy_tensor import make_fx

    def fn(v, rays, rot, cen):
        return volproject.project_volume_cuboid(v, rays, rot, cen, pos, sides, (6, 9), 8, "softmax", beta=2.0)

    graph = make_fx(fn, tracing_mode="fake")(_meta(2, 5, 3, 5, 7), _meta(2, 4, 3, 4), _meta(2, 3, 3), _meta(2, 3))
    nodes = [n for n in graph.graph.nodes if n.op == "call_function" and "mvhmr" in str(n.target)]
    assert [str(n.target) for n in nodes] == ["mvhmr.project_volume_cuboid.default"]


@pytest.mark.parametrize("method", po.METHODS)
def test_forward_and_backward_trace_and_compile_with_the_ranges_returned(method):
    """a traced backward is handed a tangent for every output, ranges included: it is dropped, not refused; the forward graph holds the one
    op, the backward graph the one backward op, and the volume alone gets a gradient"""
    from functorch.compile import aot_function, make_boxed_func
    pos, sides = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    def fn(v, rays, rot, cen):
        return volproject.project_volume_cuboid(v, rays, rot, cen, pos, sides, (6, 9), 8, method, return_ranges=True)

    def inputs():
        return [_meta(2, 5, 3, 5, 7).requires_grad_(True), _meta(2, 4, 3, 4), _meta(2, 3, 3), _meta(2, 3)]

    seen = {}

    def keep(name):
        def compiler(gm, example_inputs):
            seen[name] = [str(n.target) for n in gm.graph.nodes if n.op == "call_function" and "project_volume" in str(n.target)]
            return make_boxed_func(gm.forward)
        return compiler

    args = inputs()
    maps, ranges = aot_function(fn, fw_compiler=keep("fw"), bw_compiler=keep("bw"))(*args)
    (maps.sum() + ranges.sum()).backward()
    assert seen["fw"] == ["mvhmr.project_volume_cuboid.default"] and seen["bw"] == ["mvhmr.project_volume_backward_volumes.default"]
    assert args[0].grad is not None and args[0].grad.shape == args[0].shape
    args = inputs()
    maps, ranges = torch.compile(fn, backend="aot_eager", fullgraph=True)(*args)
    (maps.sum() + 2.0 * ranges.sum()).backward()
    assert args[0].grad is not None and args[0].grad.shape == args[0].shape


def test_opcheck_of_the_fake_implementation():
    v, rays, rot, cen = _meta(2, 5, 3, 5, 7), _meta(2, 4, 3, 4), _meta(2, 3, 3), _meta(2, 3)
    torch.library.opcheck(torch.ops.mvhmr.project_volume_cuboid, (v, rays, rot, cen, [0.0] * 3, [1.0] * 3, 6, 9, 8, 2, 1.0, 0.0, float("inf")),
                          test_utils=("test_schema",))


def test_volume_generator_project_uses_the_modules_cuboid():
    from unittest import mock
    with mock.patch.object(aggregation.VolumeGenerator, "to", lambda self, *a, **k: self):   # no HIP device here
        gen = aggregation.VolumeGenerator(volume_size=4, input_channels=4, output_channels=4)
    seen = {}

    def stub(volumes, rays, rotations, centers, position, sides, map_shape, n_samples, method, **kw):
        seen.update(position=tuple(position), sides=tuple(sides), rest=(map_shape, n_samples, method), kw=kw)
        return "result"

    with mock.patch.object(volproject, "project_volume_cuboid", stub):
        assert gen.project(1, 2, 3, 4, (6, 9), 8, "max", return_ranges=True) == "result"
    cub = gen.cuboid()
    assert seen["position"] == tuple(cub.position) and seen["sides"] == tuple(cub.sides)
    assert seen["rest"] == ((6, 9), 8, "max") and seen["kw"] == dict(return_ranges=True)


# ---- the header
def test_the_header_still_says_abi_4_and_declares_the_entry_points():
    text = open(HEADER).read()
    assert re.search(r"#define MVHMR_ABI_VERSION 4\b", text) and _capi.ABI_VERSION == 4
    for name in ("mvhmr_project_volume_forward", "mvhmr_project_volume_backward_volumes", "mvhmr_project_volume_workspace_bytes",
                 "mvhmr_project_volume_max_samples", "mvhmr_project_volume_channel_group"):
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _capi.EXPORTS and hasattr(_capi.lib(), name)
    assert [m for m in re.findall(r"MVHMR_PROJECT_(\w+) = (\d)", text)] == [("MEAN", "0"), ("MAX", "1"), ("SOFTMAX", "2")]
    assert volproject.METHODS == po.METHODS == ("mean", "max", "softmax")
    import multiviewhmr_amd
    assert multiviewhmr_amd.project_volume_cuboid is volproject.project_volume_cuboid and multiviewhmr_amd.camera_rays is volproject.camera_rays
