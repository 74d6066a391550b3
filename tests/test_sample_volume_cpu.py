"""Trilinear volume sampling without a device (multiviewhmr_amd/volsample.py): the oracle against the 5-D grid_sample and
autograd in float64, paired against the diagonal, the (voxel, point) order and chunking of the numpy emulation on the exact rig, every
refusal of the Python and C layers, the size queries, and the fake-tensor shapes."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import volsample_oracle as vo
from multiviewhmr_amd import _capi, aggregation, volsample

SHAPE = (3, 5, 7)
# S - 1 a power of two on every axis: grid_sample's normalise / un-normalise round trip is then exact for the rig's quarter fractions, so at a
# node (where the slope jumps) it picks the same cell, floor(t), as the contract
SHAPE_P2 = (3, 5, 9)


def _grid_sample_reference(pr, shape, paired=False):
    """the composition a caller writes today, in float64 with autograd: R^T (x - c) + c, normalised to [-1, 1], flipped to (z, y, x)"""
    B, C = pr["v"].shape[:2]
    S = torch.tensor(shape, dtype=torch.float64)
    vol = torch.tensor(pr["v"], dtype=torch.float64).view(B, C, *shape).requires_grad_(True)
    x = torch.tensor(np.asarray(pr["points"], np.float64)).requires_grad_(True)
    R = torch.tensor(np.asarray(pr["rot"], np.float64)).requires_grad_(True)
    c = torch.tensor(np.asarray(pr["centers"], np.float64)).requires_grad_(True)
    pos = torch.tensor(pr["position"], dtype=torch.float64)
    step = torch.tensor(vo.steps(pr["sides"], shape).astype(np.float64))
    d = torch.einsum("bia,bni->bna", R, x - c[:, None])
    t = (d + (c[:, None] - pos)) / step
    grid = (2 * t / (S - 1) - 1).flip(-1)[:, None, None]
    out = F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, :, 0, 0]
    if paired:
        out = torch.diagonal(out, dim1=1, dim2=2)
    (out * torch.tensor(pr["g"], dtype=torch.float64)).sum().backward()
    return {"t": t.detach().numpy(), "out": out.detach().numpy(), "grad_v": vol.grad.view(B, C, -1).numpy(), "grad_points": x.grad.numpy(),
            "grad_rot": R.grad.numpy(), "grad_center": c.grad.numpy()}


def _float64_problem(seed, B, C, N, paired=False, shape=SHAPE):
    """points outside, on faces and on nodes included, every number one the fp32 contract represents exactly: the exact rig with generic
    volume values.  Two of its points are moved: the NaN point (autograd has no rule for it), and t = -1 exactly, where the contract's point
    is dead while grid_sample's backward still sees the slope towards voxel 0 (its forward is 0 there as well)."""
    rig = vo.exact_rig(seed, B, C, shape, N, paired=paired)
    rng = np.random.default_rng(seed)
    rig["tt"][np.isnan(rig["tt"]).any(-1)] = 1.25
    rig["tt"][rig["tt"] == -1.0] = -1.25
    rig["points"] = vo.world_points(rig["tt"], rig["rot"], rig["centers"], rig["position"], rig["sides"], shape)
    rig["v"] = rng.normal(size=rig["v"].shape)
    rig["g"] = rng.normal(size=rig["g"].shape)
    return rig


@pytest.mark.parametrize("paired", [False, True])
def test_oracle_equals_grid_sample_and_autograd_in_float64(paired):
    B, C, N = 2, 17, 17 if paired else 70
    SHAPE = SHAPE_P2
    pr = _float64_problem(3, B, C, N, paired, SHAPE)
    ref = _grid_sample_reference(pr, SHAPE, paired)
    t = vo.index_fp32(pr["points"], pr["rot"], pr["centers"], pr["position"], pr["sides"], SHAPE)
    assert np.array_equal(t.astype(np.float64), ref["t"])                       # the rig: the fp32 index IS the float64 one
    tp = vo.taps(t, SHAPE)
    assert (~tp["live"]).any() and (tp["w"][tp["live"]] == 0).any() and (tp["live"][..., None] & ~tp["inside"]).any()   # outside, nodes, half-in cells
    out, _ = vo.forward(pr["v"], t, SHAPE, paired)
    bw = vo.backward(pr["v"], t, pr["points"], pr["rot"], pr["centers"], pr["sides"], SHAPE, pr["g"], paired)
    for name, got, want in (("forward", out, ref["out"]), ("grad_volumes", bw["grad_v"], ref["grad_v"]), ("grad_points", bw["grad_points"], ref["grad_points"]),
                            ("grad_rot", bw["grad_rot"], ref["grad_rot"]), ("grad_center", bw["grad_center"], ref["grad_center"])):
        scale = max(1.0, float(np.abs(want).max()))
        assert np.abs(got - want).max() <= 1e-12 * scale, (name, float(np.abs(got - want).max()))


def test_paired_is_the_diagonal_of_the_full_call():
    pr = _float64_problem(4, 2, 17, 17)
    t = vo.index_fp32(pr["points"], pr["rot"], pr["centers"], pr["position"], pr["sides"], SHAPE)
    full, _ = vo.forward(pr["v"], t, SHAPE)
    pair, _ = vo.forward(pr["v"], t, SHAPE, paired=True)
    assert np.array_equal(pair, np.diagonal(full, axis1=1, axis2=2))
    g = np.random.default_rng(0).normal(size=(2, 17))
    gfull = np.zeros((2, 17, 17))
    gfull[:, np.arange(17), np.arange(17)] = g
    a = vo.backward(pr["v"], t, pr["points"], pr["rot"], pr["centers"], pr["sides"], SHAPE, gfull)
    b = vo.backward(pr["v"], t, pr["points"], pr["rot"], pr["centers"], pr["sides"], SHAPE, g, paired=True)
    for k in ("grad_v", "grad_points", "grad_rot", "grad_center"):
        assert np.allclose(a[k], b[k], rtol=0, atol=1e-12), k


def test_a_node_between_minus_infinity_returns_the_node():
    v = np.full((1, 1, int(np.prod(SHAPE))), -np.inf)
    node = (1 * SHAPE[1] + 2) * SHAPE[2] + 3
    v[0, 0, node] = 0.75
    out, _ = vo.forward(v, np.array([[[1.0, 2.0, 3.0]]], np.float32), SHAPE)
    assert out[0, 0, 0] == 0.75


def test_fma32_rounds_once():
    """a case the plain float64 sum double-rounds: 1 + 2^-24 + 2^-53-ish"""
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -30)
    exact = float(a) * float(b) + float(c)                                       # 1 + 2^-11 + 2^-24 + 2^-30: above the tie
    assert vo.fma32(a, b, c) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23) and np.float32(exact) == vo.fma32(a, b, c)
    rng = np.random.default_rng(1)
    x, y, z = (rng.normal(size=4096).astype(np.float32) for _ in range(3))
    from fractions import Fraction
    got = vo.fma32(x, y, z)
    for i in range(0, 4096, 64):
        want = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(Fraction(float(got[i])) - want) <= min(abs(Fraction(float(lo)) - want), abs(Fraction(float(hi)) - want))


# ---- the documented order of the volume gradient
@pytest.mark.parametrize("case", [(2, 5, (3, 5, 7), 70, None), (2, 2, (4, 4, 8), vo.CHUNK + 3, (0, vo.CHUNK + 2)), (1, 3, (2, 2, 2), 1, None)],
                         ids=["n70", "chunk_boundary", "minimum"])
def test_emulated_order_and_chunking_reproduce_the_oracle_on_the_exact_rig(case):
    B, C, shape, N, dup = case
    rig = vo.exact_rig(11, B, C, shape, N, duplicate=dup)
    vo.assert_rig_premises(rig, shape)
    t = vo.index_fp32(rig["points"], rig["rot"], rig["centers"], rig["position"], rig["sides"], shape)
    assert np.array_equal(t.astype(np.float64), rig["tt"], equal_nan=True)
    bw = vo.backward(rig["v"], t, rig["points"], rig["rot"], rig["centers"], rig["sides"], shape, rig["g"])
    vo.assert_exact_sums(bw)
    for chunk in (vo.CHUNK, 7, 1):                                               # exact arithmetic: any chunking gives the same bits
        em = vo.emulate_grad_volumes(t, rig["g"], shape, C, chunk=chunk)
        assert np.array_equal(em.astype(np.float64), bw["grad_v"]), chunk
    if dup:                                                                      # one voxel owned in two launches
        tp = vo.taps(t, shape)
        assert set(tp["vox"][0, dup[0]][tp["inside"][0, dup[0]]]) == set(tp["vox"][0, dup[1]][tp["inside"][0, dup[1]]]) and dup[1] // vo.CHUNK == 1
    assert bw["count"].max() >= (40 if N >= 60 else 1)                           # the collisions are there


def test_emulated_order_stays_within_the_bound_on_general_inputs():
    worst = 0.0
    for seed in range(6):
        B, C, shape, N = 2, 3, (4, 4, 8), vo.CHUNK + 3
        pr = vo.general_problem(50 + seed, B, C, shape, N, duplicate=(0, N - 1))
        t = vo.index_fp32(pr["points"], pr["rot"], pr["centers"], pr["position"], pr["sides"], shape)
        bw = vo.backward(pr["v"], t, pr["points"], pr["rot"], pr["centers"], pr["sides"], shape, pr["g"].astype(np.float32))
        for store_name, dt in (("float32", None), ("bfloat16", torch.bfloat16), ("float16", torch.float16)):
            store = (lambda x: x) if dt is None else (lambda x, dt=dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).float().numpy())
            em = vo.emulate_grad_volumes(t, pr["g"], shape, C, store=store)
            bound = vo.bound_grad_volumes(bw["mag_v"], bw["count"], N, store_name)
            err = np.abs(em.astype(np.float64) - bw["grad_v"])
            assert (err <= bound).all(), (seed, store_name)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    assert 0.0 < worst < 1.0


# ---- sizes
def test_chunk_points_and_workspace_bytes_are_functions_of_the_sizes_alone():
    L = _capi.lib()
    P = L.mvhmr_sample_volume_chunk_points()
    assert P == vo.CHUNK == L.mvhmr_sample_volume_chunk_points()
    table = L.mvhmr_sample_volume_workspace_bytes(1, 1)
    assert table >= P * 8 * 8 and table % 16 == 0
    for B, N in ((1, 1), (1, P), (1, P + 1), (3, 2 * P), (32, 1024), (2, P + 3)):
        want = B * -(-N // P) * table
        assert L.mvhmr_sample_volume_workspace_bytes(B, N) == want == L.mvhmr_sample_volume_workspace_bytes(B, N)
        assert want >= B * N * 16                                                # the geometry gradient's (B, N, 4) floats fit
    assert L.mvhmr_sample_volume_workspace_bytes(0, 5) == 0 and L.mvhmr_sample_volume_workspace_bytes(5, 0) == 0
    assert L.mvhmr_sample_volume_workspace_bytes(-1, 5) == 0


# ---- refusals
def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype)


def test_python_refusals():
    v, p, rot, cen = _meta(2, 5, 3, 5, 7), _meta(2, 9, 3), _meta(2, 3, 3), _meta(2, 3)
    pos, sides = [0, 0, 0], [1, 1, 1]
    f = volsample.sample_volume_cuboid
    with pytest.raises(TypeError, match="volumes must be a tensor"):
        f(np.zeros((2, 5, 3, 5, 7), np.float32), p, rot, cen, pos, sides)
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        f(v.double(), p, rot, cen, pos, sides)
    with pytest.raises(TypeError, match="points must be a tensor"):
        f(v, [[0, 0, 0]], rot, cen, pos, sides)
    with pytest.raises(ValueError, match=r"\(B, C, X, Y, Z\)"):
        f(v[0], p, rot, cen, pos, sides)
    for bad in (_meta(2, 5, 1, 5, 7), _meta(2, 5, 3, 1, 7), _meta(2, 5, 3, 5, 1)):
        with pytest.raises(ValueError, match="every extent must be >= 2"):
            f(bad, p, rot, cen, pos, sides)
    with pytest.raises(ValueError, match="must not be empty"):
        f(_meta(2, 0, 3, 5, 7), p, rot, cen, pos, sides)
    with pytest.raises(ValueError, match="points must be"):
        f(v, p[:1], rot, cen, pos, sides)
    with pytest.raises(ValueError, match="points must be"):
        f(v, p[..., :2], rot, cen, pos, sides)
    with pytest.raises(ValueError, match="points must be"):
        f(v, p[0], rot, cen, pos, sides)
    with pytest.raises(ValueError, match="rotations must be"):
        f(v, p, rot[:1], cen, pos, sides)
    with pytest.raises(ValueError, match="centers must be"):
        f(v, p, rot, cen[:, :2], pos, sides)
    with pytest.raises(ValueError, match="needs N == C"):
        f(v, p, rot, cen, pos, sides, paired=True)
    with pytest.raises(ValueError, match="sides takes 3"):
        f(v, p, rot, cen, pos, [1, 1])
    with pytest.raises(ValueError, match="position takes 3"):
        f(v, p, rot, cen, [0, 0, float("nan")], sides)
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(torch.zeros(1, 1, 2, 2, 2), torch.zeros(1, 1, 3), torch.eye(3)[None], torch.zeros(1, 3), pos, sides)
    with pytest.raises(ValueError, match="beta"):
        volsample.volumetric_cross_entropy(v, _meta(2, 5, 3), rot, cen, pos, sides, beta=float("nan"))


def test_no_points_return_empty_results_without_a_launch():
    v = _meta(2, 5, 3, 5, 7)
    out, idx = volsample.sample_volume_cuboid(v, _meta(2, 0, 3), _meta(2, 3, 3), _meta(2, 3), [0, 0, 0], [1, 1, 1], return_index=True)
    assert tuple(out.shape) == (2, 5, 0) and tuple(idx.shape) == (2, 0, 3) and out.dtype == idx.dtype == torch.float32


def test_c_layer_refusals():
    L = _capi.lib()
    d3 = (ctypes.c_double * 3)
    pos, sides = d3(0, 0, 0), d3(1, 1, 1)
    p = ctypes.c_void_p(256)                                                     # never dereferenced: every call below is refused first
    P = L.mvhmr_sample_volume_chunk_points()
    need = L.mvhmr_sample_volume_workspace_bytes(2, P + 3)
    INVALID, WORKSPACE = _capi.ERR_INVALID_ARGUMENT, _capi.ERR_WORKSPACE

    def fwd(volumes=p, dtype=_capi.F32, points=p, rot=p, center=p, position=pos, side=sides, sizes=(2, 5, 3, 5, 7, P + 3, 0), samples=p, index=p):
        return L.mvhmr_sample_volume_forward(volumes, dtype, points, rot, center, position, side, *sizes, samples, index, None)

    def bwd_v(dtype=_capi.F32, index=p, g=p, sizes=(2, 5, 3, 5, 7, P + 3, 0), gv=p, ws=p, ws_bytes=need):
        return L.mvhmr_sample_volume_backward_volumes(dtype, index, g, *sizes, gv, ws, ws_bytes, None)

    def bwd_g(volumes=p, dtype=_capi.F32, points=p, rot=p, center=p, sizes=(2, 5, 3, 5, 7, P + 3, 0), index=p, g=p, gp=p, gr=p, gc=p, ws=p,
              ws_bytes=need):
        return L.mvhmr_sample_volume_backward_geometry(volumes, dtype, points, rot, center, pos, sides, *sizes, index, g, gp, gr, gc, ws, ws_bytes, None)

    for kw in (dict(volumes=None), dict(points=None), dict(rot=None), dict(center=None), dict(position=None), dict(side=None), dict(samples=None),
               dict(index=None), dict(dtype=7), dict(dtype=-1)):
        assert fwd(**kw) == INVALID, kw
    bad_sizes = [(0, 5, 3, 5, 7, 9, 0), (2, 0, 3, 5, 7, 9, 0), (2, 5, 3, 5, 7, 0, 0), (2, 5, 1, 5, 7, 9, 0), (2, 5, 3, 1, 7, 9, 0), (2, 5, 3, 5, 1, 9, 0),
                 (2, 5, 2048, 2048, 512, 9, 0), (2, 5, 3, 5, 7, 9, 1), (2, 5, 3, 5, 7, 9, 2), (1 << 16, 1 << 16, 3, 5, 7, 9, 0), (1 << 16, 5, 3, 5, 7, 1 << 16, 0)]
    for sizes in bad_sizes:
        assert fwd(sizes=sizes) == INVALID and bwd_v(sizes=sizes) == INVALID and bwd_g(sizes=sizes) == INVALID, sizes
    for kw in (dict(index=None), dict(g=None), dict(gv=None), dict(dtype=3)):
        assert bwd_v(**kw) == INVALID, kw
    for kw in (dict(volumes=None), dict(points=None), dict(rot=None), dict(center=None), dict(index=None), dict(g=None), dict(gp=None, gr=None, gc=None)):
        assert bwd_g(**kw) == INVALID, kw
    for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws=ctypes.c_void_p(264)), dict(ws_bytes=0)):
        assert bwd_v(**kw) == WORKSPACE and bwd_g(**kw) == WORKSPACE, kw
        assert b"workspace" in L.mvhmr_last_error()
    assert fwd(sizes=(2, 5, 3, 5, 7, 9, 1)) == INVALID and b"N == C" in L.mvhmr_last_error()      # the paired mismatch names itself
    assert fwd(sizes=(2, 5, 1, 5, 7, 9, 0)) == INVALID and b"every extent must be >= 2" in L.mvhmr_last_error()


# ---- tracing
def test_fake_shapes_and_one_node_under_fake_tensor_mode():
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        v, p, rot, cen = _meta(2, 5, 3, 5, 7, dtype=dt), _meta(2, 9, 3), _meta(2, 3, 3), _meta(2, 3)
        out, idx = volsample.sample_volume_cuboid(v, p, rot, cen, [0, 0, 0], [1, 1, 1], return_index=True)
        assert (tuple(out.shape), out.dtype, tuple(idx.shape), idx.dtype) == ((2, 5, 9), torch.float32, (2, 9, 3), torch.float32)
        out = volsample.sample_volume_cuboid(v, _meta(2, 5, 3), rot, cen, [0, 0, 0], [1, 1, 1], paired=True)
        assert tuple(out.shape) == (2, 5) and out.dtype == torch.float32
        gv = torch.ops.mvhmr.sample_volume_backward_volumes(v, idx, _meta(2, 5, 9), False)
        assert tuple(gv.shape) == tuple(v.shape) and gv.dtype == dt
        pos, sides = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
        gp, gr, gc = torch.ops.mvhmr.sample_volume_backward_geometry(v, p, rot, cen, pos, sides, False, idx, _meta(2, 5, 9), True, True)
        assert (tuple(gp.shape), tuple(gr.shape), tuple(gc.shape)) == ((2, 9, 3), (2, 3, 3), (2, 3))
        gp, gr, gc = torch.ops.mvhmr.sample_volume_backward_geometry(v, p, rot, cen, pos, sides, False, idx, _meta(2, 5, 9), False, True)
        assert gp.numel() == 0 and tuple(gr.shape) == (2, 3, 3)
        loss, idx = volsample.volumetric_cross_entropy(v, _meta(2, 5, 3), rot, cen, [0, 0, 0], [1, 1, 1], beta=2.0)
        assert tuple(loss.shape) == (2, 5) and tuple(idx.shape) == (2, 5, 3)
    from torch.fx.experimental.proxy_tensor import make_fx

    def fn(v, p, rot, cen):
        return volsample.sample_volume_cuboid(v, p, rot, cen, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0])

    graph = make_fx(fn, tracing_mode="fake")(torch.empty(2, 5, 3, 5, 7, device="meta"), torch.empty(2, 9, 3, device="meta"),
                                             torch.empty(2, 3, 3, device="meta"), torch.empty(2, 3, device="meta"))
    nodes = [n for n in graph.graph.nodes if n.op == "call_function" and "mvhmr" in str(n.target)]
    assert [str(n.target) for n in nodes] == ["mvhmr.sample_volume_cuboid.default"]


@pytest.mark.parametrize("which", ["sample_volume_cuboid", "volumetric_cross_entropy"])
def test_forward_and_backward_trace_and_compile_with_the_index_returned(which):
    """a traced backward is handed a tangent for every output that requires grad, index included: it must be dropped, not refused.  Forward
    + backward of both public functions through AOT autograd on meta tensors: the forward graph holds the one op, the backward graph the two
    backward ops, and every input gets a gradient of its own shape -- also when index itself reaches the loss"""
    from functorch.compile import aot_function, make_boxed_func
    pos, sides = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    N = 5 if which == "volumetric_cross_entropy" else 9

    def fn(v, p, rot, cen):
        if which == "volumetric_cross_entropy":
            return volsample.volumetric_cross_entropy(v, p, rot, cen, pos, sides, beta=2.0)
        return volsample.sample_volume_cuboid(v, p, rot, cen, pos, sides, return_index=True)

    def inputs():
        return [torch.empty(s, device="meta").requires_grad_(True) for s in ((2, 5, 3, 5, 7), (2, N, 3), (2, 3, 3), (2, 3))]

    seen = {}

    def keep(name):
        def compiler(gm, example_inputs):
            seen[name] = [str(n.target) for n in gm.graph.nodes if n.op == "call_function" and "sample_volume" in str(n.target)]
            return make_boxed_func(gm.forward)
        return compiler

    args = inputs()
    out, idx = aot_function(fn, fw_compiler=keep("fw"), bw_compiler=keep("bw"))(*args)
    assert tuple(idx.shape) == (2, N, 3) and tuple(out.shape) == ((2, 5) if which == "volumetric_cross_entropy" else (2, 5, N))
    (out.sum() + idx.sum()).backward()
    assert seen["fw"] == ["mvhmr.sample_volume_cuboid.default"]
    assert sorted(seen["bw"]) == ["mvhmr.sample_volume_backward_geometry.default", "mvhmr.sample_volume_backward_volumes.default"]
    assert all(a.grad is not None and a.grad.shape == a.shape for a in args)
    args = inputs()                                                             # ... and through torch.compile, as a training step would
    out, idx = torch.compile(fn, backend="aot_eager", fullgraph=True)(*args)
    (out.sum() + 2.0 * idx.sum()).backward()
    assert all(a.grad is not None and a.grad.shape == a.shape for a in args)
    args = inputs()                                                             # eager: arithmetic on index that reaches the loss
    out, idx = fn(*args)
    (out.sum() + idx.sum()).backward()
    assert all(a.grad is not None and a.grad.shape == a.shape for a in args)


def test_volume_generator_sample_uses_the_modules_cuboid():
    from unittest import mock
    with mock.patch.object(aggregation.VolumeGenerator, "to", lambda self, *a, **k: self):   # no HIP device here
        gen = aggregation.VolumeGenerator(volume_size=4, input_channels=4, output_channels=4)
    seen = {}

    def stub(volumes, points, rotations, centers, position, sides, **kw):
        seen.update(position=tuple(position), sides=tuple(sides), kw=kw)
        return "result"

    with mock.patch.object(volsample, "sample_volume_cuboid", stub):
        assert gen.sample(1, 2, 3, 4, paired=True, return_index=True) == "result"
    cub = gen.cuboid()
    assert seen["position"] == tuple(cub.position) and seen["sides"] == tuple(cub.sides) and seen["kw"] == dict(paired=True, return_index=True)
