"""Trilinear volume sampling at world points on the MI355X (multiviewhmr_amd/volsample.py, volume_sample.hip): bit equality with the float64
oracle on the exact rig, general inputs within the derived bounds (tests/volsample_oracle.py), the special values, bitwise
reproducibility, consistency with the rest of the package, graph capture and the raw C ABI.  Every error is asserted through
conftest.record_err, which also keeps it.  No point is left out of any comparison: the oracle takes the kernel's own index."""
import ctypes

import numpy as np
import pytest
import torch

import softargmax_oracle as so
import volsample_oracle as vo
from conftest import record_err
from multiviewhmr_amd import _capi, aggregation, volsample

pytestmark = pytest.mark.gpu

P = vo.CHUNK
# (B, C, volume, N, paired, duplicate): the minimum; odd extents with two lane tiles and a tail of 6; the chunk boundary, with point 0
# repeated at index P + 2 so that its voxels are owned in two launches; the paired route
BASE = [(1, 3, (2, 2, 2), 1, False, None), (2, 5, (3, 5, 7), 70, False, None), (2, 2, (4, 4, 8), P + 3, False, (0, P + 2)), (2, 17, (4, 4, 8), 17, True, None)]
# one channel count on each side of the forward's unroll boundary (vo.UNROLL = 4 channels per loop trip: 3, 4, 5) and of its channel-group
# boundary (vo.GROUP = 32 channels per block, which is also the volume-gradient sum's group: 31, 32, 33)
EDGE_CHANNELS = [vo.UNROLL - 1, vo.UNROLL, vo.UNROLL + 1, vo.GROUP - 1, vo.GROUP, vo.GROUP + 1]
EDGES = [(1, c, (3, 5, 7), 70, False, None) for c in EDGE_CHANNELS]
CASES = [(s, torch.float32) for s in BASE + EDGES] + [(s, dt) for s in (BASE[0], BASE[1], BASE[3]) for dt in (torch.float16, torch.bfloat16)]
IDS = ["b%dc%d_%s_n%d%s_%s" % (s[0], s[1], "x".join(map(str, s[2])), s[3], "_paired" if s[4] else "", str(dt)[6:]) for s, dt in CASES]


def _t(x, gpu, grad=False):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(gpu).requires_grad_(grad)


def _stored(v, dtype):
    """the values a volume of `dtype` holds, as float64 numpy"""
    return torch.from_numpy(np.ascontiguousarray(v)).to(dtype).double().numpy()


def _np(t):
    return t.detach().double().cpu().numpy()


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


def _run(gpu, pr, shape, dtype, paired, grad=(True, True, True, True)):
    """forward + backward through the public function -> dict of numpy results (float64 views of what the card wrote)"""
    B, C = pr["v"].shape[:2]
    vol = torch.from_numpy(np.ascontiguousarray(pr["v"])).to(dtype).view(B, C, *shape).to(gpu).requires_grad_(grad[0])
    pts, rot, cen = _t(pr["points"], gpu, grad[1]), _t(pr["rot"], gpu, grad[2]), _t(pr["centers"], gpu, grad[3])
    out, idx = volsample.sample_volume_cuboid(vol, pts, rot, cen, pr["position"], pr["sides"], paired=paired, return_index=True)
    assert out.dtype == idx.dtype == torch.float32 and tuple(idx.shape) == (B, pr["points"].shape[1], 3)
    if any(grad):
        (out * _t(pr["g"], gpu)).sum().backward()
    res = {"out": out.detach().cpu().numpy(), "index": idx.detach().cpu().numpy()}
    for name, leaf in (("grad_v", vol), ("grad_points", pts), ("grad_rot", rot), ("grad_center", cen)):
        res[name] = None if leaf.grad is None else leaf.grad.detach().float().cpu().numpy()
    if res["grad_v"] is not None:
        assert vol.grad.dtype == dtype
        res["grad_v"] = res["grad_v"].reshape(B, C, -1)
    return res


def test_the_library_chunks_as_the_oracle_assumes():
    assert _capi.lib().mvhmr_sample_volume_chunk_points() == P


# ------------------------------------------------------------------------------------ the exact rig: bits
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_rig_is_bit_equal_to_the_oracle(case, gpu):
    """on the rig every fp32 operation is exact, so index, samples and all four gradients must be the float64 oracle's values cast once
    (to fp32, then to the storage type for grad_volumes), collisions and the chunk boundary included"""
    (B, C, shape, N, paired, dup), dtype = case
    rig = vo.exact_rig(21, B, C, shape, N, paired=paired, duplicate=dup)
    vo.assert_rig_premises(rig, shape)
    assert np.array_equal(_stored(rig["v"], dtype), rig["v"])
    got = _run(gpu, rig, shape, dtype, paired)
    tag = "vs exact rig %s " % IDS[CASES.index(case)]
    _exact(tag + "index", got["index"], rig["tt"].astype(np.float32))
    t = got["index"]
    ref, _ = vo.forward(rig["v"], t, shape, paired)
    bw = vo.backward(rig["v"], t, rig["points"], rig["rot"], rig["centers"], rig["sides"], shape, rig["g"], paired)
    vo.assert_exact_sums(bw)
    for x in (ref, bw["grad_v"], bw["grad_points"], bw["grad_rot"], bw["grad_center"]):           # the oracle's values ARE fp32 numbers
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    _exact(tag + "samples", got["out"], ref.astype(np.float32))
    _exact(tag + "grad_volumes", got["grad_v"], torch.from_numpy(bw["grad_v"].astype(np.float32)).to(dtype).float().numpy())
    _exact(tag + "grad_points", got["grad_points"], bw["grad_points"].astype(np.float32))
    _exact(tag + "grad_rot", got["grad_rot"], bw["grad_rot"].astype(np.float32))
    _exact(tag + "grad_center", got["grad_center"], bw["grad_center"].astype(np.float32))
    if N >= 60:
        assert bw["count"].max() >= 40                                                              # the 40 identical points collide


# ------------------------------------------------------------------------------------ general inputs: the bounds
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_general_inputs_stay_within_the_bounds(case, gpu):
    """coordinates 3 to 13 m from the origin in millimetres, generic rotations; the float64 oracle on the kernel's own fp32 index, which in
    turn must be the contract's index bit for bit"""
    (B, C, shape, N, paired, dup), dtype = case
    pr = vo.general_problem(60 + B + C, B, C, shape, N, paired=paired, duplicate=dup)
    pr["v"], pr["g"] = _stored(pr["v"], dtype), pr["g"].astype(np.float32)
    got = _run(gpu, pr, shape, dtype, paired)
    tag = "vs general %s " % IDS[CASES.index(case)]
    _exact(tag + "index", got["index"], vo.index_fp32(pr["points"], pr["rot"], pr["centers"], pr["position"], pr["sides"], shape))
    t = got["index"]
    ref, mag = vo.forward(pr["v"], t, shape, paired)
    bw = vo.backward(pr["v"], t, pr["points"], pr["rot"], pr["centers"], pr["sides"], shape, pr["g"], paired)
    _hold(tag + "samples", got["out"], ref, vo.bound_forward(mag))
    _hold(tag + "grad_volumes", got["grad_v"], bw["grad_v"], vo.bound_grad_volumes(bw["mag_v"], bw["count"], N, str(dtype)[6:]))
    e_points, e_rot, e_center = vo.bound_geometry(bw, pr["rot"], pr["sides"], shape, 1 if paired else C)
    _hold(tag + "grad_points", got["grad_points"], bw["grad_points"], e_points)
    _hold(tag + "grad_rot", got["grad_rot"], bw["grad_rot"], e_rot)
    _hold(tag + "grad_center", got["grad_center"], bw["grad_center"], e_center)


# ------------------------------------------------------------------------------------ special values
def test_outside_and_nan_points_give_exact_zeros(gpu):
    B, C, shape, N = 2, 5, (3, 5, 7), 70
    pr = vo.general_problem(71, B, C, shape, N)
    got = _run(gpu, pr, shape, torch.float32, False)
    live = vo.taps(got["index"], shape)["live"]
    nan = np.isnan(pr["points"]).any(-1)
    assert nan.sum() == B and (~live & ~nan).sum() >= 2 * B                  # a NaN point and outside points on both sides are there
    assert np.isnan(got["index"][nan]).all() and np.isfinite(got["index"][~nan]).all()
    want = vo.index_fp32(pr["points"], pr["rot"], pr["centers"], pr["position"], pr["sides"], shape)
    _exact("vs special: index of outside points", got["index"][~live & ~nan], want[~live & ~nan])
    dead_out = np.moveaxis(got["out"], 2, 1)[~live]
    record_err("vs special: samples of dead points", float(np.abs(dead_out).max()) if not np.isnan(dead_out).any() else float("inf"), 0.0)
    dead_gp = got["grad_points"][~live]
    record_err("vs special: grad_points rows of dead points", float(np.abs(dead_gp).max()) if not np.isnan(dead_gp).any() else float("inf"), 0.0)
    assert np.isfinite(got["grad_rot"]).all() and np.isfinite(got["grad_center"]).all() and np.isfinite(got["grad_v"]).all()


def test_dead_points_contribute_to_no_gradient(gpu):
    """every gradient of a dead point is 0, for all four inputs: the same problem with its outside and NaN points taken out gives the same
    bits in grad_volumes, grad_rot and grad_center, and in the samples and grad_points rows of the points that stay (the sums skip dead
    points, so the live ones are added in the same order)"""
    C, shape, N = 5, (3, 5, 7), 70
    pr = vo.general_problem(72, 1, C, shape, N)
    pr["g"] = pr["g"].astype(np.float32)
    full = _run(gpu, pr, shape, torch.float32, False)
    live = vo.taps(full["index"], shape)["live"][0]
    assert 3 <= (~live).sum() < N and np.isnan(pr["points"][0, ~live]).any()
    part = _run(gpu, dict(pr, points=pr["points"][:, live], g=pr["g"][:, :, live]), shape, torch.float32, False)
    for name, a, b in (("grad_volumes", full["grad_v"], part["grad_v"]), ("grad_rot", full["grad_rot"], part["grad_rot"]),
                       ("grad_center", full["grad_center"], part["grad_center"]), ("samples", full["out"][:, :, live], part["out"]),
                       ("grad_points", full["grad_points"][:, live], part["grad_points"]), ("index", full["index"][:, live], part["index"])):
        _exact("vs special: without the dead points, " + name, a, b)
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
def test_a_node_between_minus_infinity_returns_the_node(dtype, gpu):
    shape = (3, 5, 7)
    rig = vo.exact_rig(5, 1, 2, shape, 1)
    nodes = np.array([[[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 0.0], [1.0, 2.0, 3.5]]])
    pts = vo.world_points(nodes, rig["rot"], rig["centers"], rig["position"], rig["sides"], shape)
    vol = torch.full((1, 2) + shape, -float("inf"), dtype=dtype, device=gpu)
    for c, (i, j, k) in enumerate(((1, 2, 3), (2, 4, 6))):
        vol[0, c, i, j, k] = 0.75 + c
    vol[0, 0, 0, 0, 0] = -3.0
    out = volsample.sample_volume_cuboid(vol, _t(pts, gpu), _t(rig["rot"], gpu), _t(rig["centers"], gpu), rig["position"], rig["sides"]).cpu().numpy()
    inf = -np.inf
    want = np.array([[[0.75, inf, -3.0, inf], [inf, 1.75, inf, inf]]], np.float32)              # the last point lies between two -inf voxels
    _exact("vs special: -inf neighbours %s" % str(dtype)[6:], out, want)


# ------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("deterministic", [False, True])
def test_two_runs_are_bitwise_identical(deterministic, gpu):
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(deterministic)
    try:
        for (B, C, shape, N, paired, dup), dtype in ((BASE[1], torch.float32), (BASE[2], torch.float32), (BASE[1], torch.bfloat16), (BASE[3], torch.float16)):
            pr = vo.general_problem(80, B, C, shape, N, paired=paired, duplicate=dup)
            a, b = (_run(gpu, pr, shape, dtype, paired) for _ in range(2))
            for key in a:
                assert a[key] is not None and np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
    finally:
        torch.use_deterministic_algorithms(prev)


def test_permuting_the_channels_permutes_samples_and_volume_gradient_bitwise(gpu):
    B, C, shape, N, _, _ = BASE[1]
    pr = vo.general_problem(81, B, C, shape, N)
    perm = np.array([3, 0, 4, 1, 2])
    a = _run(gpu, pr, shape, torch.float32, False)
    b = _run(gpu, dict(pr, v=pr["v"][:, perm], g=pr["g"][:, perm]), shape, torch.float32, False)
    for key in ("out", "grad_v"):
        assert np.array_equal(a[key][:, perm].view(np.uint32), b[key].view(np.uint32)), key
    assert np.array_equal(a["index"].view(np.uint32), b["index"].view(np.uint32))


def test_only_the_asked_gradients_are_computed(gpu):
    B, C, shape, N, _, _ = BASE[1]
    pr = vo.general_problem(82, B, C, shape, N)
    full = _run(gpu, pr, shape, torch.float32, False)
    names = ("grad_v", "grad_points", "grad_rot", "grad_center")
    for grad in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True), (False, True, False, True)):
        part = _run(gpu, pr, shape, torch.float32, False, grad=grad)
        for name, asked in zip(names, grad):
            assert (part[name] is not None) == asked
            if asked:
                assert np.array_equal(part[name].view(np.uint32), full[name].view(np.uint32)), (grad, name)


# ------------------------------------------------------------------------------------ consistency with the rest of the package
def test_sampling_a_volume_at_its_own_voxel_centres_returns_it(gpu):
    """the world coordinates mvhmr_build_coord_volumes gives, fed back as points: index = the voxel's own (i, j, k) to within the roundings of
    both directions (vo.bound_roundtrip_index), so the sample is the voxel's value to within that times the largest step to a neighbour"""
    B, C, S = 2, 3, 4
    shape = (S, S, S)
    pr = vo.general_problem(90, B, C, shape, 1)
    rot, cen = _t(pr["rot"], gpu), _t(pr["centers"], gpu)
    coords = torch.empty(B, S, S, S, 3, device=gpu)
    d3 = ctypes.c_double * 3
    rc = _capi.lib().mvhmr_build_coord_volumes(coords.data_ptr(), rot.data_ptr(), cen.data_ptr(), B, S, d3(*pr["position"]), d3(*pr["sides"]),
                                               aggregation._stream(gpu))
    assert rc == _capi.OK
    vol = torch.from_numpy(pr["v"].astype(np.float32)).view(B, C, *shape).to(gpu)
    out, idx = volsample.sample_volume_cuboid(vol, coords.view(B, -1, 3), rot, cen, pr["position"], pr["sides"], return_index=True)
    nodes = np.stack(np.meshgrid(*[np.arange(S)] * 3, indexing="ij"), -1).reshape(1, -1, 3).astype(np.float64)
    dt = vo.bound_roundtrip_index(coords.cpu().numpy(), pr["centers"], pr["position"], pr["sides"], shape)
    _hold("vs round trip: index", _np(idx), np.broadcast_to(nodes, (B, S ** 3, 3)), dt)
    v = pr["v"].astype(np.float32).astype(np.float64)
    slack = 2.0 * np.abs(v).max() * dt.sum(-1)[:, None, :] + vo.gamma(8) * np.abs(v).max()
    _hold("vs round trip: samples", _np(out), v, np.broadcast_to(slack, v.shape))


def test_volumetric_cross_entropy_is_lse_minus_beta_v(gpu):
    B, J, shape, beta = 2, 17, (4, 4, 8), 2.0
    pr = vo.general_problem(91, B, J, shape, J, paired=True)
    v32 = pr["v"].astype(np.float32)
    vol = torch.from_numpy(v32).view(B, J, *shape).to(gpu).requires_grad_(True)
    pts, rot, cen = _t(pr["points"], gpu, True), _t(pr["rot"], gpu, True), _t(pr["centers"], gpu, True)
    loss, idx = volsample.volumetric_cross_entropy(vol, pts, rot, cen, pr["position"], pr["sides"], beta=beta)
    assert tuple(loss.shape) == (B, J) and tuple(idx.shape) == (B, J, 3)
    gl = pr["g"].astype(np.float32)
    (loss * _t(gl, gpu)).sum().backward()
    t = idx.detach().cpu().numpy()
    u = so.cuboid_offsets(pr["position"], pr["sides"], shape, pr["centers"])
    value, mag = vo.forward(v32, t, shape, paired=True)
    L = so.forward(v32, u, beta)["L"]
    ref = L - beta * value
    bound = so.lse_bound(v32, u, beta) + beta * vo.bound_forward(mag) + 2 * vo.EPS * (np.abs(L) + beta * np.abs(value))
    _hold("vs cross-entropy: loss", _np(loss), ref, bound)
    # the gradient reaches the volume through both ops: beta * softmax * g from the logsumexp, -beta * w * g from the sample
    bw = vo.backward(v32, t, pr["points"], pr["rot"], pr["centers"], pr["sides"], shape, -beta * gl.astype(np.float64), paired=True)
    sa = so.backward(v32, u, beta, None, gl)["grad_v"]
    sa_bound = so.grad_bounds(v32, u, beta, None, gl)["grad_v"]
    total = sa + bw["grad_v"]
    tb = sa_bound + vo.bound_grad_volumes(bw["mag_v"], bw["count"], J) + vo.EPS * (np.abs(sa) + np.abs(bw["grad_v"]))
    _hold("vs cross-entropy: grad_volumes", _np(vol.grad).reshape(B, J, -1), total, tb)
    assert (np.abs(sa) > 0).all() and (bw["grad_v"] != 0).any()
    e_points, e_rot, e_center = vo.bound_geometry(bw, pr["rot"], pr["sides"], shape, 1)
    _hold("vs cross-entropy: grad_targets", _np(pts.grad), bw["grad_points"], e_points)
    _hold("vs cross-entropy: grad_rot", _np(rot.grad), bw["grad_rot"], e_rot)
    _hold("vs cross-entropy: grad_center", _np(cen.grad), bw["grad_center"], e_center)


def test_volume_generator_sample_is_the_free_function_on_its_cuboid(gpu):
    S, B, C, N = 4, 2, 3, 9
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=2500.0, device=gpu)
    cub = gen.cuboid()
    pr = vo.general_problem(92, B, C, (S, S, S), N)
    pr["position"], pr["sides"] = list(cub.position), list(cub.sides)
    tt = np.random.default_rng(0).uniform(-0.5, S - 0.5, (B, N, 3))             # the module's cuboid is centred on the world origin
    pr["points"] = vo.world_points(tt, pr["rot"], pr["centers"], pr["position"], pr["sides"], (S, S, S)).astype(np.float32)
    vol = torch.from_numpy(pr["v"].astype(np.float32)).view(B, C, S, S, S).to(gpu)
    pts, rot, cen = _t(pr["points"], gpu), _t(pr["rot"], gpu), _t(pr["centers"], gpu)
    a, ia = gen.sample(vol, pts, rot, cen, return_index=True)
    b, ib = volsample.sample_volume_cuboid(vol, pts, rot, cen, cub.position, cub.sides, return_index=True)
    assert torch.equal(a, b) and torch.equal(ia, ib) and a.abs().max() > 0
    assert torch.equal(gen.sample(vol, pts[:, :C], rot, cen, paired=True), volsample.sample_volume_cuboid(vol, pts[:, :C], rot, cen, cub.position, cub.sides, paired=True))


# ------------------------------------------------------------------------------------ graphs, the raw ABI
def test_graph_capture_and_replay_match_eager(gpu):
    """forward + backward captured into one HIP graph on a single stream; the replay on new volume values equals eager bit for bit"""
    B, C, shape, N, _, dup = BASE[2]
    pr = vo.general_problem(95, B, C, shape, N, duplicate=dup)
    vol = torch.from_numpy(pr["v"].astype(np.float32)).view(B, C, *shape).to(gpu).requires_grad_(True)
    pts, rot, cen, g = _t(pr["points"], gpu, True), _t(pr["rot"], gpu, True), _t(pr["centers"], gpu, True), _t(pr["g"], gpu)
    pos, sides = list(pr["position"]), list(pr["sides"])

    def step():
        out, idx = volsample.sample_volume_cuboid(vol, pts, rot, cen, pos, sides, return_index=True)
        return (out, idx) + torch.autograd.grad((out * g).sum(), (vol, pts, rot, cen))

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
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))           # bits: the index of the NaN point is NaN in both


def test_raw_c_abi_call_equals_the_op(gpu):
    """the C ABI through ctypes alone: forward and both backwards give the op's bits; refusals launch nothing"""
    L = _capi.lib()
    B, C, shape, N, _, dup = BASE[2]
    pr = vo.general_problem(96, B, C, shape, N, duplicate=dup)
    pr["g"] = pr["g"].astype(np.float32)
    ref = _run(gpu, pr, shape, torch.float32, False)
    vol = torch.from_numpy(pr["v"].astype(np.float32)).view(B, C, *shape).to(gpu)
    pts, rot, cen, g = _t(pr["points"], gpu), _t(pr["rot"], gpu), _t(pr["centers"], gpu), _t(pr["g"], gpu)
    d3 = ctypes.c_double * 3
    pos, sides, stream = d3(*pr["position"]), d3(*pr["sides"]), aggregation._stream(gpu)
    out, idx = torch.full((B, C, N), 7.0, device=gpu), torch.full((B, N, 3), 7.0, device=gpu)
    sizes = (B, C) + shape + (N, 0)
    assert L.mvhmr_sample_volume_forward(vol.data_ptr(), _capi.F32, pts.data_ptr(), rot.data_ptr(), cen.data_ptr(), pos, sides, *sizes, out.data_ptr(),
                                         idx.data_ptr(), stream) == _capi.OK
    need = L.mvhmr_sample_volume_workspace_bytes(B, N)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    gv = torch.full_like(vol, 7.0)                                                                # the call zero-fills it itself
    assert L.mvhmr_sample_volume_backward_volumes(_capi.F32, idx.data_ptr(), g.data_ptr(), *sizes, gv.data_ptr(), ws.data_ptr(), need, stream) == _capi.OK
    gp, gr, gc = torch.empty(B, N, 3, device=gpu), torch.empty(B, 3, 3, device=gpu), torch.empty(B, 3, device=gpu)
    assert L.mvhmr_sample_volume_backward_geometry(vol.data_ptr(), _capi.F32, pts.data_ptr(), rot.data_ptr(), cen.data_ptr(), pos, sides, *sizes,
                                                   idx.data_ptr(), g.data_ptr(), gp.data_ptr(), gr.data_ptr(), gc.data_ptr(), ws.data_ptr(), need,
                                                   stream) == _capi.OK
    torch.cuda.synchronize()
    for name, t in (("out", out), ("index", idx), ("grad_v", gv.view(B, C, -1)), ("grad_points", gp), ("grad_rot", gr), ("grad_center", gc)):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), ref[name].view(np.uint32)), name
    before = gv.clone()
    assert L.mvhmr_sample_volume_backward_volumes(_capi.F32, idx.data_ptr(), g.data_ptr(), *sizes, gv.data_ptr(), ws.data_ptr(), need - 1,
                                                  stream) == _capi.ERR_WORKSPACE
    assert b"workspace" in L.mvhmr_last_error()
    assert L.mvhmr_sample_volume_backward_volumes(_capi.F32, idx.data_ptr(), g.data_ptr(), B, C, 1, 4, 8, N, 0, gv.data_ptr(), ws.data_ptr(), need,
                                                  stream) == _capi.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert torch.equal(before, gv)
