"""Volumetric soft-argmax on the MI355X (multiviewhmr_amd/softargmax.py, soft_argmax3d.hip): bit equality with the float64 oracle on
the exact rig, general inputs within the derived bounds (tests/softargmax_oracle.py), the special values, bitwise
reproducibility, graph capture, the raw C ABI, VolumeGenerator, and the coarse-to-fine chain into unprojection_cuboid.  Every error is
asserted through conftest.record_err, which also keeps it."""
import ctypes

import numpy as np
import pytest
import torch

import softargmax_oracle as so
from conftest import record_err
from posegrad_oracle import pose_grad
from test_geometry_grad_gpu import _ring
from test_pose_grad_gpu import POSITION, REL, SIDES, _pose
from test_soft_argmax_cpu import SPLIT_SHAPE, TILE_SHAPE, _problem
from test_unproject_gpu import _rig
from multiviewhmr_amd import _capi, aggregation, softargmax

pytestmark = pytest.mark.gpu

# (B, J, vol): what each reaches is in the issue's table -- S > 1; S = 1 with tiles 4+4+4+4+1; odd N (scalar path, tiles 4+1);
# N smaller than one vector per lane; N % 4 == 0 with Z % 4 != 0 (a vector crosses a row)
SHAPES = [SPLIT_SHAPE, TILE_SHAPE, (2, 5, (3, 5, 7)), (2, 2, (2, 2, 2)), (1, 3, (4, 3, 6))]
HALF_SHAPES = [TILE_SHAPE, (2, 5, (3, 5, 7))]
CASES = [(s, torch.float32) for s in SHAPES] + [(s, dt) for s in HALF_SHAPES for dt in (torch.float16, torch.bfloat16)]
IDS = ["b%dj%d_%s_%s" % (s[0], s[1], "x".join(map(str, s[2])), str(dt)[6:]) for s, dt in CASES]
# relative rounding of the storage type, and the absolute floor its subnormals add (fp16: half the smallest subnormal 2^-24)
STORE = {torch.float32: (0.0, 0.0), torch.float16: (2.0 ** -11, 2.0 ** -25), torch.bfloat16: (2.0 ** -8, 0.0)}


def _t(x, gpu, dtype=torch.float32, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu).to(dtype).requires_grad_(grad)


def _stored(v, dtype):
    """the values a volume of `dtype` holds, as float64 numpy (B, J, N)"""
    return torch.from_numpy(np.ascontiguousarray(v)).to(dtype).double().numpy()


def _vol(v, shape, gpu, dtype, grad=False):
    B, J, _ = v.shape
    return torch.from_numpy(np.ascontiguousarray(v)).to(dtype).view(B, J, *shape).to(gpu).requires_grad_(grad)


def _np(t):
    return t.detach().double().cpu().numpy()


def _hold(name, got, ref, bound):
    """|got - ref| <= bound elementwise; the element with the largest share of its bound is the one recorded"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(ref))
    err = np.abs(got - ref)
    assert not np.isnan(err).any(), name
    share = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    i = np.unravel_index(int(np.argmax(share)), share.shape) if share.ndim else ()
    record_err(name, float(err[i]), float(bound[i]))


def _same_bits(a, b):
    """equal as fp32 numbers (NaN equals NaN; the sign of a zero is not told apart)"""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _run(gpu, v, shape, dtype, beta, g, gl, coords=None, pose=None, cuboid=None, want=(True, True, True)):
    """forward + backward of one route through the public functions -> dict of numpy results (None where no gradient was asked for)"""
    vol = _vol(v, shape, gpu, dtype, grad=want[0])
    B, J = v.shape[:2]
    if coords is not None:
        c = _t(coords.reshape(B, *shape, 3), gpu, grad=want[1])
        kp, L = softargmax.soft_argmax_3d(vol, c, beta=beta, return_logsumexp=True)
        leaves = {"grad_coords": c}
    else:
        r, ce = _t(pose[0], gpu, grad=want[1]), _t(pose[1], gpu, grad=want[2])
        kp, L = softargmax.soft_argmax_3d_cuboid(vol, r, ce, cuboid[0], cuboid[1], beta=beta, return_logsumexp=True)
        leaves = {"grad_rot": r, "grad_center": ce}
    leaves["grad_v"] = vol
    loss = 0
    if g is not None:
        loss = loss + (kp * _t(g, gpu)).sum()
    if gl is not None:
        loss = loss + (L * _t(gl, gpu)).sum()
    if torch.is_tensor(loss) and loss.requires_grad:
        loss.backward()
    out = {"kp": kp.detach().cpu().numpy(), "L": L.detach().cpu().numpy()}
    for name, leaf in leaves.items():
        out[name] = None if leaf.grad is None else leaf.grad.detach().float().cpu().numpy()
    if out["grad_v"] is not None:
        out["grad_v"] = out["grad_v"].reshape(v.shape)
    if out.get("grad_coords") is not None:
        out["grad_coords"] = out["grad_coords"].reshape(B, -1, 3)
    return out


def test_the_split_shape_splits_and_the_tile_shape_does_not():
    L = _capi.lib()
    B, J, shape = SPLIT_SHAPE
    assert L.mvhmr_soft_argmax3d_splits(B, J, int(np.prod(shape))) > 1
    B, J, shape = TILE_SHAPE
    assert L.mvhmr_soft_argmax3d_splits(B, J, int(np.prod(shape))) == 1


# ------------------------------------------------------------------------------------ the exact rig: bits
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_rig_is_bit_equal_to_the_oracle(case, gpu):
    """both routes, forward and every gradient: on the rig each fp32 operation is exact, so the kernels must give the float64 oracle's
    values cast once (to fp32, then to the storage type for grad_volumes)"""
    (B, J, shape), dtype = case
    rig = so.exact_rig(7, B, J, shape, on=16)
    v = _stored(rig["v"], dtype)                                   # fp16 turns the "off" level into -inf: it must still count exactly 0
    beta, g, gl = 1.0, rig["g"], rig["gl"]
    cub = (rig["position"], rig["sides"])
    for route, u, kw in (("cuboid", rig["offsets"], dict(pose=(rig["rot"], rig["centers"]), cuboid=cub)), ("tensor", rig["coords"], dict(coords=rig["coords"]))):
        rot, cen = (rig["rot"], rig["centers"]) if route == "cuboid" else (None, None)
        got = _run(gpu, v, shape, dtype, beta, g, gl, **kw)
        ref, bw = so.forward(v, u, beta, rot, cen), so.backward(v, u, beta, g, gl, rot)
        tag = "exact rig %s %s " % (IDS[CASES.index(case)], route)
        # the rig's own premises: the oracle's values are fp32 numbers, h . (u - mu) + g_L included
        for x in (ref["kp"], bw["grad_v"], bw["grad_coords"]):
            assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
        record_err(tag + "keypoints", float(np.abs(got["kp"].astype(np.float64) - ref["kp"]).max()), 0.0)
        assert _same_bits(got["kp"], ref["kp"].astype(np.float32))
        want_L = np.float32(np.log(rig["K"]))
        record_err(tag + "logsumexp", float(np.abs(got["L"] - want_L).max()), 4 * float(np.spacing(max(want_L, np.float32(1.0)))))
        want_gv = torch.from_numpy(bw["grad_v"].astype(np.float32)).to(dtype).float().numpy()
        record_err(tag + "grad_volumes", float(np.abs(got["grad_v"] - want_gv).max()), 0.0)
        if route == "tensor":
            record_err(tag + "grad_coords", float(np.abs(got["grad_coords"] - bw["grad_coords"]).max()), 0.0)
        else:
            record_err(tag + "grad_rot", float(np.abs(got["grad_rot"] - bw["grad_rot"]).max()), 0.0)
            record_err(tag + "grad_center", float(np.abs(got["grad_center"] - bw["grad_center"]).max()), 0.0)


# ------------------------------------------------------------------------------------ general inputs: the bounds
@pytest.mark.parametrize("beta", [1.0, 10.0])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_general_inputs_stay_within_the_bounds(case, beta, gpu):
    (B, J, shape), dtype = case
    pr = _problem(40 + B + J, B, J, shape, offset=3000.0)
    item = 4 if dtype == torch.float32 else 2
    rel, floor = STORE[dtype]
    v = _stored(pr["v"], dtype)
    rot, cen = pr["rot"].astype(np.float32), pr["centers"].astype(np.float32)
    g, gl = (0.25 * pr["g"]).astype(np.float32), pr["gl"].astype(np.float32)      # (0.25: beta p h . (u - mu) stays inside fp16's range)
    d = so.cuboid_offsets(pr["position"], pr["sides"], shape, cen)
    w = so.world_coords(d, rot, cen).astype(np.float32)
    tag = "soft-argmax %s beta=%g " % (IDS[CASES.index(case)], beta)
    got_c = _run(gpu, v, shape, dtype, beta, g, gl, pose=(rot, cen), cuboid=(pr["position"], pr["sides"]))
    got_t = _run(gpu, v, shape, dtype, beta, g, gl, coords=w)
    for route, got, u, r, c in (("cuboid ", got_c, d, rot, cen), ("tensor ", got_t, w, None, None)):
        ref, bw = so.forward(v, u, beta, r, c), so.backward(v, u, beta, g, gl, r)
        gb = so.grad_bounds(v, u, beta, g, gl, r, item, rel)
        _hold(tag + route + "keypoints", got["kp"], ref["kp"], so.moment_bound(v, u, beta, item) if r is None else so.keypoint_bound(v, u, beta, r, c, item))
        _hold(tag + route + "logsumexp", got["L"], ref["L"], so.lse_bound(v, u, beta, item))
        _hold(tag + route + "grad_volumes", got["grad_v"], bw["grad_v"], gb["grad_v"] + floor)
        for name in ("grad_coords",) if r is None else ("grad_rot", "grad_center"):
            _hold(tag + route + name, got[name], bw[name], gb[name])
    # the two routes on the same world points: within the sum of their bounds and the gap between their oracles (the coordinates' own rounding)
    ref_c, ref_t = so.forward(v, d, beta, rot, cen), so.forward(v, w, beta)
    _hold(tag + "cuboid vs tensor keypoints", got_c["kp"], got_t["kp"],
          so.keypoint_bound(v, d, beta, rot, cen, item) + so.moment_bound(v, w, beta, item) + np.abs(ref_c["kp"] - ref_t["kp"]))


def test_cuboid_route_agrees_with_the_tensor_route_on_built_coordinates(gpu):
    """the tensor route fed mvhmr_build_coord_volumes' coordinates of the same pose (VolumeGenerator.coord_volumes), forward and the
    volume gradient: within the sum of the two bounds"""
    B, J, S = 3, 17, 8
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=2500.0, device=gpu)
    cub = gen.cuboid()
    pr = _problem(77, B, J, (S, S, S))
    rot, cen = pr["rot"].astype(np.float32), (pr["centers"] * 10).astype(np.float32)
    coords = gen.coord_volumes(_t(rot, gpu), _t(cen, gpu), gpu)
    v, g = pr["v"].astype(np.float32), pr["g"].astype(np.float32)
    w = coords.cpu().numpy().reshape(B, -1, 3)
    d = so.cuboid_offsets(cub.position, cub.sides, (S, S, S), cen)
    for beta in (1.0, 10.0):
        a = _run(gpu, v, (S, S, S), torch.float32, beta, g, None, pose=(rot, cen), cuboid=(cub.position, cub.sides))
        b = _run(gpu, v, (S, S, S), torch.float32, beta, g, None, coords=w)
        ref_c, ref_t = so.forward(v, d, beta, rot, cen), so.forward(v, w, beta)
        _hold("built coordinates beta=%g keypoints" % beta, a["kp"], b["kp"],
              so.keypoint_bound(v, d, beta, rot, cen) + so.moment_bound(v, w, beta) + np.abs(ref_c["kp"] - ref_t["kp"]))
        bw_c, bw_t = so.backward(v, d, beta, g, None, rot), so.backward(v, w, beta, g, None)
        _hold("built coordinates beta=%g grad_volumes" % beta, a["grad_v"], b["grad_v"],
              so.grad_bounds(v, d, beta, g, None, rot)["grad_v"] + so.grad_bounds(v, w, beta, g, None)["grad_v"] + np.abs(bw_c["grad_v"] - bw_t["grad_v"]))


def test_directional_derivative_of_the_oracle(gpu):
    """the kernels' gradient along a random direction against a float64 central difference of the ORACLE's loss"""
    B, J, shape = 2, 5, (3, 5, 7)
    pr = _problem(12, B, J, shape)
    beta, v = 2.0, pr["v"].astype(np.float32).astype(np.float64)
    rot, cen, g, gl = pr["rot"].astype(np.float32), pr["centers"].astype(np.float32), pr["g"].astype(np.float32), pr["gl"].astype(np.float32)
    d = so.cuboid_offsets(pr["position"], pr["sides"], shape, cen)
    got = _run(gpu, v, shape, torch.float32, beta, g, gl, pose=(rot, cen), cuboid=(pr["position"], pr["sides"]))
    dv = np.random.RandomState(3).normal(size=v.shape)

    def loss(x):
        f = so.forward(x, d, beta, rot, cen)
        return float((f["kp"] * g).sum() + (f["L"] * gl).sum())

    h = 1e-5
    fd = (loss(v + h * dv) - loss(v - h * dv)) / (2 * h)
    bound = float((so.grad_bounds(v, d, beta, g, gl, rot)["grad_v"] * np.abs(dv)).sum()) + 1e-7 * abs(fd)      # + the difference's own truncation
    record_err("soft-argmax directional derivative vs the oracle's central difference", abs(float((got["grad_v"].astype(np.float64) * dv).sum()) - fd), bound)


# ------------------------------------------------------------------------------------ edges
def test_minus_inf_entries_are_ignored_exactly(gpu):
    """-inf voxels -- the first 40 of a slice among them, so that whole lanes meet nothing else first -- against the same volume with
    -1e30 in their place (exp2 gives exactly 0 there too): the same bits; and against the oracle"""
    B, J, shape = 2, 5, (3, 5, 7)
    pr = _problem(21, B, J, shape)
    v = pr["v"].astype(np.float32)
    hole = np.zeros(v.shape, bool)
    hole[:, :, :40] = True
    hole[0, 1, 60:] = True
    hole |= np.random.RandomState(2).rand(*v.shape) < 0.2
    hole[..., 50] = False
    rot, cen, g = pr["rot"].astype(np.float32), pr["centers"].astype(np.float32), pr["g"].astype(np.float32)
    kw = dict(pose=(rot, cen), cuboid=(pr["position"], pr["sides"]))
    a = _run(gpu, np.where(hole, -np.inf, v), shape, torch.float32, 1.0, g, None, **kw)
    b = _run(gpu, np.where(hole, np.float32(-1e30), v), shape, torch.float32, 1.0, g, None, **kw)
    assert _same_bits(a["kp"], b["kp"]) and _same_bits(a["L"], b["L"]) and _same_bits(a["grad_v"], b["grad_v"])
    assert np.isfinite(a["kp"]).all() and np.isfinite(a["grad_v"]).all() and (a["grad_v"][hole] == 0).all()
    vi = np.where(hole, -np.inf, v).astype(np.float64)
    d = so.cuboid_offsets(pr["position"], pr["sides"], shape, cen)
    _hold("-inf entries: keypoints", a["kp"], so.forward(vi, d, 1.0, rot, cen)["kp"], so.keypoint_bound(vi, d, 1.0, rot, cen))


@pytest.mark.parametrize("poison", ["all -inf", "nan", "+inf"])
def test_a_poisoned_slice_is_nan_alone(poison, gpu):
    """the slice gives NaN keypoints and logsumexp; its neighbours are bit-equal to a run without the poison"""
    for B, J, shape in (TILE_SHAPE, (1, 2, SPLIT_SHAPE[2]), (2, 5, (3, 5, 7))):
        pr = _problem(31, B, J, shape)
        v = pr["v"].astype(np.float32)
        bad = v.copy()
        if poison == "all -inf":
            bad[B - 1, 1] = -np.inf
        else:
            bad[B - 1, 1, v.shape[2] // 2] = np.nan if poison == "nan" else np.inf
        w = np.random.RandomState(1).normal(0, 100, (B, v.shape[2], 3)).astype(np.float32)
        clean = _run(gpu, v, shape, torch.float32, 1.0, None, None, coords=w, want=(False, False, False))
        got = _run(gpu, bad, shape, torch.float32, 1.0, None, None, coords=w, want=(False, False, False))
        assert np.isnan(got["kp"][B - 1, 1]).all() and np.isnan(got["L"][B - 1, 1])
        keep = np.ones((B, J), bool)
        keep[B - 1, 1] = False
        assert _same_bits(got["kp"][keep], clean["kp"][keep]) and _same_bits(got["L"][keep], clean["L"][keep])
        assert np.isfinite(got["kp"][keep]).all()


def test_beta_zero_gives_the_centroid(gpu):
    B, J, shape = 2, 5, (3, 5, 7)
    pr = _problem(5, B, J, shape)
    v = pr["v"].astype(np.float32)
    w = np.random.RandomState(4).normal(0, 300, (B, v.shape[2], 3)).astype(np.float32)
    got = _run(gpu, v, shape, torch.float32, 0.0, None, None, coords=w, want=(False, False, False))
    centroid = np.repeat(w.astype(np.float64).mean(1)[:, None], J, 1)
    _hold("beta = 0: the centroid", got["kp"], centroid, so.moment_bound(v, w, 0.0))
    _hold("beta = 0: ln N", got["L"], np.full((B, J), np.log(v.shape[2])), so.lse_bound(v, w, 0.0))


def test_either_gradient_may_be_absent_and_unasked_gradients_are_not_computed(gpu):
    B, J, shape = 2, 5, (3, 5, 7)
    pr = _problem(6, B, J, shape)
    v, beta = pr["v"].astype(np.float32), 1.5
    rot, cen, g, gl = pr["rot"].astype(np.float32), pr["centers"].astype(np.float32), pr["g"].astype(np.float32), pr["gl"].astype(np.float32)
    d = so.cuboid_offsets(pr["position"], pr["sides"], shape, cen)
    w = so.world_coords(d, rot, cen).astype(np.float32)
    kw = dict(pose=(rot, cen), cuboid=(pr["position"], pr["sides"]))
    for tag, gg, ll in (("g only", g, None), ("g_L only", None, gl)):
        got = _run(gpu, v, shape, torch.float32, beta, gg, ll, **kw)
        bw, gb = so.backward(v, d, beta, gg, ll, rot), so.grad_bounds(v, d, beta, gg, ll, rot)
        _hold("soft-argmax %s: grad_volumes" % tag, got["grad_v"], bw["grad_v"], gb["grad_v"])
        if gg is None:                                 # the logsumexp does not depend on the pose
            assert got["grad_rot"] is None or not got["grad_rot"].any()
            assert got["grad_center"] is None or not got["grad_center"].any()
        else:
            _hold("soft-argmax %s: grad_rot" % tag, got["grad_rot"], bw["grad_rot"], gb["grad_rot"])
        got = _run(gpu, v, shape, torch.float32, beta, gg, ll, coords=w)
        _hold("soft-argmax %s: tensor route grad_volumes" % tag, got["grad_v"], so.backward(v, w, beta, gg, ll)["grad_v"],
              so.grad_bounds(v, w, beta, gg, ll)["grad_v"])
    # requires_grad on the volumes only: neither extra kernel has anything to write into
    a = _run(gpu, v, shape, torch.float32, beta, g, gl, want=(True, False, False), **kw)
    b = _run(gpu, v, shape, torch.float32, beta, g, gl, coords=w, want=(True, False, False))
    assert a["grad_rot"] is None and a["grad_center"] is None and b["grad_coords"] is None
    assert a["grad_v"] is not None and b["grad_v"] is not None
    # and the other way round: the pose alone
    c = _run(gpu, v, shape, torch.float32, beta, g, gl, want=(False, True, True), **kw)
    assert c["grad_v"] is None and c["grad_rot"] is not None and c["grad_center"] is not None


# ------------------------------------------------------------------------------------ reproducibility, graphs, the raw ABI
@pytest.mark.parametrize("deterministic", [False, True])
def test_two_runs_are_bitwise_identical(deterministic, gpu):
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(deterministic)
    try:
        for (B, J, shape), dtype in ((SPLIT_SHAPE, torch.float32), (TILE_SHAPE, torch.bfloat16), ((2, 5, (3, 5, 7)), torch.float16)):
            pr = _problem(8, B, J, shape)
            v = _stored(pr["v"], dtype)
            rot, cen, g, gl = pr["rot"].astype(np.float32), pr["centers"].astype(np.float32), pr["g"].astype(np.float32), pr["gl"].astype(np.float32)
            w = so.world_coords(so.cuboid_offsets(pr["position"], pr["sides"], shape, cen), rot, cen).astype(np.float32)
            for kw in (dict(pose=(rot, cen), cuboid=(pr["position"], pr["sides"])), dict(coords=w)):
                a, b = (_run(gpu, v, shape, dtype, 3.0, g, gl, **kw) for _ in range(2))
                for key in a:
                    assert a[key] is not None and np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
    finally:
        torch.use_deterministic_algorithms(prev)


def test_graph_capture_and_replay_match_eager(gpu):
    """forward + backward of both routes captured into one HIP graph; the replay on new volume values equals eager bit for bit"""
    B, J, shape = 3, 17, (8, 8, 8)
    pr = _problem(9, B, J, shape)
    rot, cen = _t(pr["rot"].astype(np.float32), gpu, grad=True), _t(pr["centers"].astype(np.float32), gpu, grad=True)
    g, gl = _t(pr["g"].astype(np.float32), gpu), _t(pr["gl"].astype(np.float32), gpu)
    pos, sides = list(pr["position"]), list(pr["sides"])
    vol = _vol(pr["v"].astype(np.float32), shape, gpu, torch.float32, grad=True)
    coords = torch.randn(B, *shape, 3, device=gpu, requires_grad=True)

    def step():
        kc, lc = softargmax.soft_argmax_3d_cuboid(vol, rot, cen, pos, sides, beta=2.0, return_logsumexp=True)
        kt, lt = softargmax.soft_argmax_3d(vol, coords, beta=2.0, return_logsumexp=True)
        grads = torch.autograd.grad((kc * g).sum() + (lc * gl).sum() + (kt * g).sum() + (lt * gl).sum(), (vol, rot, cen, coords))
        return (kc, lc, kt, lt) + grads

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
        assert torch.equal(a, b)


def _raw_forward(L, vol, dtype_code, coords, out, ws, ws_bytes, beta=1.0, sizes=None):
    B, J, X, Y, Z = sizes or vol.shape
    kp, lse, mom = out
    return L.mvhmr_soft_argmax3d_forward(vol.data_ptr(), dtype_code, coords.data_ptr(), None, None, None, None, B, J, X, Y, Z, beta,
                                         kp.data_ptr(), lse.data_ptr(), mom.data_ptr(), ws.data_ptr() if ws is not None else None, ws_bytes,
                                         aggregation._stream(vol.device))


def test_raw_c_abi_call_and_its_refusals(gpu):
    """the C ABI through ctypes alone: the outputs of the op bit for bit, the moment against the oracle, and the documented statuses"""
    L = _capi.lib()
    B, J, shape = 2, 5, (4, 3, 6)
    pr = _problem(10, B, J, shape)
    v = pr["v"].astype(np.float32)
    w = np.random.RandomState(6).normal(0, 200, (B, v.shape[2], 3)).astype(np.float32)
    vol, coords = _vol(v, shape, gpu, torch.float32), _t(w.reshape(B, *shape, 3), gpu)
    need = L.mvhmr_soft_argmax3d_workspace_bytes(B, J, *shape)
    assert need == B * J * L.mvhmr_soft_argmax3d_splits(B, J, v.shape[2]) * 5 * 4
    out = [torch.full(s, 7.0, device=gpu) for s in ((B, J, 3), (B, J), (B, J, 3))]
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    assert _raw_forward(L, vol, _capi.F32, coords, out, ws, need, beta=2.0) == _capi.OK
    torch.cuda.synchronize()
    kp, lse = softargmax.soft_argmax_3d(vol, coords, beta=2.0, return_logsumexp=True)
    assert torch.equal(out[0], kp) and torch.equal(out[1], lse) and torch.equal(out[2], kp)          # tensor route: keypoint = moment
    _hold("raw ABI: moment", _np(out[2]), so.forward(v, w, 2.0)["mu"], so.moment_bound(v, w, 2.0))
    # backward through the raw ABI as well: g only (grad_logsumexp NULL)
    g = _t(pr["g"].astype(np.float32), gpu)
    gv = torch.empty_like(vol)
    rc = L.mvhmr_soft_argmax3d_backward(vol.data_ptr(), _capi.F32, coords.data_ptr(), None, None, None, None, B, J, *shape, 2.0, out[1].data_ptr(),
                                        out[2].data_ptr(), g.data_ptr(), None, gv.data_ptr(), aggregation._stream(gpu))
    assert rc == _capi.OK
    torch.cuda.synchronize()
    _hold("raw ABI: grad_volumes", _np(gv).reshape(v.shape), so.backward(v, w, 2.0, pr["g"].astype(np.float32))["grad_v"],
          so.grad_bounds(v, w, 2.0, pr["g"].astype(np.float32))["grad_v"])
    # refusals: nothing is launched, the outputs keep their values
    before = [t.clone() for t in out]
    assert _raw_forward(L, vol, _capi.F32, coords, out, ws, need - 1) == _capi.ERR_WORKSPACE
    assert b"workspace" in L.mvhmr_last_error()
    assert _raw_forward(L, vol, _capi.F32, coords, out, None, need) == _capi.ERR_WORKSPACE
    assert _raw_forward(L, vol, 3, coords, out, ws, need) == _capi.ERR_INVALID_ARGUMENT
    assert b"dtype" in L.mvhmr_last_error()
    assert _raw_forward(L, vol, _capi.F32, coords, out, ws, need, sizes=(B, 0, 4, 3, 6)) == _capi.ERR_INVALID_ARGUMENT
    assert _raw_forward(L, vol, _capi.F32, coords, out, ws, need, beta=float("nan")) == _capi.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, out))


# ------------------------------------------------------------------------------------ VolumeGenerator and the coarse-to-fine chain
def test_volume_generator_returns_the_pose_it_used(gpu):
    """train() mode, numpy seed fixed: forward_with_pose's volume is forward's, bit for bit; a volume that is -inf but for one voxel
    lands on that voxel's world coordinate -- the one mvhmr_build_coord_volumes gives for the returned rotation and centre, to the bit"""
    B, V, C, H, S, IMG = 2, 4, 8, 24, 8, 96
    cams = _rig(B, V, 5000.0, IMG, seed=3)
    rng = np.random.default_rng(3)
    batch = dict(images=np.zeros((B, V, IMG, IMG, 3), np.uint8), cameras=cams, keypoints_3d=[rng.normal(0, 100, (17, 3)).astype(np.float32) for _ in range(B)])
    proj_org = torch.from_numpy(np.stack([[cams[v][b].projection for v in range(V)] for b in range(B)]).astype(np.float32)).to(gpu)
    torch.manual_seed(1)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=C, output_channels=C, cuboid_side=2500.0, device=gpu).train()
    feats = torch.randn(B, V, C, H, H, device=gpu)
    with torch.no_grad():
        np.random.seed(17)
        plain = gen(feats, proj_org, batch)
        np.random.seed(17)
        vol, rots, centers = gen.forward_with_pose(feats, proj_org, batch)
    assert torch.equal(plain, vol) and tuple(rots.shape) == (B, 3, 3) and tuple(centers.shape) == (B, 3)
    assert rots.device == vol.device and rots.dtype == torch.float32
    np.random.seed(17)
    assert np.allclose(rots[:, 0, 0].cpu().numpy(), np.cos(np.random.uniform(0.0, 2 * np.pi, size=B)).astype(np.float32))
    heat = torch.full((B, 3, S, S, S), -float("inf"), device=gpu)
    spots = [(0, 0, (1, 2, 3)), (0, 1, (7, 7, 7)), (0, 2, (0, 0, 0)), (1, 0, (4, 0, 6)), (1, 1, (2, 5, 1)), (1, 2, (6, 3, 0))]
    for b, j, (x, y, z) in spots:
        heat[b, j, x, y, z] = 0.25
    kp = gen.soft_argmax(heat, rots, centers, beta=3.0)
    coords = gen.coord_volumes(rots, centers, gpu)
    for b, j, (x, y, z) in spots:
        assert torch.equal(kp[b, j], coords[b, x, y, z]), (b, j)


def test_coarse_to_fine_chain_reaches_the_coarse_volume(gpu):
    """the motivating use: the soft-argmax of a coarse heat volume is the `centers` of unprojection_cuboid, and .backward() carries the
    fine volume's gradient into the coarse one.  Against the oracles composed: posegrad_oracle's grad_center at the pivot the kernels
    produced, then this module's oracle; the pose gradient's own tolerance (REL of its scale, tests/test_pose_grad_gpu.py) is carried
    through the soft-argmax backward, which is linear in it."""
    B, V, C, H, W, vol = 2, 3, 5, 12, 16, (5, 4, 6)
    rng = np.random.default_rng(11)
    P = _ring(B, V, H, W, seed=5)
    rot, _ = _pose(B, seed=6)
    feats = rng.standard_normal((B, V, C, H, W)).astype(np.float32)
    go = rng.standard_normal((B, C) + vol).astype(np.float32)
    cshape, cpos, csides, beta = (4, 4, 4), (-0.3, -0.3, -0.3), (0.6, 0.6, 0.6), 2.0
    crot, ccen = _pose(B, seed=7)
    coarse_v = rng.standard_normal((B, 1, 64)).astype(np.float32)
    coarse = _vol(coarse_v, cshape, gpu, torch.float32, grad=True)
    f = _t(feats, gpu)
    kp = softargmax.soft_argmax_3d_cuboid(coarse, _t(crot, gpu), _t(ccen, gpu), cpos, csides, beta=beta)
    pivots = kp[:, 0]
    out = aggregation.unprojection_cuboid(f, _t(P, gpu), _t(rot, gpu), pivots, POSITION, SIDES, vol, aggregation_method="softmax")
    (out * _t(go, gpu)).sum().backward()
    assert coarse.grad is not None and bool(torch.isfinite(coarse.grad).all()) and float(coarse.grad.abs().sum()) > 0
    d = so.cuboid_offsets(cpos, csides, cshape, ccen)
    ref = so.forward(coarse_v, d, beta, crot, ccen)
    _hold("chain: pivots", _np(pivots), ref["kp"][:, 0], so.keypoint_bound(coarse_v, d, beta, crot, ccen)[:, 0])
    g_c = pose_grad(feats, P, rot, pivots.detach().cpu().numpy(), POSITION, SIDES, vol, go, "softmax")[2][:, None, :]      # (B, 1, 3)
    want = so.backward(coarse_v, d, beta, g_c, None, crot)["grad_v"]
    slack = so.backward(coarse_v, d, beta, np.full_like(g_c, REL * np.abs(g_c).max()), None, np.abs(crot))
    carried = np.abs(beta) * ref["p"] * np.einsum("bjc,bjnc->bjn", np.abs(slack["h"]), np.abs(d.astype(np.float64)[:, None] - ref["mu"][:, :, None, :]))
    _hold("chain: gradient w.r.t. the coarse volume", _np(coarse.grad).reshape(B, 1, 64), want,
          so.grad_bounds(coarse_v, d, beta, g_c, None, crot)["grad_v"] + carried)
