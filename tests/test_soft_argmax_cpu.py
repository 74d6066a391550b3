"""Volumetric soft-argmax, what can be held without a device: the oracle against finite differences, the declarations, the split
function's mirror, the fake ops, the argument checks, VolumeGenerator's numpy draws, and the two properties of the documented reduction
order (tests/softargmax_oracle.py::emulate_fp32) that the GPU tests then hold the kernels to: it stays inside the derived bound, and it
is exact on the exact rig."""
import os
import re
import unittest.mock as mock

import numpy as np
import pytest
import torch

import softargmax_oracle as so
from conftest import ROOT
from multiviewhmr_amd import _capi, aggregation, softargmax

SYMBOLS = ("mvhmr_soft_argmax3d_splits", "mvhmr_soft_argmax3d_workspace_bytes", "mvhmr_soft_argmax3d_forward", "mvhmr_soft_argmax3d_backward",
           "mvhmr_soft_argmax3d_backward_coords", "mvhmr_soft_argmax3d_backward_pose")
# the GPU shapes (tests/test_soft_argmax_gpu.py) and what each has to reach
SPLIT_SHAPE, TILE_SHAPE = (1, 1, (32, 32, 32)), (3, 17, (8, 8, 8))


def _problem(seed, B, J, shape, offset=0.0, spread=1.0):
    rng = np.random.RandomState(seed)
    N = int(np.prod(shape))
    v = rng.normal(0, spread, (B, J, N))
    rot = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(B)])
    centers = rng.normal(0, 50, (B, 3)) + offset
    position, sides = np.array([-400.0, -300.0, -500.0]) + offset, np.array([800.0, 600.0, 1000.0])
    return {"v": v, "rot": rot, "centers": centers, "position": position, "sides": sides, "shape": shape,
            "g": rng.normal(size=(B, J, 3)), "gl": rng.normal(size=(B, J))}


def _loss(v, u, beta, g, gl, rot=None, centers=None):
    f = so.forward(v, u, beta, rot, centers)
    return float((f["kp"] * g).sum() + (f["L"] * gl).sum())


def _fd(fun, x, idx, h):
    xp, xm = x.copy(), x.copy()
    xp[idx] += h
    xm[idx] -= h
    return (fun(xp) - fun(xm)) / (2 * h)


@pytest.mark.parametrize("beta", [1.0, -0.7, 3.0])
def test_oracle_gradients_match_finite_differences(beta):
    """every gradient formula of the issue, as the oracle states it, against central differences of the oracle's own forward in float64"""
    pr = _problem(3, 2, 3, (3, 4, 5))
    v, g, gl, rot, c = pr["v"], pr["g"], pr["gl"], pr["rot"], pr["centers"]
    rng = np.random.RandomState(9)
    # tensor route
    u = rng.normal(0, 100, (2, 60, 3))
    bw = so.backward(v, u, beta, g, gl)
    for _ in range(6):
        i = tuple(rng.randint(s) for s in v.shape)
        assert abs(_fd(lambda x: _loss(x, u, beta, g, gl), v, i, 1e-5) - bw["grad_v"][i]) <= 1e-6 * (1 + abs(bw["grad_v"][i]))
        k = tuple(rng.randint(s) for s in u.shape)
        assert abs(_fd(lambda x: _loss(v, x, beta, g, gl), u, k, 1e-3) - bw["grad_coords"][k]) <= 1e-7 * (1 + abs(bw["grad_coords"][k]))
    # cuboid route: u is the unrounded offset, a function of the centre
    off = lambda cc: so.cuboid_offsets(pr["position"], pr["sides"], pr["shape"], cc, np.float64)          # noqa: E731
    bw = so.backward(v, off(c), beta, g, gl, rot)
    for _ in range(6):
        i = tuple(rng.randint(s) for s in v.shape)
        assert abs(_fd(lambda x: _loss(x, off(c), beta, g, gl, rot, c), v, i, 1e-5) - bw["grad_v"][i]) <= 1e-6 * (1 + abs(bw["grad_v"][i]))
    for b in range(2):
        for r in range(3):
            fd = _fd(lambda x: _loss(v, off(x), beta, g, gl, rot, x), c, (b, r), 1e-3)
            assert abs(fd - bw["grad_center"][b, r]) <= 1e-6 * (1 + abs(fd))
            for k in range(3):
                fd = _fd(lambda x: _loss(v, off(c), beta, g, gl, x, c), rot, (b, r, k), 1e-4)
                assert abs(fd - bw["grad_rot"][b, r, k]) <= 1e-6 * (1 + abs(fd))


def test_symbols_are_declared_in_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "mvhmr_unproject.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _capi.EXPORTS, name
    assert "#define MVHMR_ABI_VERSION 4" in header                      # additive: the version stays


def test_split_mirror_gives_the_cases_the_gpu_shapes_rely_on():
    B, J, shape = SPLIT_SHAPE
    assert so.splits(B, J, int(np.prod(shape))) > 1
    B, J, shape = TILE_SHAPE
    assert so.splits(B, J, int(np.prod(shape))) == 1
    assert so.splits(32, 17, 64 ** 3) > 1 and so.splits(2048, 4, 64 ** 3) == 1 and so.splits(1, 1, 8) == 1
    # sizes only: monotone in the work per slice, never zero
    assert all(so.splits(b, j, n) >= 1 for b in (1, 7) for j in (1, 2, 3, 5, 17) for n in (1, 105, 2048, 4096, 2 ** 20))
    if os.path.exists(_capi.LIB_PATH):                                  # the library's own answer, where it is built (no device needed)
        L = _capi.lib()
        for b, j, n in ((1, 1, 32768), (3, 17, 512), (2, 5, 105), (32, 17, 64 ** 3), (1, 17, 64 ** 3), (4096, 1, 9), (1, 1, 2 ** 31 - 1)):
            assert L.mvhmr_soft_argmax3d_splits(b, j, n) == so.splits(b, j, n), (b, j, n)
            assert L.mvhmr_soft_argmax3d_workspace_bytes(2, 3, 4, 5, 6) == 2 * 3 * so.splits(2, 3, 120) * 5 * 4


def test_fake_ops_give_shapes_and_dtypes_on_meta():
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        v = torch.empty(2, 5, 3, 5, 7, device="meta", dtype=dt)
        kp, lse = softargmax.soft_argmax_3d(v, torch.empty(2, 3, 5, 7, 3, device="meta"), return_logsumexp=True)
        assert (tuple(kp.shape), kp.dtype, tuple(lse.shape), lse.dtype) == ((2, 5, 3), torch.float32, (2, 5), torch.float32)
        kp = softargmax.soft_argmax_3d_cuboid(v, torch.empty(2, 3, 3, device="meta"), torch.empty(2, 3, device="meta"), [0, 0, 0], [1, 1, 1], beta=-2.0)
        assert tuple(kp.shape) == (2, 5, 3) and kp.dtype == torch.float32
        lse, mom, g = torch.empty(2, 5, device="meta"), torch.empty(2, 5, 3, device="meta"), torch.empty(2, 5, 3, device="meta")
        gv = torch.ops.mvhmr.soft_argmax3d_backward(v, torch.empty(2, 3, 5, 7, 3, device="meta"), 1.0, lse, mom, g, None)
        assert tuple(gv.shape) == tuple(v.shape) and gv.dtype == dt
        assert tuple(torch.ops.mvhmr.soft_argmax3d_backward_coords(v, 1.0, lse, g).shape) == (2, 3, 5, 7, 3)
        gr, gc = torch.ops.mvhmr.soft_argmax3d_backward_pose(torch.empty(2, 3, 3, device="meta"), mom, g)
        assert tuple(gr.shape) == (2, 3, 3) and tuple(gc.shape) == (2, 3)


def test_bad_arguments_raise_before_anything_runs():
    v, c = torch.empty(2, 5, 3, 5, 7, device="meta"), torch.empty(2, 3, 5, 7, 3, device="meta")
    rot, cen = torch.empty(2, 3, 3, device="meta"), torch.empty(2, 3, device="meta")
    for beta in (float("nan"), float("inf"), -float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="beta"):
            softargmax.soft_argmax_3d(v, c, beta=beta)
        with pytest.raises(ValueError, match="beta"):
            softargmax.soft_argmax_3d_cuboid(v, rot, cen, [0, 0, 0], [1, 1, 1], beta=beta)
    with pytest.raises(ValueError, match=r"\(B, J, X, Y, Z\)"):
        softargmax.soft_argmax_3d(v[0], c)
    with pytest.raises(ValueError, match="coord_volumes must be"):
        softargmax.soft_argmax_3d(v, c[:, :, :, :6])                   # does not match the volume
    with pytest.raises(ValueError, match="coord_volumes must be"):
        softargmax.soft_argmax_3d(v, c[:1])
    with pytest.raises(ValueError, match="coord_volumes must be"):
        softargmax.soft_argmax_3d(v, c[..., 0])                        # wrong rank
    with pytest.raises(ValueError, match="rotations must be"):
        softargmax.soft_argmax_3d_cuboid(v, rot[:1], cen, [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError, match="centers must be"):
        softargmax.soft_argmax_3d_cuboid(v, rot, cen[:, :2], [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError, match="sides takes 3"):
        softargmax.soft_argmax_3d_cuboid(v, rot, cen, [0, 0, 0], [1, 1])
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        softargmax.soft_argmax_3d(v.double(), c)
    with pytest.raises(TypeError, match="must be a tensor"):
        softargmax.soft_argmax_3d(np.zeros((2, 5, 3, 5, 7), np.float32), c)
    with pytest.raises(RuntimeError, match="no CPU path"):
        softargmax.soft_argmax_3d(torch.zeros(1, 1, 2, 2, 2), torch.zeros(1, 2, 2, 2, 3))


def test_forward_with_pose_makes_the_same_numpy_draws_as_forward():
    """same stream position after either, the same rotations handed to the un-projection, and forward is forward_with_pose()[0]"""
    with mock.patch.object(aggregation.VolumeGenerator, "to", lambda self, *a, **k: self):   # no HIP device here
        gen = aggregation.VolumeGenerator(volume_size=4, input_channels=4, output_channels=4).train()
    batch = dict(images=torch.empty((2, 3, 32, 32, 3), device="meta"), keypoints_3d=torch.arange(2 * 17 * 3, dtype=torch.float32).view(2, 17, 3),
                 cameras_packed=dict(K=torch.eye(3).repeat(2, 3, 1, 1).double(), Rt=torch.eye(3, 4).repeat(2, 3, 1, 1).double()))
    feats, proj = torch.zeros(2, 3, 4, 5, 6), torch.zeros(2, 3, 3, 4)
    seen = []

    def stub(features, proj, rots, centers, position, sides, shape, **kw):
        seen.append((rots.clone(), centers.clone()))
        return torch.full((2, 4) + tuple(shape), float(len(seen)))

    with mock.patch.object(aggregation, "unprojection_cuboid", stub):
        np.random.seed(11)
        out_a = gen(feats, proj, batch)
        state_a = np.random.get_state()[1].copy(), np.random.get_state()[2]
        np.random.seed(11)
        out_b, rots, centers = gen.forward_with_pose(feats, proj, batch)
        state_b = np.random.get_state()[1].copy(), np.random.get_state()[2]
    assert np.array_equal(state_a[0], state_b[0]) and state_a[1] == state_b[1]
    assert len(seen) == 2 and torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])
    assert torch.equal(rots, seen[1][0]) and torch.equal(centers, seen[1][1]) and rots.dtype == torch.float32
    assert tuple(out_a.shape) == tuple(out_b.shape) == (2, 4, 4, 4, 4)
    assert torch.equal(centers, batch["keypoints_3d"][:, 6, :3])
    np.random.seed(11)
    assert np.allclose(rots[:, 0, 0].numpy(), np.cos(np.random.uniform(0.0, 2 * np.pi, size=2)).astype(np.float32))


# ---- the documented reduction order: inside the bound, and exact on the exact rig
@pytest.mark.parametrize("beta", [0.0, 1.0, 10.0, 100.0])
def test_emulated_order_stays_within_the_bound(beta):
    """20 seeds, coordinates several metres from the origin (the summation term's worst case): the fp32 emulation of the kernels' order
    against the float64 oracle, both routes.  The observed share of the bound is what DESIGN.md 5.17 quotes."""
    worst = 0.0
    for seed in range(20):
        pr = _problem(100 + seed, 1, 2, (8, 8, 16), offset=4000.0 + 500.0 * seed, spread=1.0 + seed % 3)
        d = so.cuboid_offsets(pr["position"], pr["sides"], pr["shape"], pr["centers"])
        rot = pr["rot"].astype(np.float32)
        v = pr["v"].astype(np.float32)
        # cuboid route: offsets centred on zero
        em = so.emulate_fp32(v, d, beta, 4, rot, pr["centers"].astype(np.float32))
        ref = so.forward(v, d, beta, rot, pr["centers"].astype(np.float32))
        checks = [(em["mu"], ref["mu"], so.moment_bound(v, d, beta)), (em["kp"], ref["kp"], so.keypoint_bound(v, d, beta, rot, pr["centers"].astype(np.float32))),
                  (em["L"], ref["L"], so.lse_bound(v, d, beta))]
        # tensor route: the world points themselves, metres from the origin
        w = so.world_coords(d, rot, pr["centers"]).astype(np.float32)
        em = so.emulate_fp32(v, w, beta, 4)
        ref = so.forward(v, w, beta)
        checks += [(em["kp"], ref["kp"], so.moment_bound(v, w, beta)), (em["L"], ref["L"], so.lse_bound(v, w, beta))]
        for got, want, bound in checks:
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= bound).all(), (seed, float(err.max()), float(bound.min()))
            worst = max(worst, float((err / bound).max()))
    print("beta %g: worst observed share of the bound %.3f" % (beta, worst))
    assert worst < 1.0


@pytest.mark.parametrize("shape,B,J,K", [((5, 6, 7), 2, 3, 16), ((4, 3, 6), 1, 3, 8), ((8, 8, 8), 1, 5, 256), ((2, 2, 2), 2, 2, 4)])
@pytest.mark.parametrize("itemsize", [4, 2])
def test_exact_rig_is_exact_for_the_emulated_order(shape, B, J, K, itemsize):
    """on the rig every fp32 operation of the documented order is exact: mu and keypoints equal the float64 oracle cast once, bit for bit;
    L = beta * level + ln K to a few ulp"""
    rig = so.exact_rig(5, B, J, shape, on=K)
    for beta in (1.0, 4.0):
        for u, rot, cen in ((rig["offsets"], rig["rot"], rig["centers"]), (rig["coords"], None, None)):
            em = so.emulate_fp32(rig["v"], u, beta, itemsize, rot, cen)
            ref = so.forward(rig["v"], u, beta, rot, cen)
            assert np.array_equal(em["mu"], ref["mu"].astype(np.float32)) and np.array_equal(em["kp"], ref["kp"].astype(np.float32))
            assert np.array_equal(ref["mu"].astype(np.float32).astype(np.float64), ref["mu"])        # the oracle's value IS an fp32 number
            want = np.log(rig["K"])
            assert np.abs(em["L"] - want).max() <= 4 * np.spacing(np.float32(max(want, 1.0)))
    # what makes the backward exact there too: 1/K from the stored L, and h . (u - mu) + g_L in fp32
    L = np.float32(np.float32(np.log2(np.float32(rig["K"]))) * np.float32(np.log(2.0)))
    assert np.float32(L * np.float32(so.LOG2E)) == np.float32(np.log2(rig["K"]))
    bw = so.backward(rig["v"], rig["offsets"], 1.0, rig["g"], rig["gl"], rig["rot"])
    assert np.array_equal(bw["grad_v"].astype(np.float32).astype(np.float64), bw["grad_v"])
