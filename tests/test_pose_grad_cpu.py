"""Gradients of the cuboid route w.r.t. the pose (rotations, centers) and of the DLT triangulation, without a GPU: the float64 oracle
(tests/posegrad_oracle.py) against float64 autograd through the reference's formulation and against goldens of the reference itself, the
ops' registration (shape functions, autograd formulas, which ops a backward dispatches) and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden_cases, load_golden
from posegrad_oracle import cuboid_points, dlt_grad, pose_grad
from test_geometry_grad_cpu import _OpNames, _desc, _loop64, _near_boundary, _problem
from multiviewhmr_amd import _capi, aggregation, volumetric  # noqa: F401  (registers the ops)

MODES = ("softmax", "sum", "mean", "max")
POSITION, SIDES = (-1.2, -1.1, -1.3), (2.4, 2.2, 2.6)


def _pose(B, seed):
    rng = np.random.default_rng(seed)
    rot = np.stack([volumetric.get_rotation_matrix(rng.normal(size=3), rng.uniform(0, 2 * np.pi)) for _ in range(B)]).astype(np.float32)
    center = rng.uniform(-0.2, 0.2, (B, 3)).astype(np.float32)
    return rot, center


@pytest.mark.parametrize("method", MODES)
@pytest.mark.parametrize("V", (1, 3, 4))
def test_pose_oracle_matches_float64_autograd(method, V):
    """R (g - c) + c in float64 autograd, then the reference loop, against the oracle's chain through the fp32 d"""
    vol = (5, 4, 6)
    feats, P, _, go = _problem(2, V, 5, 11, 16, vol, seed=20 * V + MODES.index(method))
    rot, center = _pose(2, seed=V + 7 * MODES.index(method))
    _, X32 = cuboid_points(rot, center, POSITION, SIDES, vol)
    near, frac = _near_boundary(feats, P, X32.numpy(), 1e-3)
    assert frac < 0.01, frac
    go = go * (~near).numpy().reshape((go.shape[0], 1) + go.shape[2:]).astype(np.float32)   # cell-boundary voxels take no part
    R = torch.from_numpy(rot).double().requires_grad_(True)
    c = torch.from_numpy(center).double().requires_grad_(True)
    p = torch.from_numpy(P).double().requires_grad_(True)
    g = (cuboid_points(np.tile(np.eye(3, dtype=np.float32), (2, 1, 1)), np.zeros((2, 3), np.float32), POSITION, SIDES, vol)[0]).double()
    X = torch.einsum("brk,bxyzk->bxyzr", R, g - c[:, None, None, None, :]) + c[:, None, None, None, :]
    _loop64(torch.from_numpy(feats).double(), p, X, method).backward(torch.from_numpy(go).double())
    gp, grot, gcen = pose_grad(feats, P, rot, center, POSITION, SIDES, vol, go, method)
    for name, mine, ref in (("proj", gp, p.grad.numpy()), ("rot", grot, R.grad.numpy()), ("center", gcen, c.grad.numpy())):
        scale = np.abs(ref).max()
        assert scale > 0, name
        err = np.abs(mine - ref).max()
        assert err <= 1e-4 * scale, (name, err, scale)


def test_pose_oracle_gives_a_zero_center_gradient_for_the_identity():
    vol = (4, 5, 3)
    feats, P, _, go = _problem(1, 3, 4, 10, 12, vol, seed=3)
    _, grot, gcen = pose_grad(feats, P, np.eye(3, dtype=np.float32)[None], np.array([[0.1, -0.05, 0.02]], np.float32), POSITION, SIDES, vol,
                              go, "softmax")
    assert np.abs(grot).max() > 0 and (gcen == 0).all()


def _rig(B, V, seed, noise=1.0):
    rng = np.random.default_rng(seed)
    P = np.zeros((B, V, 3, 4), np.float32)
    for b in range(B):
        for v in range(V):
            az = 2 * np.pi * v / V + 0.3 * b
            eye = np.array([np.cos(az), np.sin(az), 0.2]) * 5000.0
            fwd = -eye / np.linalg.norm(eye)
            right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
            R = np.stack([right, np.cross(fwd, right), fwd])
            K = np.array([[1100.0, 0, 480 + rng.uniform(-5, 5)], [0, 1100.0, 480 + rng.uniform(-5, 5)], [0, 0, 1]])
            P[b, v] = K @ np.hstack([R, (-R @ eye)[:, None]])
    X = rng.uniform(-400, 400, (B, 3))
    r = np.einsum("bvij,bj->bvi", P.astype(np.float64), np.concatenate([X, np.ones((B, 1))], 1))
    uv = (r[..., :2] / r[..., 2:3] + rng.normal(0, noise, (B, V, 2))).astype(np.float32)
    conf = rng.uniform(0.3, 1.0, (B, V)).astype(np.float32)
    go = rng.standard_normal((B, 3)).astype(np.float32)
    return P, uv, conf, go


def _eig_dlt_grad(P, uv, conf, go):
    """the kernel's formulation in float64 numpy: eigenpairs of A^T A, G = sum_k (e_k . gh) / (l_m - l_k) e_k h^T, g a_r = 2 sym(G) a_r"""
    B, V = P.shape[:2]
    gP, gU, gC = np.zeros((B, V, 3, 4)), np.zeros((B, V, 2)), np.zeros((B, V))
    for b in range(B):
        u = uv[b] if uv.ndim == 3 else uv
        c = np.ones(V) if conf is None else (conf[b] if conf.ndim == 2 else conf)
        Pb = P[b].astype(np.float64)
        a0 = Pb[:, 2:3, :] * u.astype(np.float64)[:, :, None] - Pb[:, :2, :]                 # (V, 2, 4)
        A = (a0 * c[:, None, None]).reshape(-1, 4)
        lam, E = np.linalg.eigh(A.T @ A)
        h = E[:, 0]
        gx = go[b].astype(np.float64)
        gh = np.concatenate([gx / h[3], [-(gx @ h[:3]) / h[3] ** 2]])
        G = sum(((E[:, k] @ gh) / (lam[0] - lam[k])) * np.outer(E[:, k], h) for k in range(1, 4))
        ga = 2.0 * (A @ (0.5 * (G + G.T)).T).reshape(V, 2, 4)                                  # rows of 2 sym(G) a_r
        gC[b] = (a0 * ga).sum((1, 2))
        gP[b, :, 2, :] = (c[:, None, None] * u[:, :, None] * ga).sum(1)
        gP[b, :, :2, :] -= c[:, None, None] * ga
        gU[b] = (c[:, None, None] * Pb[:, 2:3, :] * ga).sum(2)
    return gP, gU, gC


@pytest.mark.parametrize("V", (2, 3, 4, 8))
@pytest.mark.parametrize("shared_points", (False, True))
@pytest.mark.parametrize("conf_mode", ("none", "shared", "per_sample"))
def test_dlt_oracle_matches_the_eigen_formulation(V, shared_points, conf_mode):
    """the float64 SVD autograd oracle against the closed form the kernel evaluates (both sum shared inputs over the batch)"""
    P, uv, conf, go = _rig(3, V, seed=V)
    if shared_points:
        uv = uv[0]
    conf = None if conf_mode == "none" else conf[0] if conf_mode == "shared" else conf
    gP, gU, gC = dlt_grad(P, uv, conf, go)
    eP, eU, eC = _eig_dlt_grad(P, uv, conf, go)
    if shared_points:
        eU = eU.sum(0)
    if conf is not None and conf.ndim == 1:
        eC = eC.sum(0)
    pairs = [("proj", gP, eP), ("points", gU, eU)] + ([("conf", gC, eC)] if conf is not None else [])
    for name, mine, ref in pairs:
        scale = np.abs(ref).max()
        assert scale > 0, name
        assert np.abs(mine - ref).max() <= 1e-6 * scale, (name, np.abs(mine - ref).max(), scale)


def test_dlt_golden_matches_the_oracle():
    """the reference's fp32 torch.svd backward, per sample with confidences, against the float64 oracle"""
    d = load_golden("posegrad", "dlt_conf_v4")
    gP, gU, gC = dlt_grad(d["proj"], d["points"], d["confidences"], d["grad_out"])
    for name, mine, ref in (("proj", gP, d["gproj"]), ("points", gU, d["gpoints"]), ("conf", gC, d["gconf"])):
        scale = np.abs(mine).max()
        assert np.abs(mine - ref).max() <= 1e-2 * scale, (name, np.abs(mine - ref).max(), scale)


@pytest.mark.parametrize("case", [c for c in golden_cases("posegrad") if not c.startswith("dlt")])
def test_volume_generator_goldens_match_the_oracle(case):
    """VolumeGenerator(use_triangulation=True): the reference's proj_matricies gradient against the oracle evaluated at the pivot the
    reference itself triangulated (fp32 torch.svd).  At the float64 pivot (the stored oracle value, what the GPU test bounds against)
    the two differ by more -- the fp32 pivot moves voxels across cells -- and that distance is the reference's own fp32 error."""
    d = load_golden("posegrad", case)
    B, V, _, _, S = (int(x) for x in d["meta"][:5])
    uv, method = d["images_center"], str(d["method"])
    pos, sides = [-1250.0] * 3, [2500.0] * 3
    # process_feature (the 1x1 conv) recomputed from the stored input and parameters: the golden keeps only what rebuilds the call
    fin = torch.from_numpy(d["features_in"])
    conv = torch.nn.functional.conv2d(fin.flatten(0, 1), torch.from_numpy(d["weight"]), torch.from_numpy(d["bias"]))
    feats = conv.view(fin.shape[:2] + conv.shape[1:]).numpy()
    _, _, gcen = pose_grad(feats, d["proj"], d["rot"], d["center"], pos, sides, (S, S, S), d["grad_out"], method)
    stored = d["oracle_gproj_org"]
    scale = np.abs(stored).max()
    # the stored oracle is this oracle (up to the last bits of the host's conv, which need not be the generating host's)
    assert np.abs(dlt_grad(d["proj_org"], uv, None, gcen)[0] - stored).max() <= 1e-6 * max(scale, 1e-30)
    if not int(d["meta"][5]):                              # eval: R = I, the pivot's gradient is exactly zero in the reference too
        assert scale == 0 and (d["gproj_org"] == 0).all()
        return
    _, _, gcen_ref = pose_grad(feats, d["proj"], d["rot"], d["ref_center"], pos, sides, (S, S, S), d["grad_out"], method)
    at_ref = dlt_grad(d["proj_org"], uv, None, gcen_ref)[0]
    assert np.abs(at_ref - d["gproj_org"]).max() <= 1e-3 * np.abs(d["gproj_org"]).max()
    assert np.abs(d["gproj_org"] - stored).max() <= 0.1 * scale      # the reference's fp32 error (observed 3e-4 and 4e-4 of the scale)


def test_fake_tensor_autograd_gives_pose_and_dlt_gradients():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty(2, 4, 8, 24, 20, requires_grad=True)
        p = torch.empty(2, 4, 3, 4, requires_grad=True)
        r = torch.empty(2, 3, 3, requires_grad=True)
        c = torch.empty(2, 3, requires_grad=True)
        o = torch.ops.mvhmr.unprojection_cuboid(f, p, r, c, [-1.0] * 3, [2.0] * 3, [8, 6, 5], 0, _capi.F32, 0)
        o.sum().backward()
        assert tuple(p.grad.shape) == (2, 4, 3, 4) and tuple(r.grad.shape) == (2, 3, 3) and tuple(c.grad.shape) == (2, 3)
        assert tuple(f.grad.shape) == tuple(f.shape)
        P = torch.empty(5, 3, 3, 4, requires_grad=True)
        uv = torch.empty(3, 2, requires_grad=True)
        cf = torch.empty(5, 3, requires_grad=True)
        x = torch.ops.mvhmr.triangulate_dlt(P, uv, cf)
        assert tuple(x.shape) == (5, 3)
        x.sum().backward()
        assert tuple(P.grad.shape) == (5, 3, 3, 4) and tuple(uv.grad.shape) == (3, 2) and tuple(cf.grad.shape) == (5, 3)


def _recorded_cuboid_backward(rot_grad):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty(1, 2, 4, 6, 6, requires_grad=True)
        r = torch.empty(1, 3, 3, requires_grad=rot_grad)
        o = torch.ops.mvhmr.unprojection_cuboid(f, torch.empty(1, 2, 3, 4), r, torch.empty(1, 3), [-1.0] * 3, [2.0] * 3, [3, 3, 3], 0,
                                                _capi.F32, 0)
        rec = _OpNames()
        with rec:
            o.sum().backward()
    return rec.names


def test_features_only_cuboid_backward_never_dispatches_the_geometry_op():
    names = _recorded_cuboid_backward(False)
    assert any("mvhmr.unprojection_cuboid_backward." in n for n in names), names
    assert not any("unprojection_cuboid_backward_geometry" in n for n in names), names
    assert any("unprojection_cuboid_backward_geometry" in n for n in _recorded_cuboid_backward(True))


def _call_cuboid(d, grad_proj=1, grad_rot=1, grad_center=1):
    """the validation paths return before anything touches the (dummy, never dereferenced) pointers"""
    L = _capi.lib()
    dummy = ctypes.c_void_p(256)
    pos = (ctypes.c_double * 3)(-1.0, -1.0, -1.0)
    sides = (ctypes.c_double * 3)(2.0, 2.0, 2.0)
    nul = ctypes.c_void_p(0)
    return L.mvhmr_unproject_backward_geometry_cuboid(ctypes.byref(d), dummy, dummy, dummy, dummy, dummy, pos, sides,
                                                      dummy if grad_proj else nul, dummy if grad_rot else nul, dummy if grad_center else nul,
                                                      nul, 0, nul)


def test_cuboid_c_abi_validation():
    L = _capi.lib()
    assert _call_cuboid(_desc(), 0, 0, 0) == _capi.ERR_INVALID_ARGUMENT
    assert b"all null" in L.mvhmr_last_error()
    assert _call_cuboid(_desc(views=17)) == _capi.ERR_UNSUPPORTED
    assert _call_cuboid(_desc(feat_layout=_capi.LAYOUT_QUAD_LOG2E)) == _capi.ERR_UNSUPPORTED
    assert _call_cuboid(_desc(feat_layout=_capi.LAYOUT_QUAD, channels=6)) == _capi.ERR_UNSUPPORTED
    assert _call_cuboid(_desc(abi_version=3)) == _capi.ERR_INVALID_ARGUMENT
    for outs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        assert _call_cuboid(_desc(), *outs) == _capi.ERR_WORKSPACE           # a valid request without workspace: refused before any launch


def test_cuboid_c_abi_workspace_bytes():
    L = _capi.lib()
    tiles = (8 * 6 * 5 + 31) // 32
    up = lambda n: (n + 255) // 256 * 256                                    # noqa: E731
    part, pose = up(2 * tiles * 4 * 12 * 4), up(2 * tiles * 12 * 4)
    featT = 2 * 4 * 24 * 20 * 32 * 4
    assert L.mvhmr_unproject_backward_geometry_cuboid_workspace_bytes(ctypes.byref(_desc())) == featT + part + pose
    assert L.mvhmr_unproject_backward_geometry_cuboid_workspace_bytes(ctypes.byref(_desc(feat_layout=_capi.LAYOUT_BVHWC))) == part + pose
    assert L.mvhmr_unproject_backward_geometry_cuboid_workspace_bytes(ctypes.byref(_desc(feat_layout=_capi.LAYOUT_QUAD_LOG2E))) == 0


def test_dlt_backward_c_abi_validation():
    L = _capi.lib()
    dummy, nul = ctypes.c_void_p(256), ctypes.c_void_p(0)
    assert L.mvhmr_triangulate_dlt_backward(dummy, dummy, nul, dummy, nul, nul, nul, 2, 3, 0, 0, nul) == _capi.ERR_INVALID_ARGUMENT
    assert b"all null" in L.mvhmr_last_error()
    assert L.mvhmr_triangulate_dlt_backward(dummy, dummy, nul, nul, dummy, nul, nul, 2, 3, 0, 0, nul) == _capi.ERR_INVALID_ARGUMENT
    assert L.mvhmr_triangulate_dlt_backward(dummy, dummy, nul, dummy, dummy, nul, nul, 0, 3, 0, 0, nul) == _capi.ERR_INVALID_ARGUMENT
    assert L.mvhmr_triangulate_dlt_backward(dummy, dummy, nul, dummy, dummy, nul, nul, 2, 0, 0, 0, nul) == _capi.ERR_INVALID_ARGUMENT
