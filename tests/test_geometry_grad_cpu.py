"""Gradients of unprojection w.r.t. proj_matricies and coord_volumes, without a GPU: the float64 oracle (tests/geomgrad_oracle.py)
against autograd through the reference graph (a float64 restatement, and goldens of the reference itself), the op's registration
(shape functions, autograd formula, which ops a backward dispatches) and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_cases, load_golden
from geomgrad_oracle import geometry_grad, sample_cells
from multiviewhmr_amd import _capi, aggregation  # noqa: F401  (registers the ops)

MODES = ("softmax", "sum", "mean", "max")


def _loop64(features, proj, coords, method):
    """models/aggregation.py:20-87 in float64 with out-of-place masking: the graph autograd differentiates"""
    B, V, C, H, W = features.shape
    vol = tuple(coords.shape[1:4])
    scale = torch.tensor([float(H), float(W)], dtype=torch.float64)       # quirk Q1
    outs = []
    for b in range(B):
        pts = coords[b].reshape(-1, 3)
        ph = torch.cat([pts, torch.ones(pts.shape[0], 1, dtype=pts.dtype)], 1)
        stack = []
        for v in range(V):
            pr = ph @ proj[b, v].t()
            behind = pr[:, 2] <= 0
            depth = torch.where(pr[:, 2] == 0, torch.ones_like(pr[:, 2]), pr[:, 2])
            grid = 2.0 * (pr[:, :2] / depth[:, None] / scale - 0.5)
            s = F.grid_sample(features[b, v][None], grid[None, :, None, :], mode="bilinear", padding_mode="zeros", align_corners=True)
            stack.append(s.reshape(C, -1).masked_fill(behind[None], 0.0))
        st = torch.stack(stack)
        if method == "sum":
            r = st.sum(0)
        elif method == "mean":
            r = st.mean(0)
        elif method == "max":
            r = st.max(0)[0]
        else:
            r = (st * torch.softmax(st, dim=0)).sum(0)
        outs.append(r.reshape((C,) + vol))
    return torch.stack(outs)


def _problem(B, V, C, H, W, vol, seed):
    """cameras a few units from a unit-scale volume (well conditioned); some voxels behind a camera, some outside the frame"""
    rng = np.random.default_rng(seed)
    P = np.zeros((B, V, 3, 4), np.float32)
    for b in range(B):
        for v in range(V):
            az = 2 * np.pi * v / V + 0.4 * b + 0.1
            eye = np.array([np.cos(az), np.sin(az), 0.3]) * (1.6 if v == 0 else 4.0)   # view 0 sits inside the volume's reach
            fwd = -eye / np.linalg.norm(eye)
            right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
            down = np.cross(fwd, right)
            R = np.stack([right, down, fwd])
            K = np.array([[1.3 * H, 0, H / 2 + rng.uniform(-1, 1)], [0, 1.3 * W, W / 2 + rng.uniform(-1, 1)], [0, 0, 1]])
            P[b, v] = K @ np.hstack([R, (-R @ eye)[:, None]])
    g = np.stack(np.meshgrid(*[np.linspace(-1.2, 1.2, n) for n in vol], indexing="ij"), -1)
    coords = (g[None] + rng.uniform(-0.05, 0.05, (B,) + vol + (3,))).astype(np.float32)
    feats = rng.standard_normal((B, V, C, H, W)).astype(np.float32)
    go = rng.standard_normal((B, C) + vol).astype(np.float32)
    return feats, P, coords, go


def _near_boundary(feats, P, coords, tol):
    """(voxel mask (B,N): any taking-part view samples within tol px of a cell boundary, fraction of such (voxel, view) samples)"""
    B, V, C, H, W = feats.shape
    near, hits, total = [], 0, 0
    for b in range(B):
        pts = torch.from_numpy(coords[b].reshape(-1, 3))
        m = torch.zeros(pts.shape[0], dtype=torch.bool)
        for v in range(V):
            _, _, z, ix, iy = sample_cells(torch.from_numpy(P[b, v]), pts, H, W)
            ix, iy = ix.double(), iy.double()
            part = (z > 0) & (ix >= -1) & (ix < W) & (iy >= -1) & (iy < H)
            close = part & (((ix - ix.round()).abs() < tol) | ((iy - iy.round()).abs() < tol))
            m |= close
            hits += int(close.sum()); total += pts.shape[0]
        near.append(m)
    return torch.stack(near), hits / total


@pytest.mark.parametrize("method", MODES)
@pytest.mark.parametrize("V", (1, 3, 4))
def test_oracle_matches_float64_autograd(method, V):
    feats, P, coords, go = _problem(2, V, 5, 11, 16, (5, 4, 6), seed=10 * V + MODES.index(method))
    near, frac = _near_boundary(feats, P, coords, 1e-3)
    assert frac < 0.01, frac                    # (voxel, view) samples within 1e-3 px of a cell boundary
    go = go * (~near).numpy().reshape((go.shape[0], 1) + go.shape[2:]).astype(np.float32)   # those voxels take no part
    f = torch.from_numpy(feats).double()
    p = torch.from_numpy(P).double().requires_grad_(True)
    c = torch.from_numpy(coords).double().requires_grad_(True)
    out = _loop64(f, p, c, method)
    out.backward(torch.from_numpy(go).double())
    gp, gc = geometry_grad(feats, P, coords, go, method)
    # the geometry must exercise every branch: views behind a camera and samples outside the frame
    zs = [sample_cells(torch.from_numpy(P[b, v]), torch.from_numpy(coords[b].reshape(-1, 3)), 11, 16)[2] for b in range(2) for v in range(V)]
    assert any(bool((z <= 0).any()) for z in zs) and any(bool((z > 0).any()) for z in zs)
    for name, mine, ref in (("proj", gp, p.grad.numpy()), ("coords", gc, c.grad.numpy())):
        scale = np.abs(ref).max()
        assert scale > 0
        err = np.abs(mine - ref).max()
        assert err <= 1e-4 * scale, (name, err, scale)


@pytest.mark.parametrize("case", golden_cases("geomgrad"))
def test_reference_goldens_match_the_oracle(case):
    d = load_golden("geomgrad", case)
    for method in MODES:
        gp, gc = geometry_grad(d["features"], d["proj"], d["coords"], d["grad_out"], method)
        for name, mine, ref in (("proj", gp, d["gproj_" + method]), ("coords", gc, d["gcoords_" + method])):
            scale = np.abs(ref).max()
            assert scale > 0
            err = np.abs(mine - ref).max()
            assert err <= 1e-4 * scale, (case, method, name, err, scale)


def test_fake_tensor_autograd_gives_geometry_gradients():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty(2, 4, 8, 24, 20, requires_grad=True)
        p = torch.empty(2, 4, 3, 4, requires_grad=True)
        c = torch.empty(2, 8, 6, 5, 3, requires_grad=True)
        o = torch.ops.mvhmr.unprojection(f, p, c, 0, _capi.F32, 0)
        o.sum().backward()
        assert p.grad is not None and c.grad is not None
        assert tuple(p.grad.shape) == tuple(p.shape) and tuple(c.grad.shape) == tuple(c.shape)
        assert tuple(f.grad.shape) == tuple(f.shape)
        # geometry only: the result still has a grad_fn
        p2 = torch.empty(2, 4, 3, 4, requires_grad=True)
        o2 = torch.ops.mvhmr.unprojection(torch.empty(2, 4, 8, 24, 20), p2, torch.empty(2, 8, 6, 5, 3), 3, _capi.F32, 0)
        assert o2.grad_fn is not None
        o2.sum().backward()
        assert tuple(p2.grad.shape) == (2, 4, 3, 4)


class _OpNames(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


def _recorded_backward(grad_proj):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty(1, 2, 4, 6, 6, requires_grad=True)
        p = torch.empty(1, 2, 3, 4, requires_grad=grad_proj)
        o = torch.ops.mvhmr.unprojection(f, p, torch.empty(1, 3, 3, 3, 3), 0, _capi.F32, 0)
        rec = _OpNames()
        with rec:
            o.sum().backward()
    return rec.names


def test_features_only_backward_never_dispatches_the_geometry_op():
    names = _recorded_backward(False)
    assert any("mvhmr.unprojection_backward." in n for n in names), names
    assert not any("unprojection_backward_geometry" in n for n in names), names
    assert any("unprojection_backward_geometry" in n for n in _recorded_backward(True))


def _desc(**kw):
    d = _capi.Desc()
    d.abi_version = _capi.ABI_VERSION
    d.batch, d.views, d.channels, d.feat_h, d.feat_w = 2, 4, 32, 24, 20
    d.vol_x, d.vol_y, d.vol_z = 8, 6, 5
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(d, grad_proj=1, grad_coords=1):
    """the validation paths return before anything touches the (dummy, never dereferenced) pointers"""
    L = _capi.lib()
    dummy = ctypes.c_void_p(256)
    return L.mvhmr_unproject_backward_geometry(ctypes.byref(d), dummy, dummy, dummy, dummy,
                                               dummy if grad_proj else ctypes.c_void_p(0), dummy if grad_coords else ctypes.c_void_p(0),
                                               ctypes.c_void_p(0), 0, ctypes.c_void_p(0))


def test_c_abi_validation():
    L = _capi.lib()
    assert _call(_desc(), 0, 0) == _capi.ERR_INVALID_ARGUMENT
    assert b"both null" in L.mvhmr_last_error()
    assert _call(_desc(views=17)) == _capi.ERR_UNSUPPORTED
    assert _call(_desc(feat_layout=_capi.LAYOUT_QUAD_LOG2E)) == _capi.ERR_UNSUPPORTED
    assert _call(_desc(abi_version=3)) == _capi.ERR_INVALID_ARGUMENT
    assert _call(_desc(feat_layout=_capi.LAYOUT_QUAD, channels=6)) == _capi.ERR_UNSUPPORTED
    assert _call(_desc()) == _capi.ERR_WORKSPACE                       # valid request, no workspace: refused before any launch


def test_c_abi_workspace_bytes():
    L = _capi.lib()
    d = _desc()
    ws = L.mvhmr_unproject_backward_geometry_workspace_bytes(ctypes.byref(d))
    tiles = (8 * 6 * 5 + 31) // 32
    part = 2 * tiles * 4 * 12 * 4
    featT = 2 * 4 * 24 * 20 * 32 * 4
    assert ws == featT + (part + 255) // 256 * 256
    d_cl = _desc(feat_layout=_capi.LAYOUT_BVHWC)
    assert L.mvhmr_unproject_backward_geometry_workspace_bytes(ctypes.byref(d_cl)) == (part + 255) // 256 * 256
    assert L.mvhmr_unproject_backward_geometry_workspace_bytes(ctypes.byref(_desc(feat_layout=_capi.LAYOUT_QUAD_LOG2E))) == 0
