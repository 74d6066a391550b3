"""CPU oracle of the pose gradients of the cuboid route (mvhmr_unproject_backward_geometry_cuboid) and of the DLT triangulation's
backward (mvhmr_triangulate_dlt_backward).

TEST INFRASTRUCTURE ONLY.  The cuboid route: the voxel centres X = R d + c, d = fl(g - c), are built in fp32 with exactly the rounding of
device_common.h::voxel_xyz (so the kernels and the oracle sample the same bilinear cells), geomgrad_oracle.geometry_grad gives the
float64 gradient w.r.t. every X, and the chain rule through X = R d + c runs in float64 from the fp32 d.  The DLT: float64
torch.linalg.svd autograd of the reference's formulation (utils/multiview.py:141-168) per sample."""
import numpy as np
import torch

from geomgrad_oracle import geometry_grad
from oracle.reference_loop_torch import _fma32


def cuboid_points(rot, center, position, sides, vol):
    """fp32 (d, X), each (B, X, Y, Z, 3), in voxel_xyz's rounding: g = px + step * i (fp32 mul, add), d = g - c, X = fma chain R d + c"""
    R = torch.as_tensor(np.asarray(rot, dtype=np.float32))
    c = torch.as_tensor(np.asarray(center, dtype=np.float32))
    B = R.shape[0]
    axes = []
    for a in range(3):
        step = np.float32(float(sides[a]) / float(vol[a] - 1)) if vol[a] > 1 else np.float32(0.0)
        idx = torch.arange(vol[a], dtype=torch.float32)
        axes.append(torch.tensor(np.float32(float(position[a]))) + torch.tensor(step) * idx)
    g = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(1, -1, 3)        # (1, N, 3) fp32
    d = g - c[:, None, :]                                                              # (B, N, 3) fp32
    X = []
    for r in range(3):
        acc = d[..., 0] * R[:, r, 0:1]
        acc = _fma32(R[:, r, 1:2].expand_as(acc), d[..., 1], acc)
        acc = _fma32(R[:, r, 2:3].expand_as(acc), d[..., 2], acc)
        X.append(acc + c[:, r:r + 1])
    shape = (B,) + tuple(int(v) for v in vol) + (3,)
    return d.reshape(shape), torch.stack(X, -1).reshape(shape)


def pose_grad(features, proj, rot, center, position, sides, vol, grad_out, method):
    """-> (grad_proj (B,V,3,4), grad_rot (B,3,3), grad_center (B,3)) float64 numpy, for the cuboid recipe"""
    d, X = cuboid_points(rot, center, position, sides, vol)
    gp, gc = geometry_grad(features, proj, X, grad_out, method)
    B = gc.shape[0]
    gX = torch.from_numpy(gc).reshape(B, -1, 3)
    d64 = d.double().reshape(B, -1, 3)
    R64 = torch.as_tensor(np.asarray(rot, dtype=np.float32)).double()
    g_rot = torch.einsum("bnr,bnk->brk", gX, d64)
    s_g = gX.sum(1)
    g_cen = s_g - torch.einsum("brk,br->bk", R64, s_g)                                  # dX/dc = I - R
    return gp, g_rot.numpy(), g_cen.numpy()


def dlt_grad(proj, points, confidences, grad_out):
    """float64 autograd through the reference's DLT: proj (B,V,3,4), points (V,2) or (B,V,2), confidences None, (V,) or (B,V),
    grad_out (B,3).  -> (grad_proj (B,V,3,4), grad_points (shape of points), grad_conf (shape of confidences) or None), float64 numpy"""
    P = torch.as_tensor(np.asarray(proj, dtype=np.float32)).double().requires_grad_(True)
    uv = torch.as_tensor(np.asarray(points, dtype=np.float32)).double().requires_grad_(True)
    cf = None if confidences is None else torch.as_tensor(np.asarray(confidences, dtype=np.float32)).double().requires_grad_(True)
    go = torch.as_tensor(np.asarray(grad_out, dtype=np.float64))
    B, V = P.shape[:2]
    outs = []
    for b in range(B):
        u = uv[b] if uv.dim() == 3 else uv
        A = P[b, :, 2:3].expand(V, 2, 4) * u.view(V, 2, 1) - P[b, :, :2]
        if cf is not None:
            A = A * (cf[b] if cf.dim() == 2 else cf).view(V, 1, 1)
        _, _, vh = torch.linalg.svd(A.reshape(-1, 4), full_matrices=False)
        h = -vh[3]
        outs.append(h[:3] / h[3])
    (torch.stack(outs) * go).sum().backward()
    return P.grad.numpy(), uv.grad.numpy(), None if cf is None else cf.grad.numpy()
