"""Volumetric 3-D soft-argmax: keypoints from heat volumes, the step after un-projection.

    soft_argmax_3d(volumes, coord_volumes, *, beta=1.0, return_logsumexp=False)
    soft_argmax_3d_cuboid(volumes, rotations, centers, position, sides, *, beta=1.0, return_logsumexp=False)

Per slice (b, j) of volumes (B, J, X, Y, Z):  p = softmax(beta * v) over the X*Y*Z voxels, keypoint = sum_n p_n x_n with x_n the voxel's
world coordinate -- from coord_volumes (B, X, Y, Z, 3), or from the cuboid recipe of unprojection_cuboid, in which case no coordinate
volume exists anywhere: the kernels accumulate the un-rotated offsets and rotate the three sums.  logsumexp (B, J) is ln sum_n exp(beta
v_n), what a volumetric cross-entropy needs beside beta * v[gt].  One pass over the volume forward, one backward; the softmaxed volume is
never stored.  Differentiable w.r.t. volumes, coord_volumes (tensor route), rotations and centers (cuboid route).  Every result and
gradient is bitwise reproducible.  No fallback: CPU tensors, mixed devices and a missing library raise.
"""
import math

import torch

from . import aggregation as _agg

_VOLUME_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _ops():
    _agg._native()                                       # loads the extension (and the library behind it), or says how to build them
    return torch.ops.mvhmr_softargmax


def _check_beta(beta):
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not math.isfinite(beta):
        raise ValueError("soft_argmax_3d: beta must be a finite Python float, got %r" % (beta,))
    return float(beta)


def _check_volumes(volumes):
    if not torch.is_tensor(volumes):
        raise TypeError("soft_argmax_3d: volumes must be a tensor, got %s" % type(volumes).__name__)
    if volumes.dim() != 5:
        raise ValueError("soft_argmax_3d: volumes must be (B, J, X, Y, Z), got shape %s" % (tuple(volumes.shape),))
    if volumes.dtype not in _VOLUME_DTYPES:
        raise TypeError("soft_argmax_3d: volumes must be float32, float16 or bfloat16, got %s" % volumes.dtype)
    if volumes.numel() == 0:
        raise ValueError("soft_argmax_3d: volumes must not be empty, got shape %s" % (tuple(volumes.shape),))
    B, J, X, Y, Z = volumes.shape
    if X * Y * Z >= 2 ** 31 or B * J >= 2 ** 31:
        raise ValueError("soft_argmax_3d: X*Y*Z and B*J must stay below 2^31, got shape %s" % (tuple(volumes.shape),))


def _check_device(volumes, others):
    if volumes.device.type == "meta":
        return
    if not volumes.is_cuda:
        raise RuntimeError("soft_argmax_3d: volumes must live on a HIP device, got %s (there is no CPU path)" % volumes.device)
    for name, t in others:
        if t.device != volumes.device:
            raise RuntimeError("soft_argmax_3d: %s is on %s, volumes on %s" % (name, t.device, volumes.device))


def _three(name, values):
    values = [float(x) for x in values]
    if len(values) != 3 or not all(math.isfinite(x) for x in values):
        raise ValueError("soft_argmax_3d_cuboid: %s takes 3 finite numbers, got %r" % (name, values))
    return values


# ---- the ops: mvhmr::soft_argmax3d[_cuboid] -> (keypoints, logsumexp, moment); moment is mu in the accumulation frame, saved for the backward
def _fwd(volumes, coords, beta):
    return tuple(_ops().soft_argmax3d(volumes, coords, beta))


def _fwd_cuboid(volumes, rot, center, position, sides, beta):
    return tuple(_ops().soft_argmax3d_cuboid(volumes, rot, center, position, sides, beta))


def _fake_fwd(volumes, *rest):
    B, J = volumes.shape[:2]
    f32 = dict(dtype=torch.float32, device=volumes.device)
    return torch.empty((B, J, 3), **f32), torch.empty((B, J), **f32), torch.empty((B, J, 3), **f32)


def _grads(grad_kp, grad_lse, grad_moment):
    """what reaches the kernels: fp32 contiguous or None.  `moment` is an output of the op only to be saved; nothing differentiates it"""
    if grad_moment is not None:
        raise RuntimeError("soft_argmax_3d: the moment output is internal and carries no gradient")
    return (None if grad_kp is None else grad_kp.contiguous(), None if grad_lse is None else grad_lse.contiguous())


def _setup(ctx, inputs, output):
    volumes, coords, beta = inputs
    ctx.beta = beta
    ctx.save_for_backward(volumes, coords, output[1], output[2])
    ctx.set_materialize_grads(False)


def _autograd(ctx, grad_kp, grad_lse, grad_moment):
    volumes, coords, lse, moment = ctx.saved_tensors
    gk, gl = _grads(grad_kp, grad_lse, grad_moment)
    gv = gc = None
    if gk is None and gl is None:
        return None, None, None
    if ctx.needs_input_grad[0]:
        gv = torch.ops.mvhmr.soft_argmax3d_backward(volumes, coords, ctx.beta, lse, moment, gk, gl)
    if ctx.needs_input_grad[1] and gk is not None:
        gc = torch.ops.mvhmr.soft_argmax3d_backward_coords(volumes, ctx.beta, lse, gk)
    return gv, gc, None


def _setup_cuboid(ctx, inputs, output):
    volumes, rot, center, position, sides, beta = inputs
    ctx.beta, ctx.position, ctx.sides = beta, position, sides
    ctx.save_for_backward(volumes, rot, center, output[1], output[2])
    ctx.set_materialize_grads(False)


def _autograd_cuboid(ctx, grad_kp, grad_lse, grad_moment):
    volumes, rot, center, lse, moment = ctx.saved_tensors
    gk, gl = _grads(grad_kp, grad_lse, grad_moment)
    gv = gr = gc = None
    if gk is None and gl is None:
        return None, None, None, None, None, None
    if ctx.needs_input_grad[0]:
        gv = torch.ops.mvhmr.soft_argmax3d_cuboid_backward(volumes, rot, center, ctx.position, ctx.sides, ctx.beta, lse, moment, gk, gl)
    if (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) and gk is not None:
        gr, gc = torch.ops.mvhmr.soft_argmax3d_backward_pose(rot, moment, gk)
    return (gv, gr if ctx.needs_input_grad[1] else None, gc if ctx.needs_input_grad[2] else None, None, None, None)


def _register():
    if _agg._op_defined("soft_argmax3d"):
        return
    lib = torch.library
    out3 = "(Tensor, Tensor, Tensor)"
    lib.define("mvhmr::soft_argmax3d", "(Tensor volumes, Tensor coords, float beta) -> " + out3)
    lib.impl("mvhmr::soft_argmax3d", "CUDA")(_fwd)
    lib.register_fake("mvhmr::soft_argmax3d")(_fake_fwd)
    lib.define("mvhmr::soft_argmax3d_cuboid", "(Tensor volumes, Tensor rot, Tensor center, float[] position, float[] sides, float beta) -> " + out3)
    lib.impl("mvhmr::soft_argmax3d_cuboid", "CUDA")(_fwd_cuboid)
    lib.register_fake("mvhmr::soft_argmax3d_cuboid")(_fake_fwd)
    tail = "float beta, Tensor logsumexp, Tensor moment, Tensor? grad_keypoints, Tensor? grad_logsumexp) -> Tensor"
    lib.define("mvhmr::soft_argmax3d_backward", "(Tensor volumes, Tensor coords, " + tail)
    lib.impl("mvhmr::soft_argmax3d_backward", "CUDA")(lambda *a: _ops().soft_argmax3d_backward(*a))
    lib.register_fake("mvhmr::soft_argmax3d_backward")(lambda volumes, *a: torch.empty_like(volumes))
    lib.define("mvhmr::soft_argmax3d_cuboid_backward", "(Tensor volumes, Tensor rot, Tensor center, float[] position, float[] sides, " + tail)
    lib.impl("mvhmr::soft_argmax3d_cuboid_backward", "CUDA")(lambda *a: _ops().soft_argmax3d_cuboid_backward(*a))
    lib.register_fake("mvhmr::soft_argmax3d_cuboid_backward")(lambda volumes, *a: torch.empty_like(volumes))
    lib.define("mvhmr::soft_argmax3d_backward_coords", "(Tensor volumes, float beta, Tensor logsumexp, Tensor grad_keypoints) -> Tensor")
    lib.impl("mvhmr::soft_argmax3d_backward_coords", "CUDA")(lambda *a: _ops().soft_argmax3d_backward_coords(*a))
    lib.register_fake("mvhmr::soft_argmax3d_backward_coords")(
        lambda volumes, beta, lse, gk: torch.empty(tuple(volumes.shape[:1]) + tuple(volumes.shape[2:]) + (3,), dtype=torch.float32, device=volumes.device))
    lib.define("mvhmr::soft_argmax3d_backward_pose", "(Tensor rot, Tensor moment, Tensor grad_keypoints) -> (Tensor, Tensor)")
    lib.impl("mvhmr::soft_argmax3d_backward_pose", "CUDA")(lambda *a: tuple(_ops().soft_argmax3d_backward_pose(*a)))
    lib.register_fake("mvhmr::soft_argmax3d_backward_pose")(lambda rot, moment, gk: (torch.empty_like(rot), rot.new_empty((rot.shape[0], 3))))
    lib.register_autograd("mvhmr::soft_argmax3d", _autograd, setup_context=_setup)
    lib.register_autograd("mvhmr::soft_argmax3d_cuboid", _autograd_cuboid, setup_context=_setup_cuboid)


_register()


def _result(outputs, return_logsumexp):
    keypoints, logsumexp, _ = outputs
    return (keypoints, logsumexp) if return_logsumexp else keypoints


def soft_argmax_3d(volumes, coord_volumes, *, beta=1.0, return_logsumexp=False):
    """Keypoints (B, J, 3) float32 of heat volumes (B, J, X, Y, Z) (float32 / float16 / bfloat16) under the voxel coordinates
    coord_volumes (B, X, Y, Z, 3): sum_n softmax_n(beta * v) x_n in fp32, and with return_logsumexp also ln sum_n exp(beta v_n), (B, J).

    beta: a finite Python float (negative: soft-argmin, 0: the centroid).  A -inf voxel counts exactly 0; a slice holding NaN, +inf or
    nothing but -inf gives NaN for that slice, as torch.softmax does.  Differentiable w.r.t. volumes and coord_volumes."""
    beta = _check_beta(beta)
    _check_volumes(volumes)
    if not torch.is_tensor(coord_volumes):
        raise TypeError("soft_argmax_3d: coord_volumes must be a tensor, got %s" % type(coord_volumes).__name__)
    B, J, X, Y, Z = volumes.shape
    if tuple(coord_volumes.shape) != (B, X, Y, Z, 3):
        raise ValueError("soft_argmax_3d: coord_volumes must be %s for volumes %s, got %s"
                         % ((B, X, Y, Z, 3), tuple(volumes.shape), tuple(coord_volumes.shape)))
    _check_device(volumes, (("coord_volumes", coord_volumes),))
    coords = coord_volumes.to(torch.float32).contiguous()
    return _result(torch.ops.mvhmr.soft_argmax3d(volumes.contiguous(), coords, beta), return_logsumexp)


def soft_argmax_3d_cuboid(volumes, rotations, centers, position, sides, *, beta=1.0, return_logsumexp=False):
    """soft_argmax_3d for volumes on the cuboid of unprojection_cuboid / VolumeGenerator, without the coordinate tensor: voxel (i, j, k) of
    sample b sits at rotations[b] @ (position + sides / (shape - 1) * (i, j, k) - centers[b]) + centers[b].

    rotations (B, 3, 3), centers (B, 3): float32 on volumes' device; position, sides: 3 numbers each.  The kernels accumulate the
    un-rotated offsets and rotate the three sums, so the result agrees with the tensor route on mvhmr_build_coord_volumes' coordinates
    to a bound, not to bits.  Differentiable w.r.t. volumes, rotations and centers."""
    beta = _check_beta(beta)
    _check_volumes(volumes)
    for name, t, shape in (("rotations", rotations, (volumes.shape[0], 3, 3)), ("centers", centers, (volumes.shape[0], 3))):
        if not torch.is_tensor(t):
            raise TypeError("soft_argmax_3d_cuboid: %s must be a tensor, got %s" % (name, type(t).__name__))
        if tuple(t.shape) != shape:
            raise ValueError("soft_argmax_3d_cuboid: %s must be %s, got %s" % (name, shape, tuple(t.shape)))
    position, sides = _three("position", position), _three("sides", sides)
    _check_device(volumes, (("rotations", rotations), ("centers", centers)))
    rot, center = rotations.to(torch.float32).contiguous(), centers.to(torch.float32).contiguous()
    return _result(torch.ops.mvhmr.soft_argmax3d_cuboid(volumes.contiguous(), rot, center, position, sides, beta), return_logsumexp)
