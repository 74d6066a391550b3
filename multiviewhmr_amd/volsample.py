"""Trilinear volume sampling at world points: reading a volume back, the third step beside un-projection and soft-argmax.

    sample_volume_cuboid(volumes, points, rotations, centers, position, sides, *, paired=False, return_index=False)
    volumetric_cross_entropy(volumes, targets, rotations, centers, position, sides, beta=1.0)

volumes (B, C, X, Y, Z) live on the cuboid recipe of unprojection_cuboid / soft_argmax_3d_cuboid: voxel (i, j, k) of sample b sits at
rotations[b] @ (position + sides / (shape - 1) * (i, j, k) - centers[b]) + centers[b].  A world point is taken back through rotations[b]^T
(the rotations must be orthonormal; this is not checked) to its continuous voxel index t, and the volume is read there trilinearly with
zero padding (grid_sample's bilinear / zeros / align_corners=True, without the normalised grid, the axis flip and the float atomics of its
backward).  One departure: a tap of weight exactly 0 is not read, so a point on a lattice node returns the node's value even between -inf
neighbours.  Differentiable w.r.t. volumes, points, rotations and centers; every result and gradient is bitwise reproducible.  No
fallback: CPU tensors, mixed devices and a missing library raise.
"""
import torch

from . import aggregation as _agg
from .softargmax import _VOLUME_DTYPES, _check_beta, _check_device, _three, soft_argmax_3d_cuboid


def _ops():
    _agg._native()                                       # loads the extension (and the library behind it), or says how to build them
    return torch.ops.mvhmr_volsample


def _check_volumes(volumes):
    if not torch.is_tensor(volumes):
        raise TypeError("sample_volume_cuboid: volumes must be a tensor, got %s" % type(volumes).__name__)
    if volumes.dim() != 5:
        raise ValueError("sample_volume_cuboid: volumes must be (B, C, X, Y, Z), got shape %s" % (tuple(volumes.shape),))
    if volumes.dtype not in _VOLUME_DTYPES:
        raise TypeError("sample_volume_cuboid: volumes must be float32, float16 or bfloat16, got %s" % volumes.dtype)
    B, C, X, Y, Z = volumes.shape
    if B < 1 or C < 1:
        raise ValueError("sample_volume_cuboid: volumes must not be empty, got shape %s" % (tuple(volumes.shape),))
    if min(X, Y, Z) < 2:
        raise ValueError("sample_volume_cuboid: every extent must be >= 2 (a one-voxel axis has no step), got shape %s" % (tuple(volumes.shape),))
    if X * Y * Z >= 2 ** 31 or B * C >= 2 ** 31:
        raise ValueError("sample_volume_cuboid: X*Y*Z and B*C must stay below 2^31, got shape %s" % (tuple(volumes.shape),))


# ---- the ops: mvhmr::sample_volume_cuboid -> (samples, index); index is the continuous voxel index of every point, saved for the backward
def _fwd(volumes, points, rot, center, position, sides, paired):
    return tuple(_ops().sample_volume(volumes, points, rot, center, position, sides, paired))


def _fake_fwd(volumes, points, rot, center, position, sides, paired):
    B, C = volumes.shape[:2]
    N = points.shape[1]
    f32 = dict(dtype=torch.float32, device=volumes.device)
    return torch.empty((B, C) if paired else (B, C, N), **f32), torch.empty((B, N, 3), **f32)


def _fake_bwd_geometry(volumes, points, rot, center, position, sides, paired, index, grad_samples, need_points, need_pose):
    B = volumes.shape[0]
    return (points.new_empty((B if need_points else 0, points.shape[1], 3)), rot.new_empty((B if need_pose else 0, 3, 3)),
            rot.new_empty((B if need_pose else 0, 3)))


def _setup(ctx, inputs, output):
    volumes, points, rot, center, position, sides, paired = inputs
    ctx.position, ctx.sides, ctx.paired = position, sides, paired
    ctx.save_for_backward(volumes, points, rot, center, output[1])
    ctx.set_materialize_grads(False)


def _autograd(ctx, grad_samples, grad_index):
    """launches only what needs_input_grad asks for: the volume gradient, and one geometry call for points and / or the pose.  A gradient
    that arrives for `index` carries nothing and is ignored (a traced backward hands one in for every output): index is for masks"""
    volumes, points, rot, center, index = ctx.saved_tensors
    gv = gp = gr = gc = None
    if grad_samples is None:
        return (None,) * 7
    g = grad_samples.to(torch.float32).contiguous()
    need = ctx.needs_input_grad
    if need[0]:
        gv = torch.ops.mvhmr.sample_volume_backward_volumes(volumes, index, g, ctx.paired)
    if need[1] or need[2] or need[3]:
        gp, gr, gc = torch.ops.mvhmr.sample_volume_backward_geometry(volumes, points, rot, center, ctx.position, ctx.sides, ctx.paired, index, g,
                                                                     need[1], need[2] or need[3])
    return (gv, gp if need[1] else None, gr if need[2] else None, gc if need[3] else None, None, None, None)


def _register():
    if _agg._op_defined("sample_volume_cuboid"):
        return
    lib = torch.library
    place = "Tensor volumes, Tensor points, Tensor rot, Tensor center, float[] position, float[] sides, bool paired"
    lib.define("mvhmr::sample_volume_cuboid", "(%s) -> (Tensor, Tensor)" % place)
    lib.impl("mvhmr::sample_volume_cuboid", "CUDA")(_fwd)
    lib.register_fake("mvhmr::sample_volume_cuboid")(_fake_fwd)
    lib.define("mvhmr::sample_volume_backward_volumes", "(Tensor volumes, Tensor index, Tensor grad_samples, bool paired) -> Tensor")
    lib.impl("mvhmr::sample_volume_backward_volumes", "CUDA")(lambda *a: _ops().sample_volume_backward_volumes(*a))
    lib.register_fake("mvhmr::sample_volume_backward_volumes")(lambda volumes, *a: torch.empty_like(volumes))
    lib.define("mvhmr::sample_volume_backward_geometry",
               "(%s, Tensor index, Tensor grad_samples, bool need_points, bool need_pose) -> (Tensor, Tensor, Tensor)" % place)
    lib.impl("mvhmr::sample_volume_backward_geometry", "CUDA")(lambda *a: tuple(_ops().sample_volume_backward_geometry(*a)))
    lib.register_fake("mvhmr::sample_volume_backward_geometry")(_fake_bwd_geometry)
    lib.register_autograd("mvhmr::sample_volume_cuboid", _autograd, setup_context=_setup)


_register()


def sample_volume_cuboid(volumes, points, rotations, centers, position, sides, *, paired=False, return_index=False):
    """volumes (B, C, X, Y, Z) (float32 / float16 / bfloat16, every extent >= 2) read trilinearly at the world points (B, N, 3): float32
    samples (B, C, N), every point sampling every channel -- or, with paired=True (which needs N == C), (B, C): point j samples channel j
    only, the v[gt] of a volumetric cross-entropy.  With return_index also index (B, N, 3) float32, the continuous voxel index t of every
    point: a point lies inside the cuboid iff 0 <= t <= shape - 1; it is sampled (with zero padding) while -1 < t < shape, beyond that -- and
    for a NaN point -- the sample and every gradient through the point are exactly 0.  Nothing is differentiated through index: a
    gradient that reaches it is dropped.

    rotations (B, 3, 3) orthonormal, centers (B, 3): float32 on volumes' device; position, sides: 3 numbers each, the cuboid recipe of
    unprojection_cuboid.  Differentiable w.r.t. volumes, points, rotations and centers.  N = 0 returns empty results without a launch."""
    _check_volumes(volumes)
    B, C = volumes.shape[:2]
    for name, t, shape in (("points", points, (B, None, 3)), ("rotations", rotations, (B, 3, 3)), ("centers", centers, (B, 3))):
        if not torch.is_tensor(t):
            raise TypeError("sample_volume_cuboid: %s must be a tensor, got %s" % (name, type(t).__name__))
        if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
            raise ValueError("sample_volume_cuboid: %s must be %s, got %s" % (name, tuple("N" if s is None else s for s in shape), tuple(t.shape)))
    N = points.shape[1]
    if B * N >= 2 ** 31:
        raise ValueError("sample_volume_cuboid: B*N must stay below 2^31, got %d points for %d samples" % (N, B))
    if paired and N != C:
        raise ValueError("sample_volume_cuboid: paired=True samples channel j at point j and needs N == C, got N = %d, C = %d" % (N, C))
    position, sides = _three("position", position), _three("sides", sides)
    _check_device(volumes, (("points", points), ("rotations", rotations), ("centers", centers)))
    if N == 0:
        samples = torch.zeros((B, C, 0), dtype=torch.float32, device=volumes.device)
        return (samples, torch.zeros((B, 0, 3), dtype=torch.float32, device=volumes.device)) if return_index else samples
    pts, rot, center = (t.to(torch.float32).contiguous() for t in (points, rotations, centers))
    samples, index = torch.ops.mvhmr.sample_volume_cuboid(volumes.contiguous(), pts, rot, center, position, sides, bool(paired))
    return (samples, index) if return_index else samples


def volumetric_cross_entropy(volumes, targets, rotations, centers, position, sides, beta=1.0):
    """The volumetric cross-entropy of heat volumes (B, J, X, Y, Z) against world targets (B, J, 3), one per joint:
    loss (B, J) = ln sum_n exp(beta v_n) - beta * v[target], v[target] read trilinearly (sample_volume_cuboid, paired), and index (B, J, 3),
    by which a caller masks targets outside the cuboid.  Composed from soft_argmax_3d_cuboid's logsumexp and the paired sample: gradients
    reach volumes through both, and targets, rotations and centers through the sample."""
    beta = _check_beta(beta)
    _, lse = soft_argmax_3d_cuboid(volumes, rotations, centers, position, sides, beta=beta, return_logsumexp=True)
    value, index = sample_volume_cuboid(volumes, targets, rotations, centers, position, sides, paired=True, return_index=True)
    return lse - beta * value, index
