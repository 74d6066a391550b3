"""3-D non-maximum suppression and top-K proposals from heat volumes: the discrete step between a heat volume and one fine volume per
candidate.

    volume_peaks(volumes, k, *, radius=1, threshold=None) -> (scores, index)
    volume_peaks_cuboid(volumes, rotations, centers, position, sides, k, *, radius=1, threshold=None) -> (scores, index, positions)
    peak_proposals(scores, index, positions) -> (centers, feature_index, valid)

Per slice (b, j) of volumes (B, J, X, Y, Z), voxel n = (i*Y + j)*Z + k is a peak iff no value in its box [i-r, i+r] x [j-r, j+r] x
[k-r, k+r] (clipped to the volume) is NaN, v_n >= every value in the box (a plateau is all peaks; -0 equals +0) and v_n > threshold,
strictly.  The K outputs are the slice's peaks by value descending, ties by ascending n; slots beyond the number of peaks hold
scores = -inf, index = -1, positions = 0.  One read of the volume, O(B J K) numbers written, every output a function of the input bits.
scores is differentiable w.r.t. volumes (a scatter), positions w.r.t. rotations and centers; nothing is differentiated through index.
No fallback: CPU tensors, mixed devices and a missing library raise.
"""
import math
import numbers

import torch

from . import aggregation as _agg

_VOLUME_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
MAX_K = 128                                              # mvhmr_volume_peaks_max_k(): a constant of the library
MAX_RADIUS = 3


def _ops():
    _agg._native()                                       # loads the extension (and the library behind it), or says how to build them
    return torch.ops.mvhmr_peaks


def _check_int(name, value, lo, hi):
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
        raise ValueError("volume_peaks: %s must be an int in %d .. %d, got %r" % (name, lo, hi, value))
    return value


def _check_threshold(threshold):
    """the threshold as the fp32 the kernel compares with; None is -inf"""
    if threshold is None:
        return -math.inf
    if isinstance(threshold, bool) or not isinstance(threshold, numbers.Real) or math.isnan(threshold):      # numpy scalars are Real; tensors, str, bool are not taken
        raise ValueError("volume_peaks: threshold must be None or a real number that is not NaN, got %r" % (threshold,))
    return float(torch.tensor(float(threshold), dtype=torch.float32))


def _check_volumes(volumes):
    if not torch.is_tensor(volumes):
        raise TypeError("volume_peaks: volumes must be a tensor, got %s" % type(volumes).__name__)
    if volumes.dim() != 5:
        raise ValueError("volume_peaks: volumes must be (B, J, X, Y, Z), got shape %s" % (tuple(volumes.shape),))
    if volumes.dtype not in _VOLUME_DTYPES:
        raise TypeError("volume_peaks: volumes must be float32, float16 or bfloat16, got %s" % volumes.dtype)
    if volumes.numel() == 0:
        raise ValueError("volume_peaks: volumes must not be empty, got shape %s" % (tuple(volumes.shape),))
    B, J, X, Y, Z = volumes.shape
    if X * Y * Z >= 2 ** 31 or B * J >= 2 ** 31:
        raise ValueError("volume_peaks: X*Y*Z and B*J must stay below 2^31, got shape %s" % (tuple(volumes.shape),))


def _check_device(volumes, others):
    if volumes.device.type == "meta":
        return
    if not volumes.is_cuda:
        raise RuntimeError("volume_peaks: volumes must live on a HIP device, got %s (there is no CPU path)" % volumes.device)
    for name, t in others:
        if t.device != volumes.device:
            raise RuntimeError("volume_peaks: %s is on %s, volumes on %s" % (name, t.device, volumes.device))


def _three(name, values):
    values = [float(x) for x in values]
    if len(values) != 3 or not all(math.isfinite(x) for x in values):
        raise ValueError("volume_peaks_cuboid: %s takes 3 finite numbers, got %r" % (name, values))
    return values


# ---- the ops: mvhmr::volume_peaks -> (scores, index), mvhmr::volume_peaks_cuboid -> (scores, index, positions)
def _fake_fwd(volumes, k, radius, threshold):
    B, J = volumes.shape[:2]
    return (torch.empty((B, J, k), dtype=torch.float32, device=volumes.device), torch.empty((B, J, k), dtype=torch.int32, device=volumes.device))


def _fake_fwd_cuboid(volumes, rot, center, position, sides, k, radius, threshold):
    B, J = volumes.shape[:2]
    return _fake_fwd(volumes, k, radius, threshold) + (torch.empty((B, J, k, 3), dtype=torch.float32, device=volumes.device),)


def _setup(ctx, inputs, output):
    ctx.shape, ctx.dtype = tuple(inputs[0].shape), inputs[0].dtype
    ctx.save_for_backward(output[1])
    ctx.set_materialize_grads(False)


def _autograd(ctx, grad_scores, grad_index):
    (index,) = ctx.saved_tensors
    gv = None
    if grad_scores is not None and ctx.needs_input_grad[0]:
        gv = torch.ops.mvhmr.volume_peaks_backward(index, grad_scores.to(torch.float32).contiguous(), ctx.shape, ctx.dtype)
    return gv, None, None, None


def _setup_cuboid(ctx, inputs, output):
    volumes, rot, center, position, sides = inputs[:5]
    ctx.shape, ctx.dtype, ctx.position, ctx.sides = tuple(volumes.shape), volumes.dtype, position, sides
    ctx.save_for_backward(output[1], rot, center)
    ctx.set_materialize_grads(False)


def _autograd_cuboid(ctx, grad_scores, grad_index, grad_positions):
    index, rot, center = ctx.saved_tensors
    gv = gr = gc = None
    if grad_scores is not None and ctx.needs_input_grad[0]:
        gv = torch.ops.mvhmr.volume_peaks_backward(index, grad_scores.to(torch.float32).contiguous(), ctx.shape, ctx.dtype)
    if grad_positions is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
        gr, gc = torch.ops.mvhmr.volume_peaks_backward_pose(index, grad_positions.to(torch.float32).contiguous(), rot, center, ctx.position, ctx.sides,
                                                            list(ctx.shape[2:]))
    return (gv, gr if ctx.needs_input_grad[1] else None, gc if ctx.needs_input_grad[2] else None, None, None, None, None, None)


def _register():
    if _agg._op_defined("volume_peaks"):
        return
    lib = torch.library
    lib.define("mvhmr::volume_peaks", "(Tensor volumes, int k, int radius, float threshold) -> (Tensor, Tensor)")
    lib.impl("mvhmr::volume_peaks", "CUDA")(lambda *a: tuple(_ops().volume_peaks(*a)))
    lib.register_fake("mvhmr::volume_peaks")(_fake_fwd)
    lib.define("mvhmr::volume_peaks_cuboid",
               "(Tensor volumes, Tensor rot, Tensor center, float[] position, float[] sides, int k, int radius, float threshold) -> (Tensor, Tensor, Tensor)")
    lib.impl("mvhmr::volume_peaks_cuboid", "CUDA")(lambda *a: tuple(_ops().volume_peaks_cuboid(*a)))
    lib.register_fake("mvhmr::volume_peaks_cuboid")(_fake_fwd_cuboid)
    lib.define("mvhmr::volume_peaks_backward", "(Tensor index, Tensor grad_scores, int[] shape, ScalarType dtype) -> Tensor")
    lib.impl("mvhmr::volume_peaks_backward", "CUDA")(lambda *a: _ops().volume_peaks_backward(*a))
    lib.register_fake("mvhmr::volume_peaks_backward")(lambda index, g, shape, dtype: torch.empty(tuple(shape), dtype=dtype, device=index.device))
    lib.define("mvhmr::volume_peaks_backward_pose",
               "(Tensor index, Tensor grad_positions, Tensor rot, Tensor center, float[] position, float[] sides, int[] vol) -> (Tensor, Tensor)")
    lib.impl("mvhmr::volume_peaks_backward_pose", "CUDA")(lambda *a: tuple(_ops().volume_peaks_backward_pose(*a)))
    lib.register_fake("mvhmr::volume_peaks_backward_pose")(lambda index, g, rot, *a: (torch.empty_like(rot), rot.new_empty((rot.shape[0], 3))))
    lib.register_autograd("mvhmr::volume_peaks", _autograd, setup_context=_setup)
    lib.register_autograd("mvhmr::volume_peaks_cuboid", _autograd_cuboid, setup_context=_setup_cuboid)


_register()


def volume_peaks(volumes, k, *, radius=1, threshold=None):
    """The k largest local maxima of every slice of heat volumes (B, J, X, Y, Z) (float32 / float16 / bfloat16): (scores (B, J, k) float32,
    index (B, J, k) int32), index the flat voxel index (i*Y + j)*Z + k.

    k: int in 1 .. 128.  radius: int in 0 .. 3, the half-width of the suppression box (0: a plain thresholded top-k); it may exceed an
    extent.  threshold: None (-inf) or a number, rounded to float32; a peak is strictly above it.  Order: value descending, ties by
    ascending index.  Missing slots: scores -inf, index -1.  scores is differentiable w.r.t. volumes."""
    k, radius = _check_int("k", k, 1, MAX_K), _check_int("radius", radius, 0, MAX_RADIUS)
    threshold = _check_threshold(threshold)
    _check_volumes(volumes)
    _check_device(volumes, ())
    return torch.ops.mvhmr.volume_peaks(volumes.contiguous(), k, radius, threshold)


def volume_peaks_cuboid(volumes, rotations, centers, position, sides, k, *, radius=1, threshold=None):
    """volume_peaks for volumes on the cuboid of unprojection_cuboid / VolumeGenerator, with the peaks' world positions (B, J, k, 3) float32:
    voxel (i, j, k) of sample b sits at rotations[b] @ (position + sides / (shape - 1) * (i, j, k) - centers[b]) + centers[b], bit-equal to
    the coordinate volume's entry at that index; missing slots hold 0.

    rotations (B, 3, 3), centers (B, 3): float32 on volumes' device; position, sides: 3 numbers each.  positions is differentiable w.r.t.
    rotations and centers, scores w.r.t. volumes."""
    k, radius = _check_int("k", k, 1, MAX_K), _check_int("radius", radius, 0, MAX_RADIUS)
    threshold = _check_threshold(threshold)
    _check_volumes(volumes)
    for name, t, shape in (("rotations", rotations, (volumes.shape[0], 3, 3)), ("centers", centers, (volumes.shape[0], 3))):
        if not torch.is_tensor(t):
            raise TypeError("volume_peaks_cuboid: %s must be a tensor, got %s" % (name, type(t).__name__))
        if tuple(t.shape) != shape:
            raise ValueError("volume_peaks_cuboid: %s must be %s, got %s" % (name, shape, tuple(t.shape)))
    position, sides = _three("position", position), _three("sides", sides)
    _check_device(volumes, (("rotations", rotations), ("centers", centers)))
    rot, center = rotations.to(torch.float32).contiguous(), centers.to(torch.float32).contiguous()
    return torch.ops.mvhmr.volume_peaks_cuboid(volumes.contiguous(), rot, center, position, sides, k, radius, threshold)


def peak_proposals(scores, index, positions):
    """The outputs of volume_peaks_cuboid as the inputs of one fine volume per proposal: (centers (M, 3), feature_index (M,) int32, valid (M,)
    bool) with M = B*J*K in (b, j, slot) order.  feature_index is b for a present slot and -1 for a missing one, which
    unprojection_cuboid(..., feature_index=...) turns into a zero volume without gradient.  Tensor ops only: no host synchronisation, and
    differentiable through centers."""
    if not (torch.is_tensor(scores) and torch.is_tensor(index) and torch.is_tensor(positions)):
        raise TypeError("peak_proposals: scores, index and positions must be tensors")
    if index.dim() != 3 or tuple(scores.shape) != tuple(index.shape) or tuple(positions.shape) != tuple(index.shape) + (3,):
        raise ValueError("peak_proposals: scores and index must be (B, J, K) and positions (B, J, K, 3), got %s, %s, %s"
                         % (tuple(scores.shape), tuple(index.shape), tuple(positions.shape)))
    B = index.shape[0]
    valid = index >= 0
    sample = torch.arange(B, dtype=torch.int32, device=index.device).view(B, 1, 1).expand_as(index)
    feature_index = torch.where(valid, sample, torch.full_like(sample, -1))
    return positions.reshape(-1, 3), feature_index.reshape(-1), valid.reshape(-1)
