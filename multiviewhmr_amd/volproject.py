"""Ray-marching volumes into camera-view maps: rendering a volume into the cameras, the direction opposite to un-projection.

    camera_rays(proj_matricies) -> rays (B, V, 3, 4)
    project_volume_cuboid(volumes, rays, rotations, centers, position, sides, map_shape, n_samples, method='mean', *, beta=1.0,
                          min_depth=0.0, max_depth=inf, return_ranges=False)

volumes (B, C, X, Y, Z) live on the cuboid recipe of unprojection_cuboid / sample_volume_cuboid.  Every pixel (u, v) = (column, row) of
every view casts the ray o + lambda D (u, v, 1)^T (rays[b, v] = [D | o], camera_rays), which is clipped against the cuboid (and against
[min_depth, max_depth]: lambda is the depth of a K[R|t] camera), sampled at n_samples midpoints of equal steps by sample_volume_cuboid's
tap rule, and reduced per channel: 'mean', 'max' or 'softmax' (sum_k p_k s_k, p = softmax_k(beta s_k)).  No sample tensor is ever stored,
forward or backward; the volume gradient is accumulated in 64-bit fixed point with integer atomics and is bitwise reproducible.
Differentiable w.r.t. volumes only.  No fallback: CPU tensors, mixed devices and a missing library raise.
"""
import math

import torch

from . import aggregation as _agg
from .softargmax import _VOLUME_DTYPES, _check_device, _three

METHODS = ("mean", "max", "softmax")                       # mvhmr_project_t, in its order
MAX_SAMPLES = 1024                                         # mvhmr_project_volume_max_samples()


def _ops():
    _agg._native()                                       # loads the extension (and the library behind it), or says how to build them
    return torch.ops.mvhmr_volproject


def camera_rays(proj_matricies):
    """rays (B, V, 3, 4) float32 = [D | o] from projections (B, V, 3, 4) = [M | p4]: D = M^-1, o = -M^-1 p4 (the camera centre), computed in
    float64 with torch ops.  The world point of pixel (u, v) at parameter lambda is o + lambda D (u, v, 1)^T; it projects back to (u, v) with
    homogeneous w = lambda, the depth for K[R|t].  Pass the projection of the resolution the map is wanted at."""
    if not torch.is_tensor(proj_matricies) or proj_matricies.dim() != 4 or tuple(proj_matricies.shape[2:]) != (3, 4):
        raise ValueError("camera_rays: proj_matricies must be a (B, V, 3, 4) tensor, got %s" % (
            tuple(proj_matricies.shape) if torch.is_tensor(proj_matricies) else type(proj_matricies).__name__,))
    P = proj_matricies.detach().to(torch.float64)
    D = torch.linalg.inv(P[..., :3])
    o = -(D @ P[..., 3:])
    return torch.cat([D, o], -1).to(torch.float32)


# ---- the ops: mvhmr::project_volume_cuboid -> (maps, ranges, aux); aux (arg-k or log-sum-exp) is saved for the backward
_PLACE = ("Tensor volumes, Tensor rays, Tensor rot, Tensor center, float[] position, float[] sides, int map_h, int map_w, int n_samples, int method, "
          "float beta, float min_depth, float max_depth")


def _fwd(*a):
    return tuple(_ops().project_volume(*a))


def _fake_fwd(volumes, rays, rot, center, position, sides, map_h, map_w, n_samples, method, beta, min_depth, max_depth):
    B, C, V = volumes.shape[0], volumes.shape[1], rays.shape[1]
    f32 = dict(dtype=torch.float32, device=volumes.device)
    aux = (torch.empty((0,), **f32) if method == 0 else
           torch.empty((B, V, C, map_h, map_w), dtype=torch.int32 if method == 1 else torch.float32, device=volumes.device))
    return torch.empty((B, V, C, map_h, map_w), **f32), torch.empty((B, V, map_h, map_w, 2), **f32), aux


def _setup(ctx, inputs, output):
    ctx.args = inputs[4:]
    ctx.save_for_backward(inputs[0], inputs[1], inputs[2], inputs[3], output[0], output[2])
    ctx.set_materialize_grads(False)


def _autograd(ctx, grad_maps, grad_ranges, grad_aux):
    """the volume gradient alone; a gradient that arrives for ranges (or aux) carries nothing and is dropped"""
    volumes, rays, rot, center, maps, aux = ctx.saved_tensors
    gv = None
    if grad_maps is not None and ctx.needs_input_grad[0]:
        gv = torch.ops.mvhmr.project_volume_backward_volumes(volumes, rays, rot, center, *ctx.args, grad_maps.to(torch.float32).contiguous(), maps, aux)
    return (gv,) + (None,) * 12


def _register():
    if _agg._op_defined("project_volume_cuboid"):
        return
    lib = torch.library
    lib.define("mvhmr::project_volume_cuboid", "(%s) -> (Tensor, Tensor, Tensor)" % _PLACE)
    lib.impl("mvhmr::project_volume_cuboid", "CUDA")(_fwd)
    lib.register_fake("mvhmr::project_volume_cuboid")(_fake_fwd)
    lib.define("mvhmr::project_volume_backward_volumes", "(%s, Tensor grad_maps, Tensor maps, Tensor aux) -> Tensor" % _PLACE)
    lib.impl("mvhmr::project_volume_backward_volumes", "CUDA")(lambda *a: _ops().project_volume_backward_volumes(*a))
    lib.register_fake("mvhmr::project_volume_backward_volumes")(lambda volumes, *a: torch.empty_like(volumes))
    lib.register_autograd("mvhmr::project_volume_cuboid", _autograd, setup_context=_setup)


_register()


def _check_volumes(volumes):
    if not torch.is_tensor(volumes):
        raise TypeError("project_volume_cuboid: volumes must be a tensor, got %s" % type(volumes).__name__)
    if volumes.dim() != 5:
        raise ValueError("project_volume_cuboid: volumes must be (B, C, X, Y, Z), got shape %s" % (tuple(volumes.shape),))
    if volumes.dtype not in _VOLUME_DTYPES:
        raise TypeError("project_volume_cuboid: volumes must be float32, float16 or bfloat16, got %s" % volumes.dtype)
    B, C, X, Y, Z = volumes.shape
    if B < 1 or C < 1:
        raise ValueError("project_volume_cuboid: volumes must not be empty, got shape %s" % (tuple(volumes.shape),))
    if min(X, Y, Z) < 2:
        raise ValueError("project_volume_cuboid: every extent must be >= 2 (a one-voxel axis has no step), got shape %s" % (tuple(volumes.shape),))
    if X * Y * Z >= 2 ** 31:
        raise ValueError("project_volume_cuboid: X*Y*Z must stay below 2^31, got shape %s" % (tuple(volumes.shape),))


def _number(name, x, finite):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or math.isnan(x) or (finite and math.isinf(x)):
        raise ValueError("project_volume_cuboid: %s must be a %sPython number, got %r" % (name, "finite " if finite else "", x))
    return float(x)


def project_volume_cuboid(volumes, rays, rotations, centers, position, sides, map_shape, n_samples, method="mean", *, beta=1.0, min_depth=0.0,
                          max_depth=math.inf, return_ranges=False):
    """volumes (B, C, X, Y, Z) (float32 / float16 / bfloat16, every extent >= 2) rendered into float32 maps (B, V, C, Hm, Wm) along the rays
    (B, V, 3, 4) of camera_rays; map_shape = (Hm, Wm), pixel (u, v) = (column, row) at integer coordinates, the convention of
    project_3d_points_to_image_plane_without_distortion.  Per ray: clipped against the cuboid and [min_depth, max_depth] to (l_in, l_out),
    sampled at l_in + (k + 0.5)(l_out - l_in) / n_samples, k = 0 .. n_samples - 1 (1 <= n_samples <= 1024), by sample_volume_cuboid's tap
    rule (zero padding; a tap of weight 0 is not read), reduced by method: 'mean', 'max' (the gradient goes to the lowest k that attains
    it) or 'softmax' (sum_k p_k s_k, p = softmax_k(beta s_k), beta finite and nonzero).  A ray that misses the cuboid gives exactly 0 in every
    channel and takes part in no gradient.

    With return_ranges also ranges (B, V, Hm, Wm, 2) float32: (l_in, l_out) per ray, (0, 0) for a miss -- the loss mask and the entry / exit
    depth; nothing is differentiated through it.  There is no 'sum': a line integral is mean * (l_out - l_in) * |D (u, v, 1)|, which a
    caller forms from ranges.

    rotations (B, 3, 3) orthonormal, centers (B, 3): float32 on volumes' device; position, sides: the cuboid recipe of unprojection_cuboid.
    Differentiable w.r.t. volumes only (the gradient comes back in volumes' dtype, bitwise reproducible); rays, rotations or centers that
    require grad raise ValueError.  Empty maps return without a launch."""
    _check_volumes(volumes)
    B, C = volumes.shape[:2]
    for name, t, shape in (("rays", rays, (B, None, 3, 4)), ("rotations", rotations, (B, 3, 3)), ("centers", centers, (B, 3))):
        if not torch.is_tensor(t):
            raise TypeError("project_volume_cuboid: %s must be a tensor, got %s" % (name, type(t).__name__))
        if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
            raise ValueError("project_volume_cuboid: %s must be %s, got %s" % (name, tuple("V" if s is None else s for s in shape), tuple(t.shape)))
        if t.requires_grad:
            raise ValueError("project_volume_cuboid: %s requires grad, but the op is differentiable w.r.t. volumes only (detach it)" % name)
    if method not in METHODS:
        raise ValueError("project_volume_cuboid: method must be one of %s, got %r" % (METHODS, method))
    try:
        Hm, Wm = (int(x) for x in map_shape)
    except (TypeError, ValueError):
        raise ValueError("project_volume_cuboid: map_shape must be (Hm, Wm), got %r" % (map_shape,)) from None
    if Hm < 0 or Wm < 0:
        raise ValueError("project_volume_cuboid: map_shape must not be negative, got %r" % (map_shape,))
    if isinstance(n_samples, bool) or not isinstance(n_samples, int) or not 1 <= n_samples <= MAX_SAMPLES:
        raise ValueError("project_volume_cuboid: n_samples must be an int in 1 .. %d, got %r" % (MAX_SAMPLES, n_samples))
    V = rays.shape[1]
    if V * Hm * Wm * n_samples >= 2 ** 31 or B * C * V >= 2 ** 31:
        raise ValueError("project_volume_cuboid: V*Hm*Wm*n_samples and B*C*V must stay below 2^31, got V = %d, map %dx%d, n_samples = %d" % (V, Hm, Wm, n_samples))
    beta = _number("beta", beta, True)
    beta32 = float(torch.tensor(beta, dtype=torch.float32))              # the kernels take it as fp32
    if method == "softmax" and (beta32 == 0.0 or not math.isfinite(beta32)):
        raise ValueError("project_volume_cuboid: beta must be finite and nonzero as a float32, got %r" % (beta,))
    min_depth, max_depth = _number("min_depth", min_depth, True), _number("max_depth", max_depth, False)
    position, sides = _three("position", position), _three("sides", sides)
    _check_device(volumes, (("rays", rays), ("rotations", rotations), ("centers", centers)))
    if V == 0 or Hm == 0 or Wm == 0:
        maps = torch.zeros((B, V, C, Hm, Wm), dtype=torch.float32, device=volumes.device)
        return (maps, torch.zeros((B, V, Hm, Wm, 2), dtype=torch.float32, device=volumes.device)) if return_ranges else maps
    r, rot, center = (t.to(torch.float32).contiguous() for t in (rays, rotations, centers))
    maps, ranges, _ = torch.ops.mvhmr.project_volume_cuboid(volumes.contiguous(), r, rot, center, position, sides, Hm, Wm, n_samples, METHODS.index(method),
                                                            beta, min_depth, max_depth)
    return (maps, ranges) if return_ranges else maps
