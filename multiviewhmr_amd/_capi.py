"""ctypes binding of include/mvhmr_unproject.h -- the only way Python reaches the kernels.

No fallback: if the shared library is missing the first call raises with the build command.
"""
import ctypes
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "lib", "libmvhmr_unproject.so")

ABI_VERSION = 4
OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_WORKSPACE, ERR_LAUNCH = range(5)
AGG = {"softmax": 0, "sum": 1, "mean": 2, "max": 3}
F32, F16, BF16 = 0, 1, 2
LAYOUT_BVCHW, LAYOUT_BVHWC, LAYOUT_QUAD, LAYOUT_QUAD_LOG2E = 0, 1, 2, 3
VARIANT = {"auto": 0, "gather": 1, "brick": 2}
MOMENTS_VAR, MOMENTS_MEANVAR = 1, 2                       # mvhmr_moments_t: the cross-view variance alone / behind the mean

EXPORTS = (
    "mvhmr_abi_version", "mvhmr_status_string", "mvhmr_last_error",
    "mvhmr_unproject_forward_workspace_bytes", "mvhmr_unproject_backward_workspace_bytes",
    "mvhmr_unproject_forward", "mvhmr_unproject_backward", "mvhmr_build_coord_volumes",
    "mvhmr_unproject_selected_variant", "mvhmr_preferred_layout", "mvhmr_feature_layout_bytes", "mvhmr_convert_features",
    "mvhmr_unproject_query_variant", "mvhmr_internal_lds_cache_key", "mvhmr_internal_det_exponent_table",
    "mvhmr_unproject_forward_cuboid", "mvhmr_unproject_backward_cuboid",
    "mvhmr_conv1x1_to_quad", "mvhmr_conv1x1_to_quad_supported", "mvhmr_conv1x1_planar", "mvhmr_conv1x1_planar_supported", "mvhmr_conv1x1_wgrad", "mvhmr_conv1x1_wgrad_supported", "mvhmr_unproject_query_variant_cuboid",
    "mvhmr_unproject_backward_supported", "mvhmr_triangulate_dlt", "mvhmr_triangulate_dlt_weighted",
    "mvhmr_unproject_forward_kernel_name",
    "mvhmr_unproject_backward_geometry_workspace_bytes", "mvhmr_unproject_backward_geometry",
    "mvhmr_unproject_backward_geometry_cuboid_workspace_bytes", "mvhmr_unproject_backward_geometry_cuboid", "mvhmr_triangulate_dlt_backward",
    "mvhmr_unproject_backward_deterministic_workspace_bytes", "mvhmr_unproject_backward_deterministic",
    "mvhmr_unproject_backward_cuboid_deterministic", "mvhmr_conv1x1_wgrad_deterministic_workspace_bytes", "mvhmr_conv1x1_wgrad_deterministic",
) + tuple("mvhmr_unproject_%s_%s%s" % (n, tag, w) for n in ("forward", "forward_cuboid", "backward", "backward_cuboid", "backward_deterministic",
                                                           "backward_cuboid_deterministic", "backward_geometry", "backward_geometry_cuboid")
          for w in ("", "_workspace_bytes")       # per-sample view masks, per-view confidence weights, visibility-aware aggregation, per-pixel confidence maps, shared feature maps, lens distortion, cross-view variance
          for tag in ("masked", "weighted", "visible", "confidence", "shared", "lens", "moments")) + ("mvhmr_unproject_visibility", "mvhmr_unproject_visibility_cuboid") + (
    "mvhmr_unproject_call_workspace_bytes", "mvhmr_unproject_forward_call", "mvhmr_unproject_backward_call", "mvhmr_unproject_backward_geometry_call") + (
    # the volumetric soft-argmax (softargmax.py)
    "mvhmr_soft_argmax3d_splits", "mvhmr_soft_argmax3d_workspace_bytes", "mvhmr_soft_argmax3d_forward", "mvhmr_soft_argmax3d_backward",
    "mvhmr_soft_argmax3d_backward_coords", "mvhmr_soft_argmax3d_backward_pose") + (
    # trilinear volume sampling at world points (volsample.py)
    "mvhmr_sample_volume_chunk_points", "mvhmr_sample_volume_workspace_bytes", "mvhmr_sample_volume_forward",
    "mvhmr_sample_volume_backward_volumes", "mvhmr_sample_volume_backward_geometry") + (
    # ray-marching volumes into camera-view maps (volproject.py)
    "mvhmr_project_volume_max_samples", "mvhmr_project_volume_channel_group", "mvhmr_project_volume_workspace_bytes", "mvhmr_project_volume_forward",
    "mvhmr_project_volume_backward_volumes") + (
    # 3-D non-maximum suppression and top-K proposals (peaks.py)
    "mvhmr_volume_peaks_tile", "mvhmr_volume_peaks_max_k", "mvhmr_volume_peaks_workspace_bytes", "mvhmr_volume_peaks",
    "mvhmr_volume_peaks_backward", "mvhmr_volume_peaks_backward_pose")


class Desc(ctypes.Structure):
    """struct mvhmr_unproject_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "abi_version", "batch", "views", "channels", "feat_h", "feat_w", "vol_x", "vol_y", "vol_z",
        "method", "feat_dtype", "out_dtype", "feat_layout", "variant")]


class Call(ctypes.Structure):
    """struct mvhmr_unproject_call: zero it, set struct_size, family, placing and the fields the family takes"""
    _fields_ = ([("struct_size", ctypes.c_uint32)] +
                [(n, ctypes.c_int32) for n in ("family", "placing", "deterministic", "volumes", "visible", "moments", "reserved")] +
                [(n, ctypes.c_void_p) for n in (
                    "coords", "rot", "center", "position", "sides", "view_mask", "view_weights", "view_confidence", "feature_index", "lens",
                    "features", "proj", "grad_out", "out", "grad_features",
                    "grad_proj", "grad_coords", "grad_rot", "grad_center", "grad_weights", "grad_confidence")])


FAMILY = {"plain": 0, "masked": 1, "weighted": 2, "visible": 3, "confidence": 4, "shared": 5, "lens": 6, "moments": 7}     # mvhmr_family_t
PLACING_TENSOR, PLACING_CUBOID = 0, 1                     # mvhmr_placing_t
CALL_FORWARD, CALL_BACKWARD, CALL_GEOMETRY = 0, 1, 2      # mvhmr_call_kind_t

_vp, _i32, _int = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int
# named family -> (its arguments behind the placing, geometry outputs beyond the placing's own, the queries take `volumes`)
FAMILIES = {
    "masked": ([_vp], 0, False),                                      # view_mask
    "weighted": ([_vp, _vp], 1, False),                               # view_mask, view_weights; grad_weights
    "visible": ([_vp], 0, False),                                     # view_mask (nullable)
    "confidence": ([_vp, _vp, _int], 1, False),                       # view_mask, view_confidence, visible; grad_confidence
    "shared": ([_i32, _vp, _vp, _vp, _vp, _int], 0, True),            # volumes, feature_index, then the refused view_mask, view_weights, view_confidence, visible
    "lens": ([_vp, _vp, _vp, _vp, _int, _vp], 0, False),              # lens, then the refused view_mask, view_weights, view_confidence, visible, feature_index
    "moments": ([_vp, _i32, _i32], 0, False),                         # view_mask, visible, moments
}


def record(family, placing=PLACING_TENSOR, **fields):
    """A zeroed Call of one family with the given fields set (pointers as integers or ctypes pointers cast to c_void_p)."""
    c = Call(struct_size=ctypes.sizeof(Call), family=FAMILY[family], placing=placing)
    for name, value in fields.items():
        setattr(c, name, value)
    return c


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libmvhmr_unproject.so is not built (%s). Build it with `python -m multiviewhmr_amd.build` "
            "(hipcc, --offload-arch=gfx950); there is no CPU fallback for the un-projection path." % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32
    dp = ctypes.POINTER(Desc)
    L.mvhmr_abi_version.restype = ctypes.c_int
    L.mvhmr_status_string.restype = ctypes.c_char_p
    L.mvhmr_status_string.argtypes = [ctypes.c_int]
    L.mvhmr_last_error.restype = ctypes.c_char_p
    L.mvhmr_unproject_forward_workspace_bytes.restype = sz
    L.mvhmr_unproject_forward_workspace_bytes.argtypes = [dp]
    L.mvhmr_unproject_backward_workspace_bytes.restype = sz
    L.mvhmr_unproject_backward_workspace_bytes.argtypes = [dp]
    L.mvhmr_unproject_selected_variant.restype = ctypes.c_int
    L.mvhmr_unproject_selected_variant.argtypes = [dp]
    L.mvhmr_unproject_forward_kernel_name.restype = ctypes.c_char_p
    L.mvhmr_unproject_forward_kernel_name.argtypes = [dp]
    L.mvhmr_unproject_backward_supported.restype = ctypes.c_int
    L.mvhmr_unproject_backward_supported.argtypes = [dp]
    L.mvhmr_unproject_query_variant.restype = ctypes.c_int
    L.mvhmr_unproject_query_variant.argtypes = [dp, vp, vp, vp]
    L.mvhmr_unproject_forward.restype = ctypes.c_int
    L.mvhmr_unproject_forward.argtypes = [dp, vp, vp, vp, vp, vp, sz, vp]
    L.mvhmr_unproject_backward.restype = ctypes.c_int
    L.mvhmr_unproject_backward.argtypes = [dp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.mvhmr_unproject_backward_geometry_workspace_bytes.restype = sz
    L.mvhmr_unproject_backward_geometry_workspace_bytes.argtypes = [dp]
    L.mvhmr_unproject_backward_geometry.restype = ctypes.c_int
    L.mvhmr_unproject_backward_geometry.argtypes = [dp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    d3 = ctypes.POINTER(ctypes.c_double)
    L.mvhmr_unproject_forward_cuboid.restype = ctypes.c_int
    L.mvhmr_unproject_forward_cuboid.argtypes = [dp, vp, vp, vp, vp, d3, d3, vp, vp, sz, vp]
    L.mvhmr_unproject_backward_cuboid.restype = ctypes.c_int
    L.mvhmr_unproject_backward_cuboid.argtypes = [dp, vp, vp, vp, vp, vp, d3, d3, vp, vp, sz, vp]
    L.mvhmr_unproject_backward_geometry_cuboid_workspace_bytes.restype = sz
    L.mvhmr_unproject_backward_geometry_cuboid_workspace_bytes.argtypes = [dp]
    L.mvhmr_unproject_backward_geometry_cuboid.restype = ctypes.c_int
    L.mvhmr_unproject_backward_geometry_cuboid.argtypes = [dp, vp, vp, vp, vp, vp, d3, d3, vp, vp, vp, vp, sz, vp]
    L.mvhmr_conv1x1_to_quad.restype = ctypes.c_int
    L.mvhmr_conv1x1_to_quad.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    L.mvhmr_conv1x1_to_quad_supported.restype = ctypes.c_int
    L.mvhmr_conv1x1_to_quad_supported.argtypes = [i32, i32, i32, i32]
    L.mvhmr_conv1x1_planar.restype = ctypes.c_int
    L.mvhmr_conv1x1_planar.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.mvhmr_conv1x1_planar_supported.restype = ctypes.c_int
    L.mvhmr_conv1x1_planar_supported.argtypes = [i32, i32, i32]
    L.mvhmr_conv1x1_wgrad.restype = ctypes.c_int
    L.mvhmr_conv1x1_wgrad.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.mvhmr_conv1x1_wgrad_supported.restype = ctypes.c_int
    L.mvhmr_conv1x1_wgrad_supported.argtypes = [i32, i32, i32]
    L.mvhmr_conv1x1_wgrad_deterministic_workspace_bytes.restype = sz
    L.mvhmr_conv1x1_wgrad_deterministic_workspace_bytes.argtypes = [i32, i32, i32, i32]
    L.mvhmr_conv1x1_wgrad_deterministic.restype = ctypes.c_int
    L.mvhmr_conv1x1_wgrad_deterministic.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]
    L.mvhmr_unproject_backward_deterministic_workspace_bytes.restype = sz
    L.mvhmr_unproject_backward_deterministic_workspace_bytes.argtypes = [dp]
    L.mvhmr_unproject_backward_deterministic.restype = ctypes.c_int
    L.mvhmr_unproject_backward_deterministic.argtypes = [dp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.mvhmr_unproject_backward_cuboid_deterministic.restype = ctypes.c_int
    L.mvhmr_unproject_backward_cuboid_deterministic.argtypes = [dp, vp, vp, vp, vp, vp, d3, d3, vp, vp, sz, vp]
    L.mvhmr_unproject_query_variant_cuboid.restype = ctypes.c_int
    L.mvhmr_unproject_query_variant_cuboid.argtypes = [dp, vp, vp, vp, d3, d3, vp]
    L.mvhmr_preferred_layout.restype = ctypes.c_int
    L.mvhmr_preferred_layout.argtypes = [dp]
    L.mvhmr_feature_layout_bytes.restype = sz
    L.mvhmr_feature_layout_bytes.argtypes = [dp, ctypes.c_int]
    L.mvhmr_convert_features.restype = ctypes.c_int
    L.mvhmr_convert_features.argtypes = [dp, vp, ctypes.c_int, vp, vp]
    L.mvhmr_internal_lds_cache_key.restype = ctypes.c_ulonglong
    L.mvhmr_internal_lds_cache_key.argtypes = [ctypes.c_int, vp]
    L.mvhmr_triangulate_dlt.restype = ctypes.c_int
    L.mvhmr_triangulate_dlt.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    L.mvhmr_triangulate_dlt_weighted.restype = ctypes.c_int
    L.mvhmr_triangulate_dlt_weighted.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.mvhmr_triangulate_dlt_backward.restype = ctypes.c_int
    L.mvhmr_triangulate_dlt_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.mvhmr_build_coord_volumes.restype = ctypes.c_int
    L.mvhmr_build_coord_volumes.argtypes = [vp, vp, vp, i32, i32, ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_double), vp]
    # the named families: every launching signature is lead + placing + the family's own arguments + the outputs + (workspace, bytes, stream)
    for tag, (middle, extra_outs, query_takes_volumes) in FAMILIES.items():
        for vol, place in (("", [vp]), ("_cuboid", [vp, vp, d3, d3])):
            for name, lead, outs in (("forward" + vol, [dp, vp, vp], 1), ("backward" + vol, [dp, vp, vp, vp], 1),
                                     ("backward%s_deterministic" % vol, [dp, vp, vp, vp], 1),
                                     ("backward_geometry" + vol, [dp, vp, vp, vp], (3 if vol else 2) + extra_outs)):
                fn = getattr(L, "mvhmr_unproject_%s_%s" % (name, tag))
                fn.restype = ctypes.c_int
                fn.argtypes = lead + place + middle + [vp] * outs + [vp, sz, vp]
                q = getattr(L, "mvhmr_unproject_%s_%s_workspace_bytes" % (name, tag))
                q.restype = sz
                q.argtypes = [dp, i32] if query_takes_volumes else [dp]
    # the visibility bits: (desc, proj, placing, view_mask, bits, stream)
    for vol, place in (("", [vp]), ("_cuboid", [vp, vp, d3, d3])):
        fn = getattr(L, "mvhmr_unproject_visibility" + vol)
        fn.restype = ctypes.c_int
        fn.argtypes = [dp, vp] + place + [vp, vp, vp]
    # the call record: what every name above fills in; the way in for new callers
    cp = ctypes.POINTER(Call)
    L.mvhmr_unproject_call_workspace_bytes.restype = sz
    L.mvhmr_unproject_call_workspace_bytes.argtypes = [dp, cp, ctypes.c_int]
    for kind in ("forward", "backward", "backward_geometry"):
        fn = getattr(L, "mvhmr_unproject_%s_call" % kind)
        fn.restype = ctypes.c_int
        fn.argtypes = [dp, cp, vp, sz, vp]
    # the volumetric soft-argmax: (volumes, dtype, coords | rot, center, position, sides, B, J, X, Y, Z, beta, ...)
    place, sizes, dbl = [vp, vp, vp, d3, d3], [i32] * 5, ctypes.c_double
    L.mvhmr_soft_argmax3d_splits.restype = i32
    L.mvhmr_soft_argmax3d_splits.argtypes = [i32, i32, ctypes.c_int64]
    L.mvhmr_soft_argmax3d_workspace_bytes.restype = sz
    L.mvhmr_soft_argmax3d_workspace_bytes.argtypes = sizes
    L.mvhmr_soft_argmax3d_forward.restype = ctypes.c_int
    L.mvhmr_soft_argmax3d_forward.argtypes = [vp, i32] + place + sizes + [dbl, vp, vp, vp, vp, sz, vp]
    L.mvhmr_soft_argmax3d_backward.restype = ctypes.c_int
    L.mvhmr_soft_argmax3d_backward.argtypes = [vp, i32] + place + sizes + [dbl, vp, vp, vp, vp, vp, vp]
    L.mvhmr_soft_argmax3d_backward_coords.restype = ctypes.c_int
    L.mvhmr_soft_argmax3d_backward_coords.argtypes = [vp, i32] + sizes + [dbl, vp, vp, vp, vp]
    L.mvhmr_soft_argmax3d_backward_pose.restype = ctypes.c_int
    L.mvhmr_soft_argmax3d_backward_pose.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    # volume sampling: (..., B, C, X, Y, Z, N, paired, ...)
    L.mvhmr_sample_volume_chunk_points.restype = i32
    L.mvhmr_sample_volume_chunk_points.argtypes = []
    L.mvhmr_sample_volume_workspace_bytes.restype = sz
    L.mvhmr_sample_volume_workspace_bytes.argtypes = [i32, i32]
    L.mvhmr_sample_volume_forward.restype = ctypes.c_int
    L.mvhmr_sample_volume_forward.argtypes = [vp, i32, vp, vp, vp, d3, d3] + [i32] * 7 + [vp, vp, vp]
    L.mvhmr_sample_volume_backward_volumes.restype = ctypes.c_int
    L.mvhmr_sample_volume_backward_volumes.argtypes = [i32, vp, vp] + [i32] * 7 + [vp, vp, sz, vp]
    L.mvhmr_sample_volume_backward_geometry.restype = ctypes.c_int
    L.mvhmr_sample_volume_backward_geometry.argtypes = [vp, i32, vp, vp, vp, d3, d3] + [i32] * 7 + [vp, vp, vp, vp, vp, vp, sz, vp]
    # peaks: (volumes, dtype, B, J, X, Y, Z, K, radius, threshold, rot, center, position, sides, scores, index, positions, ws, bytes, stream)
    L.mvhmr_volume_peaks_tile.restype = None
    L.mvhmr_volume_peaks_tile.argtypes = [ctypes.POINTER(i32)]
    L.mvhmr_volume_peaks_max_k.restype = i32
    L.mvhmr_volume_peaks_max_k.argtypes = []
    L.mvhmr_volume_peaks_workspace_bytes.restype = sz
    L.mvhmr_volume_peaks_workspace_bytes.argtypes = [i32] * 6
    L.mvhmr_volume_peaks.restype = ctypes.c_int
    L.mvhmr_volume_peaks.argtypes = [vp, i32] + [i32] * 7 + [ctypes.c_float, vp, vp, d3, d3, vp, vp, vp, vp, sz, vp]
    L.mvhmr_volume_peaks_backward.restype = ctypes.c_int
    L.mvhmr_volume_peaks_backward.argtypes = [i32, vp, vp] + [i32] * 6 + [vp, vp]
    L.mvhmr_volume_peaks_backward_pose.restype = ctypes.c_int
    L.mvhmr_volume_peaks_backward_pose.argtypes = [vp, vp, vp, vp, d3, d3] + [i32] * 6 + [vp, vp, vp]
    # volume projection: (..., B, V, C, X, Y, Z, Hm, Wm, K, method, beta, min_depth, max_depth, ...)
    L.mvhmr_project_volume_max_samples.restype = i32
    L.mvhmr_project_volume_max_samples.argtypes = []
    L.mvhmr_project_volume_channel_group.restype = None
    L.mvhmr_project_volume_channel_group.argtypes = [ctypes.POINTER(i32)]
    L.mvhmr_project_volume_workspace_bytes.restype = sz
    L.mvhmr_project_volume_workspace_bytes.argtypes = [i32] * 5
    L.mvhmr_project_volume_forward.restype = ctypes.c_int
    L.mvhmr_project_volume_forward.argtypes = [vp, i32, vp, vp, vp, d3, d3] + [i32] * 10 + [dbl] * 3 + [vp, vp, vp, vp]
    L.mvhmr_project_volume_backward_volumes.restype = ctypes.c_int
    L.mvhmr_project_volume_backward_volumes.argtypes = [vp, i32, vp, vp, vp, d3, d3] + [i32] * 10 + [dbl] * 3 + [vp, vp, vp, vp, vp, sz, vp]
    L.mvhmr_internal_det_exponent_table.restype = ctypes.c_int
    L.mvhmr_internal_det_exponent_table.argtypes = [dp, cp, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    if L.mvhmr_abi_version() != ABI_VERSION:
        raise RuntimeError("libmvhmr_unproject.so speaks ABI %d, this binding %d: rebuild" %
                           (L.mvhmr_abi_version(), ABI_VERSION))
    _lib = L
    return L


def check(status):
    """Map an mvhmr_status_t to the exception the reference would have raised for the same mistake."""
    if status == OK:
        return
    msg = lib().mvhmr_last_error().decode() or lib().mvhmr_status_string(status).decode()
    if status == ERR_INVALID_ARGUMENT and msg.startswith("Unknown aggregation_method"):
        raise ValueError(msg)                       # models/aggregation.py:85
    raise RuntimeError("mvhmr_unproject: %s" % msg)  # torch shape/device errors are RuntimeError too
