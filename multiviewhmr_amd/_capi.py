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
    "mvhmr_unproject_query_variant", "mvhmr_internal_lds_cache_key",
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
          for tag in ("masked", "weighted", "visible", "confidence", "shared", "lens", "moments")) + ("mvhmr_unproject_visibility", "mvhmr_unproject_visibility_cuboid")


class Desc(ctypes.Structure):
    """struct mvhmr_unproject_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "abi_version", "batch", "views", "channels", "feat_h", "feat_w", "vol_x", "vol_y", "vol_z",
        "method", "feat_dtype", "out_dtype", "feat_layout", "variant")]


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
    # the *_weighted family: the *_masked signatures with view_weights behind view_mask, the geometry calls also with grad_weights
    for vol, place in (("", [vp]), ("_cuboid", [vp, vp, d3, d3])):
        for name, lead, outs in (("forward" + vol, [dp, vp, vp], 1), ("backward" + vol, [dp, vp, vp, vp], 1),
                                 ("backward%s_deterministic" % vol if vol else "backward_deterministic", [dp, vp, vp, vp], 1),
                                 ("backward_geometry" + vol, [dp, vp, vp, vp], 4 if vol else 3)):
            fn = getattr(L, "mvhmr_unproject_%s_weighted" % name)
            fn.restype = ctypes.c_int
            fn.argtypes = lead + place + [vp, vp] + [vp] * outs + [vp, sz, vp]
            q = getattr(L, "mvhmr_unproject_%s_weighted_workspace_bytes" % name)
            q.restype = sz
            q.argtypes = [dp]
    # the *_visible family: the *_masked signatures (view_mask nullable); then the visibility bits (desc, proj, placing, view_mask, bits, stream)
    for vol, place in (("", [vp]), ("_cuboid", [vp, vp, d3, d3])):
        for name, lead, outs in (("forward" + vol, [dp, vp, vp], 1), ("backward" + vol, [dp, vp, vp, vp], 1),
                                 ("backward%s_deterministic" % vol if vol else "backward_deterministic", [dp, vp, vp, vp], 1),
                                 ("backward_geometry" + vol, [dp, vp, vp, vp], 3 if vol else 2)):
            fn = getattr(L, "mvhmr_unproject_%s_visible" % name)
            fn.restype = ctypes.c_int
            fn.argtypes = lead + place + [vp] + [vp] * outs + [vp, sz, vp]
            q = getattr(L, "mvhmr_unproject_%s_visible_workspace_bytes" % name)
            q.restype = sz
            q.argtypes = [dp]
        fn = getattr(L, "mvhmr_unproject_visibility" + vol)
        fn.restype = ctypes.c_int
        fn.argtypes = [dp, vp] + place + [vp, vp, vp]
    # the *_confidence family: the *_visible signatures with view_confidence and the flag `visible` behind view_mask, the geometry calls also
    # with grad_confidence
    for vol, place in (("", [vp]), ("_cuboid", [vp, vp, d3, d3])):
        for name, lead, outs in (("forward" + vol, [dp, vp, vp], 1), ("backward" + vol, [dp, vp, vp, vp], 1),
                                 ("backward%s_deterministic" % vol if vol else "backward_deterministic", [dp, vp, vp, vp], 1),
                                 ("backward_geometry" + vol, [dp, vp, vp, vp], 4 if vol else 3)):
            fn = getattr(L, "mvhmr_unproject_%s_confidence" % name)
            fn.restype = ctypes.c_int
            fn.argtypes = lead + place + [vp, vp, ctypes.c_int] + [vp] * outs + [vp, sz, vp]
            q = getattr(L, "mvhmr_unproject_%s_confidence_workspace_bytes" % name)
            q.restype = sz
            q.argtypes = [dp]
    # the *_shared family: the plain signatures with volumes, feature_index and the (refused) view selections view_mask, view_weights,
    # view_confidence, visible behind what places the volume; the queries take volumes too
    for vol, place in (("", [vp]), ("_cuboid", [vp, vp, d3, d3])):
        for name, lead, outs in (("forward" + vol, [dp, vp, vp], 1), ("backward" + vol, [dp, vp, vp, vp], 1),
                                 ("backward%s_deterministic" % vol if vol else "backward_deterministic", [dp, vp, vp, vp], 1),
                                 ("backward_geometry" + vol, [dp, vp, vp, vp], 3 if vol else 2)):
            fn = getattr(L, "mvhmr_unproject_%s_shared" % name)
            fn.restype = ctypes.c_int
            fn.argtypes = lead + place + [i32, vp, vp, vp, vp, ctypes.c_int] + [vp] * outs + [vp, sz, vp]
            q = getattr(L, "mvhmr_unproject_%s_shared_workspace_bytes" % name)
            q.restype = sz
            q.argtypes = [dp, i32]
    # the *_lens family: the plain signatures with lens and the (refused) selections view_mask, view_weights, view_confidence, visible,
    # feature_index behind what places the volume
    for vol, place in (("", [vp]), ("_cuboid", [vp, vp, d3, d3])):
        for name, lead, outs in (("forward" + vol, [dp, vp, vp], 1), ("backward" + vol, [dp, vp, vp, vp], 1),
                                 ("backward%s_deterministic" % vol if vol else "backward_deterministic", [dp, vp, vp, vp], 1),
                                 ("backward_geometry" + vol, [dp, vp, vp, vp], 3 if vol else 2)):
            fn = getattr(L, "mvhmr_unproject_%s_lens" % name)
            fn.restype = ctypes.c_int
            fn.argtypes = lead + place + [vp, vp, vp, vp, ctypes.c_int, vp] + [vp] * outs + [vp, sz, vp]
            q = getattr(L, "mvhmr_unproject_%s_lens_workspace_bytes" % name)
            q.restype = sz
            q.argtypes = [dp]
    # the *_moments family: the *_visible signatures with the flag `visible` and `moments` (MOMENTS_VAR / MOMENTS_MEANVAR) behind view_mask
    for vol, place in (("", [vp]), ("_cuboid", [vp, vp, d3, d3])):
        for name, lead, outs in (("forward" + vol, [dp, vp, vp], 1), ("backward" + vol, [dp, vp, vp, vp], 1),
                                 ("backward%s_deterministic" % vol if vol else "backward_deterministic", [dp, vp, vp, vp], 1),
                                 ("backward_geometry" + vol, [dp, vp, vp, vp], 3 if vol else 2)):
            fn = getattr(L, "mvhmr_unproject_%s_moments" % name)
            fn.restype = ctypes.c_int
            fn.argtypes = lead + place + [vp, i32, i32] + [vp] * outs + [vp, sz, vp]
            q = getattr(L, "mvhmr_unproject_%s_moments_workspace_bytes" % name)
            q.restype = sz
            q.argtypes = [dp]
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
