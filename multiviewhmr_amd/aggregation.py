"""Drop-in for the reference's models/aggregation.py on MI355X.

    unprojection(features, proj_matricies, coord_volumes, aggregation_method='softmax')   aggregation.py:20-87
    VolumeGenerator(...).forward(features, proj_matricies, batch, use_gt=True)            aggregation.py:90-195
    build_volume_generator(cfg)                                                           aggregation.py:198-208

Same names, argument meaning, return shapes/dtypes, state-dict keys and quirks (SURVEY.md section 8a,
Q1-Q6).  What differs is HOW: the b x v Python loop with ~20 ATen launches per iteration and the
(V,C,X,Y,Z) intermediates is one fused HIP kernel launch behind the C ABI of include/mvhmr_unproject.h
(forward), one more for the gradient w.r.t. `features` and one for the gradients w.r.t. `proj_matricies` / `coord_volumes` when those
require grad (backward), exposed as torch.library custom ops (mvhmr::unprojection / mvhmr::unprojection_cuboid + their _backward ops,
mvhmr::unprojection_backward_geometry / mvhmr::unprojection_cuboid_backward_geometry -- the latter also w.r.t. the cuboid's rotations and
centers -- and mvhmr::triangulate_dlt[_backward] for the pivot VolumeGenerator triangulates, with fake / meta shape functions and a
registered autograd formula) whose host side runs in the PyTorch-ROCm C++ extension csrc_ext/mvhmr_torch_ext.cpp -- the one
route of every un-projection launch, VolumeGenerator's fused conv + un-projection included.  There is no CPU / eager fallback: the
call raises if the tensors are not on a HIP device or the library or the extension is not built.
"""
import collections
import ctypes
import functools
import os

import numpy as np
import torch
import torch.nn as nn

from . import _capi, multiview, volumetric

_METHODS = ("softmax", "sum", "mean", "max")            # aggregation.py:71-85
_MOMENTS = {"var": 1, "meanvar": 2}                       # extension: the cross-view variance, alone or behind the mean (mvhmr_moments_t)
_FUSED_MAX_MAPS = 65535                                 # mvhmr_conv1x1_to_quad / _planar: n_maps is the grid's z extent (mvhmr_unproject.h)
_TYPE_MSG = "Works only with numpy arrays and PyTorch tensors."


# --------------------------------------------------------------------------------------- C-ABI plumbing
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _is_channels_last5(features):
    """True when the (B,V,C,H,W) tensor is physically (B,V,H,W,C) -- e.g. a channels_last conv output."""
    return features.dim() == 5 and features.shape[2] > 1 and features.permute(0, 1, 3, 4, 2).is_contiguous()


def _feature_layout(features, vol, method, out_dtype, variant):
    """-> (what the library reads, its layout code, a tensor whose shape / dtype describe the features).
    A channels-last-strided tensor (physically (B,V,Hf,Wf,C)) feeds the gather kernels without a layout pass; where the library's AUTO
    choice for the same problem in planar layout is the brick kernels (3-4x the forward, 8x the backward at the north-star size) it is
    converted for them first: fp32 by the library's own channels-last -> quad-planar pass (the copy the brick kernels stage from; the
    backward then returns a planar gradient), fp16 through a planar copy."""
    if not _is_channels_last5(features):
        features = features.contiguous()
        return features, _capi.LAYOUT_BVCHW, features
    if variant == _capi.VARIANT["auto"]:
        L = _capi.lib()
        desc = _make_desc(features, vol, method, out_dtype, _capi.LAYOUT_BVCHW, variant)
        if L.mvhmr_unproject_selected_variant(ctypes.byref(desc)) == _capi.VARIANT["brick"]:
            if features.dtype != torch.float32:
                features = features.contiguous()
                return features, _capi.LAYOUT_BVCHW, features
            src = _make_desc(features, vol, method, out_dtype, _capi.LAYOUT_BVHWC, variant)
            with torch.cuda.device(features.device):
                quad = torch.empty(L.mvhmr_feature_layout_bytes(ctypes.byref(src), _capi.LAYOUT_QUAD), dtype=torch.uint8, device=features.device)
                _capi.check(L.mvhmr_convert_features(ctypes.byref(src), _ptr(features), _capi.LAYOUT_QUAD, _ptr(quad), _stream(features.device)))
            return quad, _capi.LAYOUT_QUAD, features
    return features, _capi.LAYOUT_BVHWC, features


def _dtype_code(dt):
    if dt == torch.float32:
        return _capi.F32
    if dt == torch.float16:
        return _capi.F16
    if dt == torch.bfloat16:
        return _capi.BF16                                # volume only (out_dtype with float32 features); the library checks the pairing
    raise RuntimeError("unprojection: features / volume must be float32 or float16 (volume: also bfloat16), got %s" % dt)


def _make_desc(features, coord_volumes, method, out_dtype, layout, variant):
    """coord_volumes: the (B,X,Y,Z,3) tensor, or just its (X, Y, Z)"""
    B, V, C, Hf, Wf = features.shape
    d = _capi.Desc()
    d.abi_version = _capi.ABI_VERSION
    d.batch, d.views, d.channels, d.feat_h, d.feat_w = B, V, C, Hf, Wf
    vol = tuple(coord_volumes.shape[1:4]) if torch.is_tensor(coord_volumes) else tuple(coord_volumes)
    d.vol_x, d.vol_y, d.vol_z = (int(s) for s in vol)
    d.method = method
    d.feat_dtype = _dtype_code(features.dtype)
    d.out_dtype = _dtype_code(out_dtype)
    d.feat_layout = layout
    d.variant = variant
    return d


# The ops are registered with torch.library (mvhmr::unprojection / mvhmr::unprojection_backward ...): eager calls dispatch to the C++
# extension, FakeTensor / meta calls to the shape functions, autograd to the registered formula -- so torch.compile and AOT autograd see one
# opaque node with a known output shape and a known backward instead of a Python autograd.Function they cannot trace into.
_DTYPES = {_capi.F32: torch.float32, _capi.F16: torch.float16, _capi.BF16: torch.bfloat16}
_ext = None


def _native():
    """torch.ops.mvhmr_native: the C++ extension that does the host work of every launch (csrc_ext/mvhmr_torch_ext.cpp, built by
    multiviewhmr_amd.build.build_ext).  Loaded on first use like _capi.lib(), so importing the package does not need it."""
    global _ext
    if _ext is None:
        from . import build as _build                    # not at import: `python -m multiviewhmr_amd.build` runs that module as __main__
        if not os.path.exists(_build.EXT):
            raise RuntimeError("mvhmr_torch_ext.so is not built (%s). Build it with `python -m multiviewhmr_amd.build`." % _build.EXT)
        _capi.lib()                                      # the extension links libmvhmr_unproject.so: same error when that is missing
        torch.ops.load_library(_build.EXT)
        if torch.ops.mvhmr_native.abi_version() != _capi.ABI_VERSION:
            raise RuntimeError("mvhmr_torch_ext.so speaks ABI %d, this package %d: rebuild (python -m multiviewhmr_amd.build)"
                               % (torch.ops.mvhmr_native.abi_version(), _capi.ABI_VERSION))
        _ext = torch.ops.mvhmr_native
    return _ext


def _native_args(features, vol, method, out_dtype, variant, layout=None):
    """_feature_layout's decision (or `layout`) as the extension's ops take it: the view the library reads, the descriptor's fields"""
    like = features
    if layout is None:
        features, layout, like = _feature_layout(features, vol, method, _DTYPES[out_dtype], variant)
    B, V, C, Hf, Wf = like.shape
    read = features.permute(0, 1, 3, 4, 2) if layout == _capi.LAYOUT_BVHWC else features
    return read, (B, V, C, Hf, Wf, method, _dtype_code(like.dtype), out_dtype, layout, variant)


def _geometry_read_layout(features):
    """the features as the geometry backward and every masked call read them: channels-last as they are (C % 4 == 0), else a planar
    contiguous copy"""
    if _is_channels_last5(features) and features.shape[2] % 4 == 0:
        return features, _capi.LAYOUT_BVHWC
    return features.contiguous(), _capi.LAYOUT_BVCHW


def _op_defined(name):
    """True when mvhmr::<name> already exists (the module imported twice under two names, importlib.reload): define() would raise"""
    try:
        getattr(torch.ops.mvhmr, name)
        return True
    except (AttributeError, RuntimeError):
        return False


# The un-projection ops are 2 placings x 9 kinds = 18 families.  Each family is mvhmr::<family> with <family>_backward,
# <family>_backward_deterministic (the feature gradient, bitwise reproducible: what autograd runs under
# torch.use_deterministic_algorithms(True)) and <family>_backward_geometry (fp32 gradients w.r.t. proj_matricies, the placing tensors and the
# differentiable option tensors; an output not asked for comes back empty; `variant` plays no part).  An op's arguments are features, proj,
# the placing tensors, the kind's option tensors, the placing's arguments, the kind's arguments, then method, out_dtype, variant.  All 18 run
# on the extension's six ops: what a kind adds travels there as defaulted keyword arguments.
class _Option(collections.namedtuple("_Option", "name optional grad", defaults=(False, None))):
    """One option tensor of a kind, behind the geometry tensors.  name: its name in the op's schema, which is also the extension keyword it
    feeds; optional: `Tensor?` in the schema -- None is the null pointer of the C entry points, with which nothing is packed or copied;
    grad: the extension keyword of its gradient buffer when the geometry backward differentiates w.r.t. it, else None"""


class _Kind(collections.namedtuple("_Kind", "options extras constants", defaults=((), (), {}))):
    """options: the _Option tensors in schema order; extras: the kind's non-tensor schema arguments, which feed the extension keywords of
    the same names; constants: the extension keywords the kind implies"""


_MASK, _NULLABLE_MASK = _Option("view_mask"), _Option("view_mask", optional=True)       # (B, V) uint8 on the features' device, nonzero = present
_WEIGHTS = _Option("view_weights", grad="grad_weights")                                   # (B, V) fp32: present = mask byte nonzero and weight > 0
_CONFIDENCE = _Option("view_confidence", grad="grad_confidence")                         # (B, V, Hf, Wf) fp32 maps, sampled like one more channel
_PLACINGS = {                                            # the tensors that place the volume, the arguments that go with them
    "unprojection": (("coords",), ()),
    "unprojection_cuboid": (("rot", "center"), ("float[] position", "float[] sides", "int[] vol")),     # the same kernels, fed the cuboid recipe
}
# Why the kinds are what they are.  A kind with a view_mask reads planar or channels-last features, never a quad-planar copy, and runs the
# gather kernels with a per-sample view count; so does _shared.  Where the mask is not nullable the C entry point wants one:
# the front door hands all ones when the caller gave none.  _shared: the placing tensors hold M entries, volume m reads sample
# feature_index[m]; M volumes come back, the feature gradient has B samples.  _lens reads features as the plain kind does (the feature
# backward takes the plane route wherever the plain gather call does).  _moments: `method` is the moment the variance is taken around, mean;
# moments 1 is the variance (C channels), 2 the mean and the variance (2C); the feature gradient has the features' C channels.
_KINDS = {
    "": _Kind(),
    "_masked": _Kind(options=(_MASK,)),
    "_weighted": _Kind(options=(_MASK, _WEIGHTS)),                                                             # 5.9
    "_visible": _Kind(options=(_MASK,), constants={"visible_only": True}),                                     # 5.10
    "_confidence": _Kind(options=(_NULLABLE_MASK, _CONFIDENCE)),                                               # 5.11
    "_confidence_visible": _Kind(options=(_NULLABLE_MASK, _CONFIDENCE), constants={"visible_only": True}),
    "_shared": _Kind(options=(_Option("feature_index"),)),                                                     # 5.12: (M,) int32
    "_lens": _Kind(options=(_Option("lens"),)),                                                                # 5.13: (B, V, 10) fp32
    "_moments": _Kind(options=(_NULLABLE_MASK,), extras=("bool visible_only", "int moments")),                 # 5.14
}


class _Family:
    """the implementations of one family's ops, each taking the ops' arguments positionally; every attribute is derived from the placing
    and the kind"""

    def __init__(self, name, native, places, place_extras, kind):
        self.name, self.native = name, native                                   # native: the extension's op, the placing's plain family
        self.options, self.constants = kind.options, kind.constants
        self.geo = ("proj",) + places                                           # the geometry tensors, behind features
        self.tensors = ("features",) + self.geo + tuple(o.name for o in kind.options)
        self.grads = self.geo + tuple(o.name for o in kind.options if o.grad)   # what the geometry backward differentiates
        self.extras = place_extras + kind.extras
        self.place_args, self.kind_args = (tuple(e.split()[1] for e in extras) for extras in (place_extras, kind.extras))
        self.names = (self.tensors + self.place_args + self.kind_args + ("method", "out_dtype", "variant")
                      + tuple("want_" + g for g in self.grads))                 # the ops' arguments in schema order (want_*: the geometry backward's)
        self.n_inputs = len(self.tensors) + len(self.extras) + 3
        self.masked, self.weighted, self.confidence, self.shared, self.lens = (
            t in self.tensors for t in ("view_mask", "view_weights", "view_confidence", "feature_index", "lens"))
        self.visible = kind.constants.get("visible_only", False)

    def schema(self):
        nullable = {o.name for o in self.options if o.optional}
        return ", ".join(["Tensor%s %s" % ("?" if t in nullable else "", t) for t in self.tensors] + list(self.extras)
                         + ["int method", "int out_dtype", "int variant"])

    def bind(self, args):
        """the ops' positional arguments by name"""
        return dict(zip(self.names, args))

    def volume(self, a):
        return tuple(a["vol"]) if self.place_args else tuple(a[self.geo[1]].shape[1:4])

    def call(self, op, a, lead=(), want=(), geometry=False, **keywords):
        """the extension's op for bound arguments `a`: the view the library reads, proj, the placing tensors and arguments, the descriptor's
        fields, the want_* flags; everything the kind adds by keyword.  A kind with a view_mask, _shared and the geometry backward read
        channels-last features as they are or a planar copy, the others what _feature_layout decides"""
        features, layout = a["features"], None
        if self.masked or self.shared or geometry:
            features, layout = _geometry_read_layout(features)
        read, desc = _native_args(features, self.volume(a), a["method"], a["out_dtype"], a["variant"], layout)
        keywords.update(self.constants)
        keywords.update((o.name, a[o.name]) for o in self.options)
        keywords.update((n, a[n]) for n in self.kind_args)
        return getattr(_native(), self.native + op)(*lead, read, *(a[n] for n in self.geo + self.place_args), *desc, *want, **keywords)

    def forward(self, *args):
        return self.call("", self.bind(args))

    def backward(self, deterministic, grad_out, *args):
        """gradient w.r.t. features (the geometry's is backward_geometry)"""
        return self.call("_backward", self.bind(args), (grad_out.contiguous(),), deterministic=deterministic)

    def backward_geometry(self, grad_out, *args):
        """planar features go through the library's channels-last pass, channels-last ones are read as they are.  The extension returns the
        gradients of the geometry tensors; the gradient w.r.t. a differentiable option tensor is written by it into the buffer handed to it,
        and may be the only one asked for"""
        a = self.bind(args)
        want = [a.get("want_" + g, True) for g in self.grads]
        n, buffers, asked = len(self.geo), [], {}
        for o, w in zip((o for o in self.options if o.grad), want[n:]):
            buffers.append(a[o.name].new_empty(a[o.name].shape if w else (0,)))
            if w:
                asked[o.grad] = buffers[-1]
        return tuple(self.call("_backward_geometry", a, (grad_out.contiguous(),), want[:n], geometry=True, **asked)) + tuple(buffers)

    def fake_forward(self, *args):
        a = self.bind(args)
        features = a["features"]
        volumes = a["feature_index"].shape[0] if self.shared else features.shape[0]
        halves = 2 if a.get("moments") == _MOMENTS["meanvar"] else 1
        return features.new_empty((volumes, halves * features.shape[2]) + self.volume(a), dtype=_DTYPES[a["out_dtype"]])

    def fake_backward(self, grad_out, features, *args):
        return torch.empty_like(features)

    def fake_backward_geometry(self, grad_out, *args):
        a = self.bind(args)
        return tuple(a[g].new_empty(a[g].shape if a.get("want_" + g, True) else (0,), dtype=torch.float32) for g in self.grads)

    def setup_context(self, ctx, inputs, output):
        ctx.save_for_backward(*inputs[:len(self.tensors)])
        ctx.args = tuple(inputs[len(self.tensors):])

    def autograd(self, ctx, grad_out):
        ops, saved = torch.ops.mvhmr, ctx.saved_tensors
        op = getattr(ops, self.name + ("_backward_deterministic" if torch.are_deterministic_algorithms_enabled() else "_backward"))
        g = op(grad_out, *saved, *ctx.args) if ctx.needs_input_grad[0] else None
        at = [self.tensors.index(g) for g in self.grads]   # the differentiable inputs behind features
        want = tuple(ctx.needs_input_grad[i] for i in at)
        grads = [g] + [None] * (self.n_inputs - 1)
        if any(want):                                      # a features-only backward launches nothing more
            geo = getattr(ops, self.name + "_backward_geometry")(grad_out, *saved, *ctx.args, *want)
            for i, t, w in zip(at, geo, want):
                grads[i] = t if w else None
        return tuple(grads)

    def register(self):
        if _op_defined(self.name):
            return
        sig, name = self.schema(), "mvhmr::" + self.name
        wants = "".join(", bool want_%s=True" % g for g in self.grads)
        for op, schema, impl, fake in (
                (name, "(%s) -> Tensor" % sig, self.forward, self.fake_forward),
                (name + "_backward", "(Tensor grad_out, %s) -> Tensor" % sig, functools.partial(self.backward, False), self.fake_backward),
                (name + "_backward_deterministic", "(Tensor grad_out, %s) -> Tensor" % sig, functools.partial(self.backward, True), self.fake_backward),
                (name + "_backward_geometry", "(Tensor grad_out, %s%s) -> (%s)" % (sig, wants, ", ".join(["Tensor"] * len(self.grads))),
                 self.backward_geometry, self.fake_backward_geometry)):
            torch.library.define(op, schema)
            torch.library.impl(op, "CUDA")(impl)
            torch.library.register_fake(op)(fake)
        torch.library.register_autograd(name, self.autograd, setup_context=self.setup_context)


_OPS = {base + suffix: _Family(base + suffix, base, places, place_extras, kind)
        for base, (places, place_extras) in _PLACINGS.items() for suffix, kind in _KINDS.items()}
for _family in _OPS.values():
    _family.register()
_op_backward = functools.partial(_OPS["unprojection"].backward, False)          # (grad_out, features, proj, coords, method, out_dtype, variant)


def _check_call(features, proj_matricies, volume, volume_shape, aggregation_method, variant, out_dtype, same_device, feature_index=None):
    """The argument checks unprojection() and unprojection_cuboid() share.  volume: the tensors that place the volume; volume_shape(n)
    raises when they do not hold n volumes (B, or the checked feature_index's M), else returns (X, Y, Z); same_device: refuse
    proj_matricies / volume on another device than features.
    -> (out_dtype with its default applied, (X, Y, Z), the zero volume when there is nothing to launch or None)"""
    for t in (features, proj_matricies) + volume:
        if not torch.is_tensor(t):
            raise TypeError(_TYPE_MSG)                       # utils/multiview.py:110
    if aggregation_method not in _METHODS and aggregation_method not in _MOMENTS:
        raise ValueError("Unknown aggregation_method: {}".format(aggregation_method))
    if variant not in _capi.VARIANT:
        raise ValueError("Unknown kernel variant: {}".format(variant))
    if features.dim() != 5:
        raise RuntimeError("unprojection: features must be (B, V, C, Hf, Wf), got %s" % (tuple(features.shape),))
    B, V = features.shape[:2]
    if tuple(proj_matricies.shape) != (B, V, 3, 4):
        raise RuntimeError("unprojection: proj_matricies must be (%d, %d, 3, 4), got %s" % (B, V, tuple(proj_matricies.shape)))
    n = B if feature_index is None else feature_index.shape[0]
    vol = volume_shape(n)
    if not features.is_cuda:
        raise RuntimeError("unprojection: features live on %s; this implementation runs only on a HIP device "
                           "(MI355X) and has no CPU path" % features.device)
    if same_device and any(t.device != features.device for t in (proj_matricies,) + volume):
        raise RuntimeError("unprojection: expected all tensors on %s, got proj_matricies on %s and coord_volumes on %s"
                           % ((features.device, proj_matricies.device) + tuple(t.device for t in volume)))
    if out_dtype is None:
        out_dtype = torch.float16 if features.dtype == torch.float16 else torch.float32
    if features.numel() == 0 or 0 in vol or n == 0:
        # empty batch / empty volume / no volumes: the reference's zero-initialised volume comes back (aggregation.py:25-28), nothing to launch
        channels = features.shape[2] * (2 if aggregation_method == "meanvar" else 1)
        return out_dtype, vol, torch.zeros((n, channels) + vol, dtype=out_dtype, device=features.device)
    return out_dtype, vol, None


def unprojection(features, proj_matricies, coord_volumes, aggregation_method='softmax', *, out_dtype=None,
                 variant='auto', view_mask=None, view_weights=None, visible_only=False, view_confidence=None, feature_index=None, lens=None):
    """Fused project -> bilinear-sample -> cross-view aggregate (reference: models/aggregation.py:20-87).

    features        (B, V, C, Hf, Wf) float32 (or float16, this package's storage mode) on a HIP device;
                    a channels-last-strided tensor (physically (B,V,Hf,Wf,C)) is consumed without a layout pass
    proj_matricies  (B, V, 3, 4)  -- feature-resolution projection matrices
    coord_volumes   (B, X, Y, Z, 3) -- voxel centres in world units
    aggregation_method  'softmax' | 'sum' | 'mean' | 'max'; anything else -> ValueError (aggregation.py:85) -- except the extensions
                    'var' and 'meanvar' (DESIGN.md 5.14): the population variance of the participating views' samples, (B, C, X, Y, Z),
                    and torch.cat([mean, var], 1), (B, 2C, X, Y, Z).  The participating views are all of them (a view behind the camera
                    or outside the map with its sample of zero, as in 'mean'), the present ones under view_mask, the present ones that
                    see the voxel under visible_only=True; one view gives variance 0, none gives zeros.  The mean half carries the bits of
                    the 'mean' call with variant='gather'.  Differentiable like the plain call; runs the gather kernels ('brick' is
                    refused); with view_weights, view_confidence, feature_index or lens it raises ValueError (not built yet).
    returns         a new (B, C, X, Y, Z) tensor on features.device, float32 like the reference (aggregation.py:25)
                    unless out_dtype is given (float16 features default to a float16 volume; float32 features may ask for a
                    bfloat16 volume -- what a half-precision consumer reads -- and then take a bfloat16 grad_out)

    `out_dtype` and `variant` ('auto' | 'gather' | 'brick') are keyword-only extensions.
    view_mask       (B, V) bool / integer tensor, any device, nonzero = the view is present (keyword-only; None = all present):
                    out[b] is the un-projection of sample b's present views alone (mean divides by their count, softmax and max range
                    over them; no views -> zeros), masked views are never read and get zero gradients.  Runs the gather kernels
                    ('brick' is refused); DESIGN.md 5.8.
    view_weights    (B, V) floating tensor, any device (keyword-only; None = unweighted): per-view confidences w.  A view with w <= 0 or
                    NaN is absent exactly as under view_mask (with a mask too: present = mask and w > 0); over the present views sum is
                    sum w_v s_v, mean that over sum w_v, softmax weighs e^{s_v} by w_v; 'max' raises ValueError.  Differentiable (the
                    gradient comes back in the caller's dtype and device); runs the gather kernels; DESIGN.md 5.9.
    visible_only    keyword-only, default False.  True: every VOXEL aggregates only the views that see it -- depth > 0 and the projection
                    inside the feature map, 0 <= ix <= Wf - 1 and 0 <= iy <= Hf - 1 -- instead of letting the others contribute zeros (the
                    reference's quirk Q2): mean divides by the number of seeing views, softmax and max range over them, a voxel no view
                    sees is 0.  Unseen views are not read for that voxel and get zero gradients there; `view_visibility` returns the sets.
                    Differentiable like the plain call, composes with view_mask; with view_weights it raises ValueError (not built yet);
                    runs the gather kernels ('brick' is refused); DESIGN.md 5.10.
    view_confidence (B, V, Hf, Wf) floating tensor, any device (keyword-only; None = none): one confidence map per view, at feature
                    resolution, bilinearly sampled at the voxel with the very taps of the view's features (one more channel).  Every voxel
                    aggregates its views weighted by that sample c: over the views with c > 0 sum is sum c_v s_v, mean that over sum c_v,
                    softmax weighs e^{s_v} by c_v; a view whose c is zero, negative or NaN for a voxel -- one behind the camera or projecting
                    wholly outside the map included -- is absent for that voxel: not read, zero gradients.  Differentiable (the gradient comes
                    back in the caller's dtype and device, and enters the geometry gradients); composes with view_mask and visible_only;
                    'max' and view_weights raise ValueError (multiply the maps by the weights); runs the gather kernels; DESIGN.md 5.11.
    feature_index   (M,) integer tensor, any device (keyword-only; None = volume b reads sample b): M volumes share the B feature samples.
                    coord_volumes is then (M, X, Y, Z, 3) and out[m] the plain un-projection of features[idx[m]] under proj_matricies[idx[m]]
                    onto coord_volumes[m]; the result is (M, C, X, Y, Z).  The index may repeat a sample, skip one and come in any order;
                    nothing is duplicated.  features.grad and proj_matricies.grad sum over the volumes that name a sample (an unnamed sample
                    gets exact zeros), coord_volumes.grad is per volume.  A CPU index is checked (IndexError outside [0, B)); a device index is
                    not inspected -- no synchronisation, graph-capturable -- and an entry outside [0, B) gives a zero volume that contributes
                    to no gradient.  M > 65535 raises ValueError, M = 0 gives an empty result.  With view_mask, view_weights, visible_only or
                    view_confidence it raises ValueError (not built yet).  Runs the gather kernels ('brick' is refused); DESIGN.md 5.12.
    lens            (B, V, 10) floating tensor, any device (keyword-only; None = pin-hole cameras): per (sample, view) the record
                    (fx, fy, cx, cy, k1, k2, p1, p2, k3, r2max) -- the intrinsics that went into proj_matricies[b, v] (feature level, zero
                    skew), the Brown-Conrady coefficients in OpenCV's order and the fold-back guard; `feature_level_lens` builds it from the
                    cameras.  The voxels are projected THROUGH the lens (OpenCV's projectPoints model, each step one rounded fp32 operation),
                    so `features` may come from raw, un-rectified images.  A ray with r2 > r2max gives an exactly zero sample, as one behind
                    the camera does; a view whose five coefficients are zero is bit-equal to the plain variant='gather' call.  Differentiable
                    w.r.t. features, proj_matricies and coord_volumes through the lens; the lens itself is not (requires_grad raises
                    ValueError).  With view_mask, view_weights, visible_only, view_confidence or feature_index it raises ValueError (not built
                    yet).  Runs the gather kernels ('auto' too; 'brick' is refused); DESIGN.md 5.13.
    """
    def volume_shape(n):
        if coord_volumes.dim() != 5 or coord_volumes.shape[0] != n or coord_volumes.shape[4] != 3:
            raise RuntimeError("unprojection: coord_volumes must be (%d, X, Y, Z, 3), got %s" % (n, tuple(coord_volumes.shape)))
        return tuple(coord_volumes.shape[1:4])

    return _unproject("unprojection", features, proj_matricies, (coord_volumes,), volume_shape, True, None, aggregation_method, out_dtype, variant,
                      dict(view_mask=view_mask, view_weights=view_weights, visible_only=visible_only, view_confidence=view_confidence,
                           feature_index=feature_index, lens=lens))


def _check_moments(aggregation_method, view_weights=None, view_confidence=None, feature_index=None, lens=None):
    """'var' / 'meanvar'  take a view mask and visible_only; the other view selections do not compose with them yet"""
    if not isinstance(aggregation_method, str) or aggregation_method not in _MOMENTS:
        return
    for given, what in ((view_weights is not None, "view_weights"), (view_confidence is not None, "view_confidence"),
                        (feature_index is not None, "feature_index"), (lens is not None, "lens")):
        if given:
            raise ValueError("unprojection: aggregation_method='%s' with %s is not built yet (the next step of DESIGN.md 5.14): "
                             "pass a view_mask and / or visible_only=True" % (aggregation_method, what))


def _check_options(shape, aggregation_method, view_mask=None, view_weights=None, visible_only=False, view_confidence=None, feature_index=None,
                   lens=None):
    """The one place the options of a call are checked, for unprojection(), unprojection_cuboid() and VolumeGenerator.forward.  shape: the
    features' (B, V, Hf, Wf), or None when they are not a 5-D tensor -- _check_call refuses those next; until then only the checks that read
    no shape run.  The order decides which refusal a call with several mistakes gets."""
    _check_moments(aggregation_method, view_weights, view_confidence, feature_index, lens)
    if shape is not None:
        views = tuple(shape[:2])
        if lens is not None:
            _check_lens(lens, views, view_mask, view_weights, visible_only, view_confidence, feature_index)
        if feature_index is not None:
            _check_feature_index(feature_index, shape[0], view_mask, view_weights, visible_only, view_confidence)
        if view_mask is not None:
            _check_view_mask(view_mask, views)
        if view_weights is not None:
            _check_view_weights(view_weights, views, aggregation_method)
    _check_visible_only(visible_only, view_weights)
    if shape is not None and view_confidence is not None:
        _check_view_confidence(view_confidence, tuple(shape), aggregation_method, view_weights)


def _check_view_mask(view_mask, views):
    """view_mask (B, V) = views, bool or an integer dtype, any device: raises TypeError / RuntimeError as _check_call does"""
    if not torch.is_tensor(view_mask):
        raise TypeError("unprojection: view_mask must be a (B, V) tensor of bool or integers, got %s" % type(view_mask).__name__)
    if view_mask.dtype.is_floating_point or view_mask.dtype.is_complex:
        raise TypeError("unprojection: view_mask must be bool or an integer dtype, got %s" % view_mask.dtype)
    if tuple(view_mask.shape) != views:
        raise RuntimeError("unprojection: view_mask must be %s, got %s" % (views, tuple(view_mask.shape)))


def _check_lens(lens, views, view_mask=None, view_weights=None, visible_only=False, view_confidence=None, feature_index=None):
    """lens (B, V, 10) of a floating dtype, any device: raises TypeError / RuntimeError as _check_view_weights does, ValueError when it requires
    grad and beside a view selection or a feature_index"""
    if not torch.is_tensor(lens):
        raise TypeError("unprojection: lens must be a (B, V, 10) floating tensor, got %s" % type(lens).__name__)
    if not lens.dtype.is_floating_point:
        raise TypeError("unprojection: lens must be a floating dtype, got %s" % lens.dtype)
    if tuple(lens.shape) != views + (10,):
        raise RuntimeError("unprojection: lens must be (B, V, 10) = %s, got %s" % (views + (10,), tuple(lens.shape)))
    if lens.requires_grad:
        raise ValueError("unprojection: lens is not differentiable in this version (DESIGN.md 5.13): pass lens.detach()")
    for given, what in ((view_mask is not None, "view_mask"), (view_weights is not None, "view_weights"), (bool(visible_only), "visible_only=True"),
                        (view_confidence is not None, "view_confidence"), (feature_index is not None, "feature_index")):
        if given:
            raise ValueError("unprojection: lens with %s is not built yet (the next step of DESIGN.md 5.13)" % what)


def _lens_fp32(lens, features):
    """the checked records as the library reads them: contiguous fp32 on features.device (a device tensor is cast there: no synchronisation)"""
    return lens.to(device=features.device, dtype=torch.float32).contiguous()


def _lens_variant(variant):
    """a lens call runs the gather family: 'auto' is 'gather' ('brick' reaches the library, which refuses it)"""
    return _capi.VARIANT["gather" if variant == "auto" else variant]


_MAX_VOLUMES = 65535                                    # the *_shared entry points: the volume index is the grid's y extent (mvhmr_unproject.h)


def _check_feature_index(feature_index, B, view_mask=None, view_weights=None, visible_only=False, view_confidence=None):
    """feature_index (M,) of an integer dtype, any device: raises TypeError / RuntimeError as _check_view_mask does, IndexError for a CPU entry
    outside [0, B) (a device index is not inspected: no synchronisation), ValueError for M > 65535 and beside a view selection"""
    if not torch.is_tensor(feature_index):
        raise TypeError("unprojection: feature_index must be an (M,) tensor of integers, got %s" % type(feature_index).__name__)
    if feature_index.dtype.is_floating_point or feature_index.dtype.is_complex or feature_index.dtype == torch.bool:
        raise TypeError("unprojection: feature_index must be an integer dtype, got %s" % feature_index.dtype)
    if feature_index.dim() != 1:
        raise RuntimeError("unprojection: feature_index must be (M,), got %s" % (tuple(feature_index.shape),))
    for given, what in ((view_mask is not None, "view_mask"), (view_weights is not None, "view_weights"), (bool(visible_only), "visible_only=True"),
                        (view_confidence is not None, "view_confidence")):
        if given:
            raise ValueError("unprojection: feature_index with %s is not built yet (the next step of DESIGN.md 5.12): un-project those samples "
                             "on their own" % what)
    if feature_index.shape[0] > _MAX_VOLUMES:
        raise ValueError("unprojection: feature_index names %d volumes, at most %d per call: split the call" % (feature_index.shape[0], _MAX_VOLUMES))
    if not feature_index.is_cuda and feature_index.device.type != "meta" and feature_index.numel():
        lo, hi = int(feature_index.min()), int(feature_index.max())
        if lo < 0 or hi >= B:
            raise IndexError("unprojection: feature_index entry %d is outside [0, %d)" % (lo if lo < 0 else hi, B))


def _index_int32(feature_index, features):
    """the checked index as the library reads it: contiguous int32 on features.device (a device tensor is cast there: no synchronisation)"""
    return feature_index.to(device=features.device, dtype=torch.int32).contiguous()


def _check_visible_only(visible_only, view_weights):
    """visibility-aware aggregation does not take per-view weights yet"""
    if visible_only and view_weights is not None:
        raise ValueError("unprojection: visible_only=True with view_weights is not supported yet (the next step of DESIGN.md 5.10): pass a view_mask, "
                         "or drop one of the two")


def _mask_bytes(view_mask, features):
    """the checked mask as the library reads it: contiguous uint8 on features.device, nonzero = present"""
    return (view_mask != 0).to(device=features.device, dtype=torch.uint8).contiguous()


def _check_view_weights(view_weights, views, aggregation_method):
    """view_weights (B, V) = views, of a floating dtype, any device: raises TypeError / RuntimeError as _check_view_mask does, ValueError for 'max'"""
    if not torch.is_tensor(view_weights):
        raise TypeError("unprojection: view_weights must be a (B, V) floating tensor, got %s" % type(view_weights).__name__)
    if not view_weights.dtype.is_floating_point:
        raise TypeError("unprojection: view_weights must be a floating dtype (a bool / integer tensor is a view_mask), got %s" % view_weights.dtype)
    if tuple(view_weights.shape) != views:
        raise RuntimeError("unprojection: view_weights must be %s, got %s" % (views, tuple(view_weights.shape)))
    if aggregation_method == "max":
        raise ValueError("unprojection: aggregation_method 'max' has no weighted form (pass a view_mask, not view_weights)")


def _check_view_confidence(view_confidence, want, aggregation_method, view_weights=None):
    """view_confidence (B, V, Hf, Wf) = want, of a floating dtype, any device: raises TypeError / RuntimeError as _check_view_weights does,
    ValueError for 'max' and together with view_weights"""
    if not torch.is_tensor(view_confidence):
        raise TypeError("unprojection: view_confidence must be a (B, V, Hf, Wf) floating tensor, got %s" % type(view_confidence).__name__)
    if not view_confidence.dtype.is_floating_point:
        raise TypeError("unprojection: view_confidence must be a floating dtype, got %s" % view_confidence.dtype)
    if tuple(view_confidence.shape) != want:
        raise RuntimeError("unprojection: view_confidence must be %s, got %s" % (want, tuple(view_confidence.shape)))
    if aggregation_method == "max":
        raise ValueError("unprojection: aggregation_method 'max' has no weighted form (pass a view_mask, not view_confidence)")
    if view_weights is not None:
        raise ValueError("unprojection: view_weights together with view_confidence is not taken: multiply the maps by the weights "
                         "(view_confidence * view_weights[:, :, None, None]), which is exactly equivalent and differentiable through torch")


def _weights_fp32(view_weights, features):
    """the checked weights as the library reads them: contiguous fp32 on features.device (no detach: the cast carries the gradient back)"""
    return view_weights.to(device=features.device, dtype=torch.float32).contiguous()


_AS_READ = {"view_mask": _mask_bytes, "view_weights": _weights_fp32, "view_confidence": _weights_fp32, "feature_index": _index_int32,
            "lens": _lens_fp32}
# Which family takes a call: the first whose needs are all given ("moments": aggregation_method is 'var' or 'meanvar').  The checks have
# refused every combination no family is built for, so what a later row would add is absent by then.
_PRECEDENCE = (
    ("_moments", {"moments"}),
    ("_lens", {"lens"}),
    ("_shared", {"feature_index"}),
    ("_confidence_visible", {"view_confidence", "visible_only"}),
    ("_confidence", {"view_confidence"}),
    ("_visible", {"visible_only"}),
    ("_weighted", {"view_weights"}),
    ("_masked", {"view_mask"}),
    ("", set()),
)


def _unproject(placing, features, proj_matricies, volume, volume_shape, same_device, cuboid, aggregation_method, out_dtype, variant, options):
    """What unprojection() and unprojection_cuboid() do.  placing: the plain family's name; volume, volume_shape, same_device: as for
    _check_call; cuboid: (position, sides) or None; options: the callers' keyword options by name, absent ones None (visible_only: False)"""
    shape = None
    if torch.is_tensor(features) and features.dim() == 5:
        B, V, _, Hf, Wf = features.shape
        shape = (B, V, Hf, Wf)
    _check_options(shape, aggregation_method, **options)
    out_dtype, vol, empty = _check_call(features, proj_matricies, volume, volume_shape, aggregation_method, variant, out_dtype, same_device,
                                        options["feature_index"])
    if empty is not None:
        return empty
    moments = _MOMENTS.get(aggregation_method, 0)
    given = {name for name, value in options.items() if (value if name == "visible_only" else value is not None)}
    if moments:
        given.add("moments")
    family = _OPS[placing + next(kind for kind, needs in _PRECEDENCE if needs <= given)]
    # no detach: the op differentiates w.r.t. the geometry too (the casts carry the gradients back to the caller's device and dtype)
    geometry = [t.to(device=features.device, dtype=torch.float32).contiguous() for t in (proj_matricies,) + volume]
    # an option tensor as the library reads it.  The one a family can be chosen without is the mask: None where the family takes a null mask,
    # else all views present
    tensors = [_AS_READ[o.name](options[o.name], features) if options[o.name] is not None
               else None if o.optional else torch.ones(shape[:2], dtype=torch.uint8, device=features.device) for o in family.options]
    place = () if cuboid is None else ([float(x) for x in cuboid[0]], [float(x) for x in cuboid[1]], list(vol))
    kind = [{"visible_only": bool(options["visible_only"]), "moments": moments}[name] for name in family.kind_args]
    return getattr(torch.ops.mvhmr, family.name)(features, *geometry, *tensors, *place, *kind, _capi.AGG["mean" if moments else aggregation_method],
                                                 _dtype_code(out_dtype), _lens_variant(variant) if family.lens else _capi.VARIANT[variant])


# DLT triangulation (mvhmr_triangulate_dlt[_weighted] and mvhmr_triangulate_dlt_backward) as mvhmr::triangulate_dlt[_backward]: proj (B,V,3,4),
# points (V,2) shared or (B,V,2), confidences None, (V,) shared or (B,V), all fp32 on one HIP device -> (B,3)
def _dlt_forward(proj, points, confidences):
    return _native().triangulate_dlt(proj, points, confidences)


def _dlt_backward(grad_out, proj, points, confidences):
    """per-sample gradients w.r.t. proj (B,V,3,4), points (B,V,2) and confidences (B,V); NaN where the gradient does not exist"""
    return tuple(_native().triangulate_dlt_backward(grad_out.contiguous(), proj, points, confidences))


def _fake_dlt_backward(grad_out, proj, points, confidences):
    B, V = proj.shape[:2]
    return proj.new_empty((B, V, 3, 4)), proj.new_empty((B, V, 2)), proj.new_empty((B, V))


def _dlt_setup(ctx, inputs, output):
    proj, points, confidences = inputs
    ctx.save_for_backward(proj, points, confidences)


def _dlt_autograd(ctx, grad_out):
    proj, points, confidences = ctx.saved_tensors
    gp, gu, gc = torch.ops.mvhmr.triangulate_dlt_backward(grad_out, proj, points, confidences)
    if points.dim() == 2:                              # per-sample gradients of shared inputs: summed over the batch
        gu = gu.sum(0)
    if confidences is not None and confidences.dim() == 1:
        gc = gc.sum(0)
    return (gp if ctx.needs_input_grad[0] else None, gu if ctx.needs_input_grad[1] else None,
            gc if confidences is not None and ctx.needs_input_grad[2] else None)


def _register_dlt_op():
    if _op_defined("triangulate_dlt"):
        return
    torch.library.define("mvhmr::triangulate_dlt", "(Tensor proj, Tensor points, Tensor? confidences) -> Tensor")
    torch.library.impl("mvhmr::triangulate_dlt", "CUDA")(_dlt_forward)
    torch.library.register_fake("mvhmr::triangulate_dlt")(lambda proj, points, confidences: proj.new_empty((proj.shape[0], 3)))
    torch.library.define("mvhmr::triangulate_dlt_backward", "(Tensor grad_out, Tensor proj, Tensor points, Tensor? confidences) -> (Tensor, Tensor, Tensor)")
    torch.library.impl("mvhmr::triangulate_dlt_backward", "CUDA")(_dlt_backward)
    torch.library.register_fake("mvhmr::triangulate_dlt_backward")(_fake_dlt_backward)
    torch.library.register_autograd("mvhmr::triangulate_dlt", _dlt_autograd, setup_context=_dlt_setup)


_register_dlt_op()


def unprojection_cuboid(features, proj_matricies, rotations, centers, position, sides, volume_shape,
                        aggregation_method='softmax', *, out_dtype=None, variant='auto', view_mask=None, view_weights=None, visible_only=False,
                        view_confidence=None, feature_index=None, lens=None):
    """`unprojection` for the volumes VolumeGenerator builds (aggregation.py:138-187), without the coordinate tensor: voxel centres
    are rot[b] @ (position + sides / (S - 1) * (i,j,k) - center[b]) + center[b], evaluated inside the kernels (bit-equal to
    mvhmr_build_coord_volumes followed by `unprojection`).

    rotations (B,3,3) and centers (B,3): float32 tensors on features.device; position, sides: 3 numbers each (cuboid corner and
    edge lengths); volume_shape: (X, Y, Z).  Differentiable w.r.t. features, proj_matricies, rotations and centers (and view_weights).
    view_mask, view_weights, visible_only, view_confidence, feature_index, lens: as for `unprojection`; with feature_index (M,) rotations are
    (M,3,3) and centers (M,3) -- one pose per volume, position / sides / volume_shape shared -- and their gradients are per volume."""
    def checked_shape(n):
        if tuple(rotations.shape) != (n, 3, 3) or tuple(centers.shape) != (n, 3):
            raise RuntimeError("unprojection: rotations must be (%d, 3, 3) and centers (%d, 3), got %s and %s"
                               % (n, n, tuple(rotations.shape), tuple(centers.shape)))
        return tuple(int(v) for v in volume_shape)

    # same_device=False: the cuboid's few numbers move to the features' device
    return _unproject("unprojection_cuboid", features, proj_matricies, (rotations, centers), checked_shape, False, (position, sides), aggregation_method,
                      out_dtype, variant, dict(view_mask=view_mask, view_weights=view_weights, visible_only=visible_only,
                                               view_confidence=view_confidence, feature_index=feature_index, lens=lens))


def _visibility_args(proj_matricies, feature_shape, view_mask):
    """the checks view_visibility and view_visibility_cuboid share -> (proj fp32 contiguous, Hf, Wf, mask bytes or None)"""
    if not torch.is_tensor(proj_matricies):
        raise TypeError(_TYPE_MSG)
    if proj_matricies.dim() != 4 or tuple(proj_matricies.shape[2:]) != (3, 4):
        raise RuntimeError("view_visibility: proj_matricies must be (B, V, 3, 4), got %s" % (tuple(proj_matricies.shape),))
    if not proj_matricies.is_cuda:
        raise RuntimeError("view_visibility: proj_matricies live on %s; this implementation runs only on a HIP device" % proj_matricies.device)
    Hf, Wf = (int(x) for x in feature_shape)
    if view_mask is not None:
        _check_view_mask(view_mask, tuple(proj_matricies.shape[:2]))
    proj = proj_matricies.detach().to(torch.float32).contiguous()
    return proj, Hf, Wf, None if view_mask is None else _mask_bytes(view_mask, proj)


def view_visibility(proj_matricies, coord_volumes, feature_shape, view_mask=None):
    """Which views see which voxel, by the rule of `unprojection(..., visible_only=True)` and from the same arithmetic.

    proj_matricies (B, V, 3, 4) and coord_volumes (B, X, Y, Z, 3) on a HIP device, feature_shape = (Hf, Wf), view_mask as for `unprojection`.
    Returns a (B, X, Y, Z) int32 tensor: bit v is set iff view v is present and sees the voxel (depth > 0, 0 <= ix <= Wf - 1, 0 <= iy <= Hf - 1).
    Not differentiable.  What a caller masks a loss with, or feeds to the network as a per-voxel view count."""
    proj, Hf, Wf, mask = _visibility_args(proj_matricies, feature_shape, view_mask)
    if not torch.is_tensor(coord_volumes):
        raise TypeError(_TYPE_MSG)
    if coord_volumes.dim() != 5 or coord_volumes.shape[0] != proj.shape[0] or coord_volumes.shape[4] != 3:
        raise RuntimeError("view_visibility: coord_volumes must be (%d, X, Y, Z, 3), got %s" % (proj.shape[0], tuple(coord_volumes.shape)))
    if coord_volumes.device != proj.device:
        raise RuntimeError("view_visibility: expected all tensors on %s, got coord_volumes on %s" % (proj.device, coord_volumes.device))
    if 0 in coord_volumes.shape or proj.shape[1] == 0:
        return torch.zeros(tuple(coord_volumes.shape[:4]), dtype=torch.int32, device=proj.device)
    _native()                                            # loads the extension: its visibility ops are mvhmr_visibility::
    return torch.ops.mvhmr_visibility.view_visibility(proj, coord_volumes.detach().to(torch.float32).contiguous(), Hf, Wf, mask)


def view_visibility_cuboid(proj_matricies, rotations, centers, position, sides, volume_shape, feature_shape, view_mask=None):
    """`view_visibility` for the volumes of `unprojection_cuboid` (same placing arguments): bit-equal to it on the coordinate tensor."""
    proj, Hf, Wf, mask = _visibility_args(proj_matricies, feature_shape, view_mask)
    B = proj.shape[0]
    if not torch.is_tensor(rotations) or not torch.is_tensor(centers):
        raise TypeError(_TYPE_MSG)
    if tuple(rotations.shape) != (B, 3, 3) or tuple(centers.shape) != (B, 3):
        raise RuntimeError("view_visibility: rotations must be (%d, 3, 3) and centers (%d, 3), got %s and %s"
                           % (B, B, tuple(rotations.shape), tuple(centers.shape)))
    vol = [int(v) for v in volume_shape]
    if 0 in vol or 0 in proj.shape:
        return torch.zeros((B,) + tuple(vol), dtype=torch.int32, device=proj.device)
    rot = rotations.detach().to(device=proj.device, dtype=torch.float32).contiguous()
    cen = centers.detach().to(device=proj.device, dtype=torch.float32).contiguous()
    _native()
    return torch.ops.mvhmr_visibility.view_visibility_cuboid(proj, rot, cen, [float(x) for x in position], [float(x) for x in sides], vol, Hf, Wf, mask)


# --------------------------------------------------------------------------------------- caller side
def feature_level_projections(cameras, images_shape, features_shape):
    """(B, V, 3, 4) float32 numpy: projection matrices at feature-map resolution.

    Reference: deep-copies every Camera, calls update_after_resize(images_shape, features_shape) and reads
    .projection (aggregation.py:127-133, utils/multiview.py:33-52) -- including quirk Q3 (features_shape
    = (Hf, Wf) is unpacked as (new_width, new_height)).  Here the same float64 arithmetic runs on copies
    of K only; `cameras` is list[V] of list[B] and is not modified.
    """
    height, width = images_shape
    new_width, new_height = features_shape
    sx, sy = new_width / width, new_height / height
    V, B = len(cameras), len(cameras[0])
    # one pass over the Python objects, then batched float64 math (same operations, same order as Camera does them)
    K = np.array([[cameras[v][b].K for v in range(V)] for b in range(B)], dtype=np.float64)          # (B,V,3,3), a copy
    Rt = np.array([[np.hstack([cameras[v][b].R, cameras[v][b].t]) for v in range(V)] for b in range(B)], dtype=np.float64)
    K[..., 0, 0] = K[..., 0, 0] * sx
    K[..., 1, 1] = K[..., 1, 1] * sy
    K[..., 0, 2] = K[..., 0, 2] * sx
    K[..., 1, 2] = K[..., 1, 2] * sy
    # K.dot([R|t]) per camera: spelled as the same k-ordered sum of products numpy's 3x3 @ 3x4 dot performs
    P = K[..., :, 0:1] * Rt[..., 0:1, :]
    P = P + K[..., :, 1:2] * Rt[..., 1:2, :]
    P = P + K[..., :, 2:3] * Rt[..., 2:3, :]
    return P.astype(np.float32)


def lens_r2max(k1, k2, k3):
    """The fold-back guard of a Brown-Conrady lens: the smallest positive root rho of 1 + 3 k1 rho + 5 k2 rho^2 + 7 k3 rho^3, i.e. of
    d(r rad(r^2)) / dr = 0 with rho = r^2 -- beyond it the radial map is no longer monotonic and far rays fold back into the frame.
    float64 numpy.roots, returned as float32 (rounded towards zero, so the guard never lets a folded ray through); FLT_MAX when there is no
    positive real root."""
    flt_max = float(np.finfo(np.float32).max)
    coeffs = [7.0 * float(k3), 5.0 * float(k2), 3.0 * float(k1), 1.0]
    while len(coeffs) > 1 and coeffs[0] == 0.0:
        coeffs = coeffs[1:]
    if len(coeffs) == 1:
        return np.float32(flt_max)
    roots = np.roots(np.array(coeffs, dtype=np.float64))
    real = [float(r.real) for r in roots if abs(r.imag) <= 1e-12 * max(1.0, abs(r.real)) and r.real > 0]
    if not real or min(real) >= flt_max:
        return np.float32(flt_max)
    rho = np.float32(min(real))
    return rho if float(rho) <= min(real) else np.nextafter(rho, np.float32(0))


def feature_level_lens(cameras, images_shape, features_shape):
    """(B, V, 10) float32 numpy: the lens records `unprojection(lens=)` reads, for the cameras `feature_level_projections` reads.

    Per camera (fx, fy, cx, cy, k1, k2, p1, p2, k3, r2max): the intrinsics are K after the same float64 scaling feature_level_projections
    applies (update_after_resize, quirk Q3 included), so they are the ones inside the projection matrix by construction; the coefficients
    are the camera's `dist` (OpenCV order; None = zeros: a pin-hole view, which takes the plain path); r2max = lens_r2max(k1, k2, k3).
    A camera with skew (K[0, 1] != 0) raises ValueError: the lens step takes the skew as zero."""
    height, width = images_shape
    new_width, new_height = features_shape
    sx, sy = new_width / width, new_height / height
    V, B = len(cameras), len(cameras[0])
    out = np.zeros((B, V, 10), dtype=np.float32)
    for b in range(B):
        for v in range(V):
            cam = cameras[v][b]
            K = np.array(cam.K, dtype=np.float64)
            if K[0, 1] != 0.0:
                raise ValueError("feature_level_lens: camera (view %d, sample %d) has skew %r; the lens step takes the skew as zero" % (v, b, K[0, 1]))
            dist = getattr(cam, "dist", None)
            d = np.zeros(5, dtype=np.float64)
            if dist is not None:
                flat = np.asarray(dist, dtype=np.float64).flatten()
                if flat.size not in (4, 5):
                    raise ValueError("feature_level_lens: dist must hold 4 or 5 coefficients (k1, k2, p1, p2[, k3]), got %d" % flat.size)
                d[:flat.size] = flat
            out[b, v, :4] = (K[0, 0] * sx, K[1, 1] * sy, K[0, 2] * sx, K[1, 2] * sy)      # float64 products, one rounding to float32
            out[b, v, 4:9] = d
            out[b, v, 9] = lens_r2max(*out[b, v, [4, 5, 8]])                                # of the coefficients as the kernels read them
    return out


class _FusedAggregate(torch.autograd.Function):
    """process_feature (1x1 conv) + un-projection with the conv output living only in the quad-planar layout the brick forward
    stages (mvhmr_conv1x1_to_quad + mvhmr_unproject_forward_cuboid on MVHMR_LAYOUT_QUAD): the planar (B,V,C,Hf,Wf) conv output
    and the layout pass over it are never written.  The un-projection runs with MVHMR_VARIANT_AUTO: the
    geometry gate decides brick / gather on the device for THIS call's cameras and pose (the gather side converts the copy to
    channels-last first), forward and backward each for their own bricks -- no cached decision, no host synchronisation.
    Backward: the un-projection backward gives the gradient w.r.t. the conv output in the planar layout; weight / bias / input
    gradients are three GEMMs on it.  proj / rot / center gradients, when asked for, come from the cuboid geometry backward on the
    saved quad-planar copy (which the library converts to channels-last for it)."""

    @staticmethod
    def forward(ctx, x, weight, bias, proj, rot, center, position, sides, vol, method, out_dtype=torch.float32):
        L = _capi.lib()
        B, V, Cin, Hf, Wf = x.shape
        Cout = weight.shape[0]
        dev = x.device
        x = x.contiguous()
        w2 = weight.reshape(Cout, Cin).contiguous()
        with torch.cuda.device(dev):
            quad = torch.empty(B * V * Cout * Hf * Wf, dtype=torch.float32, device=dev)
            _capi.check(L.mvhmr_conv1x1_to_quad(_ptr(x), _ptr(w2), _ptr(bias) if bias is not None else ctypes.c_void_p(0), _ptr(quad),
                                                B * V, Cin, Cout, Hf, Wf, _stream(dev)))
        geometry = ([float(v) for v in position], [float(v) for v in sides], [int(v) for v in vol])
        desc = (B, V, Cout, Hf, Wf, method, _capi.F32, _dtype_code(out_dtype), _capi.LAYOUT_QUAD, _capi.VARIANT["auto"])
        out = _native().unprojection_cuboid(quad, proj, rot, center, *geometry, *desc)
        ctx.save_for_backward(x, w2, quad, proj, rot, center)
        ctx.geometry, ctx.desc, ctx.has_bias, ctx.wshape = geometry, desc, bias is not None, tuple(weight.shape)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, w2, quad, proj, rot, center = ctx.saved_tensors
        L = _capi.lib()
        B, V, Cin, Hf, Wf = x.shape
        Cout = w2.shape[0]
        dev = x.device
        g_geo = (None, None, None)
        want_geo = tuple(ctx.needs_input_grad[3:6])
        if any(want_geo):
            g_geo = _native().unprojection_cuboid_backward_geometry(grad_out.contiguous(), quad, proj, rot, center, *ctx.geometry, *ctx.desc,
                                                                    *want_geo)
            g_geo = tuple(t if w else None for t, w in zip(g_geo, want_geo))
        gx = gw = gb = None
        if not any(ctx.needs_input_grad[:3]):
            return (None, None, None) + g_geo + (None,) * 5
        det = torch.are_deterministic_algorithms_enabled()                                   # bitwise reproducible feature and wgrad kernels
        gy = _native().unprojection_cuboid_backward(grad_out.contiguous(), quad, proj, rot, center, *ctx.geometry, *ctx.desc, deterministic=det).view(
            B * V, Cout, Hf * Wf)                                                                # gradient w.r.t. the conv output, planar
        xf = x.view(B * V, Cin, Hf * Wf)
        if ctx.needs_input_grad[0]:
            if L.mvhmr_conv1x1_planar_supported(Cout, Cin, Hf * Wf):                           # (Cin, Cout) @ (BV, Cout, HW) on the MFMA GEMM
                gx = torch.empty((B, V, Cin, Hf, Wf), dtype=torch.float32, device=dev)
                wt = w2.t().contiguous()
                with torch.cuda.device(dev):
                    _capi.check(L.mvhmr_conv1x1_planar(_ptr(gy), _ptr(wt), ctypes.c_void_p(0), _ptr(gx), B * V, Cout, Cin, Hf * Wf, _stream(dev)))
            else:
                gx = torch.matmul(w2.t(), gy).view(B, V, Cin, Hf, Wf)
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if det and ctx.needs_input_grad[1] and L.mvhmr_conv1x1_wgrad_supported(Cin, Cout, Hf * Wf):
            gw = torch.empty(ctx.wshape, dtype=torch.float32, device=dev)                      # written: partial slabs summed in a fixed order
            gb = torch.empty(Cout, dtype=torch.float32, device=dev) if want_b else None
            n = L.mvhmr_conv1x1_wgrad_deterministic_workspace_bytes(B * V, Cin, Cout, Hf * Wf)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev)
                # straight from the caching allocator: torch.empty would fill it under the deterministic flag, and the kernel writes every byte
                ws = torch.cuda.caching_allocator_alloc(n, dev, stream)
                try:
                    _capi.check(L.mvhmr_conv1x1_wgrad_deterministic(_ptr(gy), _ptr(x), _ptr(gw), _ptr(gb) if want_b else ctypes.c_void_p(0), B * V,
                                                                    Cin, Cout, Hf * Wf, ctypes.c_void_p(ws), n, _stream(dev)))
                finally:
                    torch.cuda.caching_allocator_delete(ws)                # stream-ordered: reused only after the kernels on this stream
        elif ctx.needs_input_grad[1] and L.mvhmr_conv1x1_wgrad_supported(Cin, Cout, Hf * Wf):
            gw = torch.zeros(ctx.wshape, dtype=torch.float32, device=dev)                      # split-K GEMM adds into it
            gb = torch.zeros(Cout, dtype=torch.float32, device=dev) if want_b else None
            with torch.cuda.device(dev):
                _capi.check(L.mvhmr_conv1x1_wgrad(_ptr(gy), _ptr(x), _ptr(gw), _ptr(gb) if want_b else ctypes.c_void_p(0), B * V, Cin, Cout,
                                                  Hf * Wf, _stream(dev)))
        else:
            if ctx.needs_input_grad[1]:
                gw = torch.einsum("nop,nip->oi", gy, xf).view(ctx.wshape)
            if want_b:
                gb = gy.sum(dim=(0, 2))
        return (gx, gw, gb) + g_geo + (None,) * 5


def _effective_weights(view_mask, view_weights, like):
    """-> (present (B, V) bool, the DLT's confidences (B, V) fp32) on like.device: the mask as 0 / 1, or the weights where mask and w > 0
    (differentiable w.r.t. view_weights) and 0 elsewhere"""
    present = None if view_mask is None else view_mask.to(device=like.device) != 0
    if view_weights is None:
        return present, present.to(torch.float32)
    w = view_weights.to(device=like.device, dtype=torch.float32)
    present = (w > 0) if present is None else present & (w > 0)
    return present, torch.where(present, w, torch.zeros((), dtype=torch.float32, device=like.device))


def pack_cameras(cameras, device):
    """One pass over batch['cameras'] (list[V] of list[B] of Camera) -> float64 device tensors K (B,V,3,3) and Rt (B,V,3,4).
    A data loader that hands `batch['cameras_packed'] = pack_cameras(...)` (or builds the two tensors itself) lets
    VolumeGenerator.forward derive the feature-level projection matrices on the device: no Python loop over B x V cameras and no
    host-to-device copy per call."""
    V, B = len(cameras), len(cameras[0])
    K = np.array([[cameras[v][b].K for v in range(V)] for b in range(B)], dtype=np.float64)
    Rt = np.array([[np.hstack([cameras[v][b].R, cameras[v][b].t]) for v in range(V)] for b in range(B)], dtype=np.float64)
    return {"K": torch.from_numpy(K).to(device), "Rt": torch.from_numpy(Rt).to(device)}


def feature_level_projections_device(packed, images_shape, features_shape):
    """feature_level_projections on the device from packed cameras: the same float64 operations in the same order
    (update_after_resize incl. quirk Q3, then K @ [R|t] as a k-ordered sum of products), cast to float32 at the end."""
    height, width = images_shape
    new_width, new_height = features_shape
    sx, sy = new_width / width, new_height / height
    K = packed["K"].clone()
    Rt = packed["Rt"]
    K[..., 0, 0] = K[..., 0, 0] * sx
    K[..., 1, 1] = K[..., 1, 1] * sy
    K[..., 0, 2] = K[..., 0, 2] * sx
    K[..., 1, 2] = K[..., 1, 2] * sy
    P = K[..., :, 0:1] * Rt[..., 0:1, :]
    P = P + K[..., :, 1:2] * Rt[..., 1:2, :]
    P = P + K[..., :, 2:3] * Rt[..., 2:3, :]
    return P.to(torch.float32)


class VolumeGenerator(nn.Module):
    """1x1 conv on the per-view feature maps + un-projection into a voxel volume (aggregation.py:90-195).

    lens_distortion (extension, default False; cfg key MODEL.AGGREGATION.LENS_DISTORTION): un-project THROUGH the cameras' lens distortion
    (DESIGN.md 5.13), so that the backbone may run on raw, un-rectified crops.  forward then reads batch['lens'] (B, V, 10) when given, else
    builds it from batch['cameras'] (feature_level_lens), and runs the gather family (the fused conv route is skipped).  The
    use_triangulation pivot is unchanged: it triangulates the image centres, which sit next to the principal points, where the lens
    displacement is of second order in the normalised radius (radially even third), far below the cuboid's voxel pitch."""

    def __init__(self, volume_size=64, input_channels=256, output_channels=32, cuboid_side=2500.0,
                 aggregation_method='softmax', use_triangulation=False, kind='mpii', device='cuda',
                 dataset='human36m', volume_dtype=None, visible_only=False, lens_distortion=False, **kwargs):
        # **kwargs swallows unknown keywords exactly like the reference (quirk Q5: build_volume_generator
        # passes volume_aggregation_method=, so aggregation_method keeps its default)
        super().__init__()
        self.volume_size = volume_size
        self.cuboid_side = cuboid_side
        self.aggregation_method = aggregation_method
        self.process_feature = nn.Sequential(nn.Conv2d(input_channels, output_channels, 1))   # keys process_feature.0.*
        self.use_triangulation = use_triangulation
        self.kind = kind
        self.dataset = dataset
        self.volume_dtype = volume_dtype  # extension: None = float32 like the reference; torch.bfloat16 / float16 for a half-precision consumer
        self.visible_only = bool(visible_only)  # extension: every voxel aggregates only the views that see it
        self.lens_distortion = bool(lens_distortion)  # extension: un-project through the cameras' lens distortion (the class docstring)
        self.output_channels = output_channels
        self.fused_conv = True            # 1x1 conv + layout pass as one MFMA GEMM wherever its shapes allow (see _fused_path_applies)
        self.to(device)

    @property
    def volume_channels(self):
        """channels of the volume forward() returns: output_channels, or twice that for aggregation_method='meanvar' (the mean and the
        cross-view variance) -- what the volumetric regressor behind it must be built for"""
        return self.output_channels * (2 if self.aggregation_method == "meanvar" else 1)

    # -- geometry the reference builds inside forward(); split out so it can be checked without a GPU
    def cuboid(self):
        sides = np.array([self.cuboid_side, self.cuboid_side, self.cuboid_side])
        position = np.array([0, 0, 0]) - sides / 2          # quirk Q4: centred on the world origin (:140-144)
        return volumetric.Cuboid3D(position, sides)

    def rotation_axis(self):
        if self.kind == "coco":
            return [0, 1, 0]
        if self.kind == "mpii":
            return [0, 0, 1]
        raise ValueError("Unknown kind: {}".format(self.kind))  # the reference fails with UnboundLocalError here

    def volume_pose(self, batch, proj_matricies_org, images_shape, view_mask=None, view_weights=None, feature_index=None):
        """Per-sample rotation (B,3,3) and pivot (B,3), float32 numpy/tensor (aggregation.py:163-181).

        Training draws theta ~ U(0, 2 pi) from the GLOBAL numpy stream, one draw per sample in order
        (quirk Q6); eval uses theta = 0.  The pivot is keypoints_3d[b][6, :3], or the DLT-triangulated
        image centre when use_triangulation is set -- a function of proj_matricies_org that carries its gradient (the reference
        triangulates from the caller's proj_matricies with torch.svd).  With a view mask (B, V) the pivot is the weighted DLT with the mask as
        the confidences, on projections whose masked rows are zeroed first (0 * NaN is not 0); fewer than two present views is undefined.
        With view_weights (B, V) the confidences are the effective weights (mask ? w : 0 where w > 0, else 0), which carry their gradient.
        With a feature_index (M,) there is one pose per VOLUME: M draws of theta in order (the identity index consumes the stream as no index
        does), keypoints_3d holds M entries, and the per-sample DLT pivots are gathered by the index with torch indexing (differentiable)."""
        batch_size = proj_matricies_org.shape[0] if feature_index is None else feature_index.shape[0]
        axis = self.rotation_axis()
        if self.training:
            # one draw per sample, in order, from the GLOBAL numpy stream (Q6): a sized draw consumes the same stream
            thetas = np.random.uniform(0.0, 2 * np.pi, size=batch_size)
            rots = volumetric.get_rotation_matrices(axis, thetas).astype(np.float32)
        else:
            # theta = 0 for every sample: the same matrices call after call -- kept on the device, so that an eval forward with packed
            # cameras and tensor keypoints copies nothing from the host (and can be captured into a HIP graph: scripts/graph_volgen.py)
            key = (batch_size, proj_matricies_org.device)
            cache = self.__dict__.setdefault("_eval_rots", {})
            if key not in cache:
                r0 = np.broadcast_to(volumetric.get_rotation_matrix(axis, 0.0).astype(np.float32), (batch_size, 3, 3))
                cache[key] = torch.from_numpy(np.array(r0, dtype=np.float32)).to(proj_matricies_org.device)
            rots = None
        if self.use_triangulation:
            # one batched DLT on the device, no per-sample .cpu(); stays a device tensor
            n_views = proj_matricies_org.shape[1]
            images_center = (torch.tensor(images_shape, dtype=torch.float32) / 2).expand(n_views, 2)
            if view_mask is None and view_weights is None:
                centers = multiview.triangulate_points_from_multiple_views_linear_batch(proj_matricies_org, images_center)   # differentiable
            else:
                present, conf = _effective_weights(view_mask, view_weights, proj_matricies_org)
                P = torch.where(present[:, :, None, None], proj_matricies_org, torch.zeros((), dtype=proj_matricies_org.dtype,
                                                                                          device=proj_matricies_org.device))
                centers = multiview.triangulate_points_from_multiple_views_linear_batch(P, images_center, conf)
            if feature_index is not None:
                centers = centers[feature_index.to(device=centers.device, dtype=torch.long)]
        else:
            kp = batch['keypoints_3d']
            if torch.is_tensor(kp):                                          # already a (B, 17, 3|4) tensor (any device)
                centers = kp[:, 6, :3].to(torch.float32)
            else:
                centers = torch.from_numpy(np.stack([np.asarray(kp[b][6, :3], dtype=np.float32) for b in range(batch_size)]))
        if rots is None:
            return cache[key], centers
        return torch.from_numpy(np.ascontiguousarray(rots)), centers

    def coord_volumes(self, rots, centers, device):
        """(B,S,S,S,3) float32 on `device`: rot @ (grid - center) + center, built by one kernel
        (mvhmr_build_coord_volumes) instead of B x (meshgrid + 3 strided writes + mm) (aggregation.py:138-187)."""
        L = _capi.lib()
        B, S = rots.shape[0], self.volume_size
        cub = self.cuboid()
        rots = rots.to(device=device, dtype=torch.float32).contiguous()
        centers = centers.to(device=device, dtype=torch.float32).contiguous()
        with torch.cuda.device(device):
            coords = torch.empty(B, S, S, S, 3, dtype=torch.float32, device=device)
            pos = (ctypes.c_double * 3)(*[float(x) for x in cub.position])
            sides = (ctypes.c_double * 3)(*[float(x) for x in cub.sides])
            _capi.check(L.mvhmr_build_coord_volumes(_ptr(coords), _ptr(rots), _ptr(centers), B, S, pos, sides, _stream(device)))
        return coords

    def forward(self, features, proj_matricies, batch, use_gt=True):
        return self.forward_with_pose(features, proj_matricies, batch, use_gt=use_gt)[0]

    def forward_with_pose(self, features, proj_matricies, batch, use_gt=True):
        """forward(), and the pose it placed the volume with: (volumes, rotations (B,3,3), centers (B,3)), the float32 device tensors the
        un-projection read.  In training the rotation is a draw from numpy's global stream, which a caller cannot repeat; soft_argmax()
        needs exactly these two to map the volume back to world points.  The same numpy draws and launches as forward()."""
        features_shape = tuple(features.shape[-2:])
        images_shape = tuple(batch['images'].shape[2:-1])
        batch_size, n_views = batch['images'].shape[:2]
        device = features.device

        proj_org = proj_matricies                                           # only read (reference clones, :124)
        if 'cameras_packed' in batch:                                       # device tensors: no camera loop, no H2D copy
            proj = feature_level_projections_device(batch['cameras_packed'], images_shape, features_shape)
        else:
            proj = torch.from_numpy(feature_level_projections(batch['cameras'], images_shape, features_shape))
        # the kernels take raw device pointers: whatever device the packed cameras live on (a loader may pack them on the host)
        proj = proj.to(device=device, dtype=torch.float32).contiguous()
        # the batch's optional keys: view_mask (B, V) per-sample present views, view_weights (B, V) per-view confidences (5.9),
        # view_confidence (B, V, Hf, Wf) per-pixel confidence maps (5.11), feature_index (M,): M volumes share the samples' feature maps,
        # -> (M, C, S, S, S) (5.12), lens (B, V, 10): the lens records, read only under lens_distortion (5.13)
        options = {key: batch.get(key) for key in ("view_mask", "view_weights", "view_confidence", "feature_index")}
        options["visible_only"] = self.visible_only
        options["lens"] = batch.get('lens') if self.lens_distortion else None
        if self.lens_distortion and options["lens"] is None:
            options["lens"] = torch.from_numpy(feature_level_lens(batch['cameras'], images_shape, features_shape))
        _check_options((batch_size, n_views) + features_shape, self.aggregation_method, **options)     # before anything runs
        given = {key: value for key, value in options.items() if value is not None and value is not False}
        # (a batch without options calls volume_pose and unprojection_cuboid exactly as one before the options existed)
        rots, centers = self.volume_pose(batch, proj_org, images_shape, **{key: given[key] for key in ("view_mask", "view_weights", "feature_index")
                                                                          if key in given})
        cub = self.cuboid()
        S = self.volume_size
        rots = rots.to(device=device, dtype=torch.float32).contiguous()
        centers = centers.to(device=device, dtype=torch.float32).contiguous()

        # (the fused conv writes the quad-planar copy, which no option takes: a lens call runs the gather family, the others read planar or
        # channels-last features)
        if not given and self._fused_path_applies(features, S):
            # 1x1 conv and layout pass in one MFMA GEMM, its output only ever exists in the layout the brick forward stages
            conv = self.process_feature[0]
            return _FusedAggregate.apply(features, conv.weight, conv.bias, proj, rots, centers, tuple(cub.position), tuple(cub.sides),
                                         (S, S, S), _capi.AGG[self.aggregation_method], self.volume_dtype or torch.float32), rots, centers

        features = features.view(-1, *features.shape[2:])
        features = self.process_feature(features)
        features = features.view(batch_size, n_views, *features.shape[1:])
        # the coordinate volumes (aggregation.py:138-187) are never materialised: the kernels evaluate the cuboid recipe per voxel
        return unprojection_cuboid(features, proj, rots, centers, cub.position, cub.sides, (S, S, S),
                                   aggregation_method=self.aggregation_method, out_dtype=self.volume_dtype, **given), rots, centers

    def soft_argmax(self, volumes, rotations, centers, beta=1.0, return_logsumexp=False):
        """World keypoints (B, J, 3) of heat volumes (B, J, S, S, S) that live on this module's cuboid, placed by the rotations and centers
        forward_with_pose returned (softargmax.soft_argmax_3d_cuboid: no coordinate volume; differentiable w.r.t. all three tensors)."""
        from . import softargmax
        cub = self.cuboid()
        return softargmax.soft_argmax_3d_cuboid(volumes, rotations, centers, cub.position, cub.sides, beta=beta, return_logsumexp=return_logsumexp)

    def sample(self, volumes, points, rotations, centers, paired=False, return_index=False):
        """Volumes (B, C, S, S, S) that live on this module's cuboid, placed by the rotations and centers forward_with_pose returned, read
        trilinearly at the world points (B, N, 3) (volsample.sample_volume_cuboid; differentiable w.r.t. all four tensors)."""
        from . import volsample
        cub = self.cuboid()
        return volsample.sample_volume_cuboid(volumes, points, rotations, centers, cub.position, cub.sides, paired=paired, return_index=return_index)

    def project(self, volumes, rays, rotations, centers, map_shape, n_samples, method="mean", **kwargs):
        """Volumes (B, C, S, S, S) that live on this module's cuboid, placed by the rotations and centers forward_with_pose returned, rendered
        into camera-view maps (B, V, C, Hm, Wm) along rays (B, V, 3, 4) = volproject.camera_rays(proj_matricies)
        (volproject.project_volume_cuboid, which takes the keywords beta, min_depth, max_depth, return_ranges; differentiable w.r.t. volumes)."""
        from . import volproject
        cub = self.cuboid()
        return volproject.project_volume_cuboid(volumes, rays, rotations, centers, cub.position, cub.sides, map_shape, n_samples, method, **kwargs)

    def peaks(self, volumes, rotations, centers, k, radius=1, threshold=None):
        """(scores, index, positions) of the k largest local maxima of every slice of heat volumes (B, J, S, S, S) that live on this module's
        cuboid, placed by the rotations and centers forward_with_pose returned (peaks.volume_peaks_cuboid: 3-D non-maximum suppression of
        half-width `radius`, strictly above `threshold`; peaks.peak_proposals turns the result into one fine volume per proposal)."""
        from . import peaks
        cub = self.cuboid()
        return peaks.volume_peaks_cuboid(volumes, rotations, centers, cub.position, cub.sides, k, radius=radius, threshold=threshold)

    def _fused_path_applies(self, features, S):
        """The fused conv writes the quad-planar layout, which the un-projection consumes for every geometry (brick kernels as it
        is, gather kernels through one conversion; the device-side gate picks per call).  So only shapes, dtypes and devices
        decide here -- checked on every call, nothing cached: fp32 everywhere, conv parameters on the features' device, a shape the
        fused GEMM takes and one whose quad-planar copy the un-projection (forward and backward) accepts.  The GEMMs read their operands
        with 16-byte loads and put the B * V maps in the grid's z extent: memory the route would hand them as it is (a contiguous
        tensor is not copied) must sit on a 16-byte boundary, and B * V must not exceed _FUSED_MAX_MAPS."""
        if not self.fused_conv or not features.is_cuda or features.dtype != torch.float32 or self.aggregation_method not in _METHODS:
            return False
        if self.volume_dtype not in (None, torch.float32, torch.bfloat16):
            return False                                                          # fp32 conv output with an fp16 volume: not a storage mode of the library
        conv = self.process_feature[0]
        params = [conv.weight] + ([conv.bias] if conv.bias is not None else [])
        if any(t.dtype != torch.float32 or t.device != features.device for t in params):
            return False
        if any(t.is_contiguous() and t.data_ptr() % 16 != 0 for t in (features, conv.weight)):
            return False
        if conv.bias is not None and conv.bias.data_ptr() % 16 != 0:             # (the bias is never copied)
            return False
        B, V, Cin, Hf, Wf = features.shape
        Cout = conv.out_channels
        L = _capi.lib()
        if B * V > _FUSED_MAX_MAPS or not L.mvhmr_conv1x1_to_quad_supported(Cin, Cout, Hf, Wf):
            return False
        meta = torch.empty((B, V, Cout, Hf, Wf), dtype=torch.float32, device="meta")
        desc = _make_desc(meta, (S, S, S), _capi.AGG[self.aggregation_method], self.volume_dtype or torch.float32, _capi.LAYOUT_QUAD, _capi.VARIANT["auto"])
        return L.mvhmr_unproject_selected_variant(ctypes.byref(desc)) > 0 and L.mvhmr_unproject_backward_supported(ctypes.byref(desc)) == 1


def _cfg_flag(cfg, key):
    """MODEL.AGGREGATION.<key>, an extension key the reference's cfg tree does not have: absent (however the tree says so) = False"""
    try:
        return bool(getattr(cfg.MODEL.AGGREGATION, key))
    except (AttributeError, KeyError):
        return False


def build_volume_generator(cfg):
    """cfg is the reference's yacs tree (cfg/defaults.py:18-30,89-90); same wiring as aggregation.py:198-208."""
    input_channels = cfg.MODEL.BACKBONE.DECONV_FILTERS[-1] if cfg.MODEL.BACKBONE.DECONV_LAYERS != 0 else 2048
    return VolumeGenerator(volume_size=cfg.MODEL.AGGREGATION.VOLUME_SIZE,
                           input_channels=input_channels,
                           output_channels=cfg.MODEL.AGGREGATION.OUTPUT_CHANNELS,
                           cuboid_side=cfg.MODEL.AGGREGATION.CUBOID_SIDE,
                           use_triangulation=cfg.MODEL.AGGREGATION.USE_TRIANGULATION,
                           kind=cfg.DATASET.KIND,
                           dataset=cfg.DATASET.TYPE,
                           volume_aggregation_method=cfg.MODEL.AGGREGATION.METHOD,
                           visible_only=_cfg_flag(cfg, "VISIBLE_ONLY"),
                           lens_distortion=_cfg_flag(cfg, "LENS_DISTORTION"))
