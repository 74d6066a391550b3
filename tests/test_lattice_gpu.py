"""Every un-projection route held to BIT equality with one float64 oracle on the exact lattice rig (tests/lattice_rig.py),
and the layout passes compared as memory images with a plain numpy permutation.

The rig's inputs make every fp32 operation of projection, normalisation, bilinear sampling, `sum`, `max` and power-of-two `mean` exact
(tests/test_lattice_cpu.py checks that premise on the CPU), so a kernel's order of additions and of float atomics cannot matter and any
difference from the oracle -- a tap on the wrong side of an inclusive border, a pad channel that is not zero, a window one line short, a
ragged band transposed wrongly -- is a whole quantum of the rig, not something a tolerance could hide.  The oracle's float64 result is
cast once to the storage type (round to nearest even) and compared through torch.equal on the raw bits; every comparison also goes
through conftest.record_err with bound 0.0.  Softmax is not exact and stays with tests/test_unproject_gpu.py; the plane backward is not
bit-exact by design (its fixed-point scale is not a power of two) and is held to a bound derived from its code instead
(test_plane_backward_stays_inside_its_derived_bound).

The geometry gradients (grad_proj, grad_coords, the cuboid's grad_rot / grad_center) are held to the bits of lattice_rig.geo_oracle on the
geometry rigs (power-of-two maps), every route and option family, and the kept ix == -1 / iy == -1 boundary to a bound derived from the
code: the section "the geometry path" at the end.

Deterministic mode: every backward runs again under torch.use_deterministic_algorithms(True).  Its int64 fixed point uses a power-of-two
exponent (det_scale.h) whose quantum lies orders of magnitude below the rig's, so the result must have the oracle's bits too."""
import ctypes

import numpy as np
import pytest
import torch

import lattice_rig as rig
from conftest import record_err
from multiviewhmr_amd import _capi, aggregation

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
INT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
K_LOG2E = np.float32(1.4426950408889634)
vp = ctypes.c_void_p


def _cast(ref64, dtype, device):
    """the float64 oracle cast ONCE to the storage type: float64 -> fp32 is exact on the rig (asserted), fp32 -> 16 bit rounds to nearest even"""
    r32 = np.asarray(ref64).astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), np.asarray(ref64, np.float64)), "the oracle's value is not an fp32 number: rig error"
    return torch.from_numpy(r32).to(device).to(dtype)


def _hold(name, got, ref64):
    """bit equality with the oracle, recorded with bound 0.0"""
    want = _cast(ref64, got.dtype, got.device)
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    err = float((got.double() - want.double()).abs().max()) if got.numel() else 0.0
    record_err("lattice " + name, err if err == err else float("inf"), 0.0)
    assert torch.equal(got.contiguous().view(INT[got.dtype]), want.contiguous().view(INT[want.dtype])), name + ": equal values, different bits"


def _methods(V, masked=False):
    return ("sum", "max") + (("mean",) if not masked and V in (1, 2, 4, 8) else ())


def _desc(shape, vol, method, feat, out, layout, variant):
    like = torch.empty(shape, dtype=DT[feat], device="meta")
    return aggregation._make_desc(like, tuple(vol), _capi.AGG[method], DT[out], layout, _capi.VARIANT[variant])


def _kernel(d):
    return _capi.lib().mvhmr_unproject_forward_kernel_name(ctypes.byref(d))


def _stream(gpu):
    return vp(torch.cuda.current_stream(gpu).cuda_stream)


class _Deterministic:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        torch.use_deterministic_algorithms(self.on)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(False)


# ----------------------------------------------------------------------------------------------- routes through aggregation.unprojection
def _c(rig_name, variant, kernels, feat="f32", out=None, channels_last=False):
    out = out or feat
    tag = "%s %s %s->%s%s" % (rig_name, variant, feat, out, " channels-last" if channels_last else "")
    return pytest.param(dict(rig=rig_name, variant=variant, kernels=kernels, feat=feat, out=out, cl=channels_last, tag=tag), id=tag.replace(" ", "_"))


GATHER, BRICK, GROUPS, WS = (b"k_fwd_gather",), (b"k_fwd_brick",), (b"k_fwd_brick_groups",), (b"k_fwd_ws",)
ROUTES = [
    # the gather forward with the per-tap scatter backward and k_grad_to_planar (V = 3, C % 4 != 0: never the plane kernel)
    _c("gather_v3", "gather", GATHER),
    _c("gather_cl", "gather", GATHER, channels_last=True),          # (C % 4 == 0) the backward goes in place, and through k_grad_cast for fp16
    _c("gather_v3", "gather", GATHER, feat="f16"),
    _c("gather_cl", "gather", GATHER, feat="f16", channels_last=True),
    _c("gather_v3", "gather", GATHER, out="bf16"),
    _c("gather_v1", "gather", GATHER), _c("gather_v2", "gather", GATHER), _c("gather_v4", "gather", GATHER), _c("gather_v8", "gather", GATHER),
    _c("gather_v12", "gather", GATHER),                             # V > 8: the VT = 0 instances
    # k_fwd_brick / k_bwd_brick
    _c("brick_v2", "brick", BRICK), _c("brick_v4", "brick", BRICK), _c("brick_v8", "brick", GROUPS),
    _c("brick_v3", "brick", BRICK), _c("brick_v6", "brick", GROUPS),                                 # absent view slots
    _c("brick_ragged", "brick", BRICK),
    _c("brick_c4", "brick", BRICK), _c("brick_c6", "brick", BRICK), _c("brick_c9", "brick", BRICK),  # k_fwd_tail / k_bwd_tail
    _c("brick_slow", "brick", BRICK),                                                                # windows overflow LDS: the slow path
    _c("brick_v4", "brick", BRICK, feat="f16"), _c("brick_v4", "brick", BRICK, out="bf16"),          # 16-bit volumes, even Z
    _c("brick_v8", "brick", GROUPS, out="bf16"),
    # k_fwd_ws: 256 bricks, the least brick_fwd_ws_shape_impl accepts
    _c("ws_v3", "brick", WS), _c("ws_v4", "brick", WS), _c("ws_v3", "brick", WS, feat="f16"), _c("ws_v4", "brick", WS, out="bf16"),
    # k_quad_planar_to_planar: its band width changes between H = 124 and 125 (grad_band)
    _c("band_h124_w5", "brick", BRICK), _c("band_h125_w5", "brick", BRICK), _c("band_h124_w33", "brick", BRICK), _c("band_h125_w33", "brick", BRICK),
]


def _features(feats, case, gpu):
    f = torch.from_numpy(feats).to(gpu).to(DT[case["feat"]])
    if case["cl"]:
        f = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
        assert aggregation._is_channels_last5(f)
    return f.requires_grad_(True)


@pytest.mark.parametrize("case", ROUTES)
def test_route_has_the_oracles_bits(case, gpu):
    """Forward, backward and deterministic backward of one route against the oracle, `sum`, `max` and power-of-two `mean`.

    Bits include the sign of zero: a view that misses the map contributes +0.0 (the +0.0 rule: the comment in fwd_global_voxel,
    csrc/brick_fwd_kernel.h), so a voxel outside every map, or a `max` won by such a view over negative samples, is +0.0 on every route."""
    feats, proj, coords, _ = rig.problem(case["rig"])
    B, V, C, H, W = feats.shape
    vol = coords.shape[1:4]
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    layout = _capi.LAYOUT_BVHWC if case["cl"] else _capi.LAYOUT_BVCHW
    for method in _methods(V):
        d = _desc(feats.shape, vol, method, case["feat"], case["out"], layout, case["variant"])
        assert _kernel(d) in case["kernels"], (case["tag"], method, _kernel(d))
        assert _capi.lib().mvhmr_unproject_backward_supported(ctypes.byref(d)) == 1
        out64, grad, gf64, _ = rig.reference(case["rig"], method)
        go = torch.from_numpy(grad).to(gpu).to(DT[case["out"]])
        for det in (False, True):
            f = _features(feats, case, gpu)
            out = aggregation.unprojection(f, p, c, aggregation_method=method, variant=case["variant"], out_dtype=DT[case["out"]])
            if not det:
                _hold("%s %s fwd" % (case["tag"], method), out.detach(), out64)
            with _Deterministic(det):
                out.backward(go)
            _hold("%s %s bwd%s" % (case["tag"], method, " deterministic" if det else ""), f.grad, gf64)


def test_brick_slow_path_rig_is_one_the_gate_would_not_give_the_bricks(gpu):
    """the windows of `brick_slow` overflow LDS: on the same maps with enough voxels for AUTO to ask, the gate's own query answers gather
    (the rig of the slow path above is that geometry at one brick per sample, forced onto the bricks)"""
    feats, proj, coords, _ = rig.problem("auto_gather")
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    d = _desc(feats.shape, coords.shape[1:4], "sum", "f32", "f32", _capi.LAYOUT_BVCHW, "auto")
    assert _capi.lib().mvhmr_unproject_query_variant(ctypes.byref(d), vp(p.data_ptr()), vp(c.data_ptr()), _stream(gpu)) == _capi.VARIANT["gather"]
    assert rig.RIGS["brick_slow"]["H"] == rig.RIGS["auto_gather"]["H"] and rig.RIGS["brick_slow"]["W"] == rig.RIGS["auto_gather"]["W"]
    assert all(8 * a >= b for a, b in zip(rig.RIGS["brick_slow"]["vol"], rig.RIGS["auto_gather"]["vol"]))     # a brick of it covers no less of a map


@pytest.mark.parametrize("name,expect", [("auto_brick", "brick"), ("auto_gather", "gather")])
def test_auto_runs_the_side_its_gate_picks_with_the_oracles_bits(name, expect, gpu):
    """AUTO launches both variants behind the device-side gate and one runs: `auto_brick` (maps that fit the plane kernel: the backward
    pairing GatedBrickPlane, whose gate picks the bricks) and `auto_gather` (maps too large for it: GatedBrickGather, whose gate picks the
    per-tap scatter).  Whichever side ran, the bits are the oracle's."""
    feats, proj, coords, _ = rig.problem(name)
    V = feats.shape[1]
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    d = _desc(feats.shape, coords.shape[1:4], "sum", "f32", "f32", _capi.LAYOUT_BVCHW, "auto")
    assert _capi.lib().mvhmr_unproject_selected_variant(ctypes.byref(d)) == _capi.VARIANT["brick"]          # a gated shape
    assert _capi.lib().mvhmr_unproject_query_variant(ctypes.byref(d), vp(p.data_ptr()), vp(c.data_ptr()), _stream(gpu)) == _capi.VARIANT[expect]
    for method in ("sum", "max"):
        out64, grad, gf64, _ = rig.reference(name, method)
        go = torch.from_numpy(grad).to(gpu)
        for det in (False, True):
            f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
            out = aggregation.unprojection(f, p, c, aggregation_method=method)
            if not det:
                _hold("%s auto %s fwd" % (name, method), out.detach(), out64)
            with _Deterministic(det):
                out.backward(go)
            _hold("%s auto %s bwd%s" % (name, method, " deterministic" if det else ""), f.grad, gf64)


# ----------------------------------------------------------------------------------------------- the plane backward: a derived bound
@pytest.mark.parametrize("V", [2, 4, 8])
def test_plane_backward_stays_inside_its_derived_bound(V, gpu):
    """The plane backward (csrc/unproject_plane_bwd.hip: k_plane_ds + k_bwd_plane; the shipped configuration's kernel: C = 8, 12 x 12 maps, a
    16^3 volume) is NOT bit-exact on the rig by design: its fixed-point scale is 2139095040 / full with full = gmax (8-byte cells, these
    maps; cm * gmax with int32 cells, a form not run here) -- not a power of two ("scale per channel").  It is held, per gradient element, to a bound derived from
    that code.  With u = 2^-24, S = 2139095040, every tap k of the pixel contributes

        round_int(fl(fl(ds_k * scale) * w_k)),   scale = fl(S / full),          then   val = (float)((double)acc * (double)inv),  inv = fl(full / S)

    so  acc * inv = sum ds_k w_k (1 + d1)(1 + d2)(1 + d3)(1 + d4) + sum e_k (full / S)(1 + d4)  with |d| <= u, |e_k| <= 1/2:

      1. n * (unit / 2) * (1 + u): n taps of non-zero weight meet in the pixel, each rounded to a whole unit.  unit = full / S, taken at its
         upper value cm * gmax / S (cm = the plane's largest n, gmax = max |ds| of the sample's view and channel, both from the oracle);
      2. ((1 + u)^4 - 1) * sum |ds_k w_k|: the FOUR fp32 roundings counted in the code -- ds * scale, * w, the division that makes `scale`,
         the division that makes `inv` (the sum itself is exact in int64, the product with inv is in double);
      3. u * (|ref| + 1. + 2.): the final cast to fp32, half an ulp of the result.

    The bound is derived for the 8-byte-cell form only, which these maps take (plane_wide4; asserted below from its LDS formula).  The
    int32-cell form writes `(float)cell * inv` instead: an int-to-float rounding and an fp32 product more, which this bound does not count.

    Every term comes from the oracle, none from the kernel's output.  Both modes run the same kernels (no global atomics).  The forward of
    these calls is the gather kernel and has the oracle's bits.

    The library has no query for the backward's route, so that the plane kernel ran cannot be asserted.  What can be is every condition
    capi.hip's bwd_uses_plane / plane_bwd_supported put on it: planar unmasked features, V in {2, 4, 8}, C % 4 == 0, a supported backward,
    maps whose planes fit the kernel's LDS, and AUTO choosing the gather family (fewer bricks than CUs).  A quiet per-tap scatter would be
    bit-exact and pass; the bound is an upper one."""
    name = "plane_v%d" % V
    feats, proj, coords, _ = rig.problem(name)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    u, S = 2.0 ** -24, 2139095040.0
    _, _, C, H, W = feats.shape
    cells = H * (W | 1)                                                                       # plane_lds_bytes with 8-byte cells of four channels
    assert feats.shape[1] == V and V in (2, 4, 8) and C % 4 == 0
    assert 4 * cells * 8 + 4 * ((cells + 31) // 32) * 4 + 16 <= 160 * 1024 - 512              # plane_wide4: the form the bound is derived for
    for method in _methods(V):
        d = _desc(feats.shape, coords.shape[1:4], method, "f32", "f32", _capi.LAYOUT_BVCHW, "auto")
        assert _capi.lib().mvhmr_unproject_selected_variant(ctypes.byref(d)) == _capi.VARIANT["gather"] and _kernel(d) in GATHER
        assert _capi.lib().mvhmr_unproject_backward_supported(ctypes.byref(d)) == 1
        out64, grad, gf64, res = rig.reference(name, method)
        n = res["tap_count"].astype(np.float64)[:, :, None]                                   # (B,V,1,H,W)
        cm = res["tap_count"].reshape(res["tap_count"].shape[:2] + (-1,)).max(2).astype(np.float64)
        unit = (cm[:, :, None] * res["ds_max"] / S)[:, :, :, None, None]                      # (B,V,C,1,1)
        e1 = n * 0.5 * unit * (1 + u)
        e2 = ((1 + u) ** 4 - 1) * res["bwd_abs"]
        bound = e1 + e2 + u * (np.abs(gf64) + e1 + e2)
        go = torch.from_numpy(grad).to(gpu)
        for det in (False, True):
            f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
            out = aggregation.unprojection(f, p, c, aggregation_method=method)
            if not det:
                _hold("%s auto %s fwd" % (name, method), out.detach(), out64)
            with _Deterministic(det):
                out.backward(go)
            err = np.abs(f.grad.cpu().numpy().astype(np.float64) - gf64)
            worst = int(np.argmax(err - bound))
            print("plane bwd %s %s%s: max err %.3e, its bound %.3e, max bound %.3e" % (name, method, " det" if det else "", err.max(), bound.ravel()[np.argmax(err)], bound.max()))
            record_err("lattice %s plane %s bwd%s (derived bound)" % (name, method, " deterministic" if det else ""), float(err.ravel()[worst]), float(bound.ravel()[worst]))
            assert (err <= bound).all()


# ----------------------------------------------------------------------------------------------- caller-held quad-planar features (C ABI)
def _abi_forward(d, feat, p, c, out, gpu):
    L = _capi.lib()
    nb = L.mvhmr_unproject_forward_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=gpu)
    _capi.check(L.mvhmr_unproject_forward(ctypes.byref(d), vp(feat.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(out.data_ptr()), vp(ws.data_ptr()), nb, _stream(gpu)))
    torch.cuda.synchronize(gpu)


def _abi_backward(d, go, feat, p, c, grad, det, gpu):
    L = _capi.lib()
    size = L.mvhmr_unproject_backward_deterministic_workspace_bytes if det else L.mvhmr_unproject_backward_workspace_bytes
    run = L.mvhmr_unproject_backward_deterministic if det else L.mvhmr_unproject_backward
    nb = size(ctypes.byref(d))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=gpu)
    _capi.check(run(ctypes.byref(d), vp(go.data_ptr()), vp(feat.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(grad.data_ptr()), vp(ws.data_ptr()), nb, _stream(gpu)))
    torch.cuda.synchronize(gpu)


@pytest.mark.parametrize("name,variant,kernels", [("brick_v4", "brick", BRICK), ("brick_c6", "brick", BRICK),
                                                  ("quad_c8", "gather", GATHER), ("quad_c512", "gather", GATHER)])
def test_caller_held_quad_features(name, variant, kernels, gpu):
    """MVHMR_LAYOUT_QUAD features made by mvhmr_convert_features and handed to forward and backward: into the brick kernels as they are, and
    with variant = gather through k_quad_to_channels_last (C = 512 is the first channel count at which quad_band_log2 drops from 5 to 4);
    the backward writes the planar gradient"""
    feats, proj, coords, _ = rig.problem(name)
    B, V, C, H, W = feats.shape
    vol = tuple(coords.shape[1:4])
    L = _capi.lib()
    f, p, c = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    d0 = _desc(feats.shape, vol, "sum", "f32", "f32", _capi.LAYOUT_BVCHW, variant)
    quad = torch.empty(L.mvhmr_feature_layout_bytes(ctypes.byref(d0), _capi.LAYOUT_QUAD), dtype=torch.uint8, device=gpu)
    _capi.check(L.mvhmr_convert_features(ctypes.byref(d0), vp(f.data_ptr()), _capi.LAYOUT_QUAD, vp(quad.data_ptr()), _stream(gpu)))
    for method in _methods(V):
        d = _desc(feats.shape, vol, method, "f32", "f32", _capi.LAYOUT_QUAD, variant)
        assert _kernel(d) in kernels and L.mvhmr_unproject_backward_supported(ctypes.byref(d)) == 1
        out64, grad, gf64, _ = rig.reference(name, method)
        out = torch.full((B, C) + vol, float("nan"), device=gpu)
        _abi_forward(d, quad, p, c, out, gpu)
        _hold("%s quad %s %s fwd" % (name, variant, method), out, out64)
        go = torch.from_numpy(grad).to(gpu)
        for det in (False, True):
            g = torch.full((B, V, C, H, W), float("nan"), device=gpu)
            _abi_backward(d, go, quad, p, c, g, det, gpu)
            _hold("%s quad %s %s bwd%s" % (name, variant, method, " deterministic" if det else ""), g, gf64)


# ----------------------------------------------------------------------------------------------- option routes
@pytest.mark.parametrize("tag", [t[0] for t in rig.option_cases()])
def test_option_route_has_the_oracles_bits(tag, gpu):
    """view_mask (a full, a single-view and an empty sample), view_weights (dyadic), visible_only (alone and with a mask), view_confidence
    (dyadic maps with zeros) and feature_index (a repeated, a skipped and an out-of-range entry), each restated in the float64 oracle from
    the README's definition (lattice_rig.oracle): forward, feature backward in both modes, view_visibility's bitmask, and on the small rig
    grad_weights / grad_confidence"""
    _, name, method, kw = next(t for t in rig.option_cases() if t[0] == tag)
    res = rig.option_reference(tag)
    feats, proj, coords, _ = rig.problem(name)
    H, W = feats.shape[3:]
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    go = torch.from_numpy(res["grad_out"]).to(gpu)
    side = kw.get("want_side_grads", False)
    for det in (False, True):
        f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
        args = {}
        if "view_mask" in kw:
            args["view_mask"] = torch.from_numpy(kw["view_mask"]).to(gpu)
        if "view_weights" in kw:
            args["view_weights"] = torch.from_numpy(kw["view_weights"]).to(gpu).requires_grad_(side)
        if "view_confidence" in kw:
            args["view_confidence"] = torch.from_numpy(kw["view_confidence"]).to(gpu).requires_grad_(side)
        if "feature_index" in kw:
            args["feature_index"] = torch.from_numpy(kw["feature_index"]).to(gpu)      # a device index is not inspected: 7 is out of range
        if kw.get("visible_only"):
            args["visible_only"] = True
        out = aggregation.unprojection(f, p, c, aggregation_method=method, variant="gather", **args)
        if not det:
            _hold("option %s fwd" % tag, out.detach(), res["out"])
        with _Deterministic(det):
            out.backward(go)
        _hold("option %s bwd%s" % (tag, " deterministic" if det else ""), f.grad, res["grad_features"])
        if side and "view_weights" in kw:
            _hold("option %s grad_weights%s" % (tag, " deterministic" if det else ""), args["view_weights"].grad, res["grad_weights"])
        if side and "view_confidence" in kw:
            _hold("option %s grad_confidence%s" % (tag, " deterministic" if det else ""), args["view_confidence"].grad, res["grad_confidence"])
    if "feature_index" not in kw:
        # voxels exactly on ix = 0 and ix = W - 1 are seen, the ones half a step outside are not
        bits = aggregation.view_visibility(p, c, (H, W), view_mask=args.get("view_mask"))
        want = torch.from_numpy(res["visibility"]).to(gpu)
        record_err("lattice option %s visibility bits" % tag, float((bits != want).sum()), 0.0)
        assert bits.dtype == torch.int32 and torch.equal(bits, want)


# ----------------------------------------------------------------------------------------------- layout passes as memory images
def _convert(src, shape, feat, src_layout, dst_layout, gpu, offset):
    """mvhmr_convert_features of `src` (numpy, in the source layout's order) into a buffer of exactly mvhmr_feature_layout_bytes, prefilled
    with 0xFF bytes; offset = 1 moves the source's base pointer by one element (off the 16-byte grid) -> (bytes as numpy uint8, their count)"""
    L = _capi.lib()
    B, V, C, H, W = shape
    d = _desc(shape, (2, 2, 2), "sum", feat, feat, src_layout, "auto")
    nb = L.mvhmr_feature_layout_bytes(ctypes.byref(d), dst_layout)
    flat = torch.from_numpy(np.ascontiguousarray(src).ravel()).to(gpu).to(DT[feat])
    hold = torch.zeros(flat.numel() + 8, dtype=DT[feat], device=gpu)
    view = hold[offset:offset + flat.numel()]
    view.copy_(flat)
    assert (view.data_ptr() % 16 == 0) == (offset == 0)
    dst = torch.full((nb,), 0xFF, dtype=torch.uint8, device=gpu)
    _capi.check(L.mvhmr_convert_features(ctypes.byref(d), vp(view.data_ptr()), dst_layout, vp(dst.data_ptr()), _stream(gpu)))
    torch.cuda.synchronize(gpu)
    return dst.cpu().numpy(), nb


def _ints(shape, seed):
    return np.random.default_rng(seed).integers(-8, 9, shape).astype(np.float32)


def _image_equal(name, got_bytes, want):
    """`want` (numpy, the destination's element type) against the head of the buffer, bit for bit; pad elements are +0.0"""
    raw = np.ascontiguousarray(want).view(np.uint8).ravel()
    assert len(got_bytes) >= len(raw) and len(got_bytes) - len(raw) < 256, (name, len(got_bytes), len(raw))
    diff = int((got_bytes[:len(raw)] != raw).sum())
    record_err("lattice layout " + name, float(diff), 0.0)


@pytest.mark.parametrize("feat", ["f32", "f16"])
@pytest.mark.parametrize("offset", [0, 1])
def test_planar_to_channels_last_image(feat, offset, gpu):
    """k_to_channels_last: (B,V,C,H,W) -> (B,V,H,W,C4) in the features' type, channels C ... C4 are +0.0; the vector instance (aligned, HW % 4
    == 0) and the scalar one"""
    np_t = np.float32 if feat == "f32" else np.float16
    for C in (3, 4, 65, 130):
        for H, W in ((7, 9), (8, 8), (20, 13)):                      # HW = 63, 64, 65 * 4
            src = _ints((1, 2, C, H, W), C * 1000 + H)
            got, _ = _convert(src, src.shape, feat, _capi.LAYOUT_BVCHW, _capi.LAYOUT_BVHWC, gpu, offset)
            C4 = (C + 3) // 4 * 4
            want = np.zeros((1, 2, H, W, C4), np_t)
            want[..., :C] = src.transpose(0, 1, 3, 4, 2)
            _image_equal("planar->BVHWC %s C%d %dx%d offset %d" % (feat, C, H, W, offset), got, want)


def _quad_image(src, scale=None):
    """(B,V,C,H,W) -> (B,V,C4/4,W,H,4) fp32, pad channels +0.0; scale: one fp32 multiply per element"""
    B, V, C, H, W = src.shape
    C4 = (C + 3) // 4 * 4
    padded = np.zeros((B, V, C4, H, W), np.float32)
    padded[:, :, :C] = src.astype(np.float32)
    if scale is not None:
        padded = padded * np.float32(scale)
    return np.ascontiguousarray(padded.reshape(B, V, C4 // 4, 4, H, W).transpose(0, 1, 2, 5, 4, 3))


@pytest.mark.parametrize("feat", ["f32", "f16"])
@pytest.mark.parametrize("W", [5, 127, 128, 129])
def test_planar_to_quad_image(feat, W, gpu):
    """k_to_quad_planar_t_band (W <= 127) and k_to_quad_planar_t (from 128): (B,V,C,H,W) -> (B,V,C4/4,W,H,4) fp32; W % 4 != 0 and
    (H * W) % 4 != 0 among the shapes, an aligned and a misaligned base pointer; MVHMR_LAYOUT_QUAD_LOG2E is one fp32 multiply per element"""
    for H in (31, 32, 33, 70):
        for C in (4, 6):
            src = _ints((1, 2, C, H, W), W * 100 + H + C)
            for offset in (0, 1):
                got, _ = _convert(src, src.shape, feat, _capi.LAYOUT_BVCHW, _capi.LAYOUT_QUAD, gpu, offset)
                _image_equal("planar->QUAD %s C%d %dx%d offset %d" % (feat, C, H, W, offset), got, _quad_image(src))
            got, _ = _convert(src, src.shape, feat, _capi.LAYOUT_BVCHW, _capi.LAYOUT_QUAD_LOG2E, gpu, 0)
            _image_equal("planar->QUAD_LOG2E %s C%d %dx%d" % (feat, C, H, W), got, _quad_image(src, K_LOG2E))


@pytest.mark.parametrize("feat", ["f32", "f16"])
def test_channels_last_to_quad_image(feat, gpu):
    """k_channels_last_to_quad_t: (B,V,H,W,C) -> (B,V,C/4,W,H,4) fp32; C = 260 is 65 quads, so the 64-quad loop runs twice with a ragged
    second pass; H = 15, 16, 17 around its 16-row blocks"""
    for C in (4, 256, 260):
        for H in (15, 16, 17):
            src = _ints((1, 2, C, H, 5), C + H)
            got, _ = _convert(src.transpose(0, 1, 3, 4, 2), src.shape, feat, _capi.LAYOUT_BVHWC, _capi.LAYOUT_QUAD, gpu, 0)
            _image_equal("BVHWC->QUAD %s C%d H%d" % (feat, C, H), got, _quad_image(src))


# ----------------------------------------------------------------------------------------------- the geometry path
# grad_proj, grad_coords and the cuboid's grad_rot / grad_center against lattice_rig.geo_oracle on the geometry rigs (power-of-two maps: kx
# and ky are dyadic, every step of k_bwd_geom's chain is exact; tests/test_lattice_cpu.py checks that premise).  grad_proj[b, v] sums every
# voxel of a sample, so ONE voxel handled wrongly -- the tail of the last tile, a tap in a border band, a tap whose value must be zero at a
# valid clamped address -- moves it by a whole quantum of the rig although it stays far below 1e-4 of the sum.
def _geo_hold(tag, grads, res, extras):
    for key, got in grads.items():
        if got is not None:
            _hold("geometry %s %s" % (tag, key), got, res[key])


def _geo_call(name, method, gpu, feat="f32", out=None, variant="gather", proj_grad=True, coords_grad=True, det=False, channels_last=False, grad=None, **options):
    """one call of the tensor route on a geometry rig -> dict(grad_proj, grad_coords) (None where no gradient was asked for)"""
    feats, proj, coords, _, _ = rig.geo_problem(name)
    grad = rig.geo_reference(name, method)[0] if grad is None else grad
    f = _features(feats, dict(feat=feat, cl=channels_last), gpu).detach()
    p = torch.from_numpy(proj).to(gpu).requires_grad_(proj_grad)
    c = torch.from_numpy(coords).to(gpu).requires_grad_(coords_grad)
    res = aggregation.unprojection(f, p, c, aggregation_method=method, variant=variant, out_dtype=DT[out or feat], **options)
    with _Deterministic(det):
        res.backward(torch.from_numpy(grad).to(gpu).to(res.dtype))
    return dict(grad_proj=p.grad, grad_coords=c.grad)


GEO_TENSOR_RIGS = ["geo_v1", "geo_v3", "geo_v4", "geo_v5", "geo_v8", "geo_v9", "geo_v16", "geo_c260", "geo_h16", "geo_coords_big", "geo_many_tiles"]


@pytest.mark.parametrize("name", GEO_TENSOR_RIGS)
def test_geometry_gradients_have_the_oracles_bits(name, gpu):
    """k_bwd_geom + k_geom_reduce on every rig, `sum`, `max` and power-of-two `mean`: 1, 3, 4, 5, 8, 9 and 16 views (each CPL, kMaxViews),
    a ragged last tile, C % 4 != 0, a second 256-channel group, non-square maps, a volume whose grad_coords alone is asked for (part ==
    nullptr) and one of 272 tiles per sample with a sparse grad_out (k_geom_reduce's stride takes a second trip)"""
    extras = rig.geo_problem(name)[4]
    V = rig.GEO_RIGS[name]["V"]
    for method in ("sum", "max") + (("mean",) if V & (V - 1) == 0 else ()):
        _, res, _ = rig.geo_reference(name, method)
        got = _geo_call(name, method, gpu, proj_grad="proj" in extras["want"])
        assert (got["grad_proj"] is None) == ("proj" not in extras["want"])
        _geo_hold("%s %s" % (name, method), got, res, extras)


@pytest.mark.parametrize("proj_grad,coords_grad", [(True, False), (False, True), (True, True)])
def test_geometry_gradients_whichever_tensor_asks(proj_grad, coords_grad, gpu):
    """the three requires_grad combinations of (proj_matricies, coord_volumes): a null `part` resp. `grad_coords` in the launch"""
    for method in ("sum", "max"):
        _, res, _ = rig.geo_reference("geo_v3", method)
        got = _geo_call("geo_v3", method, gpu, proj_grad=proj_grad, coords_grad=coords_grad)
        assert (got["grad_proj"] is not None) == proj_grad and (got["grad_coords"] is not None) == coords_grad
        _geo_hold("geo_v3 %s proj=%d coords=%d" % (method, proj_grad, coords_grad), got, res, None)


@pytest.mark.parametrize("variant,det", [("gather", False), ("gather", True), ("auto", False), ("brick", False)])
def test_geometry_gradients_do_not_depend_on_mode_or_forward_route(variant, det, gpu):
    """geo_v4 in default and deterministic mode, and behind the AUTO and the brick forward: the geometry backward is the same kernel"""
    for method in ("sum", "max", "mean"):
        _, res, _ = rig.geo_reference("geo_v4", method)
        _geo_hold("geo_v4 %s %s%s" % (method, variant, " deterministic" if det else ""), _geo_call("geo_v4", method, gpu, variant=variant, det=det), res, None)


@pytest.mark.parametrize("name", ["geo_v3", "geo_v5", "geo_v9"])
@pytest.mark.parametrize("feat,out", [("f32", "f32"), ("f32", "bf16"), ("f16", "f16"), ("f16", "f32")])
def test_geometry_gradients_in_every_storage_combination(name, feat, out, gpu):
    """the four (feature, volume) type pairs geom_dispatch instantiates, on one rig per Row<T, CPL> specialisation (CPL = 4, 2, 1): the
    rig's whole-number features and grad_out are exact in fp16 / bf16, so the fp32 gradients keep the oracle's bits"""
    for method in ("sum", "max"):
        _, res, _ = rig.geo_reference(name, method)
        _geo_hold("%s %s %s->%s" % (name, method, feat, out), _geo_call(name, method, gpu, feat=feat, out=out), res, None)


@pytest.mark.parametrize("feat", ["f32", "f16"])
def test_geometry_gradients_from_channels_last_features(feat, gpu):
    for method in ("sum", "mean"):
        _, res, _ = rig.geo_reference("geo_v4", method)
        _geo_hold("geo_v4 %s %s channels-last" % (method, feat), _geo_call("geo_v4", method, gpu, feat=feat, channels_last=True), res, None)


def test_cuboid_route_pose_gradients_have_the_oracles_bits(gpu):
    """The POSE instances: grad_rot, grad_center and grad_proj of unprojection_cuboid with sides = extent - 1 (step 1), whole-number
    centres, sample 0 unrotated (its grad_center must be exactly 0: dX/dc = I - R) and the others a quarter turn of the lattice about its
    centre, so every voxel centre R d + c is a whole number again"""
    feats, proj, coords, _, ex = rig.geo_problem("geo_pose")
    for method in ("sum", "max"):
        grad, res, _ = rig.geo_reference("geo_pose", method)
        f = torch.from_numpy(feats).to(gpu)
        p = torch.from_numpy(proj).to(gpu).requires_grad_(True)
        r = torch.from_numpy(ex["rotations"]).to(gpu).requires_grad_(True)
        c = torch.from_numpy(ex["centers"]).to(gpu).requires_grad_(True)
        out = aggregation.unprojection_cuboid(f, p, r, c, ex["position"], ex["sides"], coords.shape[1:4], method, variant="gather")
        out.backward(torch.from_numpy(grad).to(gpu))
        _geo_hold("geo_pose %s" % method, dict(grad_proj=p.grad, grad_rot=r.grad, grad_center=c.grad), res, None)
        assert not c.grad[0].any() and c.grad[1:].any()


@pytest.mark.parametrize("tag", [t[0] for t in rig.geo_option_cases()])
def test_option_route_geometry_gradients(tag, gpu):
    """The geometry backward of every option family on its own rig: view_mask (the MASK instances: a full, a single-view and an empty sample),
    view_weights (with grad_weights, which the same kernel produces), visible_only (alone and with a mask), feature_index (a repeated, a skipped and an out-of-range entry: grad_proj sums over
    the volumes naming a sample, an unnamed sample gets exact zeros) and view_confidence (the gradient also flows through the sampled
    confidence).  All share k_bwd_geom's arithmetic chain: bit equality."""
    _, name, method, kw = next(t for t in rig.geo_option_cases() if t[0] == tag)
    res = rig.geo_option_reference(tag)
    args = {k: (torch.from_numpy(v).to(gpu) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    if "view_weights" in kw:
        args["view_weights"].requires_grad_(True)
    got = _geo_call(name, method, gpu, grad=res["grad_out"], **args)
    if "view_weights" in kw:
        got["grad_weights"] = args["view_weights"].grad
    _geo_hold("option %s" % tag, got, res, None)
    if "feature_index" in kw:
        assert not got["grad_proj"][2].any() and not got["grad_coords"][3].any()      # sample 2 is never named; volume 3 names sample 7


def test_zero_lens_geometry_gradients_carry_the_plain_bits(gpu):
    """lens= with all five coefficients zero (arbitrary intrinsics, a large r2max): k_bwd_geom_lens must give the plain call's bits"""
    B, V = rig.GEO_RIGS["geo_v3"]["B"], rig.GEO_RIGS["geo_v3"]["V"]
    lens = np.zeros((B, V, 10), np.float32)
    lens[..., :4] = np.random.default_rng(3).uniform(-50, 50, (B, V, 4))
    lens[..., 9] = 1e30
    for method in ("sum", "max"):
        _, res, _ = rig.geo_reference("geo_v3", method)
        _geo_hold("geo_v3 %s zero lens" % method, _geo_call("geo_v3", method, gpu, lens=torch.from_numpy(lens).to(gpu)), res, None)


def _kept_boundary_problem():
    """V = 1, a 5 x 9 map (W - 1 = 8 and H - 1 = 4 are powers of two), a (4, 4, 3) volume at (i, j, k), depth 2.  Sample 0: ix = i - 1
    (voxels with i = 0 land on ix == -1 exactly), iy = j / 2 + 1 / 4 inside; sample 1: iy = j - 1 (j = 0 lands on iy == -1), ix = i + 1 / 2.
    Every fp32 step of the POSITION is exact (u = H (i - 1) / 8 with H / 8 = 0.625, and 0.625 m / 5 = m / 8 is a representable
    quotient; likewise w = W (2 j + 1) / 16 with W / 16 = 0.5625), so kernel and oracle agree on ix, iy and the fractions bit for bit;
    the features and grad_out are random reals, and kx = 8 / 5, ky = 4 / 9 round: the gradient itself is not exact."""
    H, W, vol = 5, 9, (4, 4, 3)
    rng = np.random.default_rng(91)
    feats = rng.standard_normal((2, 1, 6, H, W)).astype(np.float32)
    feats[:, :, :, 0, :] += np.sign(feats[:, :, :, 0, :])             # row 0 and column 0 well away from zero
    feats[:, :, :, :, 0] += np.sign(feats[:, :, :, :, 0])
    grad = rng.standard_normal((2, 6) + vol).astype(np.float32)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in vol], indexing="ij"), -1).astype(np.float32)
    coords = np.broadcast_to(grid, (2,) + grid.shape).copy()
    d = 2.0
    proj = np.zeros((2, 1, 3, 4), np.float32)
    proj[0, 0, 0] = (d * H / 8, 0, 0, -d * H / 8)                     # u = H (i - 1) / 8      -> ix = i - 1
    proj[0, 0, 1] = (0, d * W / 8, 0, d * W / 16)                     # w = W (2 j + 1) / 16   -> iy = j / 2 + 1 / 4
    proj[1, 0, 0] = (d * H / 8, 0, 0, d * H / 16)                     # u = H (2 i + 1) / 16   -> ix = i + 1 / 2
    proj[1, 0, 1] = (0, d * W / 4, 0, -d * W / 4)                     # w = W (j - 1) / 4      -> iy = j - 1
    proj[:, 0, 2, 3] = d
    return feats, proj, coords, grad, H, W


def test_the_kept_boundary_has_its_gradient(gpu):
    """make_geo_rec keeps ix == -1 and iy == -1 ("the tap at x = 0 has weight 0 but a gradient"): there the sample is 0 but ds/dix is the
    interpolated value of column 0.  No lattice point can lie there (the lattice has ix = (c + t) (W - 1) / (q d); -q d / (W - 1) is no
    half-integer), so this problem is built by hand (_kept_boundary_problem) and grad_coords is compared PER VOXEL, each against a bound of
    its own derived from the code, with every term taken from the float64 oracle:

        |got - ref| <= ((1 + u)^R - 1) * T,   u = 2^-24,   T = sum_r |P[r][k]| * (the chain evaluated with every tap value, every ds and
                                                              u, w replaced by their magnitudes: the sum |terms| of that element)

    R = 24 counts the fp32 roundings on the longest path from a feature value to grad_coords in k_bwd_geom:  3 in ds/dix (the difference of
    two taps, ty * difference, the fmaf with wy0 * difference);  11 in the channel sum (CPL = 4 fmaf per lane, the 6 additions of
    wave_sum's tree, one into acc);  3 for du (the division that makes kx, G * kx, / z);  4 more for dh[2] (u = a / z, dw * w, the fmaf,
    / z);  3 fmaf of P^T dh.  The positions, fractions and weights are exact by construction (asserted below against fp32)."""
    feats, proj, coords, grad, H, W = _kept_boundary_problem()
    B, V, C = feats.shape[:3]
    N = int(np.prod(coords.shape[1:4]))
    ref = rig.geo_oracle(feats, proj, coords, grad, "sum")["grad_coords"].reshape(B, N, 3)
    bound = np.zeros((B, N, 3))
    edge = np.zeros((B, N), bool)
    kx, ky = (W - 1) / H, (H - 1) / W
    for b in range(B):
        pts = coords[b].reshape(N, 3)
        t = rig.geotaps64(proj[b, 0], pts, feats[b, 0].reshape(C, H * W), H, W)
        for key in ("ix", "iy", "u", "w"):
            assert np.array_equal(t[key].astype(np.float32).astype(np.float64), t[key]), "the position is not exact in fp32: test error"
        assert t["valid"].all()
        edge[b] = (t["ix"] == -1) if b == 0 else (t["iy"] == -1)
        assert edge[b].sum() == 12 and ((t["iy"] > 0) & (t["iy"] < H - 1) if b == 0 else (t["ix"] > 0) & (t["ix"] < W - 1))[edge[b]].all()
        g = np.abs(grad[b].reshape(C, N).astype(np.float64))
        du, dw = (g * t["adx"]).sum(0) * kx, (g * t["ady"]).sum(0) * ky
        dh = np.stack([du / t["z"], dw / t["z"], (du * np.abs(t["u"]) + dw * np.abs(t["w"])) / t["z"]], 1)          # (N, 3) magnitudes
        bound[b] = ((1 + 2.0 ** -24) ** 24 - 1) * (dh @ np.abs(proj[b, 0, :, :3].astype(np.float64)))
    for b in range(B):                               # non-zero, and by far more than the bound: a kernel that drops the boundary cannot pass
        assert (np.abs(ref[b][edge[b]][:, b]) > 1e3 * bound[b][edge[b]][:, b]).all(), "the oracle's boundary gradient must not be zero"
    f = torch.from_numpy(feats).to(gpu)
    c = torch.from_numpy(coords).to(gpu).requires_grad_(True)
    out = aggregation.unprojection(f, torch.from_numpy(proj).to(gpu), c, aggregation_method="sum", variant="gather")
    assert not out.detach().reshape(B, C, N).permute(0, 2, 1)[torch.from_numpy(edge).to(gpu)].any()                # the SAMPLE there is zero
    out.backward(torch.from_numpy(grad).to(gpu))
    err = np.abs(c.grad.cpu().numpy().astype(np.float64).reshape(B, N, 3) - ref)
    worst = int(np.argmax(err - bound))
    print("kept boundary: max err %.3e (on the boundary %.3e), its bound %.3e, largest |ref| %.3e" % (err.max(), err[edge].max(), bound.ravel()[np.argmax(err)], np.abs(ref).max()))
    record_err("lattice kept boundary grad_coords per voxel (derived bound)", float(err.ravel()[worst]), float(bound.ravel()[worst]))
    assert (err <= bound).all()
