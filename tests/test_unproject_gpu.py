"""Parity tests proper: the HIP path (through the C ABI) against the reference's golden vectors and the
CPU oracle on the same seeded inputs.  Tolerance for fp32: 1e-4 max-abs (BASELINE.json north_star).  The kernels
mirror the reference's rounding order, so the observed error is ~1e-6; every comparison goes through
conftest.record_err, which asserts the bound and writes the observed value to gpurun_out/parity_observed.json.
Bounds: TOL = 1e-4 absolute wherever the reference values are O(1..16); for the one golden whose values are O(1e2)
(saturated softmax) and for gradients that sum thousands of taps, 2e-6 relative to the largest reference value
(a few fp32 ulps) -- `_bound` spells that out, nothing else is loosened."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden_cases, load_golden, record_err
from multiviewhmr_amd import _capi, aggregation, multiview
from oracle import cport

pytestmark = pytest.mark.gpu
MODES = ("softmax", "sum", "mean", "max")
TOL = 1e-4                      # fp32 bar from BASELINE.json
VARIANTS = ("gather", "auto", "brick")


def _dev(d, key, gpu, dtype=torch.float32):
    return torch.from_numpy(d[key]).to(device=gpu, dtype=dtype)


def _brick_ok(f, c):
    """shapes the brick forward takes (r04): 2 ... 8 views (3 / 5 / 6 / 7 run the next larger kernel with the missing views absent),
    C >= 4 (r05: C % 4 != 0 -- the last, partial quad per voxel behind the brick kernel), ANY volume (bricks that stick out idle their
    outside lanes); 16-bit volumes store z pairs and need an even Z"""
    Z = c.shape[3]
    V = f.shape[1]
    return 1 <= V <= 8 and f.shape[2] >= 4 and (f.dtype == torch.float32 or Z % 2 == 0)


def _bound(ref):
    """1e-4 absolute for O(1..16) references; a few fp32 ulps of the largest value beyond that."""
    m = float(np.abs(ref).max())
    return TOL if m <= 16.0 else max(TOL, 8e-6 * m)


def _err(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())


# ------------------------------------------------------------------------------------ goldens, forward + backward
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", golden_cases("unproj"))
def test_forward_matches_reference_goldens(case, variant, gpu):
    d = load_golden("unproj", case)
    f, p, c = _dev(d, "features", gpu), _dev(d, "proj", gpu), _dev(d, "coords", gpu)
    if variant == "brick" and not _brick_ok(f, c):
        with pytest.raises(RuntimeError, match="brick variant does not support"):
            aggregation.unprojection(f, p, c, variant="brick")
        return
    for mode in MODES:
        if "out_" + mode not in d:
            continue
        out = aggregation.unprojection(f, p, c, aggregation_method=mode, variant=variant)
        ref = d["out_" + mode]
        assert out.dtype == torch.float32 and tuple(out.shape) == ref.shape and out.device == f.device
        record_err("golden fwd %s %s %s" % (case, mode, variant), _err(out.cpu().numpy(), ref), _bound(ref))


@pytest.mark.parametrize("case", golden_cases("unproj"))
def test_backward_matches_reference_goldens(case, gpu):
    d = load_golden("unproj", case)
    p, c, go = _dev(d, "proj", gpu), _dev(d, "coords", gpu), _dev(d, "grad_out", gpu)
    for mode in MODES:
        if "gfeat_" + mode not in d:
            continue
        f = _dev(d, "features", gpu).requires_grad_(True)
        out = aggregation.unprojection(f, p, c, aggregation_method=mode)
        out.backward(go)
        ref = d["gfeat_" + mode]
        record_err("golden bwd %s %s" % (case, mode), _err(f.grad.cpu().numpy(), ref), _bound(ref))   # float atomics: order-dependent low bits only


def test_inputs_are_not_mutated_and_output_is_fresh(gpu):
    d = load_golden("unproj", "adversarial_v4c6")
    f, p, c = _dev(d, "features", gpu), _dev(d, "proj", gpu), _dev(d, "coords", gpu)
    f0, p0, c0 = f.clone(), p.clone(), c.clone()
    a = aggregation.unprojection(f, p, c)
    b = aggregation.unprojection(f, p, c)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)             # forward is deterministic
    assert torch.equal(f, f0) and torch.equal(p, p0) and torch.equal(c, c0)


# ------------------------------------------------------------------------------------ seeded inputs vs the oracle
def _ring_problem(B, V, C, H, W, vol, seed, theta=0.3):
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((B, V, C, H, W), dtype=np.float32)
    proj = np.empty((B, V, 3, 4), np.float32)
    for b in range(B):
        for v in range(V):
            az = 2 * np.pi * v / V + 0.3 + 0.1 * b
            eye = np.array([5000 * np.cos(az), 5000 * np.sin(az), 1500.0])
            fwd = -eye / np.linalg.norm(eye)
            right = np.cross(fwd, [0, 0, 1.0]); right /= np.linalg.norm(right)
            R = np.stack([right, np.cross(fwd, right), fwd])
            cam = multiview.Camera(R, -R @ eye, [[1145.0, 0, 512], [0, 1145.0, 512], [0, 0, 1]])
            cam.update_after_crop((150, 150, 850, 850))
            cam.update_after_resize((700, 700), (4 * W, 4 * H))
            cam.update_after_resize((4 * H, 4 * W), (H, W))
            proj[b, v] = cam.projection
    X, Y, Z = vol
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).astype(np.float64)
    pts = -1250.0 + g * (2500.0 / (np.array([X, Y, Z]) - 1))
    ct, st = np.cos(theta), np.sin(theta)
    pts = pts @ np.array([[ct, -st, 0], [st, ct, 0], [0, 0, 1.0]]).T
    coords = np.broadcast_to(pts.astype(np.float32), (B,) + pts.shape).copy()
    return feats, proj, coords


@pytest.mark.parametrize("shape", [
    dict(B=2, V=4, C=64, H=48, W=48, vol=(16, 16, 32)),       # V=4 compiled path, several channel quads
    dict(B=1, V=3, C=20, H=24, W=40, vol=(9, 7, 13)),         # run-time V path, N % 64 != 0, non-square map
    dict(B=1, V=5, C=6, H=16, W=16, vol=(5, 5, 5)),           # C % 4 != 0, run-time V
    dict(B=1, V=8, C=300, H=24, W=24, vol=(4, 8, 16)),        # two channel groups (C > 256), V=8 compiled path
    dict(B=3, V=2, C=16, H=32, W=32, vol=(8, 8, 8)),          # V=2 compiled path
    dict(B=1, V=12, C=8, H=16, W=16, vol=(4, 4, 8)),          # many views (run-time path, > 8)
])
@pytest.mark.parametrize("mode", MODES)
def test_forward_and_backward_vs_oracle(shape, mode, gpu):
    feats, proj, coords = _ring_problem(seed=MODES.index(mode) * 100 + shape["C"], **shape)
    f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    out = aggregation.unprojection(f, p, c, aggregation_method=mode)
    ref = cport.forward(feats, proj, coords, mode)
    name = "oracle %s V%d C%d %dx%d vol%s" % (mode, shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"])
    record_err(name + " fwd", _err(out.detach().cpu().numpy(), ref), TOL)
    go = np.random.default_rng(5).standard_normal(ref.shape, dtype=np.float32)
    out.backward(torch.from_numpy(go).to(gpu))
    gref = cport.backward(go, feats, proj, coords, mode)
    record_err(name + " bwd", _err(f.grad.cpu().numpy(), gref), _bound(gref))


@pytest.mark.parametrize("shape", [
    dict(B=2, V=4, C=32, H=48, W=48, vol=(8, 16, 32)),        # windows of ~4 000 slots: the 2-deep ring
    dict(B=1, V=4, C=32, H=40, W=40, vol=(16, 16, 32)),       # windows of ~2 100 slots: the 3-deep ring, 8 bricks per sample
    dict(B=1, V=2, C=8, H=24, W=24, vol=(4, 8, 64)),          # two z bricks per column
    dict(B=1, V=2, C=12, H=32, W=32, vol=(4, 8, 32)),         # odd number of quads
    dict(B=1, V=4, C=8, H=320, W=320, vol=(4, 8, 32)),        # huge maps: the brick's taps overflow the LDS window -> global fallback
    dict(B=1, V=4, C=16, H=12, W=12, vol=(8, 8, 32)),         # tiny maps: most taps fall outside the image (zero padding)
    dict(B=2, V=8, C=16, H=24, W=24, vol=(8, 8, 32)),         # 8 views, y % 8 == 0: 1024 threads, 4 x 8 x 32 bricks, two view groups
    dict(B=1, V=8, C=8, H=16, W=16, vol=(4, 4, 64)),          # 8 views, y % 8 != 0: 512-thread bricks (4 x 4 x 32), two z bricks
    dict(B=2, V=8, C=16, H=32, W=32, vol=(16, 16, 32)),       # 8 views, 16 bricks per sample
    dict(B=2, V=8, C=16, H=48, W=48, vol=(8, 8, 32)),         # 8 views, group windows of ~4 000 slots: still the 2-deep ring
    dict(B=1, V=8, C=8, H=200, W=200, vol=(4, 8, 32)),        # 8 views, huge maps: the group windows overflow -> out-of-line global path
    dict(B=2, V=3, C=16, H=24, W=24, vol=(8, 8, 32)),         # 3 views on the 4-view kernel: the fourth view absent
    dict(B=2, V=1, C=8, H=24, W=24, vol=(8, 8, 32)),          # a single view on the 2-view kernel
    dict(B=1, V=4, C=64, H=48, W=48, vol=(32, 32, 32)),       # 16 bricks, 16 quads: the channel quads divided among 2 blocks per brick
    dict(B=1, V=4, C=128, H=24, W=24, vol=(16, 16, 32)),      # 4 bricks, 32 quads: 4 blocks per brick
    dict(B=1, V=8, C=64, H=32, W=32, vol=(16, 16, 32)),       # 8 views (view groups), 16 bricks, 2 blocks per brick
    dict(B=1, V=3, C=64, H=32, W=32, vol=(9, 16, 40)),        # split + absent view + ragged volume
    dict(B=1, V=5, C=8, H=24, W=24, vol=(8, 8, 32)),          # 5 views on the 8-view kernel (second group: one real view)
    dict(B=2, V=6, C=16, H=32, W=32, vol=(9, 7, 40)),         # 6 views, ragged volume
    dict(B=1, V=7, C=8, H=24, W=24, vol=(4, 8, 32)),          # 7 views
    dict(B=1, V=3, C=8, H=320, W=320, vol=(4, 8, 32)),        # 3 views, windows overflow: out-of-line path with an absent view
    dict(B=1, V=6, C=8, H=200, W=200, vol=(4, 8, 32)),        # 6 views, group windows overflow
    dict(B=1, V=8, C=8, H=200, W=200, vol=(4, 4, 32)),        # ... and the same for the 512-thread form
])
@pytest.mark.parametrize("mode", MODES)
def test_brick_variant_vs_oracle(shape, mode, gpu):
    feats, proj, coords = _ring_problem(seed=7 + MODES.index(mode), **shape)
    f, p, c = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    assert _brick_ok(f, c)
    out = aggregation.unprojection(f, p, c, aggregation_method=mode, variant="brick")
    ref = cport.forward(feats, proj, coords, mode)
    record_err("brick fwd %s V%d C%d %dx%d vol%s" % (mode, shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"]),
               _err(out.cpu().numpy(), ref), TOL)
    assert torch.equal(out, aggregation.unprojection(f, p, c, aggregation_method=mode, variant="brick"))   # deterministic
    gat = aggregation.unprojection(f, p, c, aggregation_method=mode, variant="gather")
    record_err("brick vs gather fwd %s V%d C%d %dx%d vol%s" % (mode, shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"]),
               float((out - gat).abs().max()), 4e-6)         # same samples; the softmax in two algebraically equal forms


@pytest.mark.parametrize("views", (2, 4, 8))
def test_brick_softmax_over_the_whole_float_range(views, gpu):
    """The brick forward takes its softmax exponentials relative to view 0 (one v_exp_f32 and the max fewer per channel) and
    falls back to the max form, per wave, when that overflows (s_v - s_0 > 88.7) or meets a non-finite sample
    (brick_fwd_kernel.h, fwd_aggregate2).  Samples spread over +-300, +-3e4 and +-1e30 take both branches; the answer stays the
    oracle's -- relative bound, the values are large -- and never turns non-finite where the reference is finite."""
    feats, proj, coords = _ring_problem(B=1, V=views, C=8, H=24, W=24, vol=(8, 8, 32), seed=77)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    for scale in (100.0, 1e4, 1e30):
        f = np.ascontiguousarray(feats * np.float32(scale))
        f[0, :, 1] = feats[0, :, 1]                                               # one channel of each quad stays O(1): mixed waves
        f[0, 0, 2] -= np.float32(0.9 * scale)                                     # view 0 far below the others: e_v overflows
        f[0, 0, 3] += np.float32(0.9 * scale)                                     # view 0 far above: every e_v underflows to 0
        with np.errstate(all="ignore"):
            ref = cport.forward(f, proj, coords, "softmax")
        assert np.isfinite(ref).all()
        out = aggregation.unprojection(torch.from_numpy(f).to(gpu), p, c, aggregation_method="softmax", variant="brick").cpu().numpy()
        assert np.isfinite(out).all()
        big = [0, 2, 3, 4, 5, 6, 7]                                               # the O(1) channel keeps the absolute bar
        record_err("brick softmax range V%d x%g, O(1) channel" % (views, scale), _err(out[0, 1], ref[0, 1]), TOL)
        record_err("brick softmax range V%d x%g, relative to max |ref|" % (views, scale),
                   _err(out[0, big], ref[0, big]) / float(np.abs(ref[0, big]).max()), 8e-6)
    fn = feats.copy()
    fn[0, 0, 5, 10:14, 10:14] = np.nan                                            # NaN samples in view 0, Inf in view 1
    fn[0, 1, 6, 8:12, 8:12] = np.inf
    with np.errstate(all="ignore"):
        ref = cport.forward(fn, proj, coords, "softmax")
    out = aggregation.unprojection(torch.from_numpy(fn).to(gpu), p, c, aggregation_method="softmax", variant="brick").cpu().numpy()
    gat = aggregation.unprojection(torch.from_numpy(fn).to(gpu), p, c, aggregation_method="softmax", variant="gather").cpu().numpy()
    assert np.array_equal(np.isfinite(out), np.isfinite(gat)) and (~np.isfinite(out)).any()      # the max form's pixels exactly
    fin = np.isfinite(ref) & np.isfinite(out)
    assert fin[0, [0, 1, 2, 3, 4, 7]].all()
    record_err("brick softmax non-finite samples V%d, finite part" % views, _err(out[fin], ref[fin]), TOL)


@pytest.mark.parametrize("shape", [
    dict(B=2, V=4, C=8, H=24, W=24, vol=(8, 8, 32)),          # windows fit (1 800 of 3 200 slots): fixed-point LDS accumulation + flush
    dict(B=1, V=4, C=16, H=40, W=40, vol=(16, 16, 32)),       # windows fit, 8 bricks per sample
    dict(B=2, V=4, C=8, H=48, W=48, vol=(8, 8, 32)),          # 6 100 slots: out-of-line global-atomic path
    dict(B=1, V=2, C=12, H=32, W=32, vol=(4, 8, 64)),         # odd number of quads, two z bricks per column (fits)
    dict(B=1, V=4, C=8, H=320, W=320, vol=(4, 8, 32)),        # windows overflow the LDS pool: out-of-line global-atomic path
    dict(B=1, V=4, C=16, H=12, W=12, vol=(8, 8, 32)),         # tiny maps: most taps outside the image, lanes masked out of the adds
    dict(B=2, V=8, C=16, H=24, W=24, vol=(8, 8, 32)),         # 8 views: 512-thread bricks, one feature window in LDS (fits: 2 500 of 4 900)
    dict(B=1, V=8, C=8, H=16, W=16, vol=(4, 4, 64)),          # 8 views, two z bricks (fits)
    dict(B=2, V=8, C=16, H=48, W=48, vol=(8, 8, 32)),         # 8 views, overflow: out-of-line path
    dict(B=1, V=4, C=8, H=24, W=40, vol=(8, 8, 32)),          # non-square maps (column-major windows), W not a multiple of the 32-column gradient band
    dict(B=1, V=2, C=8, H=136, W=20, vol=(8, 8, 32)),         # tall maps: the gradient layout pass falls back to 8-column bands
    dict(B=2, V=4, C=8, H=24, W=24, vol=(9, 7, 13)),          # extents that do not divide into bricks: 8 x 8 x 16 bricks, outside lanes idle
    dict(B=1, V=4, C=8, H=32, W=32, vol=(12, 20, 40)),        # ragged in all three axes, several bricks per axis
    dict(B=1, V=8, C=8, H=24, W=24, vol=(6, 10, 33)),         # 8 views, ragged (8 x 4 x 16 bricks)
    dict(B=1, V=2, C=8, H=24, W=24, vol=(4, 8, 33)),          # ragged in z only: the 4 x 8 x 32 bricks cover it with fewer idle lanes
    dict(B=2, V=3, C=16, H=24, W=24, vol=(8, 8, 32)),         # 3 views on the 4-view kernel: the fourth view absent (ds forced to zero)
    dict(B=2, V=1, C=8, H=24, W=24, vol=(8, 8, 32)),          # a single view on the 2-view kernel
    dict(B=1, V=5, C=8, H=24, W=24, vol=(8, 8, 32)),          # 5 views on the 8-view kernel
    dict(B=2, V=6, C=16, H=32, W=32, vol=(9, 7, 40)),         # 6 views, ragged volume
    dict(B=1, V=7, C=8, H=24, W=24, vol=(4, 8, 32)),          # 7 views
    dict(B=1, V=3, C=8, H=320, W=320, vol=(4, 8, 32)),        # 3 views, windows overflow: out-of-line path with an absent view
    dict(B=1, V=6, C=8, H=48, W=48, vol=(8, 8, 32)),          # 6 views, overflow
])
@pytest.mark.parametrize("mode", MODES)
def test_brick_backward_vs_oracle(shape, mode, gpu):
    """the brick backward (window gradients accumulated in LDS in fixed point), the default where the brick forward runs"""
    feats, proj, coords = _ring_problem(seed=31, **shape)
    f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    out = aggregation.unprojection(f, p, c, aggregation_method=mode, variant="brick")
    go = np.random.default_rng(6).standard_normal(tuple(out.shape), dtype=np.float32)
    out.backward(torch.from_numpy(go).to(gpu))
    gref = cport.backward(go, feats, proj, coords, mode)
    record_err("brick bwd %s V%d C%d %dx%d vol%s" % (mode, shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"]),
               _err(f.grad.cpu().numpy(), gref), _bound(gref))


@pytest.mark.parametrize("shape", [
    dict(B=2, V=4, C=6, H=24, W=24, vol=(8, 8, 32)),          # k_fwd_brick / k_bwd_brick: one whole quad + 2 channels
    dict(B=1, V=4, C=13, H=32, W=40, vol=(12, 20, 40)),       # ragged volume, non-square maps, 3 whole quads + 1 channel
    dict(B=1, V=8, C=7, H=24, W=24, vol=(6, 10, 33)),         # 8 views (view groups / 8 x 4 x 16 bricks), 1 quad + 3 channels
    dict(B=2, V=3, C=10, H=24, W=24, vol=(8, 8, 32)),         # an absent view in the partial quad as well
    dict(B=1, V=4, C=70, H=48, W=48, vol=(32, 32, 32)),       # 17 whole quads: the channel split of small launches leaves the partial quad to the tail
    dict(B=9, V=4, C=6, H=40, W=56, vol=(20, 36, 44)),        # >= 256 bricks: k_fwd_ws (prescaled copy for the softmax: the tail undoes the scale too)
    dict(B=1, V=4, C=6, H=320, W=320, vol=(8, 8, 32)),        # windows overflow: whole quads through the in-kernel path, the partial one through the tail
])
@pytest.mark.parametrize("mode", MODES)
def test_brick_kernels_take_channel_counts_that_are_not_multiples_of_four(shape, mode, gpu):
    """round 5: C % 4 != 0 no longer falls to the gather kernels.  The staged copy holds (C + 3) / 4 quads per view (the
    last one zero-padded by the layout pass), the brick kernels' loops run the C / 4 whole quads, and k_fwd_tail / k_bwd_tail do the last
    1 ... 3 channels per voxel from global memory (the backward's with float atomics)"""
    feats, proj, coords = _ring_problem(seed=91 + MODES.index(mode), **shape)
    f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    d = aggregation._make_desc(f, tuple(c.shape[1:4]), _capi.AGG[mode], torch.float32, _capi.LAYOUT_BVCHW, _capi.VARIANT["brick"])
    assert _capi.lib().mvhmr_unproject_forward_kernel_name(ctypes.byref(d)) in (b"k_fwd_brick", b"k_fwd_brick_groups", b"k_fwd_ws")
    assert _capi.lib().mvhmr_unproject_backward_supported(ctypes.byref(d)) == 1
    out = aggregation.unprojection(f, p, c, aggregation_method=mode, variant="brick")
    ref = cport.forward(feats, proj, coords, mode)
    name = "C %% 4 != 0: %s V%d C%d %dx%d vol%s" % (mode, shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"])
    record_err(name + " fwd", _err(out.detach().cpu().numpy(), ref), TOL)
    go = np.random.default_rng(8).standard_normal(tuple(out.shape), dtype=np.float32)
    out.backward(torch.from_numpy(go).to(gpu))
    gref = cport.backward(go, feats, proj, coords, mode)
    record_err(name + " bwd", _err(f.grad.cpu().numpy(), gref), _bound(gref))
    # the whole quads are what they are at C rounded down: bit for bit the same kernels on the same data
    c4 = shape["C"] // 4 * 4
    out4 = aggregation.unprojection(f.detach()[:, :, :c4].contiguous(), p, c, aggregation_method=mode, variant="brick")
    if mode != "softmax" or _capi.lib().mvhmr_unproject_forward_kernel_name(ctypes.byref(d)) != b"k_fwd_ws":
        assert torch.equal(out.detach()[:, :c4], out4)
    gat = aggregation.unprojection(f.detach(), p, c, aggregation_method=mode, variant="gather")
    record_err(name + " vs gather", float((out.detach() - gat).abs().max()), 4e-6)
    auto = aggregation.unprojection(f.detach(), p, c, aggregation_method=mode, variant="auto")
    record_err(name + " auto", _err(auto.cpu().numpy(), ref), TOL)
    # a caller-held quad-planar copy ((C + 3) / 4 quads per view, the last one zero-padded by mvhmr_convert_features): the same volume
    L, vp = _capi.lib(), ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(gpu).cuda_stream)
    lay = L.mvhmr_preferred_layout(ctypes.byref(d))
    nb = L.mvhmr_feature_layout_bytes(ctypes.byref(d), lay)
    B_, V_, C_, H_, W_ = f.shape
    assert nb >= B_ * V_ * ((C_ + 3) // 4) * H_ * W_ * 16
    quad = torch.empty(nb // 4, device=gpu)
    _capi.check(L.mvhmr_convert_features(ctypes.byref(d), vp(f.data_ptr()), lay, vp(quad.data_ptr()), stream))
    dq = _capi.Desc.from_buffer_copy(d)
    dq.feat_layout = lay
    outq = torch.empty_like(out.detach())
    wsb = L.mvhmr_unproject_forward_workspace_bytes(ctypes.byref(dq))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=gpu)
    _capi.check(L.mvhmr_unproject_forward(ctypes.byref(dq), vp(quad.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(outq.data_ptr()), vp(ws.data_ptr()), wsb, stream))
    assert torch.equal(outq, out.detach())
    if f.shape[3] < 300 and c.shape[3] % 2 == 0:                                   # 16-bit volumes (even Z): fp32 features -> bf16 volume
        ob = aggregation.unprojection(f.detach(), p, c, aggregation_method=mode, variant="brick", out_dtype=torch.bfloat16)
        db = aggregation._make_desc(f, tuple(c.shape[1:4]), _capi.AGG[mode], torch.bfloat16, _capi.LAYOUT_BVCHW, _capi.VARIANT["brick"])
        same_kernel = _capi.lib().mvhmr_unproject_forward_kernel_name(ctypes.byref(db)) == _capi.lib().mvhmr_unproject_forward_kernel_name(ctypes.byref(d))
        if same_kernel or mode != "softmax": assert torch.equal(ob, out.detach().to(torch.bfloat16))      # (k_fwd_ws needs Z % 8 == 0 for a 16-bit volume; its softmax differs from k_fwd_brick's by ~1e-7)
        else: record_err(name + " bf16 volume", float((ob.float() - out.detach()).abs().max()), 2.0 ** -8 * max(1.0, float(out.detach().abs().max())))


def test_random_geometries_through_the_gate(gpu):
    """seeded sweep: random view counts, channel counts, map sizes (non-square), volume extents, cuboid sizes / offsets /
    rotations, camera distances and focal lengths (some cameras inside the volume: voxels behind them) -- forward and
    backward of the AUTO path (whatever the device-side gate picks) against the C oracle, all four aggregation modes"""
    rng = np.random.default_rng(2025)
    for case in range(14):
        V = int(rng.choice([2, 4, 4, 8]))
        C = int(rng.choice([4, 8, 12, 20]))
        H, W = int(rng.integers(12, 41)), int(rng.integers(12, 41))
        X, Y, Z = int(rng.choice([4, 8, 12])), int(rng.choice([8, 16])), int(rng.choice([32, 64]))
        B = int(rng.integers(1, 3))
        side = float(rng.uniform(800.0, 3000.0))
        centre = rng.uniform(-300.0, 300.0, 3)
        theta = float(rng.uniform(0, 2 * np.pi))
        radius = float(rng.uniform(1200.0, 6000.0))        # < ~2000: the camera sits inside a large cuboid
        focal = float(rng.uniform(700.0, 1800.0))
        feats = rng.standard_normal((B, V, C, H, W), dtype=np.float32) * float(rng.choice([0.3, 1.0, 4.0]))
        proj = np.empty((B, V, 3, 4), np.float32)
        for b in range(B):
            for v in range(V):
                az = 2 * np.pi * v / V + rng.uniform(-0.2, 0.2)
                eye = np.array([radius * np.cos(az), radius * np.sin(az), rng.uniform(500.0, 2500.0)])
                fwd = (centre - eye) / np.linalg.norm(centre - eye)
                right = np.cross(fwd, [0, 0, 1.0]); right /= np.linalg.norm(right)
                R = np.stack([right, np.cross(fwd, right), fwd])
                cam = multiview.Camera(R, -R @ eye, [[focal, 0, 512], [0, focal, 512], [0, 0, 1]])
                cam.update_after_resize((1024, 1024), (W, H))
                proj[b, v] = cam.projection
        g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).astype(np.float64)
        pts = -side / 2 + g * (side / (np.array([X, Y, Z]) - 1))
        ct, st = np.cos(theta), np.sin(theta)
        pts = pts @ np.array([[ct, -st, 0], [st, ct, 0], [0, 0, 1.0]]).T + centre
        coords = np.broadcast_to(pts.astype(np.float32), (B,) + pts.shape).copy()
        mode = MODES[case % 4]
        f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
        p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
        out = aggregation.unprojection(f, p, c, aggregation_method=mode)
        ref = cport.forward(feats, proj, coords, mode)
        tag = (case, V, C, H, W, (X, Y, Z), mode)
        record_err("random geometry fwd %s" % (tag,), _err(out.detach().cpu().numpy(), ref), _bound(ref))
        go = rng.standard_normal(ref.shape, dtype=np.float32)
        out.backward(torch.from_numpy(go).to(gpu))
        gref = cport.backward(go, feats, proj, coords, mode)
        record_err("random geometry bwd %s" % (tag,), _err(f.grad.cpu().numpy(), gref), _bound(gref))


def test_empty_batch_and_non_contiguous_inputs(gpu):
    """edge cases of the tensor contract: B = 0 returns the reference's empty zero volume; strided (non-contiguous)
    features, projection matrices and coordinate volumes give the same result as their contiguous copies"""
    feats, proj, coords = _ring_problem(B=2, V=4, C=8, H=24, W=24, vol=(8, 8, 32), seed=3)
    f, p, c = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    empty = aggregation.unprojection(f[:0], p[:0], c[:0])
    assert tuple(empty.shape) == (0, 8, 8, 8, 32) and empty.dtype == torch.float32
    ref = aggregation.unprojection(f, p, c)
    f_nc = torch.empty(2, 4, 8, 24, 48, device=gpu)[..., ::2]
    f_nc.copy_(f)
    p_nc = p.transpose(2, 3).contiguous().transpose(2, 3)
    c_nc = torch.empty(2, 8, 8, 32, 6, device=gpu)[..., ::2]
    c_nc.copy_(c)
    assert not f_nc.is_contiguous() and not p_nc.is_contiguous() and not c_nc.is_contiguous()
    assert torch.equal(aggregation.unprojection(f_nc, p_nc, c_nc), ref)


def test_geometry_gate_picks_the_variant_on_the_device(gpu):
    """AUTO launches both variants behind a device-side gate (csrc/gate.h): coarse grids whose bricks overflow the LDS
    windows run the gather kernels, the others the brick kernels -- bit-identical to the explicit variants"""
    # (AUTO considers the bricks from 96 bricks' worth of voxels on: both shapes hold 128)
    for shape, expect in ((dict(B=2, V=4, C=8, H=320, W=320, vol=(32, 64, 64)), "gather"),    # every brick overflows
                          (dict(B=2, V=4, C=8, H=24, W=24, vol=(64, 64, 32)), "brick")):      # every brick fits
        feats, proj, coords = _ring_problem(seed=5, **shape)
        p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
        outs = {}
        for variant in ("auto", "brick", "gather"):
            f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
            out = aggregation.unprojection(f, p, c, variant=variant)
            outs[variant] = out.detach()
        other = "brick" if expect == "gather" else "gather"
        assert torch.equal(outs["auto"], outs[expect]), shape
        assert not torch.equal(outs["auto"], outs[other]) or torch.equal(outs["brick"], outs["gather"])
        # the synchronous planning query (for callers that run the layout pass themselves) agrees with the gate
        L = _capi.lib()
        desc = aggregation._make_desc(torch.from_numpy(feats).to(gpu), c, _capi.AGG["softmax"], torch.float32, _capi.LAYOUT_BVCHW,
                                      _capi.VARIANT["auto"])
        got = L.mvhmr_unproject_query_variant(ctypes.byref(desc), ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(c.data_ptr()),
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert got == _capi.VARIANT[expect]
        # backward through the gate against the oracle
        f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
        out = aggregation.unprojection(f, p, c)
        go = np.random.default_rng(9).standard_normal(tuple(out.shape), dtype=np.float32)
        out.backward(torch.from_numpy(go).to(gpu))
        gref = cport.backward(go, feats, proj, coords, "softmax")
        record_err("gate bwd %s" % expect, _err(f.grad.cpu().numpy(), gref), _bound(gref))


def test_brick_backward_keeps_per_channel_precision(gpu):
    """the fixed-point window accumulation scales every channel by its own power of two: channels of one quad that differ
    by 20 orders of magnitude (and an all-zero one) each keep fp32-like relative accuracy"""
    feats, proj, coords = _ring_problem(B=1, V=4, C=8, H=24, W=24, vol=(8, 8, 32), seed=77)     # windows fit: the LDS path
    f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    out = aggregation.unprojection(f, p, c, variant="brick")
    mag = np.array([1e-12, 1e8, 1.0, 0.0, 3e-30, 1e20, 1e-3, 7.0], np.float32)
    go = np.random.default_rng(8).standard_normal(tuple(out.shape), dtype=np.float32) * mag[None, :, None, None, None]
    out.backward(torch.from_numpy(go).to(gpu))
    gref = cport.backward(go, feats, proj, coords, "softmax")
    got = f.grad.cpu().numpy()
    for ch in range(8):
        ref_c, got_c = gref[:, :, ch], got[:, :, ch]
        scale = float(np.abs(ref_c).max())
        record_err("brick bwd per-channel precision, channel %d (scale %.1e)" % (ch, scale), _err(got_c, ref_c), 2e-5 * scale)
    assert not got[:, :, 3].any()


def test_brick_variant_with_cameras_inside_the_volume(gpu):
    """adversarial geometry for the window logic: behind-camera voxels, bricks with no valid voxel for a view"""
    d = load_golden("unproj", "adversarial_v4c6")
    rng = np.random.default_rng(0)
    feats = rng.standard_normal((1, 4, 8, 16, 16), dtype=np.float32)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(32), indexing="ij"), -1).astype(np.float32)
    coords = (-1250.0 + g * np.array([2500.0 / 7, 2500.0 / 7, 2500.0 / 31], np.float32))[None]
    f, p, c = torch.from_numpy(feats).to(gpu), _dev(d, "proj", gpu), torch.from_numpy(coords).to(gpu)
    for mode in MODES:
        out = aggregation.unprojection(f, p, c, aggregation_method=mode, variant="brick")
        ref = cport.forward(feats, d["proj"], coords, mode)
        record_err("brick fwd, cameras inside the volume (%s)" % mode, _err(out.cpu().numpy(), ref), TOL)


def test_channels_last_features_skip_the_layout_pass(gpu):
    feats, proj, coords = _ring_problem(B=2, V=4, C=32, H=24, W=24, vol=(8, 8, 16), seed=3)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    planar = torch.from_numpy(feats).to(gpu)
    cl = planar.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)       # (B,V,C,H,W) view of (B,V,H,W,C) memory
    assert not cl.is_contiguous() and aggregation._is_channels_last5(cl)
    a = aggregation.unprojection(planar, p, c, variant="gather")                  # planar + layout pass -> the gather kernels (AUTO would take the bricks)
    cl = cl.detach().requires_grad_(True)
    b = aggregation.unprojection(cl, p, c)
    assert torch.equal(a, b)
    go = torch.randn_like(b)
    b.backward(go)
    pl = planar.detach().requires_grad_(True)
    aggregation.unprojection(pl, p, c).backward(go)
    assert cl.grad.shape == cl.shape
    record_err("channels-last vs planar features, bwd", float((cl.grad - pl.grad).abs().max()), 1e-5)


@pytest.mark.parametrize("views", (4, 8))
def test_fp16_storage_mode(views, gpu):
    """fp16 features / volume, fp32 geometry and accumulation; oracle evaluated on the fp16-rounded inputs.
    Bound: half an fp16 ulp of the output magnitude (~2^-11 * |x|) plus the fp32 bar."""
    feats, proj, coords = _ring_problem(B=1, V=views, C=32, H=32, W=32, vol=(8, 8, 32), seed=11)
    f16 = torch.from_numpy(feats).to(gpu).half()
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    ref = cport.forward(f16.float().cpu().numpy(), proj, coords, "softmax")
    out16 = aggregation.unprojection(f16, p, c)
    assert out16.dtype == torch.float16
    bound = TOL + np.abs(ref).max() * 2.0 ** -11
    record_err("fp16 storage fwd auto V%d" % views, _err(out16.float().cpu().numpy(), ref), bound)
    for variant in ("brick", "gather"):         # both kernel families serve fp16 storage (brick: fp16 or fp32 staging, fp16 stores)
        o = aggregation.unprojection(f16, p, c, variant=variant)
        assert o.dtype == torch.float16
        record_err("fp16 storage fwd %s V%d" % (variant, views), _err(o.float().cpu().numpy(), ref), bound)
        fg = f16.clone().requires_grad_(True)
        gg = torch.ones_like(o)
        aggregation.unprojection(fg, p, c, variant=variant).backward(gg)
        gr = cport.backward(gg.float().cpu().numpy(), f16.float().cpu().numpy(), proj, coords, "softmax")
        record_err("fp16 storage bwd %s V%d" % (variant, views), _err(fg.grad.float().cpu().numpy(), gr), TOL + np.abs(gr).max() * 2.0 ** -10)
    out32 = aggregation.unprojection(f16, p, c, out_dtype=torch.float32)
    assert out32.dtype == torch.float32
    record_err("fp16 features, fp32 volume V%d" % views, _err(out32.cpu().numpy(), ref), TOL)
    # ... and its backward on every kernel family (r04: the brick backward takes this pairing too -- fp32 grad_out, fp16 feature gradient)
    go32 = torch.randn(out32.shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(17))
    g32ref = cport.backward(go32.cpu().numpy(), f16.float().cpu().numpy(), proj, coords, "softmax")
    for variant in ("auto", "brick", "gather"):
        fm = f16.clone().requires_grad_(True)
        aggregation.unprojection(fm, p, c, out_dtype=torch.float32, variant=variant).backward(go32)
        assert fm.grad.dtype == torch.float16
        record_err("fp16 features, fp32 volume bwd %s V%d" % (variant, views), _err(fm.grad.float().cpu().numpy(), g32ref),
                   TOL + np.abs(g32ref).max() * 2.0 ** -10)
    f16g = f16.clone().requires_grad_(True)
    go = torch.randn_like(out16)
    aggregation.unprojection(f16g, p, c).backward(go)
    gref = cport.backward(go.float().cpu().numpy(), f16.float().cpu().numpy(), proj, coords, "softmax")
    gb = TOL + np.abs(gref).max() * 2.0 ** -10
    assert f16g.grad.dtype == torch.float16
    record_err("fp16 storage bwd auto, random grad_out V%d" % views, _err(f16g.grad.float().cpu().numpy(), gref), gb)


# ------------------------------------------------------------------------------------ size-independent properties at BASELINE config[1]
@pytest.fixture(scope="module")
def config1(gpu):
    """32^3 grid, 4 views, 256 ch, 96x96 maps, batch 8 fp32 (BASELINE.json configs[1])."""
    feats, proj, coords = _ring_problem(B=8, V=4, C=256, H=96, W=96, vol=(32, 32, 32), seed=1, theta=0.0)
    return torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)


def test_config1_properties(config1):
    f, p, c = config1
    V = f.shape[1]
    s = aggregation.unprojection(f, p, c, aggregation_method="sum")
    # mean == sum / V, max >= mean, softmax-weighted mean lies between mean and max
    mean = aggregation.unprojection(f, p, c, aggregation_method="mean")
    mx = aggregation.unprojection(f, p, c, aggregation_method="max")
    sm = aggregation.unprojection(f, p, c, aggregation_method="softmax")
    record_err("configs[1] mean == sum / V", float((mean - s / V).abs().max()), 1e-6)
    assert bool((mx >= mean - 1e-6).all()) and bool((sm <= mx + 1e-5).all()) and bool((sm >= mean - 1e-5).all())
    # 'sum' is linear in the features
    g = torch.randn_like(f)
    s2 = aggregation.unprojection(2.0 * f + g, p, c, aggregation_method="sum")
    sg = aggregation.unprojection(g, p, c, aggregation_method="sum")
    record_err("configs[1] linearity of sum", float((s2 - (2.0 * s + sg)).abs().max()), 2e-5)
    # the aggregate does not care about the order of the views
    perm = torch.tensor([2, 0, 3, 1], device=f.device)
    smp = aggregation.unprojection(f[:, perm].contiguous(), p[:, perm].contiguous(), c, aggregation_method="softmax")
    record_err("configs[1] view permutation", float((smp - sm).abs().max()), 2e-6)
    # samples are independent: a batch shard equals the same rows of the full batch (what multi-GPU sharding relies on)
    half = aggregation.unprojection(f[4:].contiguous(), p[4:].contiguous(), c[4:].contiguous())
    assert torch.equal(half, sm[4:])
    # constant feature maps: every in-frustum voxel aggregates to that constant (weights sum to 1)
    ones = torch.full_like(f, 1.5)
    so = aggregation.unprojection(ones, p, c, aggregation_method="max")
    assert float(so.max()) <= 1.5 + 1e-5 and float(so.min()) >= 0.0
    assert float(((so - 1.5).abs() <= 1e-5).float().mean()) > 0.3


def test_config1_sample_vs_oracle(config1):
    """Full BASELINE config[1] inputs, checked against the oracle on one sample (keeps the CPU side to seconds)."""
    f, p, c = config1
    out = aggregation.unprojection(f, p, c)
    ref = cport.forward(f[5:6].cpu().numpy(), p[5:6].cpu().numpy(), c[5:6].cpu().numpy(), "softmax")
    record_err("configs[1] fwd (sample 5, all channels)", _err(out[5:6].cpu().numpy(), ref), TOL)


# ------------------------------------------------------------------------------------ VolumeGenerator end to end
def _rebuild(d, gpu):
    B, V, C_in, C_out, S, training, use_tri, seed = (int(x) for x in d["meta"])
    cams = [[multiview.Camera(d["R"][v, b], d["t"][v, b], d["K"][v, b]) for b in range(B)] for v in range(V)]
    batch = dict(images=np.zeros((B, V, int(d["image_hw"][0]), int(d["image_hw"][1]), 3), dtype=np.uint8),
                 cameras=cams, keypoints_3d=[k for k in d["keypoints"]])
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=C_in, output_channels=C_out, cuboid_side=2500.0,
                                      use_triangulation=bool(use_tri), kind=str(d["kind"]), device=gpu)
    gen.load_state_dict({"process_feature.0.weight": torch.from_numpy(d["weight"]),
                         "process_feature.0.bias": torch.from_numpy(d["bias"])})
    gen.train(bool(training))
    return gen, batch, seed


@pytest.mark.parametrize("case", golden_cases("volgen"))
def test_volume_generator_end_to_end(case, gpu):
    d = load_golden("volgen", case)
    gen, batch, seed = _rebuild(d, gpu)
    np.random.seed(seed)
    rots, centers = gen.volume_pose(batch, _dev(d, "proj_org", gpu), tuple(batch["images"].shape[2:-1]))
    coords = gen.coord_volumes(rots, centers, gpu)
    tri = bool(int(d["meta"][6]))
    # use_triangulation: the pivot is a DLT null vector.  The reference takes it from a per-sample fp32 torch.svd; this build
    # solves the same system once, batched, in float64 on the device.  Observed (profiles/r02_parity_observed.json): the
    # coordinates of the train_tri golden (training + triangulation, the one case where the pivot reaches the output) agree
    # to 2.4e-4 mm and its volume to 1.1e-6 -- the same bounds as every other case hold.
    record_err("volgen coords %s (mm)" % case, _err(coords.cpu().numpy(), d["coords"]), 1e-3)
    np.random.seed(seed)
    with torch.no_grad():
        vol = gen(_dev(d, "features_in", gpu), _dev(d, "proj_org", gpu), batch)
    assert vol.dtype == torch.float32 and tuple(vol.shape) == d["volume"].shape
    record_err("volgen volume %s" % case, _err(vol.cpu().numpy(), d["volume"]), TOL)


def test_volume_generator_trains(gpu):
    d = load_golden("volgen", "train_mpii")
    gen, batch, seed = _rebuild(d, gpu)
    np.random.seed(seed)
    feats = _dev(d, "features_in", gpu).requires_grad_(True)
    vol = gen(feats, _dev(d, "proj_org", gpu), batch)
    vol.square().mean().backward()
    w = gen.process_feature[0].weight
    assert w.grad is not None and torch.isfinite(w.grad).all() and float(w.grad.abs().sum()) > 0
    assert feats.grad is not None and torch.isfinite(feats.grad).all()


# ------------------------------------------------------------------------------------ raw C ABI
def test_raw_c_abi_call(gpu):
    """Bind the library the way INTEGRATION.md shows (plain pointers + sizes), no package helpers."""
    d = load_golden("unproj", "tiles_v4c16")
    f, p, c = _dev(d, "features", gpu), _dev(d, "proj", gpu), _dev(d, "coords", gpu)
    L = ctypes.CDLL(_capi.LIB_PATH)
    L.mvhmr_unproject_forward_workspace_bytes.restype = ctypes.c_size_t
    desc = _capi.Desc()
    desc.abi_version = _capi.ABI_VERSION
    desc.batch, desc.views, desc.channels, desc.feat_h, desc.feat_w = f.shape
    desc.vol_x, desc.vol_y, desc.vol_z = c.shape[1:4]
    desc.method, desc.feat_dtype, desc.out_dtype, desc.feat_layout, desc.variant = 0, 0, 0, 0, 0
    need = L.mvhmr_unproject_forward_workspace_bytes(ctypes.byref(desc))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=gpu)
    out = torch.empty(f.shape[0], f.shape[2], *c.shape[1:4], device=gpu)
    vp = ctypes.c_void_p
    rc = L.mvhmr_unproject_forward(ctypes.byref(desc), vp(f.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(out.data_ptr()),
                                   vp(ws.data_ptr()), ctypes.c_size_t(need), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    record_err("raw C-ABI call vs reference golden", _err(out.cpu().numpy(), d["out_softmax"]), TOL)


def test_wrong_device_and_dtype_raise(gpu):
    d = load_golden("unproj", "tiny_b2v2c4")
    f, p, c = _dev(d, "features", gpu), _dev(d, "proj", gpu), _dev(d, "coords", gpu)
    with pytest.raises(RuntimeError, match="expected all tensors on"):
        aggregation.unprojection(f, p.cpu(), c)
    with pytest.raises(RuntimeError, match="float32 or float16"):
        aggregation.unprojection(f.double(), p, c)
    with pytest.raises(ValueError, match="Unknown aggregation_method"):
        aggregation.unprojection(f, p, c, aggregation_method="median")


# ------------------------------------------------------------------------------------ BASELINE configs[2..4] at full per-GPU size
def _oracle_on_channels(f, p, c, out, chans, b, mode="softmax"):
    """channels are independent: check a few of them (one sample) against the CPU oracle"""
    fs = f[b:b + 1, :, chans].float().cpu().numpy()
    ref = cport.forward(fs, p[b:b + 1].cpu().numpy(), c[b:b + 1].cpu().numpy(), mode)
    return float(np.abs(out[b:b + 1, chans].float().cpu().numpy() - ref).max()), ref


def test_config2_fp16_forward_backward_full_size(gpu):
    """configs[2]: 64^3 grid, 4 views, 256 ch, batch 32, fp16 storage, forward + backward."""
    torch.manual_seed(2)
    B, V, C, H, S = 32, 4, 256, 96, 64
    _, proj, coords = _ring_problem(B=1, V=V, C=1, H=H, W=H, vol=(S, S, S), seed=2, theta=0.0)
    f = torch.randn(B, V, C, H, H, device=gpu, dtype=torch.float16).requires_grad_(True)
    p = torch.from_numpy(proj).to(gpu).expand(B, -1, -1, -1).contiguous()
    c = torch.from_numpy(coords).to(gpu).expand(B, -1, -1, -1, -1).contiguous()
    out = aggregation.unprojection(f, p, c)
    assert out.dtype == torch.float16 and tuple(out.shape) == (B, C, S, S, S)
    chans = [0, 1, 127, 255]
    err, ref = _oracle_on_channels(f.detach(), p, c, out.detach(), chans, b=31)
    record_err("configs[2] fp16 fwd (sample 31, 4 channels)", err, TOL + np.abs(ref).max() * 2.0 ** -11)
    # backward: gradient of sum(out * g) for a sparse g touches every code path; check it on a channel slice
    g = torch.zeros_like(out)
    g[31, chans] = torch.randn(len(chans), S, S, S, device=gpu, dtype=torch.float16)
    out.backward(g)
    assert f.grad.dtype == torch.float16 and bool(torch.isfinite(f.grad).all())
    gref = cport.backward(g[31:32, chans].float().cpu().numpy(), f[31:32, :, chans].detach().float().cpu().numpy(),
                          proj, coords, "softmax")
    got = f.grad[31:32, :, chans].float().cpu().numpy()
    record_err("configs[2] fp16 bwd (sample 31, 4 channels)", _err(got, gref), TOL + np.abs(gref).max() * 2.0 ** -10)
    assert float(f.grad[:31].abs().max()) == 0.0 and float(f.grad[31, :, 2:127].abs().max()) == 0.0   # nothing leaks across samples / channels
    del out, g, f
    torch.cuda.empty_cache()


def test_config3_eight_views_per_gpu_shard(gpu):
    """configs[3]: 64^3 grid, 8 views (MPI-INF-like ring), 256 ch, batch 64 over 4 GPUs = 16 samples per GPU."""
    torch.manual_seed(3)
    B, V, C, H, S = 16, 8, 256, 96, 64
    _, proj, coords = _ring_problem(B=1, V=V, C=1, H=H, W=H, vol=(S, S, S), seed=3, theta=0.0)
    f = torch.randn(B, V, C, H, H, device=gpu)
    p = torch.from_numpy(proj).to(gpu).expand(B, -1, -1, -1).contiguous()
    c = torch.from_numpy(coords).to(gpu).expand(B, -1, -1, -1, -1).contiguous()
    out = aggregation.unprojection(f, p, c)
    err, _ = _oracle_on_channels(f, p, c, out, [0, 200, 255], b=15)
    record_err("configs[3] shard fwd (sample 15, 3 channels)", err, TOL)
    # the geometry gate must keep this shard on the brick kernels (a doubled 8-view brick would overflow the LDS windows)
    L = _capi.lib()
    desc = aggregation._make_desc(f, c, _capi.AGG["softmax"], torch.float32, _capi.LAYOUT_BVCHW, _capi.VARIANT["auto"])
    assert L.mvhmr_unproject_query_variant(ctypes.byref(desc), ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(c.data_ptr()),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == _capi.VARIANT["brick"]
    mean = aggregation.unprojection(f, p, c, aggregation_method="mean")
    s = aggregation.unprojection(f, p, c, aggregation_method="sum")
    record_err("configs[3] mean == sum / V", float((mean - s / V).abs().max()), 1e-6)
    # a rank's shard equals the same rows of the whole batch (what the 4-GPU run relies on)
    part = aggregation.unprojection(f[4:8].contiguous(), p[4:8].contiguous(), c[4:8].contiguous())
    assert torch.equal(part, out[4:8])
    del out, mean, s, part
    torch.cuda.empty_cache()


def test_config4_large_volume_64bit_indexing(gpu):
    """configs[4] geometry: 128^3 grid, 4 views, 512 ch -- one sample's volume is 4.3 GB (> 2^32 bytes), two samples
    are checked so that every 64-bit offset path (sample, channel, voxel) is exercised by both kernels."""
    torch.manual_seed(4)
    B, V, C, H, S = 2, 4, 512, 96, 128
    _, proj, coords = _ring_problem(B=1, V=V, C=1, H=H, W=H, vol=(S, S, S), seed=4, theta=0.0)
    f = torch.randn(B, V, C, H, H, device=gpu)
    p = torch.from_numpy(proj).to(gpu).expand(B, -1, -1, -1).contiguous()
    c = torch.from_numpy(coords).to(gpu).expand(B, -1, -1, -1, -1).contiguous()
    out = aggregation.unprojection(f, p, c)                    # brick variant
    assert out.numel() * 4 >= 2 ** 33 and out[0].numel() * 4 >= 2 ** 32
    err, _ = _oracle_on_channels(f, p, c, out, [0, 511], b=1)
    record_err("configs[4] geometry B=2 fwd (sample 1, 2 channels)", err, TOL)
    gat = aggregation.unprojection(f, p, c, variant="gather")
    worst = 0.0
    for ch in (0, 255, 256, 511):                              # compare kernels plane by plane (keeps temporaries small)
        worst = max(worst, float((out[:, ch] - gat[:, ch]).abs().max()))
    record_err("configs[4] geometry B=2, brick vs gather (4 channel planes)", worst, 2e-6)
    del out, gat
    torch.cuda.empty_cache()


def test_forward_is_graph_capturable(gpu):
    """The C ABI promises no allocation / no host sync inside a call: capture the two calls of a step into a HIP graph
    (after one eager warm-up) and replay it on new input values."""
    feats, proj, coords = _ring_problem(B=2, V=4, C=16, H=32, W=32, vol=(4, 8, 32), seed=21)
    f, p, c = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    L = _capi.lib()
    desc = aggregation._make_desc(f, c, _capi.AGG["softmax"], torch.float32, _capi.LAYOUT_BVCHW, _capi.VARIANT["auto"])
    need = L.mvhmr_unproject_forward_workspace_bytes(ctypes.byref(desc))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=gpu)
    out = torch.empty(2, 16, 4, 8, 32, device=gpu)
    vp = ctypes.c_void_p

    def call(stream):
        _capi.check(L.mvhmr_unproject_forward(ctypes.byref(desc), vp(f.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(out.data_ptr()),
                                              vp(ws.data_ptr()), need, vp(stream.cuda_stream)))

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call(side)                                   # warm-up outside the capture (one-time kernel attribute set-up)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call(torch.cuda.current_stream())
    f.copy_(torch.randn_like(f))                     # new values, same buffers
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    ref = cport.forward(f.cpu().numpy(), proj, coords, "softmax")
    record_err("HIP-graph replay fwd", _err(out.cpu().numpy(), ref), TOL)


def test_channels_last_features_take_the_bricks_where_they_pay(gpu):
    """a channels-last-strided feature tensor feeds the gather kernels without a layout pass -- except where the library's AUTO choice
    for the problem is the brick kernels (from 96 bricks' worth of voxels on): the binding then makes it planar first.  Same values
    and gradients as the planar tensor, bit for bit, and the gradient keeps working through autograd whatever its strides."""
    feats, proj, coords = _ring_problem(B=1, V=4, C=16, H=48, W=48, vol=(64, 64, 48), seed=13)      # 196 608 voxels
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    planar = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    cl = torch.from_numpy(feats).to(gpu).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3).requires_grad_(True)
    assert aggregation._is_channels_last5(cl) and not cl.is_contiguous()
    # fp32: the library's own channels-last -> quad-planar pass (the copy the bricks stage from); fp16: a planar copy
    assert aggregation._feature_layout(cl, c, _capi.AGG["softmax"], torch.float32, _capi.VARIANT["auto"])[1] == _capi.LAYOUT_QUAD
    assert aggregation._feature_layout(cl.detach().half(), c, _capi.AGG["softmax"], torch.float16, _capi.VARIANT["auto"])[1] == _capi.LAYOUT_BVCHW
    assert aggregation._feature_layout(cl, c, _capi.AGG["softmax"], torch.float32, _capi.VARIANT["gather"])[1] == _capi.LAYOUT_BVHWC
    # the pass itself against the planar -> quad-planar pass
    L = _capi.lib()
    d_pl = aggregation._make_desc(planar, c, _capi.AGG["softmax"], torch.float32, _capi.LAYOUT_BVCHW, _capi.VARIANT["auto"])
    d_cl = aggregation._make_desc(cl, c, _capi.AGG["softmax"], torch.float32, _capi.LAYOUT_BVHWC, _capi.VARIANT["auto"])
    nb = L.mvhmr_feature_layout_bytes(ctypes.byref(d_pl), _capi.LAYOUT_QUAD)
    qa, qb = torch.zeros(nb, dtype=torch.uint8, device=gpu), torch.ones(nb, dtype=torch.uint8, device=gpu)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(L.mvhmr_convert_features(ctypes.byref(d_pl), ctypes.c_void_p(planar.data_ptr()), _capi.LAYOUT_QUAD, ctypes.c_void_p(qa.data_ptr()), stream))
    _capi.check(L.mvhmr_convert_features(ctypes.byref(d_cl), ctypes.c_void_p(cl.data_ptr()), _capi.LAYOUT_QUAD, ctypes.c_void_p(qb.data_ptr()), stream))
    assert torch.equal(qa, qb)
    go = torch.randn(1, 16, 64, 64, 48, device=gpu, generator=torch.Generator(device=gpu).manual_seed(3))
    outs, grads = [], []
    for f in (planar, cl):
        out = aggregation.unprojection(f, p, c)
        out.backward(go)
        outs.append(out.detach()); grads.append(f.grad.clone())
    assert torch.equal(outs[0], outs[1])
    record_err("channels-last input through the bricks: gradient vs the planar input's", float((grads[0] - grads[1]).abs().max()),
               2e-5 * float(grads[0].abs().max()))                       # float atomics in the flush: last-bit differences run to run
    small = torch.from_numpy(feats[:, :, :, :24, :24].copy()).to(gpu).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    assert aggregation._feature_layout(small, (8, 8, 32), _capi.AGG["softmax"], torch.float32, _capi.VARIANT["auto"])[1] == _capi.LAYOUT_BVHWC
    # fp16 channels-last features through the planar copy: forward + backward against the planar fp16 tensor
    ph = torch.from_numpy(feats).to(gpu).half().requires_grad_(True)
    ch = torch.from_numpy(feats).to(gpu).half().permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3).requires_grad_(True)
    oh = [aggregation.unprojection(t, p, c) for t in (ph, ch)]
    assert torch.equal(oh[0], oh[1])
    for o in oh: o.backward(go.half())
    record_err("fp16 channels-last input through the bricks: gradient vs the planar input's", float((ph.grad.float() - ch.grad.float()).abs().max()),
               2.0 ** -9 * float(ph.grad.float().abs().max()))


def test_volume_generator_eval_forward_is_graph_capturable(gpu):
    """the whole eval forward of VolumeGenerator -- packed cameras and tensor keypoints: projections, pose, fused conv, gate and
    un-projection all on the device, nothing copied from the host -- captured into a HIP graph; the replay on new feature values
    equals the eager call bit for bit (scripts/graph_volgen.py times both)"""
    B, V, C, H, S, IMG = 2, 4, 128, 32, 32, 128
    cams = _rig(B, V, 5000.0, IMG, seed=4)
    batch = dict(images=np.zeros((B, V, IMG, IMG, 3), np.uint8), cameras=cams, cameras_packed=aggregation.pack_cameras(cams, gpu),
                 keypoints_3d=torch.zeros(B, 17, 3, device=gpu))
    proj_org = torch.from_numpy(np.stack([[cams[v][b].projection for v in range(V)] for b in range(B)]).astype(np.float32)).to(gpu)
    torch.manual_seed(2)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=C, output_channels=C, device=gpu).eval()
    x = torch.randn(B, V, C, H, H, device=gpu)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            gen(x, proj_org, batch)                      # warm-up outside the capture (kernel attributes, the cached eval rotations)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = gen(x, proj_org, batch)
        x.copy_(torch.randn_like(x))                     # new values, same buffers
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, gen(x, proj_org, batch))


# ------------------------------------------------------------------------------------ round 2: shard-size forward AND backward
def _sparse_backward_check(f, p, c, proj, coords, out, b, chans, name, half=False):
    """gradient of sum(out * g) for a g that is non-zero on one sample and a few channels: the oracle only has to run on
    that slice, and everything outside it must stay exactly zero (nothing leaks across samples / channels)"""
    S = out.shape[2:]
    g = torch.zeros_like(out)
    g[b, chans] = torch.randn(len(chans), *S, device=out.device, dtype=out.dtype)
    out.backward(g)
    assert bool(torch.isfinite(f.grad).all())
    gref = cport.backward(g[b:b + 1, chans].float().cpu().numpy(), f[b:b + 1, :, chans].detach().float().cpu().numpy(), proj, coords, "softmax")
    got = f.grad[b:b + 1, :, chans].float().cpu().numpy()
    record_err(name, _err(got, gref), (TOL + np.abs(gref).max() * 2.0 ** -10) if half else _bound(gref))
    other = [ch for ch in range(f.shape[2]) if ch not in chans][:64]
    assert float(f.grad[b, :, other].abs().max()) == 0.0
    if b > 0:
        assert float(f.grad[:b].abs().max()) == 0.0


def _big_problem(gpu, B, V, C, S, seed, H=96, dtype=torch.float32):
    torch.manual_seed(seed)
    _, proj, coords = _ring_problem(B=1, V=V, C=1, H=H, W=H, vol=(S, S, S), seed=seed, theta=0.0)
    f = torch.randn(B, V, C, H, H, device=gpu, dtype=dtype).requires_grad_(True)
    p = torch.from_numpy(proj).to(gpu).expand(B, -1, -1, -1).contiguous()
    c = torch.from_numpy(coords).to(gpu).expand(B, -1, -1, -1, -1).contiguous()
    return f, p, c, proj, coords


def test_northstar_fp32_forward_backward_full_size(gpu):
    """the headline workload itself (64^3, 4 views, 256 ch, batch 32, fp32): forward and backward against the oracle"""
    f, p, c, proj, coords = _big_problem(gpu, 32, 4, 256, 64, seed=12)
    out = aggregation.unprojection(f, p, c)
    err, _ = _oracle_on_channels(f.detach(), p, c, out.detach(), [0, 63, 128, 255], b=17)
    record_err("north star fp32 fwd (sample 17, 4 channels)", err, TOL)
    _sparse_backward_check(f, p, c, proj, coords, out, 17, [0, 63, 128, 255], "north star fp32 bwd (sample 17, 4 channels)")
    del out, f
    torch.cuda.empty_cache()


def test_config3_backward_at_shard_size(gpu):
    """configs[3] per-GPU shard (16 samples, 8 views, 256 ch, 64^3): backward against the oracle"""
    f, p, c, proj, coords = _big_problem(gpu, 16, 8, 256, 64, seed=13)
    out = aggregation.unprojection(f, p, c)
    _sparse_backward_check(f, p, c, proj, coords, out, 9, [5, 250], "configs[3] shard bwd (sample 9, 2 channels)")
    del out, f
    torch.cuda.empty_cache()


def test_config4_full_shard_forward_backward(gpu):
    """configs[4] per-GPU shard: 128^3 grid, 4 views, 512 ch, 16 samples -- 68.7 GB of output and as much grad_out: the size
    that stresses 64-bit offsets and the allocator.  Forward and backward against the oracle on a channel slice."""
    f, p, c, proj, coords = _big_problem(gpu, 16, 4, 512, 128, seed=14)
    out = aggregation.unprojection(f, p, c)
    assert out.numel() * 4 > 68 * 10 ** 9
    err, _ = _oracle_on_channels(f.detach(), p, c, out.detach(), [0, 511], b=15)
    record_err("configs[4] shard fwd (sample 15, 2 channels)", err, TOL)
    _sparse_backward_check(f, p, c, proj, coords, out, 15, [0, 511], "configs[4] shard bwd (sample 15, 2 channels)")
    del out, f
    torch.cuda.empty_cache()


def test_config4_volume_generator_train_step(gpu):
    """one VolumeGenerator training step at the configs[4] shard (1x1 conv 512 -> 512, 128^3, 16 samples): runs, gradients
    finite and non-zero; the conv's weight gradient equals the one autograd gives for the same grad w.r.t. the conv output"""
    B, V, C, H, S, IMG = 16, 4, 512, 96, 128, 384
    rng = np.random.default_rng(44)
    cams = [[None] * B for _ in range(V)]
    for v in range(V):
        az = 2 * np.pi * v / V + 0.3
        eye = np.array([5000 * np.cos(az), 5000 * np.sin(az), 1500.0])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0, 0, 1.0]); right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        for b in range(B):
            cam = multiview.Camera(R, -R @ eye, [[1145.0, 0, 512], [0, 1145.0, 512], [0, 0, 1]])
            cam.update_after_crop((200, 200, 824, 824))
            cam.update_after_resize((624, 624), (IMG, IMG))
            cams[v][b] = cam
    batch = dict(images=np.zeros((B, V, IMG, IMG, 3), np.uint8), cameras=cams,
                 keypoints_3d=[rng.normal(0, 100, (17, 3)).astype(np.float32) for _ in range(B)])
    torch.manual_seed(5)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=C, output_channels=C, device=gpu).train()
    np.random.seed(5)
    feats = torch.randn(B, V, C, H, H, device=gpu, requires_grad=True)
    proj_org = torch.from_numpy(np.stack([[cams[v][b].projection for v in range(V)] for b in range(B)]).astype(np.float32)).to(gpu)
    vol = gen(feats, proj_org, batch)
    assert tuple(vol.shape) == (B, C, S, S, S)
    (vol * vol).mean().backward()
    w = gen.process_feature[0].weight
    assert bool(torch.isfinite(w.grad).all()) and float(w.grad.abs().sum()) > 0
    assert bool(torch.isfinite(feats.grad).all()) and float(feats.grad.abs().sum()) > 0
    del vol
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------ non-finite values (include/mvhmr_unproject.h)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_grad_out_stays_visible_in_both_backward_variants(bad, gpu):
    """an Inf / NaN in grad_out (fp16 overflow, divergence) must make grad_features non-finite in the brick backward too
    (its fixed-point LDS accumulation cannot carry it: the affected brick's windows get NaN), finite values elsewhere agree"""
    feats, proj, coords = _ring_problem(B=2, V=4, C=8, H=24, W=24, vol=(8, 8, 32), seed=41)      # windows fit: the LDS path
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    go = np.random.default_rng(42).standard_normal((2, 8, 8, 8, 32), dtype=np.float32)
    go[1, 5, 3, 4, 17] = bad
    grads = {}
    for variant in ("brick", "gather"):
        f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
        aggregation.unprojection(f, p, c, variant=variant).backward(torch.from_numpy(go).to(gpu))
        grads[variant] = f.grad
        assert not bool(torch.isfinite(f.grad[1, :, 5]).all()), variant        # visible in the poisoned sample and channel
        assert bool(torch.isfinite(f.grad[0]).all()) and bool(torch.isfinite(f.grad[1, :, :5]).all()) and bool(torch.isfinite(f.grad[1, :, 6:]).all())
    # everything outside the poisoned (sample, channel) agrees between the two kernels
    a, b = grads["brick"].clone(), grads["gather"].clone()
    a[1, :, 5] = 0; b[1, :, 5] = 0
    record_err("non-finite grad_out (%s): brick vs gather outside the poisoned channel" % bad, float((a - b).abs().max()), TOL)
    # the gather variant poisons exactly the reference's pixels (float scatter); the brick variant a superset of them
    bad_g, bad_b = ~torch.isfinite(grads["gather"]), ~torch.isfinite(grads["brick"])
    assert bool((bad_b | ~bad_g).all())


def test_non_finite_features_and_depth_behaviour_is_pinned(gpu):
    """documented behaviour (header): (1) Inf feature values in the BORDER pixels: a tap outside the image contributes
    0 * (clamped border pixel) where grid_sample's zero padding (and the oracle) skips it -- the set of non-finite samples is
    the reference's (such a sample taps the border pixel itself with a non-zero weight), only Inf may read NaN; everything
    finite agrees, both variants alike; an Inf in an interior pixel reaches exactly the samples that tap it.  (2) a NaN depth (NaN in the projection matrix) gives an
    exactly zero sample for that view, so 'sum' equals the sum over the other views."""
    feats, proj, coords = _ring_problem(B=1, V=4, C=8, H=12, W=12, vol=(8, 8, 32), seed=43)
    coords = np.ascontiguousarray(coords * np.float32(2.2))                       # a 5.5 m cuboid: the taps cross every image border
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    fb = feats.copy()
    fb[0, 1, 3, 0, :] = np.inf; fb[0, 1, 3, -1, :] = np.inf; fb[0, 1, 3, :, 0] = np.inf; fb[0, 1, 3, :, -1] = np.inf   # border of view 1, channel 3
    fi = feats.copy(); fi[0, 1, 3, 6, 6] = np.inf                                 # interior pixel
    with np.errstate(all="ignore"):
        ref_b, ref_i = cport.forward(fb, proj, coords, "sum"), cport.forward(fi, proj, coords, "sum")
    outs = {}
    for variant in ("brick", "gather"):
        ob = aggregation.unprojection(torch.from_numpy(fb).to(gpu), p, c, aggregation_method="sum", variant=variant).cpu().numpy()
        oi = aggregation.unprojection(torch.from_numpy(fi).to(gpu), p, c, aggregation_method="sum", variant=variant).cpu().numpy()
        outs[variant] = ob
        # interior Inf: exactly the reference's pixels, a weighted Inf and never 0 * Inf
        assert np.array_equal(np.isfinite(oi), np.isfinite(ref_i)) and not np.isnan(oi).any() and np.isinf(oi).any()
        fin = np.isfinite(ref_i)
        record_err("interior Inf, finite part (%s)" % variant, _err(oi[fin], ref_i[fin]), TOL)
        # border Inf: the SAME samples are non-finite as in the reference (a sample whose clamped zero-weight tap lands on a
        # border pixel also taps that pixel with a non-zero weight); only the kind can differ: Inf + 0 * Inf = NaN here
        bad_ref, bad = ~np.isfinite(ref_b), ~np.isfinite(ob)
        assert np.array_equal(bad, bad_ref) and bad.any()
        assert not bad[0, :3].any() and not bad[0, 4:].any()                      # other channels never see it
        both = ~bad
        record_err("border Inf, finite part (%s)" % variant, _err(ob[both], ref_b[both]), TOL)
    assert np.array_equal(np.isfinite(outs["brick"]), np.isfinite(outs["gather"]))
    pn = proj.copy(); pn[0, 2, 2, :] = np.nan                                     # view 2: depth row NaN -> z is NaN for every voxel
    keep = [0, 1, 3]
    ref = cport.forward(np.ascontiguousarray(feats[:, keep]), np.ascontiguousarray(proj[:, keep]), coords, "sum")
    for variant in ("brick", "gather"):
        o = aggregation.unprojection(torch.from_numpy(feats).to(gpu), torch.from_numpy(pn).to(gpu), c, aggregation_method="sum", variant=variant)
        record_err("NaN depth: view dropped (%s)" % variant, _err(o.cpu().numpy(), ref), TOL)


def test_dynamic_lds_opt_in_is_remembered_per_device_and_kernel():
    """hipFuncSetAttribute(MaxDynamicSharedMemorySize) acts on the current device's function object: the library's cache must
    key on (device, kernel), or a second GPU driven from the same process never gets its 160 KB opt-in"""
    L = _capi.lib()
    k1, k2 = ctypes.c_void_p(0x7f0000001000), ctypes.c_void_p(0x7f0000002000)
    keys = {(d, k.value): L.mvhmr_internal_lds_cache_key(d, k) for d in range(8) for k in (k1, k2)}
    assert len(set(keys.values())) == len(keys)
    if torch.cuda.device_count() >= 2:                                            # where the hardware allows: the real thing
        feats, proj, coords = _ring_problem(B=1, V=4, C=8, H=24, W=24, vol=(8, 8, 32), seed=3)
        outs = []
        for dev in ("cuda:0", "cuda:1"):
            f, p, c = (torch.from_numpy(x).to(dev) for x in (feats, proj, coords))
            outs.append(aggregation.unprojection(f, p, c, variant="brick").cpu())
        assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------ cuboid recipe evaluated in the kernels
@pytest.mark.parametrize("variant", ("brick", "gather", "auto"))
def test_cuboid_entry_is_bit_equal_to_the_coordinate_tensor_route(variant, gpu):
    """mvhmr_unproject_*_cuboid evaluates rot @ (pos + step * ijk - center) + center per voxel with the rounding order of
    mvhmr_build_coord_volumes: forward bit-equal, backward equal up to the order of the float atomics"""
    B, V, C, H, S = 3, 4, 16, 32, 32
    rng = np.random.default_rng(17)
    feats, proj, _ = _ring_problem(B=B, V=V, C=C, H=H, W=H, vol=(S, S, S), seed=17)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=C, output_channels=C, device=gpu)
    thetas = rng.uniform(0, 2 * np.pi, B)
    from multiviewhmr_amd import volumetric
    rots = torch.from_numpy(volumetric.get_rotation_matrices([0, 0, 1], thetas).astype(np.float32)).to(gpu)
    centers = torch.from_numpy(rng.normal(0, 100, (B, 3)).astype(np.float32)).to(gpu)
    coords = gen.coord_volumes(rots, centers, gpu)                              # mvhmr_build_coord_volumes
    cub = gen.cuboid()
    p = torch.from_numpy(proj).to(gpu)
    fa = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    fb = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    a = aggregation.unprojection(fa, p, coords, variant=variant)
    b = aggregation.unprojection_cuboid(fb, p, rots, centers, cub.position, cub.sides, (S, S, S), variant=variant)
    assert torch.equal(a, b)
    go = torch.randn_like(a)
    a.backward(go); b.backward(go)
    record_err("cuboid vs tensor route, bwd (%s)" % variant, float((fa.grad - fb.grad).abs().max()), 2e-5)
    ref = cport.forward(feats, proj, coords.cpu().numpy(), "softmax")
    record_err("cuboid route fwd vs oracle (%s)" % variant, _err(b.detach().cpu().numpy(), ref), TOL)


def test_packed_cameras_give_the_same_volume_without_the_camera_loop(gpu):
    d = load_golden("volgen", "train_mpii")
    gen, batch, seed = _rebuild(d, gpu)
    np.random.seed(seed)
    with torch.no_grad():
        a = gen(_dev(d, "features_in", gpu), _dev(d, "proj_org", gpu), batch)
    packed = dict(batch)
    packed["cameras_packed"] = aggregation.pack_cameras(batch["cameras"], gpu)
    packed["keypoints_3d"] = torch.from_numpy(np.stack(batch["keypoints_3d"])).to(gpu)
    del packed["cameras"]                                                        # never touched on this route
    np.random.seed(seed)
    with torch.no_grad():
        b = gen(_dev(d, "features_in", gpu), _dev(d, "proj_org", gpu), packed)
    assert torch.equal(a, b)
    record_err("volgen volume train_mpii (packed cameras)", _err(b.cpu().numpy(), d["volume"]), TOL)
    # a loader may pack the cameras on the HOST: the projections must reach the kernels as device memory
    packed["cameras_packed"] = aggregation.pack_cameras(batch["cameras"], "cpu")
    np.random.seed(seed)
    with torch.no_grad():
        c = gen(_dev(d, "features_in", gpu), _dev(d, "proj_org", gpu), packed)
    assert torch.equal(a, c)


# ------------------------------------------------------------------------------------ 1x1 conv fused with the layout pass
def test_conv1x1_to_quad_matches_conv2d_and_the_layout_pass(gpu):
    """mvhmr_conv1x1_to_quad (fp32 MFMA GEMM, epilogue in MVHMR_LAYOUT_QUAD) == nn.Conv2d followed by mvhmr_convert_features"""
    L = _capi.lib()
    torch.manual_seed(3)
    BV, Cin, Cout, H, W = 6, 48, 256, 20, 64
    x = torch.randn(BV, Cin, H, W, device=gpu)
    conv = torch.nn.Conv2d(Cin, Cout, 1).to(gpu)
    with torch.no_grad():
        y = conv(x).contiguous()                                                  # (BV, Cout, H, W)
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    assert L.mvhmr_conv1x1_to_quad_supported(Cin, Cout, H, W) == 1 and L.mvhmr_conv1x1_to_quad_supported(Cin, Cout, H, 40) == 0
    quad = torch.empty(BV * Cout * H * W, device=gpu)
    w2 = conv.weight.detach().reshape(Cout, Cin).contiguous()
    _capi.check(L.mvhmr_conv1x1_to_quad(vp(x.data_ptr()), vp(w2.data_ptr()), vp(conv.bias.data_ptr()), vp(quad.data_ptr()), BV, Cin, Cout, H, W, stream))
    ref = y.view(BV, Cout // 4, 4, H, W).permute(0, 1, 4, 3, 2).contiguous()     # (BV, C/4, W, H, 4)
    record_err("fused 1x1 conv vs nn.Conv2d", float((quad.view_as(ref) - ref).abs().max()), 2e-5 * float(ref.abs().max()) + 1e-6)
    # and the layout pass proper gives the same memory image from the planar conv output
    desc = aggregation._make_desc(y.view(1, BV, Cout, H, W), (4, 8, 32), 0, torch.float32, _capi.LAYOUT_BVCHW, _capi.VARIANT["brick"])
    conv_copy = torch.empty(L.mvhmr_feature_layout_bytes(ctypes.byref(desc), _capi.LAYOUT_QUAD) // 4, device=gpu)
    _capi.check(L.mvhmr_convert_features(ctypes.byref(desc), vp(y.data_ptr()), _capi.LAYOUT_QUAD, vp(conv_copy.data_ptr()), stream))
    assert torch.equal(conv_copy[: ref.numel()].view_as(ref), ref)


def test_conv1x1_planar_matches_matmul(gpu):
    """mvhmr_conv1x1_planar (the same MFMA GEMM with a planar epilogue; the fused route's input gradient) == W @ x (+ bias)"""
    L = _capi.lib()
    torch.manual_seed(4)
    BV, Cin, Cout, HW = 5, 80, 128, 3 * 128
    x = torch.randn(BV, Cin, HW, device=gpu)
    w = torch.randn(Cout, Cin, device=gpu) * 0.1
    b = torch.randn(Cout, device=gpu)
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    assert L.mvhmr_conv1x1_planar_supported(Cin, Cout, HW) == 1
    assert L.mvhmr_conv1x1_planar_supported(Cin, Cout, HW + 64) == 0 and L.mvhmr_conv1x1_planar_supported(Cin + 8, Cout, HW) == 0
    ref64 = torch.matmul(w.double(), x.double())
    for bias in (None, b):
        y = torch.empty(BV, Cout, HW, device=gpu)
        _capi.check(L.mvhmr_conv1x1_planar(vp(x.data_ptr()), vp(w.data_ptr()), vp(bias.data_ptr()) if bias is not None else vp(0), vp(y.data_ptr()),
                                           BV, Cin, Cout, HW, stream))
        ref = ref64 + (bias.double().view(1, -1, 1) if bias is not None else 0)
        record_err("planar 1x1 conv vs float64 matmul (bias %s)" % (bias is not None), float((y.double() - ref).abs().max()),
                   2e-6 * float(ref.abs().max()) * Cin ** 0.5 + 1e-6)
    with pytest.raises(RuntimeError):
        _capi.check(L.mvhmr_conv1x1_planar(vp(x.data_ptr()), vp(w.data_ptr()), vp(0), vp(y.data_ptr()), BV, Cin, Cout, HW + 64, stream))


def test_conv1x1_wgrad_matches_einsum(gpu):
    """mvhmr_conv1x1_wgrad (split-K MFMA GEMM + float atomics) == sum_n gy[n] @ x[n]^T and the row sums of gy, added into the outputs"""
    L = _capi.lib()
    torch.manual_seed(5)
    BV, Cin, Cout, HW = 7, 128, 256, 20 * 32
    x = torch.randn(BV, Cin, HW, device=gpu)
    gy = torch.randn(BV, Cout, HW, device=gpu)
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    assert L.mvhmr_conv1x1_wgrad_supported(Cin, Cout, HW) == 1
    assert L.mvhmr_conv1x1_wgrad_supported(Cin + 64, Cout, HW) == 0 and L.mvhmr_conv1x1_wgrad_supported(Cin, Cout, HW + 16) == 0
    ref_w = torch.einsum("nop,nip->oi", gy.double(), x.double())
    ref_b = gy.double().sum(dim=(0, 2))
    gw = torch.full((Cout, Cin), 1.0, device=gpu)                                 # "added into": starts from ones
    gb = torch.zeros(Cout, device=gpu)
    _capi.check(L.mvhmr_conv1x1_wgrad(vp(gy.data_ptr()), vp(x.data_ptr()), vp(gw.data_ptr()), vp(gb.data_ptr()), BV, Cin, Cout, HW, stream))
    K = BV * HW
    record_err("1x1 conv weight gradient vs float64 einsum", float((gw.double() - 1.0 - ref_w).abs().max()), 4e-7 * K ** 0.5 * 8 + 1e-5)
    record_err("1x1 conv bias gradient vs float64 sum", float((gb.double() - ref_b).abs().max()), 4e-7 * K ** 0.5 * 8 + 1e-5)
    gw2 = torch.zeros(Cout, Cin, device=gpu)
    _capi.check(L.mvhmr_conv1x1_wgrad(vp(gy.data_ptr()), vp(x.data_ptr()), vp(gw2.data_ptr()), vp(0), BV, Cin, Cout, HW, stream))   # no bias
    record_err("1x1 conv weight gradient (no bias) vs float64 einsum", float((gw2.double() - ref_w).abs().max()), 4e-7 * K ** 0.5 * 8 + 1e-5)


@pytest.mark.parametrize("rig", ((2, 4, 32), (6, 3, 32), (1, 6, 64)))     # (B, V, S): the last two run the brick kernels with absent views
@pytest.mark.parametrize("training", (False, True))
def test_volume_generator_fused_path_equals_the_unfused_one(training, rig, gpu, monkeypatch):
    """VolumeGenerator with the fused conv (default where the brick kernels run) against the same module with fused_conv off:
    volume, and in training the gradients of the input features, the conv weight and its bias"""
    (B, V, S), C, H, IMG = rig, 128, 32, 128
    rng = np.random.default_rng(61)
    cams = [[None] * B for _ in range(V)]
    for v in range(V):
        az = 2 * np.pi * v / V + 0.3
        eye = np.array([5000 * np.cos(az), 5000 * np.sin(az), 1500.0])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0, 0, 1.0]); right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        for b in range(B):
            cam = multiview.Camera(R, -R @ eye, [[1145.0, 0, 512], [0, 1145.0, 512], [0, 0, 1]])
            cam.update_after_crop((150, 150, 850, 850))
            cam.update_after_resize((700, 700), (IMG, IMG))
            cams[v][b] = cam
    batch = dict(images=np.zeros((B, V, IMG, IMG, 3), np.uint8), cameras=cams,
                 keypoints_3d=[rng.normal(0, 100, (17, 3)).astype(np.float32) for _ in range(B)])
    proj_org = torch.from_numpy(np.stack([[cams[v][b].projection for v in range(V)] for b in range(B)]).astype(np.float32)).to(gpu)
    torch.manual_seed(9)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=C, output_channels=C, device=gpu).train(training)
    x = torch.randn(B, V, C, H, H, device=gpu)
    outs, grads = {}, {}
    fused_calls = []
    real_apply = aggregation._FusedAggregate.apply
    monkeypatch.setattr(aggregation._FusedAggregate, "apply", lambda *a: (fused_calls.append(1), real_apply(*a))[1])
    for fused in (True, False):
        gen.fused_conv = fused
        gen.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(training)
        np.random.seed(77)
        with torch.set_grad_enabled(training):
            vol = gen(xi, proj_org, batch)
        outs[fused] = vol.detach()
        if training:
            go = torch.randn(vol.shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(5))
            vol.backward(go)
            grads[fused] = (xi.grad.clone(), gen.process_feature[0].weight.grad.clone(), gen.process_feature[0].bias.grad.clone())
    assert len(fused_calls) == 1                                                    # the fused path really ran, and only when switched on
    scale = float(outs[False].abs().max())
    record_err("fused vs unfused volume (training=%s)" % training, float((outs[True] - outs[False]).abs().max()), 2e-5 * scale + 1e-6)
    if training:
        # two fp32 summation orders of up to B*V*Hf*Wf terms: a few dozen ulps of the largest gradient (observed: ~5)
        for name, a, b in zip(("input", "weight", "bias"), grads[True], grads[False]):
            record_err("fused vs unfused grad %s" % name, float((a - b).abs().max()), 32 * 2.0 ** -23 * float(b.abs().max()) + 1e-6)


def _rig(B, V, radius, img, seed):
    rng = np.random.default_rng(seed)
    cams = [[None] * B for _ in range(V)]
    for v in range(V):
        az = 2 * np.pi * v / V + 0.3
        for b in range(B):
            eye = np.array([np.cos(az), np.sin(az), 0.0]) * radius * rng.uniform(0.95, 1.05) + np.array([0, 0, 0.3 * radius])
            fwd = -eye / np.linalg.norm(eye)
            right = np.cross(fwd, [0, 0, 1.0]); right /= np.linalg.norm(right)
            R = np.stack([right, np.cross(fwd, right), fwd])
            cam = multiview.Camera(R, -R @ eye, [[1145.0, 0, 512], [0, 1145.0, 512], [0, 0, 1]])
            cam.update_after_crop((150, 150, 850, 850))
            cam.update_after_resize((700, 700), (img, img))
            cams[v][b] = cam
    return cams


def test_fused_route_follows_the_gate_when_the_rig_changes_between_calls(gpu):
    """Same module, same shapes, two camera rigs: the fused route decides brick / gather on the device per call.
    Each call's volume is bit-equal to the explicit variant the gate's own (synchronous) query names for that rig, run on the same
    quad-planar conv output -- and the two rigs really get different answers."""
    B, V, C, H, S, IMG = 6, 4, 128, 96, 32, 384                                     # 96 bricks' worth of voxels: AUTO asks the gate
    L = _capi.lib()
    vp = ctypes.c_void_p
    torch.manual_seed(3)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=C, output_channels=C, cuboid_side=1250.0, device=gpu).eval()
    conv = gen.process_feature[0]
    x = torch.randn(B, V, C, H, H, device=gpu)
    stream = vp(torch.cuda.current_stream().cuda_stream)
    answers = []
    for radius in (5000.0, 1400.0, 5000.0):                                         # far rig, near rig, far rig again
        cams = _rig(B, V, radius, IMG, seed=int(radius))
        batch = dict(images=np.zeros((B, V, IMG, IMG, 3), np.uint8), cameras=cams,
                     keypoints_3d=[np.zeros((17, 3), np.float32) for _ in range(B)])
        proj_org = torch.from_numpy(np.stack([[cams[v][b].projection for v in range(V)] for b in range(B)]).astype(np.float32)).to(gpu)
        with torch.no_grad():
            vol = gen(x, proj_org, batch)
        # the same pieces by hand: conv -> quad copy, the gate's answer for this rig, the explicit variants on that copy
        proj = torch.from_numpy(aggregation.feature_level_projections(cams, (IMG, IMG), (H, H))).to(gpu)
        rots, centers = gen.volume_pose(batch, proj_org, (IMG, IMG))
        rots, centers = rots.to(gpu).contiguous(), centers.to(gpu).contiguous()
        cub = gen.cuboid()
        pos = (ctypes.c_double * 3)(*[float(v) for v in cub.position])
        sid = (ctypes.c_double * 3)(*[float(v) for v in cub.sides])
        quad = torch.empty(B * V * C * H * H, device=gpu)
        _capi.check(L.mvhmr_conv1x1_to_quad(vp(x.data_ptr()), vp(conv.weight.data_ptr()), vp(conv.bias.data_ptr()), vp(quad.data_ptr()),
                                            B * V, C, C, H, H, stream))
        meta = torch.empty((B, V, C, H, H), dtype=torch.float32, device="meta")
        dq = aggregation._make_desc(meta, (S, S, S), _capi.AGG["softmax"], torch.float32, _capi.LAYOUT_BVCHW, _capi.VARIANT["auto"])
        got = L.mvhmr_unproject_query_variant_cuboid(ctypes.byref(dq), vp(proj.data_ptr()), vp(rots.data_ptr()), vp(centers.data_ptr()), pos, sid, stream)
        assert got in (_capi.VARIANT["brick"], _capi.VARIANT["gather"])
        answers.append(got)
        outs = {}
        for name in ("brick", "gather"):
            d = aggregation._make_desc(meta, (S, S, S), _capi.AGG["softmax"], torch.float32, _capi.LAYOUT_QUAD, _capi.VARIANT[name])
            o = torch.empty(B, C, S, S, S, device=gpu)
            nb = L.mvhmr_unproject_forward_workspace_bytes(ctypes.byref(d))
            ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=gpu)
            _capi.check(L.mvhmr_unproject_forward_cuboid(ctypes.byref(d), vp(quad.data_ptr()), vp(proj.data_ptr()), vp(rots.data_ptr()),
                                                         vp(centers.data_ptr()), pos, sid, vp(o.data_ptr()), vp(ws.data_ptr()), nb, stream))
            outs[name] = o
        chosen = "brick" if got == _capi.VARIANT["brick"] else "gather"
        other = "gather" if chosen == "brick" else "brick"
        assert torch.equal(vol, outs[chosen]), (radius, chosen)
        assert not torch.equal(vol, outs[other]) or torch.equal(outs["brick"], outs["gather"])
        record_err("fused route, rig radius %d: %s vs the other variant" % (radius, chosen), float((outs["brick"] - outs["gather"]).abs().max()), 2e-5)
    assert answers == [_capi.VARIANT["brick"], _capi.VARIANT["gather"], _capi.VARIANT["brick"]], answers


def test_quad_planar_features_through_the_gate_backward(gpu):
    """MVHMR_LAYOUT_QUAD + AUTO in the backward: the gradient (planar) equals the one from planar features for both gate answers"""
    L = _capi.lib()
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    for shape, expect in ((dict(B=1, V=4, C=8, H=320, W=320, vol=(8, 8, 32)), "gather"), (dict(B=2, V=4, C=8, H=24, W=24, vol=(8, 8, 32)), "brick")):
        feats, proj, coords = _ring_problem(seed=5, **shape)
        f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
        p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
        out = aggregation.unprojection(f, p, c)
        go = torch.from_numpy(np.random.default_rng(9).standard_normal(tuple(out.shape), dtype=np.float32)).to(gpu)
        out.backward(go)
        d = aggregation._make_desc(f, c, _capi.AGG["softmax"], torch.float32, _capi.LAYOUT_BVCHW, _capi.VARIANT["auto"])
        quad = torch.empty(L.mvhmr_feature_layout_bytes(ctypes.byref(d), _capi.LAYOUT_QUAD), dtype=torch.uint8, device=gpu)
        _capi.check(L.mvhmr_convert_features(ctypes.byref(d), vp(f.data_ptr()), _capi.LAYOUT_QUAD, vp(quad.data_ptr()), stream))
        d.feat_layout = _capi.LAYOUT_QUAD
        assert L.mvhmr_unproject_backward_supported(ctypes.byref(d)) == 1
        o2 = torch.empty_like(out)
        nb = L.mvhmr_unproject_forward_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=gpu)
        _capi.check(L.mvhmr_unproject_forward(ctypes.byref(d), vp(quad.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(o2.data_ptr()), vp(ws.data_ptr()), nb, stream))
        assert torch.equal(o2, out.detach()), expect
        g2 = torch.empty_like(f)
        nb = L.mvhmr_unproject_backward_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=gpu)
        _capi.check(L.mvhmr_unproject_backward(ctypes.byref(d), vp(go.data_ptr()), vp(quad.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(g2.data_ptr()),
                                               vp(ws.data_ptr()), nb, stream))
        record_err("quad-planar features through the gate, bwd (%s)" % expect, float((g2 - f.grad).abs().max()), _bound(f.grad.cpu().numpy()))


# ------------------------------------------------------------------------------------ plane backward (coarse grids: no global atomics)
def _channels_last(t):
    return t.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [
    dict(B=2, V=4, C=8, H=40, W=56, vol=(12, 10, 9)),          # ragged volume (last chunk partly idle), non-square maps (Q1)
    dict(B=1, V=2, C=64, H=56, W=56, vol=(16, 16, 16)),        # BASELINE configs[0] / the reference's shipped VOLUME_SIZE
    dict(B=1, V=8, C=4, H=24, W=24, vol=(8, 8, 8)),
])
def test_plane_backward_vs_oracle_and_vs_the_scatter_kernel(shape, mode, gpu):
    """Planar features + the gather family = the plane kernel (maps fit LDS); channels-last features keep the per-tap scatter"""
    feats, proj, coords = _ring_problem(seed=13, **shape)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    go = np.random.default_rng(2).standard_normal((shape["B"], shape["C"]) + shape["vol"], dtype=np.float32)
    gref = cport.backward(go, feats, proj, coords, mode)
    grads = {}
    for layout in ("planar", "channels_last"):
        f = torch.from_numpy(feats).to(gpu)
        f = (_channels_last(f) if layout == "channels_last" else f).requires_grad_(True)
        aggregation.unprojection(f, p, c, aggregation_method=mode, variant="gather").backward(torch.from_numpy(go).to(gpu))
        grads[layout] = f.grad
        record_err("plane family bwd %s %s V%d vol%s" % (layout, mode, shape["V"], shape["vol"]), _err(f.grad.cpu().numpy(), gref), _bound(gref))
    record_err("plane vs scatter bwd %s V%d vol%s" % (mode, shape["V"], shape["vol"]), float((grads["planar"] - grads["channels_last"]).abs().max()), _bound(gref))


def test_plane_backward_rescales_when_later_voxels_bring_larger_gradients(gpu):
    """grad_out grows by 2^40 along the voxel index: the fixed-point scale of a plane comes from the max |ds| of the whole sample (the
    Jacobian pass's per-block maxima), so the result keeps the relative precision of the LARGEST contributions whatever the order of
    the walk.  32 taps per pixel on average: the finest grid the plane route takes (plane_bwd_supported)"""
    shape = dict(B=1, V=4, C=4, H=32, W=32, vol=(16, 16, 32))
    feats, proj, coords = _ring_problem(seed=17, **shape)
    n = np.arange(16 * 16 * 32, dtype=np.float64).reshape(16, 16, 32)
    go = (np.random.default_rng(3).standard_normal((1, 4, 16, 16, 32)) * 2.0 ** (n / n.max() * 40 - 20)).astype(np.float32)
    gref = cport.backward(go, feats, proj, coords, "softmax")
    f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    aggregation.unprojection(f, torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu), variant="gather").backward(torch.from_numpy(go).to(gpu))
    record_err("plane bwd, 2^40 dynamic range along the walk", _err(f.grad.cpu().numpy(), gref), 8e-6 * float(np.abs(gref).max()))


def test_config1_backward_plane_kernel(config1, gpu):
    """BASELINE configs[1] (32^3, 4 views, 256 ch, batch 8): the geometry gate sends it to the gather family, whose backward is the
    plane kernel; checked against the oracle on one sample and 8 channels, and nothing leaks into untouched channels"""
    f, p, c = config1
    f = f.clone().requires_grad_(True)
    out = aggregation.unprojection(f, p, c)
    chans = [0, 1, 2, 3, 128, 129, 254, 255]
    g = torch.zeros_like(out)
    g[5, chans] = torch.randn(len(chans), 32, 32, 32, device=gpu, generator=torch.Generator(device=gpu).manual_seed(8))
    out.backward(g)
    gref = cport.backward(g[5:6, chans].cpu().numpy(), f[5:6, :, chans].detach().cpu().numpy(), p[5:6].cpu().numpy(), c[5:6].cpu().numpy(), "softmax")
    record_err("configs[1] bwd (sample 5, 8 channels)", _err(f.grad[5:6, :, chans].cpu().numpy(), gref), _bound(gref))
    assert float(f.grad[:5].abs().max()) == 0.0 and float(f.grad[5, :, 4:128].abs().max()) == 0.0


# ------------------------------------------------------------------------------------ bf16 volume (the consumer's dtype)
@pytest.mark.parametrize("variant", VARIANTS)
def test_bf16_volume_forward_and_backward(variant, gpu):
    """out_dtype = bfloat16 with fp32 features: the volume is the fp32 result rounded once (half a bf16 ulp: up to 2^-8 relative), and the
    backward takes a bf16 grad_out: fp32 arithmetic on exactly those values (checked against the oracle fed the rounded grad_out)"""
    feats, proj, coords = _ring_problem(B=2, V=4, C=16, H=32, W=32, vol=(8, 8, 32), seed=23)
    f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    ref = cport.forward(feats, proj, coords, "softmax")
    out = aggregation.unprojection(f, p, c, out_dtype=torch.bfloat16, variant=variant)
    assert out.dtype == torch.bfloat16
    record_err("bf16 volume fwd (%s)" % variant, _err(out.float().detach().cpu().numpy(), ref), TOL + np.abs(ref).max() * 2.0 ** -8)
    o32 = aggregation.unprojection(f.detach(), p, c, variant=variant)
    assert torch.equal(out.detach(), o32.to(torch.bfloat16))                       # exactly the fp32 volume, rounded to nearest even
    go = torch.randn(out.shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(4)).to(torch.bfloat16)
    out.backward(go)
    gref = cport.backward(go.float().cpu().numpy(), feats, proj, coords, "softmax")
    assert f.grad.dtype == torch.float32
    record_err("bf16 volume bwd (%s)" % variant, _err(f.grad.cpu().numpy(), gref), _bound(gref))


def test_bf16_volume_through_the_volume_generator(gpu):
    """VolumeGenerator(volume_dtype=torch.bfloat16): fused and unfused routes give the bf16 rounding of their fp32 volumes"""
    d = load_golden("volgen", "train_mpii")
    gen, batch, seed = _rebuild(d, gpu)
    np.random.seed(seed)
    with torch.no_grad():
        a = gen(_dev(d, "features_in", gpu), _dev(d, "proj_org", gpu), batch)
    gen.volume_dtype = torch.bfloat16
    np.random.seed(seed)
    with torch.no_grad():
        b = gen(_dev(d, "features_in", gpu), _dev(d, "proj_org", gpu), batch)
    assert b.dtype == torch.bfloat16 and torch.equal(b, a.to(torch.bfloat16))
    record_err("volgen bf16 volume train_mpii", _err(b.float().cpu().numpy(), d["volume"]), TOL + np.abs(d["volume"]).max() * 2.0 ** -8)
    with pytest.raises(RuntimeError):                                              # bf16 is not a feature storage type
        aggregation.unprojection(_dev(d, "features_in", gpu).to(torch.bfloat16)[:, :, :4], _dev(d, "proj_org", gpu),
                                 torch.zeros(a.shape[0], 4, 4, 4, 3, device=gpu))


def test_unprojection_traces_under_torch_compile(gpu):
    """The op is a torch.library custom op: AOT autograd (torch.compile, backend aot_eager: no code generator involved) captures
    forward and backward as single nodes; the results are the eager ones bit for bit"""
    feats, proj, coords = _ring_problem(B=2, V=4, C=8, H=24, W=24, vol=(8, 8, 32), seed=31)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)

    def fn(f):
        return aggregation.unprojection(2.0 * f, p, c, aggregation_method="softmax").sum(dim=1)

    fe = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    oe = fn(fe)
    go = torch.randn_like(oe)
    oe.backward(go)
    fc = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    oc = torch.compile(fn, backend="aot_eager", fullgraph=True)(fc)
    oc.backward(go)
    assert torch.equal(oc, oe)
    record_err("torch.compile (aot_eager) vs eager, grad", float((fc.grad - fe.grad).abs().max()), 1e-5)


def test_plane_backward_storage_modes_and_quad_planar_features(gpu):
    """The plane kernel behind every storage mode the gather family serves, and fed the caller's own quad-planar copy"""
    shape = dict(B=2, V=4, C=8, H=40, W=56, vol=(12, 10, 9))
    feats, proj, coords = _ring_problem(seed=19, **shape)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    go = np.random.default_rng(6).standard_normal((2, 8, 12, 10, 9), dtype=np.float32)
    # fp16 storage throughout
    f16 = torch.from_numpy(feats).to(gpu).half().requires_grad_(True)
    g16 = torch.from_numpy(go).to(gpu).half()
    aggregation.unprojection(f16, p, c, variant="gather").backward(g16)
    gref = cport.backward(g16.float().cpu().numpy(), f16.detach().float().cpu().numpy(), proj, coords, "softmax")
    record_err("plane bwd, fp16 storage", _err(f16.grad.float().cpu().numpy(), gref), TOL + np.abs(gref).max() * 2.0 ** -10)
    # fp16 features, fp32 volume / grad_out
    f16b = torch.from_numpy(feats).to(gpu).half().requires_grad_(True)
    aggregation.unprojection(f16b, p, c, variant="gather", out_dtype=torch.float32).backward(torch.from_numpy(go).to(gpu))
    gref = cport.backward(go, f16b.detach().float().cpu().numpy(), proj, coords, "softmax")
    record_err("plane bwd, fp16 features + fp32 grad_out", _err(f16b.grad.float().cpu().numpy(), gref), TOL + np.abs(gref).max() * 2.0 ** -10)
    # fp32 features, bf16 grad_out
    f32 = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    gb = torch.from_numpy(go).to(gpu).to(torch.bfloat16)
    aggregation.unprojection(f32, p, c, variant="gather", out_dtype=torch.bfloat16).backward(gb)
    gref = cport.backward(gb.float().cpu().numpy(), feats, proj, coords, "softmax")
    record_err("plane bwd, bf16 grad_out", _err(f32.grad.cpu().numpy(), gref), _bound(gref))
    # the caller's quad-planar copy, explicit gather variant: no layout pass at all in the backward
    L = _capi.lib()
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    f = torch.from_numpy(feats).to(gpu)
    d = aggregation._make_desc(f, c, _capi.AGG["softmax"], torch.float32, _capi.LAYOUT_BVCHW, _capi.VARIANT["gather"])
    quad = torch.empty(L.mvhmr_feature_layout_bytes(ctypes.byref(d), _capi.LAYOUT_QUAD), dtype=torch.uint8, device=gpu)
    _capi.check(L.mvhmr_convert_features(ctypes.byref(d), vp(f.data_ptr()), _capi.LAYOUT_QUAD, vp(quad.data_ptr()), stream))
    d.feat_layout = _capi.LAYOUT_QUAD
    g = torch.empty_like(f)
    nb = L.mvhmr_unproject_backward_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=gpu)
    got = torch.from_numpy(go).to(gpu)
    _capi.check(L.mvhmr_unproject_backward(ctypes.byref(d), vp(got.data_ptr()), vp(quad.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(g.data_ptr()),
                                           vp(ws.data_ptr()), nb, stream))
    gref = cport.backward(go, feats, proj, coords, "softmax")
    record_err("plane bwd from quad-planar features", _err(g.cpu().numpy(), gref), _bound(gref))


def test_dlt_triangulation_kernel_matches_the_svd(gpu):
    """mvhmr_triangulate_dlt (SVD-free, on the device) against numpy's float64 SVD per sample (the reference's formulation,
    utils/multiview.py:112-139) on ring rigs with 2, 4 and 8 views, exact and noisy image points"""
    rng = np.random.default_rng(12)
    for V in (2, 4, 8):
        P = bench_projections(6, V)
        X = rng.uniform(-800, 800, (6, 3))
        hom = np.concatenate([X, np.ones((6, 1))], 1)
        for noise in (0.0, 1.5):
            got_all = []
            for b in range(6):
                r = np.einsum("vij,j->vi", P[b].astype(np.float64), hom[b])
                uv = r[:, :2] / r[:, 2:3] + rng.normal(0, noise, (V, 2))
                ref = multiview.triangulate_point_from_multiple_views_linear(P[b].astype(np.float64), uv)
                got = multiview.triangulate_points_from_multiple_views_linear_batch(torch.from_numpy(P[b:b + 1]).to(gpu),
                                                                                    torch.from_numpy(uv.astype(np.float32)).to(gpu))[0].cpu().numpy()
                ref32 = multiview.triangulate_point_from_multiple_views_linear(P[b].astype(np.float64), uv.astype(np.float32).astype(np.float64))
                got_all.append(np.abs(got - ref32).max())
                if noise == 0.0:
                    assert np.abs(ref - X[b]).max() < 1e-2
            record_err("DLT kernel vs float64 SVD (mm), V=%d noise=%.1f" % (V, noise), float(max(got_all)), 2e-3)


def bench_projections(B, V):
    import bench
    return bench.ring_projections(B, V, (96, 96), seed=5)


def test_weighted_dlt_kernel_matches_the_reference_formulation(gpu):
    """mvhmr_triangulate_dlt_weighted: rows of view v times c_v (utils/multiview.py:156-161) -- against the torch mirror of the reference
    (float64 SVD of the weighted system) per sample, with per-sample points and per-sample confidences; a view with confidence 0
    drops out (its outlier observation no longer moves the point)"""
    rng = np.random.default_rng(21)
    B, V = 5, 4
    P = bench_projections(B, V)
    X = rng.uniform(-800, 800, (B, 3))
    hom = np.concatenate([X, np.ones((B, 1))], 1)
    r = np.einsum("bvij,bj->bvi", P.astype(np.float64), hom)
    uv = (r[..., :2] / r[..., 2:3] + rng.normal(0, 1.0, (B, V, 2))).astype(np.float32)
    conf = rng.uniform(0.2, 1.0, (B, V)).astype(np.float32)
    got = multiview.triangulate_points_from_multiple_views_linear_batch(torch.from_numpy(P).to(gpu), torch.from_numpy(uv).to(gpu), torch.from_numpy(conf).to(gpu)).cpu().numpy()
    worst = 0.0
    for b in range(B):
        ref = multiview.triangulate_point_from_multiple_views_linear_torch(torch.from_numpy(P[b].astype(np.float64)), torch.from_numpy(uv[b].astype(np.float64)),
                                                                          torch.from_numpy(conf[b].astype(np.float64))).numpy()
        worst = max(worst, float(np.abs(got[b] - ref).max()))
    record_err("weighted DLT kernel vs float64 SVD of the weighted system (mm)", worst, 2e-3)
    # shared confidences (V,), one view switched off: its 300 px outlier must not matter
    uv2 = uv.copy(); uv2[:, 2] += 300.0
    c0 = torch.tensor([1.0, 1.0, 0.0, 1.0])
    a = multiview.triangulate_points_from_multiple_views_linear_batch(torch.from_numpy(P).to(gpu), torch.from_numpy(uv2).to(gpu), c0.to(gpu)).cpu().numpy()
    bb = multiview.triangulate_points_from_multiple_views_linear_batch(torch.from_numpy(P).to(gpu), torch.from_numpy(uv).to(gpu), c0.to(gpu)).cpu().numpy()
    record_err("weighted DLT: a zero-confidence view drops out (mm)", float(np.abs(a - bb).max()), 1e-3)
    # CPU mirror (no GPU) takes the same arguments
    cpu = multiview.triangulate_points_from_multiple_views_linear_batch(torch.from_numpy(P), torch.from_numpy(uv), torch.from_numpy(conf)).numpy()
    record_err("weighted DLT: device kernel vs the CPU mirror (mm)", float(np.abs(cpu - got).max()), 2e-3)


def test_plane_backward_poisons_when_a_channel_has_only_non_finite_gradients(gpu):
    """A channel whose grad_out is NaN wherever it is not zero has no finite magnitude to scale by: its NaN contributions must still
    reach exactly their pixels (and a finite gradient so large that the int32 bound overflows fp32 is carried by the 64-bit form)"""
    shape = dict(B=1, V=4, C=4, H=24, W=24, vol=(8, 8, 8))
    feats, proj, coords = _ring_problem(seed=41, **shape)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    go = np.zeros((1, 4, 8, 8, 8), np.float32)
    go[0, 1, 3, 4, 5] = np.nan                                                  # channel 1: one NaN, everything else zero
    go[0, 2] = np.random.default_rng(1).standard_normal((8, 8, 8)).astype(np.float32)
    grads = {}
    for layout in ("planar", "channels_last"):                                   # plane kernel / per-tap scatter
        f = torch.from_numpy(feats).to(gpu)
        f = (_channels_last(f) if layout == "channels_last" else f).requires_grad_(True)
        aggregation.unprojection(f, p, c, variant="gather").backward(torch.from_numpy(go).to(gpu))
        grads[layout] = f.grad
    a, b = grads["planar"], grads["channels_last"]
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and bool(torch.isnan(a[0, :, 1]).any())      # the same pixels, and there are some
    assert not bool(torch.isnan(a[0, :, 0]).any()) and not bool(torch.isnan(a[0, :, 2]).any())
    record_err("plane vs scatter bwd next to a NaN channel", float((a[0, :, 2] - b[0, :, 2]).abs().max()), 1e-5)
    huge = np.zeros_like(go)
    huge[0, 0, 2, 2, 2] = 3e38                                                   # times the tap multiplicity the int32 bound overflows fp32:
    f = torch.from_numpy(feats).to(gpu).requires_grad_(True)                     # the 64-bit form carries it (round 3 wrote NaN there)
    aggregation.unprojection(f, p, c, variant="gather").backward(torch.from_numpy(huge).to(gpu))
    gref = cport.backward(huge, feats, proj, coords, "softmax")
    assert np.isfinite(gref).all() and float(np.abs(gref).max()) > 1e36
    assert bool(torch.isfinite(f.grad).all())
    record_err("plane bwd, one 3e38 gradient (finite: carried, not poisoned)", _err(f.grad.cpu().numpy(), gref), 8e-6 * float(np.abs(gref).max()))


# ------------------------------------------------------------------------------------ the reference's shipped configuration
# cfg/defaults.py:18,24-25 + cfg/baseline.yaml:28-34: VOLUME_SIZE = 16, DECONV_LAYERS = 0 -> 2048 input channels on stride-32 maps
# (12 x 12 for 384 px crops, 8 x 8 for 256 px), VOLUME_CHANNEL 256, 4 views.  16^3 is not brick-divisible (gather forward); its 4 bricks
# per sample would leave the brick backward on 1 / 64 of the chip per sample, so AUTO takes the plane backward, whose planes sum
# ~114 taps per pixel there: the 64-bit form.
@pytest.mark.parametrize("hw", [12, 8])
def test_shipped_config_unprojection_vs_oracle(hw, gpu):
    shape = dict(B=2, V=4, C=256, H=hw, W=hw, vol=(16, 16, 16))
    feats, proj, coords = _ring_problem(seed=40 + hw, **shape)
    f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    out = aggregation.unprojection(f, p, c)
    ref = cport.forward(feats, proj, coords, "softmax")
    record_err("shipped config 16^3 x 256 ch, %dx%d maps, fwd" % (hw, hw), _err(out.detach().cpu().numpy(), ref), TOL)
    go = np.random.default_rng(6).standard_normal(ref.shape, dtype=np.float32)
    out.backward(torch.from_numpy(go).to(gpu))
    gref = cport.backward(go, feats, proj, coords, "softmax")
    # ~114 (12 x 12) / ~256 (8 x 8) taps per pixel: the bound is a few fp32 ulps of the largest gradient, as for every summed gradient
    record_err("shipped config 16^3 x 256 ch, %dx%d maps, bwd (plane kernel, 64-bit sums)" % (hw, hw), _err(f.grad.cpu().numpy(), gref), _bound(gref))
    # the brick backward, forced, agrees
    f2 = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    aggregation.unprojection(f2, p, c, variant="brick" if _brick_ok(f2, c) else "auto").backward(torch.from_numpy(go).to(gpu))
    record_err("shipped config %dx%d maps, bwd twice" % (hw, hw), float((f2.grad - f.grad).abs().max()), _bound(gref))


def test_shipped_config_volume_generator(gpu):
    """VolumeGenerator as build_volume_generator wires it for the shipped cfg (2048 -> 256 conv, 16^3, cuboid 2500 mm), eval pose:
    the volume and the gradient w.r.t. the input features against nn.functional.conv2d + the C oracle"""
    B, V, Cin, Cout, S, hw, IMG = 2, 4, 2048, 256, 16, 12, 384
    cams = _rig(B, V, 5000.0, IMG, seed=9)
    batch = dict(images=np.zeros((B, V, IMG, IMG, 3), np.uint8), cameras=cams,
                 keypoints_3d=[np.random.default_rng(b).normal(0, 100, (17, 3)).astype(np.float32) for b in range(B)])
    proj_org = torch.from_numpy(np.stack([[cams[v][b].projection for v in range(V)] for b in range(B)]).astype(np.float32)).to(gpu)
    torch.manual_seed(3)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=Cin, output_channels=Cout, cuboid_side=2500.0, device=gpu).eval()
    feats = torch.randn(B, V, Cin, hw, hw, device=gpu, requires_grad=True)
    vol = gen(feats, proj_org, batch)
    assert tuple(vol.shape) == (B, Cout, S, S, S) and vol.dtype == torch.float32
    # the same through plain torch + the oracle (eval: theta = 0, cuboid centred on the world origin, Q4)
    w, bias = gen.process_feature[0].weight.detach(), gen.process_feature[0].bias.detach()
    conv = torch.nn.functional.conv2d(feats.detach().reshape(B * V, Cin, hw, hw), w, bias).reshape(B, V, Cout, hw, hw)
    P = aggregation.feature_level_projections(cams, (IMG, IMG), (hw, hw)).astype(np.float32)
    g = np.stack(np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij"), -1).astype(np.float32)
    coords = (np.float32(-1250.0) + np.float32(2500.0 / (S - 1)) * g).astype(np.float32)
    coords = np.broadcast_to(coords, (B,) + coords.shape).copy()
    conv_np = conv.cpu().numpy()
    ref = cport.forward(conv_np, P, coords, "softmax")
    # the conv sums 2048 products in an order of its own: a few dozen ulps of its largest output on top of the path's bar
    slack = 64 * 2.0 ** -23 * float(np.abs(conv_np).max())
    record_err("shipped cfg VolumeGenerator fwd (2048 -> 256, 16^3, 12x12)", _err(vol.detach().cpu().numpy(), ref), TOL + slack)
    go = torch.randn(vol.shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(5))
    vol.backward(go)
    gconv = cport.backward(go.cpu().numpy(), conv_np, P, coords, "softmax")
    gfeat_ref = torch.nn.functional.conv_transpose2d(torch.from_numpy(gconv).reshape(B * V, Cout, hw, hw).to(gpu), w).reshape(B, V, Cin, hw, hw)
    record_err("shipped cfg VolumeGenerator bwd w.r.t. the input features", float((feats.grad - gfeat_ref).abs().max()),
               64 * 2.0 ** -23 * float(gfeat_ref.abs().max()) + 1e-4)


# ------------------------------------------------------------------------------------ plane backward: concentrated projections, outliers
def _far_rig_problem(B, V, C, H, W, vol, seed, radius=60000.0):
    """a rig so far away that the whole volume lands on a few pixels of every map: hundreds of taps per pixel"""
    feats, proj, coords = _ring_problem(B, V, C, H, W, vol, seed)
    for b in range(B):
        for v in range(V):
            az = 2 * np.pi * v / V + 0.3
            eye = np.array([radius * np.cos(az), radius * np.sin(az), 0.3 * radius])
            fwd = -eye / np.linalg.norm(eye)
            right = np.cross(fwd, [0, 0, 1.0]); right /= np.linalg.norm(right)
            R = np.stack([right, np.cross(fwd, right), fwd])
            cam = multiview.Camera(R, -R @ eye, [[1145.0, 0, 512], [0, 1145.0, 512], [0, 0, 1]])
            cam.update_after_resize((1024, 1024), (W, H))
            proj[b, v] = cam.projection
    return feats, proj, coords


@pytest.mark.parametrize("mode", ("softmax", "sum"))
def test_plane_backward_concentrated_projection_with_an_outlier(mode, gpu):
    """a far camera puts the whole volume on a few pixels (tap multiplicity in the thousands) and one voxel of grad_out is
    2^20 larger than the rest.  The error is measured PER VIEW against that view's own largest gradient, with the outlier's pixels
    left out of a second measurement so that the quiet part of the plane has to be right as well."""
    shape = dict(B=1, V=4, C=8, H=48, W=48, vol=(24, 24, 24))
    feats, proj, coords = _far_rig_problem(seed=23, **shape)
    go = np.random.default_rng(4).standard_normal((1, 8, 24, 24, 24), dtype=np.float32)
    go_out = go.copy()
    go_out[0, :, 5, 7, 11] *= 2.0 ** 20
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    for name, g in (("plain", go), ("outlier", go_out)):
        gref = cport.backward(g, feats, proj, coords, mode)
        f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
        aggregation.unprojection(f, p, c, aggregation_method=mode, variant="gather").backward(torch.from_numpy(g).to(gpu))
        got = f.grad.cpu().numpy()
        for v in range(4):
            m = float(np.abs(gref[0, v]).max())
            record_err("plane bwd far rig %s %s view %d (rel. to the view's max %.3g)" % (mode, name, v, m), _err(got[0, v], gref[0, v]), 8e-6 * m)
    # the quiet pixels under the outlier: everything the outlier voxel does not touch must match the run without it to the resolution
    # of the fixed point (2^-31 of the view's max |ds| per contribution, 64-bit sums), i.e. stay within the plain run's own bound
    gq = cport.backward(go, feats, proj, coords, mode)
    go_only = np.zeros_like(go); go_only[0, :, 5, 7, 11] = go_out[0, :, 5, 7, 11] - go[0, :, 5, 7, 11]
    touched = cport.backward(go_only, feats, proj, coords, "sum") != 0            # pixels the outlier voxel reaches (any mode: same taps)
    quiet = ~touched
    if mode == "sum":                                                            # linear: the outlier leaves the quiet pixels alone exactly
        err = float(np.abs(got - gq)[quiet].max())
        # resolution there: 2^-31 * max |ds| of the view (2^20 larger now) per contribution, thousands of contributions per pixel
        record_err("plane bwd far rig sum, quiet pixels beside a 2^20 outlier", err, 2.0 ** 20 * 2.0 ** -31 * 4096 * float(np.abs(go).max()) + 1e-4)


# ------------------------------------------------------------------------------------ full-tensor parity at the headline size
def _max_diff_chunked(a, b, chunk=4):
    """max |a - b| over two (B, C, X, Y, Z) device tensors without a full-size temporary"""
    worst = 0.0
    for i in range(0, a.shape[0], chunk):
        worst = max(worst, float((a[i:i + chunk].float() - b[i:i + chunk].float()).abs().max()))
    return worst


def test_northstar_full_tensor_brick_vs_gather_with_the_bench_rigs(gpu):
    """the headline workload exactly as bench.py builds it (per-sample camera radii, bench.ring_projections), every one
    of the 32 x 256 channel planes: the brick kernels (LDS windows, parity split, z-run lane map) against the gather kernels (one wave
    per voxel, channels-last rows) -- two decompositions that share only make_taps.  The oracle pins a slice."""
    import bench
    B, V, C, H, S = 32, 4, 256, 96, 64
    torch.manual_seed(0)
    f = torch.randn(B, V, C, H, H, device=gpu)
    P = bench.ring_projections(B, V, (H, H), seed=0)
    coords_np = bench.cuboid_volume(1, S)
    p = torch.from_numpy(P).to(gpu)
    c = torch.from_numpy(coords_np).to(gpu).expand(B, S, S, S, 3).contiguous()
    out_b = aggregation.unprojection(f, p, c, variant="brick")
    out_g = aggregation.unprojection(f, p, c, variant="gather")
    # same taps, same weights; the bilinear sum runs in another order for odd rows (brick_fwd_kernel.h) and the softmax relative to
    # view 0 instead of the maximum: a few ulps of values of magnitude ~5
    record_err("north star, all 32 x 256 planes: brick vs gather fwd", _max_diff_chunked(out_b, out_g), 1e-5)
    for b in (0, 17, 31):                                                          # different radii per sample
        err, ref = _oracle_on_channels(f, p, c, out_b, [3, 200], b=b)
        record_err("north star bench rig, sample %d, 2 channels vs oracle" % b, err, TOL)
    del out_g
    # backward: grad_out = the forward output; brick (LDS fixed point + float atomics) vs gather (per-tap float atomics)
    go = out_b
    gb = aggregation._op_backward(go, f, p, c, 0, _capi.F32, _capi.VARIANT["brick"])
    gg = aggregation._op_backward(go, f, p, c, 0, _capi.F32, _capi.VARIANT["gather"])
    m = float(gg.abs().max())
    record_err("north star, all 32 x 4 x 256 gradient planes: brick vs gather bwd (largest %.3g)" % m, _max_diff_chunked(gb, gg), 8e-6 * m + 1e-5)


def test_northstar_full_tensor_cuboid_route_rotated(gpu):
    """The cuboid route (voxel centres evaluated in the kernels) at the headline size with theta != 0 and per-sample pivots, as
    VolumeGenerator drives it in training: brick vs gather over the whole tensor, and against the tensor route on coordinates
    materialised by mvhmr_build_coord_volumes (bit-equal centres: the two routes must agree exactly, kernel by kernel)"""
    import bench
    from multiviewhmr_amd import volumetric
    B, V, C, H, S = 32, 4, 256, 96, 64
    torch.manual_seed(1)
    rng = np.random.default_rng(11)
    f = torch.randn(B, V, C, H, H, device=gpu)
    p = torch.from_numpy(bench.ring_projections(B, V, (H, H), seed=3)).to(gpu)
    thetas = rng.uniform(0.0, 2 * np.pi, B)
    rots = torch.from_numpy(np.stack([volumetric.get_rotation_matrix([0, 0, 1], t) for t in thetas]).astype(np.float32)).to(gpu)
    centers = torch.from_numpy(rng.normal(0, 100, (B, 3)).astype(np.float32)).to(gpu)
    position, sides = (-1250.0, -1250.0, -1250.0), (2500.0, 2500.0, 2500.0)
    kw = dict(position=position, sides=sides, volume_shape=(S, S, S))
    out_b = aggregation.unprojection_cuboid(f, p, rots, centers, variant="brick", **kw)
    out_g = aggregation.unprojection_cuboid(f, p, rots, centers, variant="gather", **kw)
    record_err("north star cuboid route, theta != 0, all planes: brick vs gather fwd", _max_diff_chunked(out_b, out_g), 1e-5)
    del out_g
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=2500.0, device=gpu)
    assert tuple(gen.cuboid().position) == position and tuple(gen.cuboid().sides) == sides
    coords = gen.coord_volumes(rots, centers, gpu)                                 # mvhmr_build_coord_volumes
    out_t = aggregation.unprojection(f, p, coords, variant="brick")
    assert torch.equal(out_t, out_b)                                               # same centres, same kernel: bit-equal
    err, ref = _oracle_on_channels(f, p, coords, out_b, [0, 131], b=9)
    record_err("north star cuboid route, sample 9, 2 channels vs oracle", err, TOL)


@pytest.mark.parametrize("seed,big", [(1, False), (22, False), (5, True), (101, False), (201, False)])
def test_fuzz_parity_fixed_seeds(seed, big, gpu):
    """fixed seeds of scripts/fuzz_parity.py (random rigs incl. rolled ones, cuboids, volumes, maps, every variant, forward +
    backward against the C oracle); seed 22 is the one that found the fine-grid plane route in round 3; seeds >= 100 draw the view
    counts without kernels of their own (1, 3, 5, 6, 7), seeds >= 200 any view count, any volume extents and 8 ... 16 channel quads"""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(os.path.dirname(os.path.dirname(__file__)), "scripts", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    n, worst = fz.run(seed=seed, cases=16 if big else 24, big=big, verbose=False)
    record_err("fuzz seed %d%s: %d runs, worst error / bound" % (seed, " --big" if big else "", n), worst, 1.0)


# ------------------------------------------------------------------------------------ (f)3: the consumer's first stage on a bf16 volume
def test_bf16_volume_through_the_regressors_first_stage(gpu):
    """VolumeGenerator(volume_dtype=bfloat16) feeding the encoder's first stage -- Conv3d(256 -> 128, 3) + BatchNorm3d
    + ReLU (models/regressor.py:26-32,78-80) -- under autocast, and back: the gradient w.r.t. the input features against the fp32
    route with the bf16 bound (the volume and its gradient are rounded to 8 bits once each)."""
    B, V, C, H, S, IMG = 2, 4, 256, 32, 32, 128
    cams = _rig(B, V, 5000.0, IMG, seed=4)
    batch = dict(images=np.zeros((B, V, IMG, IMG, 3), np.uint8), cameras=cams,
                 keypoints_3d=[np.random.default_rng(b).normal(0, 100, (17, 3)).astype(np.float32) for b in range(B)])
    proj_org = torch.from_numpy(np.stack([[cams[v][b].projection for v in range(V)] for b in range(B)]).astype(np.float32)).to(gpu)
    torch.manual_seed(8)
    stage = torch.nn.Sequential(torch.nn.Conv3d(C, 128, 3, padding=1), torch.nn.BatchNorm3d(128), torch.nn.ReLU(True)).to(gpu).train()
    x = torch.randn(B, V, C, H, H, device=gpu)
    go = torch.randn(B, 128, S, S, S, device=gpu) / (B * 128 * S ** 3) ** 0.5
    grads, vols = {}, {}
    # three routes: fp32 volume + fp32 stage | bf16 volume from the kernels + autocast stage | fp32 volume rounded by torch + autocast stage
    for route in ("fp32", "bf16", "fp32->bf16"):
        torch.manual_seed(9)
        dt = torch.bfloat16 if route == "bf16" else torch.float32
        gen = aggregation.VolumeGenerator(volume_size=S, input_channels=C, output_channels=C, device=gpu, volume_dtype=dt).eval()
        xi = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=route != "fp32"):
            vol = gen(xi, proj_org, batch)
            assert vol.dtype == dt
            y = stage(vol.to(torch.bfloat16) if route == "fp32->bf16" else vol)
        y.float().backward(go)
        grads[route], vols[route] = xi.grad.clone(), vol.detach().float()
        stage.zero_grad(set_to_none=True)
    vm = float(vols["fp32"].abs().max())
    record_err("bf16 volume vs fp32 volume (consumer test)", float((vols["bf16"] - vols["fp32"]).abs().max()), vm * 2.0 ** -8 + 1e-4)
    assert torch.equal(vols["bf16"], vols["fp32"].to(torch.bfloat16).float())      # the kernels' bf16 volume IS the fp32 volume rounded once
    # so the consumer sees identical inputs on the last two routes and hands back identical bf16 gradients: the feature gradients may
    # differ only by the order of the float atomics
    gm = float(grads["fp32->bf16"].abs().max())
    record_err("bf16 volume route vs fp32 volume rounded by torch: gradient w.r.t. the features (largest %.3g)" % gm,
               float((grads["bf16"] - grads["fp32->bf16"]).abs().max()), 8e-6 * gm + 1e-7)
    # against the all-fp32 route the difference is the consumer's own bf16 arithmetic (conv inputs, BatchNorm statistics, ReLU masks)
    rel = float((grads["bf16"] - grads["fp32"]).norm() / grads["fp32"].norm())
    record_err("bf16 consumer route vs the all-fp32 route: relative L2 error of the feature gradient", rel, 0.1)


def test_layout_pass_takes_misaligned_feature_pointers(gpu):
    """features that are a slice of a flat buffer start at an odd element -- the layout pass must not use its 16-byte /
    8-byte vector loads on them.  Same values, shifted storage: bit-equal results"""
    shape = dict(B=1, V=4, C=8, H=32, W=32, vol=(8, 8, 32))
    feats, proj, coords = _ring_problem(seed=77, **shape)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    for dt in (torch.float32, torch.float16):
        f = torch.from_numpy(feats).to(gpu).to(dt)
        flat = torch.empty(f.numel() + 3, device=gpu, dtype=dt)
        outs = []
        for off in (0, 1, 3):
            fo = flat[off:off + f.numel()].view_as(f)
            fo.copy_(f)
            assert fo.is_contiguous() and fo.data_ptr() == flat.data_ptr() + off * f.element_size()
            fo = fo.detach().requires_grad_(True)
            out = aggregation.unprojection(fo, p, c, variant="brick")
            out.float().sum().backward()
            outs.append((out.detach().clone(), fo.grad.clone()))
        for o, g in outs[1:]:
            assert torch.equal(o, outs[0][0])
            record_err("misaligned features (%s): gradient vs the aligned run" % str(dt), float((g.float() - outs[0][1].float()).abs().max()), 1e-3 * float(outs[0][1].float().abs().max()))


# ------------------------------------------------------------------------------------ round 5: the wave-specialised forward (k_fwd_ws)
def _ws_desc(f, c, mode, layout=_capi.LAYOUT_BVCHW, variant="brick"):
    return aggregation._make_desc(f, tuple(c.shape[1:4]), _capi.AGG[mode], torch.float32, layout, _capi.VARIANT[variant])


@pytest.mark.parametrize("shape", [
    dict(B=16, V=4, C=8, H=48, W=48, vol=(32, 32, 32)),       # 256 bricks: whole bricks, two quads (both window buffers, the odd-quad offset)
    dict(B=9, V=4, C=12, H=40, W=56, vol=(20, 36, 44)),       # ragged in x, y and z (z % 4 == 0), odd number of quads, non-square maps
    dict(B=9, V=3, C=8, H=40, W=40, vol=(20, 36, 44)),        # three views on the four-view kernel: the fourth absent
    dict(B=4, V=4, C=4, H=400, W=400, vol=(64, 64, 32)),      # huge maps: no brick's windows fit -> the compute waves' global-memory path
    dict(B=5, V=4, C=8, H=96, W=96, vol=(64, 64, 32)),        # the north star's geometry (1.45 px per voxel): rounded and unrounded windows
])
@pytest.mark.parametrize("mode", MODES)
def test_wave_specialised_forward_vs_oracle(shape, mode, gpu):
    """launches of >= 256 bricks with 3 / 4 views and an fp32 volume run k_fwd_ws (brick_fwd_ws.h): memory waves + compute waves,
    results through LDS; its softmax reads a log2(e)-prescaled copy (mvhmr_preferred_layout says so)"""
    feats, proj, coords = _ring_problem(seed=31 + MODES.index(mode), **shape)
    f, p, c = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    d = _ws_desc(f, c, mode)
    lay = _capi.lib().mvhmr_preferred_layout(ctypes.byref(d))
    assert lay == (_capi.LAYOUT_QUAD_LOG2E if mode == "softmax" else _capi.LAYOUT_QUAD)    # i.e. this shape runs k_fwd_ws
    out = aggregation.unprojection(f, p, c, aggregation_method=mode, variant="brick")
    ref = cport.forward(feats, proj, coords, mode)
    name = "ws fwd %s V%d C%d %dx%d vol%s" % (mode, shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"])
    record_err(name, _err(out.cpu().numpy(), ref), TOL)
    assert torch.equal(out, aggregation.unprojection(f, p, c, aggregation_method=mode, variant="brick"))   # deterministic
    gat = aggregation.unprojection(f, p, c, aggregation_method=mode, variant="gather")
    # sum / mean / max: the same samples in the same order; softmax: exp2 of prescaled samples against exp of the samples
    record_err(name + " vs gather", float((out - gat).abs().max()), 4e-6 if mode == "softmax" else 1e-6)
    auto = aggregation.unprojection(f, p, c, aggregation_method=mode, variant="auto")        # through the device-side gate
    record_err(name + " auto", _err(auto.cpu().numpy(), ref), TOL)


@pytest.mark.parametrize("shape", [
    dict(B=16, V=4, C=8, H=48, W=48, vol=(32, 32, 32)),       # whole bricks
    dict(B=9, V=3, C=12, H=40, W=56, vol=(20, 35, 40)),       # ragged in x, y (an odd row pair at the y edge) and z (z % 8 == 0), absent view
    dict(B=4, V=4, C=4, H=400, W=400, vol=(64, 64, 32)),      # windows never fit: the compute waves' global-memory path stores 16-bit too
])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_wave_specialised_forward_16_bit_volumes(shape, mode, dt, gpu):
    """k_fwd_ws with a 16-bit volume: the memory waves round the fp32 results once (8 per lane, one 16-B store): the volume is the fp32
    volume of the same kernel rounded to nearest even, bit for bit; fp16 / bf16 features are widened by the layout pass as for k_fwd_brick"""
    feats, proj, coords = _ring_problem(seed=57 + MODES.index(mode), **shape)
    f, p, c = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    # the two 16-bit storage modes of the ABI: fp16 features -> fp16 volume (autocast), fp32 features -> bf16 volume (VolumeGenerator.volume_dtype)
    fin = f.half() if dt == torch.float16 else f
    d = aggregation._make_desc(fin, tuple(c.shape[1:4]), _capi.AGG[mode], dt, _capi.LAYOUT_BVCHW, _capi.VARIANT["brick"])
    assert _capi.lib().mvhmr_unproject_forward_kernel_name(ctypes.byref(d)) == b"k_fwd_ws"
    o32 = aggregation.unprojection(fin, p, c, aggregation_method=mode, variant="brick", out_dtype=torch.float32)
    out16 = aggregation.unprojection(fin, p, c, aggregation_method=mode, variant="brick", out_dtype=dt)
    assert out16.dtype == dt and torch.equal(out16, o32.to(dt))
    ref = cport.forward(fin.float().cpu().numpy(), proj, coords, mode)
    name = "ws fwd %s storage %s V%d vol%s" % (mode, str(dt).split(".")[1], shape["V"], shape["vol"])
    tol16 = (2.0 ** -10 if dt == torch.float16 else 2.0 ** -7) * max(1.0, float(np.abs(ref).max()))
    record_err(name + " (fp32 volume)", _err(o32.cpu().numpy(), ref), TOL)
    record_err(name, float((out16.float().cpu() - torch.from_numpy(ref).to(dt).float()).abs().max()), tol16)
    auto = aggregation.unprojection(fin, p, c, aggregation_method=mode, variant="auto", out_dtype=dt)   # the gate sends the shape whose windows never fit to k_fwd_gather
    record_err(name + " auto", float((auto.float().cpu() - torch.from_numpy(ref).to(dt).float()).abs().max()), tol16)
    if shape["H"] < 400: assert torch.equal(auto, out16)


def test_wave_specialised_softmax_over_the_whole_float_range(gpu):
    """as test_brick_softmax_over_the_whole_float_range, at a shape k_fwd_ws takes: exponentials relative to view 0 on prescaled
    samples, overflow test per channel pair (denominators below 2^60), the max form as the fallback"""
    feats, proj, coords = _ring_problem(B=4, V=4, C=8, H=48, W=48, vol=(64, 64, 32), seed=78)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    for scale in (100.0, 1e4, 1e30):
        f = np.ascontiguousarray(feats * np.float32(scale))
        f[:, :, 1] = feats[:, :, 1]
        f[:, 0, 2] -= np.float32(0.9 * scale)
        f[:, 0, 3] += np.float32(0.9 * scale)
        with np.errstate(all="ignore"):
            ref = cport.forward(f, proj, coords, "softmax")
        assert np.isfinite(ref).all()
        out = aggregation.unprojection(torch.from_numpy(f).to(gpu), p, c, aggregation_method="softmax", variant="brick").cpu().numpy()
        assert np.isfinite(out).all()
        big = [0, 2, 3, 4, 5, 6, 7]
        record_err("ws softmax range x%g, O(1) channel" % scale, _err(out[:, 1], ref[:, 1]), TOL)
        record_err("ws softmax range x%g, relative to max |ref|" % scale, _err(out[:, big], ref[:, big]) / float(np.abs(ref[:, big]).max()), 8e-6)
    fn = feats.copy()
    fn[0, 0, 5, 20:28, 20:28] = np.nan
    fn[0, 1, 6, 16:24, 16:24] = np.inf
    out = aggregation.unprojection(torch.from_numpy(fn).to(gpu), p, c, aggregation_method="softmax", variant="brick").cpu().numpy()
    gat = aggregation.unprojection(torch.from_numpy(fn).to(gpu), p, c, aggregation_method="softmax", variant="gather").cpu().numpy()
    assert np.array_equal(np.isfinite(out), np.isfinite(gat)) and (~np.isfinite(out)).any()
    with np.errstate(all="ignore"):
        ref = cport.forward(fn, proj, coords, "softmax")
    fin = np.isfinite(ref) & np.isfinite(out)
    record_err("ws softmax non-finite samples, finite part", _err(out[fin], ref[fin]), TOL)


def test_prescaled_quad_layout_contract(gpu):
    """MVHMR_LAYOUT_QUAD_LOG2E (ABI 4): produced by mvhmr_convert_features, accepted by exactly the forward that asks for it"""
    feats, proj, coords = _ring_problem(B=16, V=4, C=8, H=48, W=48, vol=(32, 32, 32), seed=5)
    f, p, c = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    L, vp = _capi.lib(), ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(gpu).cuda_stream)
    d = _ws_desc(f, c, "softmax")
    assert L.mvhmr_preferred_layout(ctypes.byref(d)) == _capi.LAYOUT_QUAD_LOG2E
    nb = L.mvhmr_feature_layout_bytes(ctypes.byref(d), _capi.LAYOUT_QUAD_LOG2E)
    assert nb == L.mvhmr_feature_layout_bytes(ctypes.byref(d), _capi.LAYOUT_QUAD) > 0
    q1 = torch.empty(nb // 4, device=gpu)
    q0 = torch.empty(nb // 4, device=gpu)
    _capi.check(L.mvhmr_convert_features(ctypes.byref(d), vp(f.data_ptr()), _capi.LAYOUT_QUAD_LOG2E, vp(q1.data_ptr()), stream))
    _capi.check(L.mvhmr_convert_features(ctypes.byref(d), vp(f.data_ptr()), _capi.LAYOUT_QUAD, vp(q0.data_ptr()), stream))
    assert torch.equal(q1, q0 * np.float32(1.4426950408889634))                              # one fp32 multiply per value
    out = torch.empty(16, 8, 32, 32, 32, device=gpu)
    dk = _capi.Desc.from_buffer_copy(d)
    dk.feat_layout = _capi.LAYOUT_QUAD_LOG2E
    assert L.mvhmr_unproject_forward_workspace_bytes(ctypes.byref(dk)) == 0
    _capi.check(L.mvhmr_unproject_forward(ctypes.byref(dk), vp(q1.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(out.data_ptr()), vp(0), 0, stream))
    assert torch.equal(out, aggregation.unprojection(f, p, c, variant="brick"))              # the planar route makes the same copy itself
    # the unscaled copy through the same kernel family: within the two softmax forms' rounding
    dk.feat_layout = _capi.LAYOUT_QUAD
    out0 = torch.empty_like(out)
    _capi.check(L.mvhmr_unproject_forward(ctypes.byref(dk), vp(q0.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(out0.data_ptr()), vp(0), 0, stream))
    record_err("prescaled vs unscaled quad copy", float((out - out0).abs().max()), 4e-6)
    # everything else refuses it: another aggregate, the gather variant, the backward
    dk.feat_layout = _capi.LAYOUT_QUAD_LOG2E
    for field, value in (("method", _capi.AGG["sum"]), ("variant", _capi.VARIANT["gather"])):
        bad = _capi.Desc.from_buffer_copy(dk)
        setattr(bad, field, value)
        assert L.mvhmr_unproject_forward(ctypes.byref(bad), vp(q1.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(out.data_ptr()), vp(0), 0, stream) == _capi.ERR_UNSUPPORTED
    assert L.mvhmr_unproject_backward_supported(ctypes.byref(dk)) == 0
    g = torch.empty_like(f)
    assert L.mvhmr_unproject_backward(ctypes.byref(dk), vp(out.data_ptr()), vp(q1.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(g.data_ptr()), vp(0), 0, stream) == _capi.ERR_UNSUPPORTED
    small = _ws_desc(f[:2], c[:2], "softmax")                                                # 32 bricks: k_fwd_brick, unscaled
    assert L.mvhmr_preferred_layout(ctypes.byref(small)) == _capi.LAYOUT_QUAD


@pytest.mark.parametrize("views", (3, 6))
def test_mean_over_absent_views_is_one_division_by_the_real_views(views, gpu):
    """3 / 6 views run the 4- / 8-view brick kernels with the missing views absent.  Their mean is sum / V (one IEEE division, the
    reference's volume.mean(0)) -- not sum / 4 * (4 / 3).  Checked on the brick kernels' own sum: their samples may differ
    from the gather kernels' in the last bit (the parity-split windows add the four bilinear products in another order)"""
    feats, proj, coords = _ring_problem(B=2, V=views, C=8, H=24, W=24, vol=(8, 8, 32), seed=300 + views)
    f, p, c = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    brick = aggregation.unprojection(f, p, c, aggregation_method="mean", variant="brick")
    total = aggregation.unprojection(f, p, c, aggregation_method="sum", variant="brick")
    # one correctly rounded fp32 division (numpy: torch's GPU division by a scalar multiplies by the reciprocal)
    assert np.array_equal(brick.cpu().numpy(), total.cpu().numpy() / np.float32(views))
    gather = aggregation.unprojection(f, p, c, aggregation_method="mean", variant="gather")
    record_err("mean V%d brick vs gather" % views, float((brick - gather).abs().max()), 1e-6)
    ref = cport.forward(feats, proj, coords, "mean")
    record_err("mean V%d brick fwd" % views, _err(brick.cpu().numpy(), ref), TOL)
    fb = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    go = np.random.default_rng(9).standard_normal(ref.shape, dtype=np.float32)
    aggregation.unprojection(fb, p, c, aggregation_method="mean", variant="brick").backward(torch.from_numpy(go).to(gpu))
    gref = cport.backward(go, feats, proj, coords, "mean")
    record_err("mean V%d brick bwd" % views, _err(fb.grad.cpu().numpy(), gref), _bound(gref))


def _capi_route(f, p, c, go):
    """forward + feature backward as direct C-ABI calls through _capi (as bench.py makes them): the layout decision and the
    descriptor the custom op uses, outputs and workspaces allocated here"""
    L, vp = _capi.lib(), ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(f.device).cuda_stream)
    method, auto = _capi.AGG["softmax"], _capi.VARIANT["auto"]
    feats, layout, like = aggregation._feature_layout(f, c, method, torch.float32, auto)
    desc = ctypes.byref(aggregation._make_desc(like, c, method, torch.float32, layout, auto))
    out = torch.empty((like.shape[0], like.shape[2]) + tuple(c.shape[1:4]), device=f.device)
    grad = torch.empty(like.shape, device=f.device) if layout == _capi.LAYOUT_QUAD else torch.empty_like(feats)
    ws = torch.empty(L.mvhmr_unproject_forward_workspace_bytes(desc), dtype=torch.uint8, device=f.device)
    _capi.check(L.mvhmr_unproject_forward(desc, vp(feats.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()), vp(out.data_ptr()),
                                          vp(ws.data_ptr() if ws.numel() else 0), ws.numel(), stream))
    ws = torch.empty(L.mvhmr_unproject_backward_workspace_bytes(desc), dtype=torch.uint8, device=f.device)
    _capi.check(L.mvhmr_unproject_backward(desc, vp(go.data_ptr()), vp(feats.data_ptr()), vp(p.data_ptr()), vp(c.data_ptr()),
                                           vp(grad.data_ptr()), vp(ws.data_ptr() if ws.numel() else 0), ws.numel(), stream))
    return out, grad


def test_native_extension_is_the_route_and_equals_direct_c_abi_calls(gpu):
    """north_star: "drop-in ... via a PyTorch-ROCm C++/HIP extension".  The custom ops' host work runs in lib_ext/mvhmr_torch_ext.so
    (csrc_ext/mvhmr_torch_ext.cpp over the C ABI); the same C-ABI calls made directly through the ctypes binding give a bit-equal
    forward, and a backward equal up to the float atomics' order"""
    d = load_golden("unproj", "bricks_v4c8")
    p, c, go = _dev(d, "proj", gpu), _dev(d, "coords", gpu), _dev(d, "grad_out", gpu)
    outs, grads = [], []
    for feats in (_dev(d, "features", gpu), _dev(d, "features", gpu).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)):
        f = feats.detach().requires_grad_(True)
        out = aggregation.unprojection(f, p, c)
        out.backward(go)
        ref_out, ref_grad = _capi_route(feats, p, c, go)
        outs.append((out.detach(), ref_out)); grads.append((f.grad, ref_grad))
    assert torch.equal(*outs[0]) and torch.equal(*outs[1])                                   # planar, channels-last
    record_err("extension vs C ABI, planar bwd", float((grads[0][0] - grads[0][1]).abs().max()), 1e-5)
    record_err("extension vs C ABI, channels-last bwd", float((grads[1][0] - grads[1][1]).abs().max()), 1e-5)
    assert grads[1][0].stride() == grads[1][1].stride()                                      # channels-last gradient for channels-last features
    record_err("extension route vs golden", _err(outs[0][0].cpu().numpy(), d["out_softmax"]), TOL)
    # the C ABI trusts its descriptor: the extension checks every tensor against it BEFORE anything is launched
    fe = _dev(d, "features", gpu)
    B, V, C, H, W = fe.shape
    with pytest.raises(RuntimeError, match="features hold"):
        torch.ops.mvhmr_native.unprojection(fe, p, c, B, V, C, H + 1, W, 0, 0, 0, 0, 2)
    with pytest.raises(RuntimeError, match="proj_matricies"):
        torch.ops.mvhmr_native.unprojection(fe, p[:, :1].contiguous(), c, B, V, C, H, W, 0, 0, 0, 0, 2)
    with pytest.raises(RuntimeError, match="mvhmr_unproject"):                               # library errors surface as RuntimeError
        torch.ops.mvhmr_native.unprojection(fe, p, c, B, V, C, H, W, 7, 0, 0, 0, 2)         # unknown aggregate
    # a host tensor is refused, not handed to a kernel as a device pointer
    with pytest.raises(RuntimeError, match="proj_matricies .* contiguous tensor on"):
        torch.ops.mvhmr_native.unprojection(fe, p.cpu(), c, B, V, C, H, W, 0, 0, 0, 0, 2)
    with pytest.raises(RuntimeError, match="proj_matricies .* contiguous tensor on"):
        torch.ops.mvhmr_native.unprojection_backward(go, fe, p.cpu(), c, B, V, C, H, W, 0, 0, 0, 0, 2)
    rot, cen = torch.eye(3).expand(B, 3, 3).contiguous(), torch.zeros(B, 3, device=gpu)
    with pytest.raises(RuntimeError, match="rot .* contiguous tensor on"):
        torch.ops.mvhmr_native.unprojection_cuboid(fe, p, rot, cen, [0.0] * 3, [1.0] * 3, [4, 4, 4], B, V, C, H, W, 0, 0, 0, 0, 2)
