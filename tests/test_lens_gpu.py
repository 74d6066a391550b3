"""Lens-distortion-aware un-projection on the GPU (unprojection(lens=), mvhmr_unproject_*_lens): zero coefficients are the
plain gather call bit for bit, parity with the float64 oracle (tests/lens_oracle.py) under barrel, tangential and full lenses, the fold-back
guard, bit equality on the exact rig, deterministic mode, routes, storage modes, VolumeGenerator(lens_distortion=True) and the workspace
between guard bands.  tests/test_lens_cpu.py checks the premises (rigs, oracle anchor) without a GPU.

Feature gradients and float atomics: the per-tap scatter of the DEFAULT mode adds with float atomics, whose low bits depend on the arrival
order (the plain call does not repeat itself bitwise there either), so "bit-equal to the plain call" is asserted for the feature gradient in
deterministic mode everywhere and in default mode wherever the plane route runs (no atomics); where the default scatter runs it is held to the
plain call within _bound, the bar tests/test_unproject_gpu.py holds that scatter to."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lens_oracle
from conftest import load_golden, record_err
from multiviewhmr_amd import _capi, aggregation, multiview
from posegrad_oracle import cuboid_points
from test_guard_bands_gpu import POISONS, _cl, _guarded, _lib
from test_guard_bands_gpu import _desc as _abi_desc
from test_lens_cpu import RIGS
from test_unproject_gpu import _bound, _err

pytestmark = pytest.mark.gpu

MODES = ("softmax", "sum", "mean", "max")
REL = 1e-4                                  # geometry gradients: 1e-4 of the largest oracle value (test_geometry_grad_gpu.py)


class Deterministic:
    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        self.was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(self.on)

    def __exit__(self, *a):
        torch.use_deterministic_algorithms(self.was)


def _t(a, gpu, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t if dtype is None else t.to(dtype)


def _run(gpu, f, p, c, lens, go, method, det=False, features=None, **kw):
    """one forward + backward of the tensor route -> dict(out, gf, gp, gc) of device tensors; numpy inputs (features: a prepared device tensor)"""
    ft = (_t(f, gpu) if features is None else features.detach()).requires_grad_(True)       # (a prepared tensor is read where it lies: no copy)
    pt, ct = _t(p, gpu).requires_grad_(True), _t(c, gpu).requires_grad_(True)
    with Deterministic(det):
        out = aggregation.unprojection(ft, pt, ct, method, lens=None if lens is None else _t(lens, gpu), **kw)
        out.backward(_t(go, gpu).to(out.dtype))
    return dict(out=out.detach(), gf=ft.grad, gp=pt.grad, gc=ct.grad)


def _run_cuboid(gpu, f, p, rot, cen, cub, lens, go, method, det=False, **kw):
    ft, pt = _t(f, gpu).requires_grad_(True), _t(p, gpu).requires_grad_(True)
    rt, cet = _t(rot, gpu).requires_grad_(True), _t(cen, gpu).requires_grad_(True)
    with Deterministic(det):
        out = aggregation.unprojection_cuboid(ft, pt, rt, cet, *cub, method, lens=None if lens is None else _t(lens, gpu), **kw)
        out.backward(_t(go, gpu).to(out.dtype))
    return dict(out=out.detach(), gf=ft.grad, gp=pt.grad, gr=rt.grad, gce=cet.grad)


def _plane_route(f):
    """the plain variant='gather' call on PLANAR features takes the plane backward (no atomics) for 2 / 4 / 8 views and C % 4 == 0"""
    return f.shape[1] in (2, 4, 8) and f.shape[2] % 4 == 0


def _zero_lens(B, V, seed=1):
    """zero coefficients (+0.0 and -0.0) under arbitrary intrinsics and guards"""
    rng = np.random.default_rng(seed)
    lens = np.zeros((B, V, 10), np.float32)
    lens[..., :4] = rng.uniform(-50, 50, (B, V, 4))
    lens[..., 9] = rng.uniform(0, 1e-3, (B, V))
    lens[:, ::2, 4:9] = -0.0
    return lens


def _grad_out(shape, seed=5):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def _pose(B, c, seed=2):
    """a cuboid about the golden's coordinates: per-sample rotation about z and a pivot near the centre"""
    rng = np.random.default_rng(seed)
    lo, hi = c.reshape(-1, 3).min(0).astype(np.float64), c.reshape(-1, 3).max(0).astype(np.float64)
    th = rng.uniform(0, 2 * np.pi, B)
    rot = np.stack([np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1.0]]) for t in th]).astype(np.float32)
    cen = ((lo + hi) / 2 + rng.normal(0, 30, (B, 3))).astype(np.float32)
    return rot, cen, (tuple(lo), tuple(hi - lo), tuple(c.shape[1:4]))


# ------------------------------------------------------------------------------------ 1. zero coefficients
@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("case", ["tiny_b2v2c4", "nonsquare_v3c5", "tiles_v4c16", "eight_views_c7", "adversarial_v4c6"])
def test_zero_coefficients_are_the_plain_gather_call(case, det, gpu):
    d = load_golden("unproj", case)
    f, p, c, go = d["features"], d["proj"], d["coords"], d["grad_out"]
    lens = _zero_lens(*f.shape[:2])
    for method in MODES:
        plain = _run(gpu, f, p, c, None, go, method, det, variant="gather")
        got = _run(gpu, f, p, c, lens, go, method, det)
        for k in ("out", "gp", "gc"):
            assert torch.equal(got[k], plain[k]), (case, method, k)
        if det or _plane_route(f):
            assert torch.equal(got["gf"], plain["gf"]), (case, method)
        else:                                                               # float atomics: order-dependent low bits (see the module docstring)
            ref = plain["gf"].double().cpu().numpy()
            record_err("lens zero coefficients default scatter %s %s" % (case, method), _err(got["gf"].cpu().numpy(), ref), _bound(ref))
    # the cuboid route: pose gradients
    rot, cen, cub = _pose(f.shape[0], c)
    for method in ("softmax", "max"):
        plain = _run_cuboid(gpu, f, p, rot, cen, cub, None, go, method, True, variant="gather")
        got = _run_cuboid(gpu, f, p, rot, cen, cub, lens, go, method, True)
        for k in plain:
            assert torch.equal(got[k], plain[k]), (case, method, k)


def test_a_batch_mixing_zero_and_distorted_views_keeps_the_zero_views_bit_equal(gpu):
    """`sum`: a view's feature and projection gradients depend on no other view.  Sample 0 is all zero coefficients, sample 1 alternates"""
    d = load_golden("unproj", "tiles_v4c16")
    f, p, c, go = d["features"], d["proj"], d["coords"], d["grad_out"]
    B, V, C, H, W = f.shape
    lens = _zero_lens(B, V)
    lens[1, 1::2] = (H / 2.0, W / 2.0, H / 2.0, W / 2.0, -0.2, 0.05, 0.001, -0.002, 0.0, np.finfo(np.float32).max)
    for det in (False, True):                                               # planar V = 4, C = 16: the plane route in both modes
        plain = _run(gpu, f, p, c, None, go, "sum", det, variant="gather")
        got = _run(gpu, f, p, c, lens, go, "sum", det)
        for k in ("out", "gf", "gp", "gc"):
            assert torch.equal(got[k][0], plain[k][0]), k
        assert torch.equal(got["gf"][1, 0::2], plain["gf"][1, 0::2]) and torch.equal(got["gp"][1, 0::2], plain["gp"][1, 0::2])
        assert not torch.equal(got["gf"][1, 1], plain["gf"][1, 1]) and not torch.equal(got["out"][1], plain["out"][1])
    softmax = _run(gpu, f, p, c, lens, go, "softmax", True)
    assert torch.equal(softmax["out"][0], _run(gpu, f, p, c, None, go, "softmax", True, variant="gather")["out"][0])


# ------------------------------------------------------------------------------------ 2. parity with the oracle
@functools.lru_cache(maxsize=None)
def _rig(idx, kind):
    arrs = lens_oracle.ring_rig(seed=5, dists=lens_oracle.LENSES[kind], **RIGS[idx])
    for a in arrs:
        a.setflags(write=False)
    return arrs


@functools.lru_cache(maxsize=None)
def _reference(idx, kind, method):
    f, p, c, lens = _rig(idx, kind)
    go = _grad_out((f.shape[0], f.shape[2]) + c.shape[1:4])
    res = lens_oracle.lens_unprojection(f, p, c, lens, go, method)
    assert 3 * int(res["live"].sum()) >= res["live"].size, "a rig must keep a third of its voxel-views inside the frame and the guard"
    return go, res


def _parity(tag, got, ref):
    record_err(tag + " fwd", _err(got["out"].float().cpu().numpy(), ref["out"]), _bound(ref["out"]))
    record_err(tag + " grad_features", _err(got["gf"].float().cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))
    record_err(tag + " grad_proj", _err(got["gp"].cpu().numpy(), ref["grad_proj"]), REL * float(np.abs(ref["grad_proj"]).max()))
    record_err(tag + " grad_coords", _err(got["gc"].cpu().numpy(), ref["grad_coords"]), REL * float(np.abs(ref["grad_coords"]).max()))


@pytest.mark.parametrize("kind", ["barrel", "tangential", "full", "mixed"])
@pytest.mark.parametrize("idx", range(len(RIGS)), ids=lambda i: "v%dc%d" % (RIGS[i]["V"], RIGS[i]["C"]))
def test_parity_with_the_oracle(idx, kind, gpu):
    f, p, c, lens = _rig(idx, kind)
    for method in MODES:
        go, ref = _reference(idx, kind, method)
        got = _run(gpu, f, p, c, lens, go, method)
        _parity("lens %s v%dc%d %s" % (kind, f.shape[1], f.shape[2], method), got, ref)
        assert float(np.abs(ref["grad_features"]).max()) > 0 and float(np.abs(ref["grad_proj"]).max()) > 0


@pytest.mark.parametrize("idx", [1, 2], ids=["v3c16", "v4c16"])
def test_parity_on_the_cuboid_route(idx, gpu):
    """the cuboid recipe's voxel centres in the kernels' rounding (posegrad_oracle.cuboid_points), the lens oracle on them, and the chain rule
    through X = R d + c in float64 as posegrad_oracle.pose_grad runs it"""
    f, p, c, lens = _rig(idx, "full")
    B = f.shape[0]
    rot, cen, cub = _pose(B, c, seed=3)
    dd, X = cuboid_points(rot, cen, *cub)
    go = _grad_out((B, f.shape[2]) + c.shape[1:4], seed=6)
    for method in MODES:
        ref = lens_oracle.lens_unprojection(f, p, X.numpy(), lens, go, method)
        assert 3 * int(ref["live"].sum()) >= ref["live"].size
        gX = torch.from_numpy(ref["grad_coords"]).reshape(B, -1, 3)
        g_rot = torch.einsum("bnr,bnk->brk", gX, dd.double().reshape(B, -1, 3)).numpy()
        s_g = gX.sum(1)
        g_cen = (s_g - torch.einsum("brk,br->bk", torch.from_numpy(rot).double(), s_g)).numpy()
        got = _run_cuboid(gpu, f, p, rot, cen, cub, lens, go, method)
        tag = "lens cuboid v%d %s" % (f.shape[1], method)
        record_err(tag + " fwd", _err(got["out"].cpu().numpy(), ref["out"]), _bound(ref["out"]))
        record_err(tag + " grad_features", _err(got["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))
        record_err(tag + " grad_proj", _err(got["gp"].cpu().numpy(), ref["grad_proj"]), REL * float(np.abs(ref["grad_proj"]).max()))
        record_err(tag + " grad_rot", _err(got["gr"].cpu().numpy(), g_rot), REL * float(np.abs(g_rot).max()))
        record_err(tag + " grad_center", _err(got["gce"].cpu().numpy(), g_cen), REL * float(np.abs(g_cen).max()))
        # and bit-equal to the tensor route on the coordinates the cuboid builds
        tens = _run(gpu, f, p, X.numpy(), lens, go, method, det=True)
        cub_det = _run_cuboid(gpu, f, p, rot, cen, cub, lens, go, method, det=True)
        assert torch.equal(tens["out"], cub_det["out"]) and torch.equal(tens["gf"], cub_det["gf"]) and torch.equal(tens["gp"], cub_det["gp"])


# ------------------------------------------------------------------------------------ 3. fold-back
def test_rays_past_the_guard_are_exactly_zero_and_read_nothing(gpu):
    f, p, c, lens = lens_oracle.foldback_rig()
    B, V, C, H, W = f.shape
    N = int(np.prod(c.shape[1:4]))
    go = _grad_out((B, C) + c.shape[1:4])
    ref = lens_oracle.lens_unprojection(f, p, c, lens, go, "sum")
    guarded, live = ref["guarded"], ref["live"]
    assert guarded.sum() >= 8 and live.sum() >= 8
    # pixels that only FOLDED rays would tap (where the raw polynomial lands them) hold NaN: a zero weight times NaN would show
    poison = np.zeros((B, V, H, W), bool)
    tapped = np.zeros((B, V, H, W), bool)
    for b in range(B):
        pts = torch.from_numpy(c[b].reshape(-1, 3))
        for v in range(V):
            z, ix, iy, ok = (t.numpy() for t in lens_oracle.raw_positions(torch.from_numpy(p[b, v]), lens[b, v], pts, H, W))
            for n in range(N):
                if not (z[n] > 0 and -1 < ix[n] < W and -1 < iy[n] < H):
                    continue
                x0, y0 = int(np.floor(ix[n])), int(np.floor(iy[n]))
                for yy in (y0, y0 + 1):
                    for xx in (x0, x0 + 1):
                        if ok[n]:                                           # a live ray reads all four taps, those outside the map clamped into it
                            tapped[b, v, min(max(yy, 0), H - 1), min(max(xx, 0), W - 1)] = True
                        elif 0 <= xx < W and 0 <= yy < H:
                            poison[b, v, yy, xx] = True
    poison &= ~tapped
    assert poison.sum() >= 4
    fp = f.copy()
    fp[np.broadcast_to(poison[:, :, None], f.shape)] = np.nan
    # channels-last features are read in place: NaN guard bands around them (tests/test_guard_bands_gpu.py)
    band = 1 << 16
    arena = torch.full((2 * band + f.size,), float("nan"), device=gpu)
    arena[band:band + f.size] = _t(fp, gpu).permute(0, 1, 3, 4, 2).reshape(-1)
    feats = arena[band:band + f.size].view(B, V, H, W, C).permute(0, 1, 4, 2, 3)
    for method in MODES:
        ref = lens_oracle.lens_unprojection(f, p, c, lens, go, method)
        # (deterministic softmax bounds |ds| by the largest feature of the whole map, poisoned pixels included: default mode there)
        for det in ((False,) if method == "softmax" else (False, True)):
            got = _run(gpu, f, p, c, lens, go, method, det, features=feats)
            clean = _run(gpu, f, p, c, lens, go, method, det, features=_t(f, gpu).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3))
            assert torch.isfinite(got["out"]).all() and torch.equal(got["out"], clean["out"]), method
            assert torch.equal(got["gp"], clean["gp"]) and torch.equal(got["gc"], clean["gc"])
            gf = got["gf"].cpu().numpy()
            assert np.isfinite(gf[~np.broadcast_to(poison[:, :, None], f.shape)]).all()
            assert not gf[np.broadcast_to(poison[:, :, None], f.shape)].any()      # exact zeros: nothing is scattered there either
            record_err("lens fold-back %s det=%d fwd" % (method, det), _err(got["out"].cpu().numpy(), ref["out"]), _bound(ref["out"]))
    # a voxel none of whose views is live and some of whose views lie past the guard: exactly zero volume (sum) and coordinate gradient
    dead = ~live.any(1) & guarded.any(1)
    assert dead.sum() >= 1
    got = _run(gpu, f, p, c, lens, go, "sum")
    assert not got["out"].reshape(B, C, N).permute(0, 2, 1)[torch.from_numpy(dead).to(gpu)].any()
    assert not got["gc"].reshape(B, N, 3)[torch.from_numpy(dead).to(gpu)].any()
    one = _run(gpu, f[:, :1], p[:, :1], c, lens[:, :1], go, "max")                 # a single view: its guarded voxels are zeros outright
    g0 = torch.from_numpy(guarded[:, 0]).to(gpu)
    assert g0.any() and not one["out"].reshape(B, C, N).permute(0, 2, 1)[g0].any() and not one["gc"].reshape(B, N, 3)[g0].any()


# ------------------------------------------------------------------------------------ 4. exactness
@pytest.mark.parametrize("method", ["sum", "max"])
def test_the_exact_rig_is_bit_equal_to_the_float64_oracle(method, gpu):
    f, p, c, go, lens = lens_oracle.exact_rig()
    ref = lens_oracle.lens_unprojection(f, p, c, lens, go, method, geometry=False)
    assert np.array_equal(ref["out"], ref["out"].astype(np.float32)) and np.array_equal(ref["grad_features"], ref["grad_features"].astype(np.float32))
    assert ref["guarded"].sum() >= 10 and np.abs(ref["out"]).max() > 0
    for kw in (dict(), dict(variant="gather")):
        got = _run(gpu, f, p, c, lens, go, method, **kw)
        assert torch.equal(got["out"].cpu(), torch.from_numpy(ref["out"].astype(np.float32))), method
        assert torch.equal(got["gf"].cpu(), torch.from_numpy(ref["grad_features"].astype(np.float32))), method


# ------------------------------------------------------------------------------------ 5. deterministic mode
@pytest.mark.parametrize("idx", [0, 2, 3], ids=["v2c6 scatter", "v4c16 plane", "v8c260 plane"])
def test_deterministic_mode_repeats_bitwise_and_stays_within_parity(idx, gpu):
    f, p, c, lens = _rig(idx, "full")
    for method in MODES:
        go, ref = _reference(idx, "full", method)
        a = _run(gpu, f, p, c, lens, go, method, det=True)
        b = _run(gpu, f, p, c, lens, go, method, det=True)
        for k in a:
            assert torch.equal(a[k], b[k]), (method, k)
        _parity("lens deterministic v%dc%d %s" % (f.shape[1], f.shape[2], method), a, ref)
        cl = _t(f, gpu).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)   # channels-last: the deterministic scatter, whatever V and C
        if f.shape[2] % 4 == 0:
            x = _run(gpu, f, p, c, lens, go, method, det=True, features=cl)
            y = _run(gpu, f, p, c, lens, go, method, det=True, features=cl)
            assert torch.equal(x["gf"], y["gf"]) and torch.equal(x["out"], a["out"])
            record_err("lens deterministic scatter v%dc%d %s" % (f.shape[1], f.shape[2], method), _err(x["gf"].cpu().numpy(), ref["grad_features"]),
                       _bound(ref["grad_features"]))


@pytest.mark.parametrize("method,log2", [("sum", 120), ("max", 120), ("mean", 120), ("softmax", 100)])
def test_deterministic_scale_pass_near_its_limit(method, log2, gpu):
    """grad_out a few binades below the bound at which the scale pass poisons a channel (2^128 for |ds|): the fixed-point exponents go far
    negative, the gradient stays finite and is the oracle's, scaled -- the bound does not depend on where the lens puts the taps"""
    f, p, c, lens = _rig(0, "barrel")                                       # V = 2, C = 6: the deterministic scatter
    go, ref = _reference(0, "barrel", method)
    s = 2.0 ** log2
    a = _run(gpu, f, p, c, lens, go * np.float32(s), method, det=True)
    b = _run(gpu, f, p, c, lens, go * np.float32(s), method, det=True)
    assert torch.isfinite(a["gf"]).all() and torch.equal(a["gf"], b["gf"])
    record_err("lens deterministic near the limit %s" % method, _err((a["gf"].double() / s).cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))


# ------------------------------------------------------------------------------------ 6. routes
def test_the_plane_backward_runs_where_the_plain_gather_call_takes_it(gpu):
    """planar V = 4, C = 16: the plain gather call takes the plane kernels in both modes, and so does the lens call -- its default-mode gradient
    has the deterministic one's bits and repeats (the float-atomic scatter has neither property: shown on channels-last features, which keep
    the scatter), and its workspace is the plain twin's, tap table included"""
    f, p, c, lens = _rig(2, "full")
    go, ref = _reference(2, "full", "softmax")
    dflt = _run(gpu, f, p, c, lens, go, "softmax", det=False)
    again = _run(gpu, f, p, c, lens, go, "softmax", det=False)
    det = _run(gpu, f, p, c, lens, go, "softmax", det=True)
    assert torch.equal(dflt["gf"], det["gf"]) and torch.equal(dflt["gf"], again["gf"])
    cl = _t(f, gpu).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    scat, scat_det = _run(gpu, f, p, c, lens, go, "softmax", features=cl), _run(gpu, f, p, c, lens, go, "softmax", det=True, features=cl)
    assert not torch.equal(scat["gf"], scat_det["gf"])                      # float atomics vs int64 fixed point
    L = _capi.lib()
    B, V, C, H, W = f.shape
    d = _abi_desc(B, V, C, H, W, c.shape[1:4], variant="gather")
    plain = ctypes.CDLL(_capi.LIB_PATH).mvhmr_unproject_backward_workspace_bytes
    plain.restype, plain.argtypes = ctypes.c_size_t, [ctypes.POINTER(_capi.Desc)]
    assert L.mvhmr_unproject_backward_lens_workspace_bytes(ctypes.byref(d)) == plain(ctypes.byref(d)) > B * V * int(np.prod(c.shape[1:4])) * 20


@pytest.mark.parametrize("idx", [1, 2], ids=["v3c16", "v4c16"])
def test_auto_is_gather_and_brick_is_refused(idx, gpu):
    f, p, c, lens = _rig(idx, "mixed")
    go, _ = _reference(idx, "mixed", "softmax")
    a = _run(gpu, f, p, c, lens, go, "softmax", det=True)
    g = _run(gpu, f, p, c, lens, go, "softmax", det=True, variant="gather")
    for k in a:
        assert torch.equal(a[k], g[k]), k
    cl = _t(f, gpu).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    assert torch.equal(_run(gpu, f, p, c, lens, go, "softmax", det=True, features=cl)["out"], a["out"])
    with pytest.raises(RuntimeError, match="lens distortion runs the gather kernels"):
        aggregation.unprojection(_t(f, gpu), _t(p, gpu), _t(c, gpu), lens=_t(lens, gpu), variant="brick")
    # the records may come in any floating dtype and from any device
    out = aggregation.unprojection(_t(f, gpu), _t(p, gpu), _t(c, gpu), lens=torch.from_numpy(lens).double())
    assert torch.equal(out, a["out"])


# ------------------------------------------------------------------------------------ 7. storage
def test_storage_modes(gpu):
    f, p, c, lens = _rig(2, "full")
    ft, pt, ct, lt = _t(f, gpu), _t(p, gpu), _t(c, gpu), _t(lens, gpu)
    for method in MODES:
        go, ref = _reference(2, "full", method)
        out32 = aggregation.unprojection(ft, pt, ct, method, lens=lt)
        # bf16 volume: the fp32 volume rounded once
        assert torch.equal(aggregation.unprojection(ft, pt, ct, method, lens=lt, out_dtype=torch.bfloat16), out32.to(torch.bfloat16)), method
        # fp16 features: the oracle on the rounded features; an fp16 volume is the fp32 one of the same call rounded once
        f16 = ft.half()
        ref16 = lens_oracle.lens_unprojection(f16.float().cpu().numpy(), p, c, lens, go, method)
        h = f16.clone().requires_grad_(True)
        o = aggregation.unprojection(h, pt, ct, method, lens=lt, out_dtype=torch.float32)
        o.backward(_t(go, gpu))
        record_err("lens fp16 features %s fwd" % method, _err(o.detach().cpu().numpy(), ref16["out"]), _bound(ref16["out"]))
        record_err("lens fp16 features %s grad_features" % method, _err(h.grad.float().cpu().numpy(), ref16["grad_features"]),
                   _bound(ref16["grad_features"]) + 2.0 ** -11 * float(np.abs(ref16["grad_features"]).max()))      # the gradient is stored in fp16
        assert torch.equal(aggregation.unprojection(f16, pt, ct, method, lens=lt), o.detach().half()), method
        # channels-last features: read in place, the same volume; the scatter's gradient against the oracle
        cl = ft.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
        got = _run(gpu, f, p, c, lens, go, method, features=cl)
        assert torch.equal(got["out"], out32), method
        _parity("lens channels-last %s" % method, got, ref)


# ------------------------------------------------------------------------------------ 8. VolumeGenerator
def _cams(B, V, img, dists):
    cams = [[None] * B for _ in range(V)]
    for v in range(V):
        az = 2 * np.pi * v / V + 0.3
        eye = np.array([5000 * np.cos(az), 5000 * np.sin(az), 1500.0])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0, 0, 1.0]); right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        for b in range(B):
            cam = multiview.Camera(R, -R @ eye, [[1145.0, 0, 512], [0, 1145.0, 512], [0, 0, 1]], dist=dists[(b * V + v) % len(dists)])
            cam.update_after_crop((150, 150, 850, 850))
            cam.update_after_resize((700, 700), (img, img))
            cams[v][b] = cam
    return cams


def test_volume_generator_with_lens_distortion(gpu, monkeypatch):
    """equals unprojection_cuboid(lens=feature_level_lens(...)) bit for bit on a shape the fused conv route would otherwise take, which it
    skips; batch['lens'] overrides the cameras; the eval forward is capturable in a HIP graph with nothing copied from the host"""
    B, V, C, H, S, IMG = 2, 4, 128, 32, 32, 128
    cams = _cams(B, V, IMG, (lens_oracle.FULL, lens_oracle.BARREL, None))
    kp = torch.zeros(B, 17, 3, device=gpu)
    kp[:, 6] = torch.tensor([[30.0, -20.0, 10.0], [-15.0, 25.0, 5.0]], device=gpu)
    batch = dict(images=np.zeros((B, V, IMG, IMG, 3), np.uint8), cameras=cams, cameras_packed=aggregation.pack_cameras(cams, gpu), keypoints_3d=kp)
    proj_org = torch.from_numpy(np.stack([[cams[v][b].projection for v in range(V)] for b in range(B)]).astype(np.float32)).to(gpu)
    torch.manual_seed(2)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=C, output_channels=C, device=gpu, lens_distortion=True).eval()
    x = torch.randn(B, V, C, H, H, device=gpu)
    fused = []
    real_apply = aggregation._FusedAggregate.apply
    monkeypatch.setattr(aggregation._FusedAggregate, "apply", lambda *a: (fused.append(1), real_apply(*a))[1])
    with torch.no_grad():
        out = gen(x, proj_org, batch)
        assert not fused
        gen.lens_distortion = False
        plain = gen(x, proj_org, batch)
        assert len(fused) == 1                                              # the same shape without the lens takes the fused route
        gen.lens_distortion = True
        lens = aggregation.feature_level_lens(cams, (IMG, IMG), (H, H))
        feats = gen.process_feature(x.view(-1, C, H, H)).view(B, V, C, H, H)
        proj = aggregation.feature_level_projections_device(batch["cameras_packed"], (IMG, IMG), (H, H)).to(gpu)
        rots, centers = gen.volume_pose(batch, proj_org, (IMG, IMG))
        cub = gen.cuboid()
        want = aggregation.unprojection_cuboid(feats, proj, rots.to(gpu), centers.to(gpu), cub.position, cub.sides, (S, S, S), lens=torch.from_numpy(lens))
        assert torch.equal(out, want) and not torch.equal(out, plain.to(out.dtype))
        # batch['lens']: a device tensor (nothing copied from the host); zero records give the plain gather volume
        dev = dict(batch, lens=torch.from_numpy(lens).to(gpu))
        del dev["cameras"]
        assert torch.equal(gen(x, proj_org, dev), out)
        zero = gen(x, proj_org, dict(dev, lens=torch.zeros(B, V, 10, device=gpu)))
        assert torch.equal(zero, aggregation.unprojection_cuboid(feats, proj, rots.to(gpu), centers.to(gpu), cub.position, cub.sides, (S, S, S), variant="gather"))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            gen(x, proj_org, dev)                        # warm-up outside the capture (kernel attributes, the cached eval rotations)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            cap = gen(x, proj_org, dev)
        x.copy_(torch.randn_like(x))                     # new values, same buffers
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap, gen(x, proj_org, dev))
    # and it trains: gradients reach the conv and the input through the lens
    gen.train()
    np.random.seed(3)
    xi = x.clone().requires_grad_(True)
    gen(xi, proj_org, batch).square().mean().backward()
    assert torch.isfinite(xi.grad).all() and float(xi.grad.abs().max()) > 0 and float(gen.process_feature[0].weight.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------ 9. workspace between guard bands
def _queries(L, name, D, plain_name):
    q = getattr(L, "mvhmr_unproject_%s_lens_workspace_bytes" % name)
    q.restype = ctypes.c_size_t
    pq = getattr(L, "mvhmr_unproject_%s_workspace_bytes" % plain_name)
    pq.restype = ctypes.c_size_t
    need = q(D)
    assert need >= pq(D), name
    return need


@pytest.mark.parametrize("layout", ["planar", "channels_last"])
def test_every_lens_entry_point_with_exactly_the_queried_workspace(layout, gpu):
    """inputs, outputs and the workspace at exactly its queried size lie between guard bands (tests/test_guard_bands_gpu.py): the bands stay
    intact, the inputs unwritten, and the results are those of the Python route"""
    L = _lib()
    f, p, c, lens = _rig(2, "mixed")
    B, V, C, H, W = f.shape
    vol = tuple(c.shape[1:4])
    go, _ = _reference(2, "mixed", "softmax")
    ft, pt, ct, lt, gt = _t(f, gpu), _t(p, gpu), _t(c, gpu), _t(lens, gpu), _t(go, gpu)
    lay = _capi.LAYOUT_BVHWC if layout == "channels_last" else _capi.LAYOUT_BVCHW
    fin = _cl(ft) if layout == "channels_last" else ft
    feats = fin.permute(0, 1, 4, 2, 3) if layout == "channels_last" else ft
    d = _abi_desc(B, V, C, H, W, vol, "softmax", layout=lay, variant="auto")
    D = ctypes.byref(d)
    null = ctypes.c_void_p(0)
    sel = lambda q: (q["l"], null, null, null, 0, null)                    # noqa: E731  lens, then the (refused) selections
    want = _run(gpu, f, p, c, lens, go, "softmax", det=True, features=feats)
    ins = {"f": fin, "p": pt, "c": ct, "l": lt}
    out_shape, gshape = (B, C) + vol, (tuple(fin.shape) if layout == "channels_last" else (B, V, C, H, W))
    for poison in POISONS:
        r = _guarded(gpu, ins, {"out": (torch.float32, out_shape)}, _queries(L, "forward", D, "forward"), poison,
                     lambda q: L.mvhmr_unproject_forward_lens(D, q["f"], q["p"], q["c"], *sel(q), q["out"], q["ws"], q["ws_bytes"], q["stream"]))
        assert torch.equal(r["out"], want["out"])
        bins = dict(ins, g=gt)
        for name in ("backward", "backward_deterministic"):
            r = _guarded(gpu, bins, {"gf": (torch.float32, gshape)}, _queries(L, name, D, name), poison,
                         lambda q, fn=getattr(L, "mvhmr_unproject_%s_lens" % name): fn(D, q["g"], q["f"], q["p"], q["c"], *sel(q), q["gf"], q["ws"], q["ws_bytes"], q["stream"]))
            gf = r["gf"].permute(0, 1, 4, 2, 3) if layout == "channels_last" else r["gf"]
            if name == "backward_deterministic" or layout == "planar":        # (planar: the plane route in both modes)
                assert torch.equal(gf, want["gf"]), name
            else:
                ref = want["gf"].double().cpu().numpy()
                record_err("lens guard bands default scatter", _err(gf.cpu().numpy(), ref), _bound(ref))
        r = _guarded(gpu, bins, {"gp": (torch.float32, (B, V, 3, 4)), "gc": (torch.float32, (B,) + vol + (3,))},
                     _queries(L, "backward_geometry", D, "backward_geometry"), poison,
                     lambda q: L.mvhmr_unproject_backward_geometry_lens(D, q["g"], q["f"], q["p"], q["c"], *sel(q), q["gp"], q["gc"], q["ws"], q["ws_bytes"], q["stream"]))
        assert torch.equal(r["gp"], want["gp"]) and torch.equal(r["gc"], want["gc"])
    # the cuboid entry points
    rot, cen, cub = _pose(B, c, seed=3)
    rt, cet = _t(rot, gpu), _t(cen, gpu)
    pos, sides = (ctypes.c_double * 3)(*cub[0]), (ctypes.c_double * 3)(*cub[1])
    wantc = _run_cuboid(gpu, f, p, rot, cen, cub, lens, go, "softmax", det=True) if layout == "planar" else None
    cins = {"f": fin, "p": pt, "r": rt, "ce": cet, "l": lt, "g": gt}
    place = lambda q: (q["r"], q["ce"], pos, sides)                         # noqa: E731
    r = _guarded(gpu, cins, {"out": (torch.float32, out_shape)}, _queries(L, "forward_cuboid", D, "forward"), 0xFF,
                 lambda q: L.mvhmr_unproject_forward_cuboid_lens(D, q["f"], q["p"], *place(q), *sel(q), q["out"], q["ws"], q["ws_bytes"], q["stream"]))
    if wantc:
        assert torch.equal(r["out"], wantc["out"])
    for name, plain_name in (("backward_cuboid", "backward"), ("backward_cuboid_deterministic", "backward_deterministic")):
        r = _guarded(gpu, cins, {"gf": (torch.float32, gshape)}, _queries(L, name, D, plain_name), 0xFF,
                     lambda q, fn=getattr(L, "mvhmr_unproject_%s_lens" % name): fn(D, q["g"], q["f"], q["p"], *place(q), *sel(q), q["gf"], q["ws"], q["ws_bytes"], q["stream"]))
        if wantc:
            assert torch.equal(r["gf"], wantc["gf"]), name
    r = _guarded(gpu, cins, {"gp": (torch.float32, (B, V, 3, 4)), "gr": (torch.float32, (B, 3, 3)), "gce": (torch.float32, (B, 3))},
                 _queries(L, "backward_geometry_cuboid", D, "backward_geometry_cuboid"), 0xFF,
                 lambda q: L.mvhmr_unproject_backward_geometry_cuboid_lens(D, q["g"], q["f"], q["p"], *place(q), *sel(q), q["gp"], q["gr"], q["gce"], q["ws"],
                                                                           q["ws_bytes"], q["stream"]))
    if wantc:
        assert torch.equal(r["gp"], wantc["gp"]) and torch.equal(r["gr"], wantc["gr"]) and torch.equal(r["gce"], wantc["gce"])
