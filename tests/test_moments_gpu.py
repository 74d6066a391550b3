"""The cross-view variance aggregates (unprojection(..., 'var' | 'meanvar'), mvhmr_unproject_*_moments) on the device: bit
equality with the float64 oracle on the exact lattice rig, parity with the float64 oracle (tests/moments_oracle.py) on general inputs --
forward, feature gradient and the geometry gradients of both routes --, the identities with the 'mean' call, between the two methods and
between the routes, the edges (one view, no view, data only unseen views would tap), deterministic mode and its scale bound, storage
modes, variants, graph capture and VolumeGenerator."""
import numpy as np
import pytest
import torch

import lattice_rig
import moments_oracle as mo
import posegrad_oracle
from conftest import record_err
from multiviewhmr_amd import aggregation
from test_geometry_grad_gpu import REL
from test_moments_cpu import LATTICE, LATTICE_GEO, LATTICE_V2, lattice_cases, lattice_geometry_reference, lattice_reference, var_bound
from test_unproject_gpu import _bound, _err, _ring_problem
from test_view_mask_gpu import SHAPES, _mask

pytestmark = pytest.mark.gpu

METHODS = ("var", "meanvar")
MORE_SHAPES = [
    dict(B=1, V=8, C=300, H=24, W=24, vol=(4, 8, 16)),     # two channel groups; the variance half starts at channel 300
    dict(B=1, V=3, C=20, H=24, W=40, vol=(9, 7, 13)),      # tile tail
    dict(B=2, V=1, C=5, H=12, W=12, vol=(4, 4, 5)),        # n = 1, C % 4 != 0: variance exactly 0
    dict(B=1, V=12, C=8, H=16, W=16, vol=(4, 4, 8)),       # run-time-V instance
]
SCALES = (1.6, 4.0)                                        # every count populated / voxel-views behind a camera
MODES = ("plain", "masked", "visible", "both")


def _id(s):
    return "B%dV%dC%d" % (s["B"], s["V"], s["C"])


def _problem(shape, scale, seed=None):
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=shape["V"] if seed is None else seed)
    return feats, proj, (coords * np.float32(scale)).astype(np.float32)


def _mode_mask(mode, B, V, seed):
    """the view mask of a mode (numpy bool or None); a one-sample problem keeps its full first row"""
    if mode not in ("masked", "both"):
        return None
    m = np.random.default_rng(seed).random((B, V)) < 0.6
    m[0] = True                                                                            # sample 0 all views,
    if B > 1:
        m[1] = False
        m[1, V - 1] = True                                                                 # sample 1 one view,
    if B > 2:
        m[2] = False                                                                       # sample 2 none (test_view_mask_gpu._mask for any B)
    return m


def _t(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _run(f, p, c, method, variant="auto", out_dtype=None, go=None, geometry=True, mask=None, visible=False):
    f = f.detach().clone().requires_grad_(True)
    p = p.detach().clone().requires_grad_(geometry)
    c = c.detach().clone().requires_grad_(geometry)
    out = aggregation.unprojection(f, p, c, method, variant=variant, out_dtype=out_dtype, view_mask=mask, visible_only=visible)
    if go is None:
        go = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(out.device, out.dtype)
    out.backward(go)
    torch.cuda.synchronize()
    return dict(out=out.detach(), gf=f.grad, gp=p.grad, gc=c.grad, go=go)


def _rel(name, got, ref):
    """the geometry tests' bound: 1e-4 of the largest oracle value of the tensor"""
    scale = float(np.abs(ref).max())
    assert scale > 0, name
    record_err(name, _err(got.double().cpu().numpy(), ref), REL * scale)


class _Deterministic:
    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        self.was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(self.on)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.was)


def grad_bound(gref, eps, gv_max, taps_max):
    """_bound(gref) plus the samples' bar eps propagated through ds_v = (2 g_v / n)(s_v - mu) + g_m / n: s_v - mu is off by at most 2 eps and
    n >= 1, so ds_v is off by at most 4 max|g_v| eps; a pixel's gradient sums ds_v w over the taps that meet in it, every weight <= 1."""
    return _bound(gref) + 4.0 * gv_max * eps * taps_max


# ------------------------------------------------------------------------------------ 1. bit equality on the exact rig
@pytest.mark.parametrize("deterministic", [True, False], ids=["det", "default"])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("cfg", [LATTICE, LATTICE_V2], ids=["v4", "v2"])
def test_bit_equality_on_the_lattice_rig(cfg, method, deterministic, gpu):
    """torch.equal with the float64 oracle cast once, at the voxels whose n is a power of two (every voxel in the plain mode), for both halves
    of the volume and for features.grad in both modes: the sums are exact, so arrival order cannot matter.  grad_out is zero at the voxels
    that are not compared.  tests/test_moments_cpu.py::test_lattice_premise holds the budgets."""
    for tag, kw in lattice_cases(cfg["B"], cfg["V"]):
        (feats, proj, coords), grad, ref = lattice_reference(cfg, method, kw)
        f, p, c, go = (_t(x, gpu) for x in (feats, proj, coords, grad))
        mask = None if "view_mask" not in kw else torch.from_numpy(kw["view_mask"])
        with _Deterministic(deterministic):
            r = _run(f, p, c, method, go=go, geometry=False, mask=mask, visible=kw.get("visible_only", False))
        cmp_ = torch.from_numpy(np.broadcast_to(ref["compared"][:, None], ref["out"].shape).copy()).to(gpu)
        want = torch.from_numpy(ref["out"]).to(torch.float32).to(gpu)
        assert cmp_.float().mean() >= 0.5, tag
        assert torch.equal(r["out"][cmp_], want[cmp_]), (tag, method, "forward")
        assert torch.equal(r["gf"], torch.from_numpy(ref["grad_features"]).to(torch.float32).to(gpu)), (tag, method, "features.grad")


@pytest.mark.parametrize("method", METHODS)
def test_geometry_bit_equality_on_the_lattice_rig(method, gpu):
    """The lattice case on power-of-two maps (kx and ky dyadic; lattice_rig.GEO_RIGS' construction): grad_proj and grad_coords of
    k_bwd_geom_moments carry the bits of the float64 oracle, plain, masked and under visible_only.  grad_out is zero at the voxels whose
    participating count is no power of two, where the division by n rounds.  tests/test_moments_cpu.py::test_lattice_geometry_premise
    holds the budget and the agreement of the two oracles."""
    for tag, kw in lattice_cases(LATTICE_GEO["B"], LATTICE_GEO["V"]):
        (feats, proj, coords), grad, ref = lattice_geometry_reference(method, kw)
        f, p, c, go = (_t(x, gpu) for x in (feats, proj, coords, grad))
        mask = None if "view_mask" not in kw else torch.from_numpy(kw["view_mask"])
        r = _run(f, p, c, method, variant="gather", go=go, mask=mask, visible=kw.get("visible_only", False))
        for key, name in (("gp", "grad_proj"), ("gc", "grad_coords")):
            want = ref[name].astype(np.float32)
            assert np.array_equal(want.astype(np.float64), ref[name]), "the oracle's value is not an fp32 number: rig error"
            record_err("lattice moments geometry %s %s %s" % (method, tag, name), _err(r[key].double().cpu().numpy(), ref[name]), 0.0)
            assert torch.equal(r[key].view(torch.int32), torch.from_numpy(want).to(gpu).view(torch.int32)), (tag, method, name)


# ------------------------------------------------------------------------------------ 2. the float64 oracle on general inputs
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES + MORE_SHAPES, ids=_id)
def test_oracle_parity(shape, scale, mode, gpu):
    """Both methods, tensor route: forward, feature gradient, proj and coords gradients.  No voxel is left out (the geometries keep the
    edge voxels under the 2 % cap of test_visible_gpu.py, which is therefore not needed): a voxel whose seeing set fp32 and float64 would
    decide differently does not exist for this oracle, which decides it from the fp32 positions.

    Tolerances, from the project's own bars.  Mean half: _bound(ref).  Variance half: with eps = _bound(the oracle's per-view samples) and
    D = max |s_v - mu| of the oracle, every s_v is off by at most eps, mu by at most eps, d_v by at most 2 eps, d_v^2 by at most
    4 eps D + 4 eps^2, and so is their mean (test_moments_cpu.var_bound).  Feature gradient: _bound(gref) + 4 max|g_v| eps T with T the
    largest number of taps that meet in a pixel (grad_bound).  Geometry gradients: REL (1e-4) of the oracle's largest value."""
    B, V, C, H, W = (shape[k] for k in "BVCHW")
    feats, proj, coords = _problem(shape, scale)
    mask = _mode_mask(mode, B, V, seed=C)
    visible = mode in ("visible", "both")
    f, p, c = (_t(x, gpu) for x in (feats, proj, coords))
    for method in METHODS:
        r = _run(f, p, c, method, mask=None if mask is None else torch.from_numpy(mask), visible=visible)
        go = r["go"].cpu().numpy()
        ref = mo.moments_unprojection(feats, proj, coords, go, method, mask=mask, visible=visible)
        if visible and mask is None and scale == 1.6 and V > 1:
            counts = np.bincount(ref["count"].ravel(), minlength=V + 1)
            assert counts[0] > 0 and counts[V] > 0, counts
        eps = _bound(np.float64(ref["samples_max"]))
        tag = "moments %s %s x%.1f B%d V%d C%d" % (method, mode, scale, B, V, C)
        out = r["out"].cpu().numpy()
        if method == "meanvar":
            record_err(tag + " fwd mean", _err(out[:, :C], ref["mean"]), _bound(ref["mean"]))
        record_err(tag + " fwd var", _err(out[:, -C:], ref["var"]), var_bound(eps, ref["dev_max"]))
        assert out[:, -C:].min() >= 0                                                      # non-negative by construction
        gv_max = float(np.abs(go[:, -C:]).max())
        record_err(tag + " bwd", _err(r["gf"].cpu().numpy(), ref["grad_features"]),
                   grad_bound(ref["grad_features"], eps, gv_max, int(ref["tap_count"].max())))
        if np.abs(ref["grad_proj"]).max() > 0:                                             # (one view and the variance alone: every gradient is zero)
            _rel(tag + " proj grad", r["gp"], ref["grad_proj"])
            _rel(tag + " coord grad", r["gc"], ref["grad_coords"])
        else:
            assert V == 1 and method == "var" and torch.count_nonzero(r["gp"]) == 0 and torch.count_nonzero(r["gc"]) == 0
        nobody = torch.from_numpy((ref["count"] == 0).reshape((B,) + tuple(shape["vol"]))).to(gpu)
        if nobody.any():                                                                   # exact zeros where no view takes part
            assert torch.count_nonzero(r["out"].permute(0, 2, 3, 4, 1)[nobody]) == 0 and torch.count_nonzero(r["gc"][nobody]) == 0
        if mask is not None:
            m = torch.from_numpy(mask).to(gpu)
            assert torch.count_nonzero(r["gf"][~m]) == 0 and torch.count_nonzero(r["gp"][~m]) == 0


@pytest.mark.parametrize("mode", ["plain", "both"])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], MORE_SHAPES[3]], ids=_id)
def test_cuboid_route_pose_gradients(shape, method, mode, gpu):
    """rot / center gradients of the cuboid route against the oracle's grad_coords carried through X = R d + c (posegrad_oracle's chain)"""
    B, V, C, H, W = (shape[k] for k in "BVCHW")
    feats, proj, _ = _ring_problem(B, V, C, H, W, shape["vol"], seed=40 + V)
    rng = np.random.default_rng(41)
    th = rng.uniform(0, 2 * np.pi, B)
    rot = np.stack([[[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]] for t in th]).astype(np.float32)
    cen = rng.uniform(-100, 100, (B, 3)).astype(np.float32)
    position, sides = (-2000.0, -2000.0, -2000.0), (4000.0, 4000.0, 4000.0)
    mask = _mode_mask(mode, B, V, seed=42)
    visible = mode == "both"
    f = _t(feats, gpu).requires_grad_(True)
    p, r, ce = (_t(x, gpu).requires_grad_(True) for x in (proj, rot, cen))
    out = aggregation.unprojection_cuboid(f, p, r, ce, position, sides, shape["vol"], method, view_mask=None if mask is None else torch.from_numpy(mask),
                                          visible_only=visible)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(43)).to(gpu)
    out.backward(go)
    d, X = posegrad_oracle.cuboid_points(rot, cen, position, sides, shape["vol"])
    ref = mo.moments_unprojection(feats, proj, X.numpy(), go.cpu().numpy(), method, mask=mask, visible=visible)
    gX = torch.from_numpy(ref["grad_coords"]).reshape(B, -1, 3)
    g_rot = torch.einsum("bnr,bnk->brk", gX, d.double().reshape(B, -1, 3)).numpy()
    s_g = gX.sum(1)
    g_cen = (s_g - torch.einsum("brk,br->bk", torch.from_numpy(rot).double(), s_g)).numpy()
    tag = "moments cuboid %s %s V%d C%d" % (method, mode, V, C)
    eps = _bound(np.float64(ref["samples_max"]))
    record_err(tag + " fwd var", _err(out.detach().cpu().numpy()[:, -C:], ref["var"]), var_bound(eps, ref["dev_max"]))
    _rel(tag + " proj grad", p.grad, ref["grad_proj"])
    _rel(tag + " rot grad", r.grad, g_rot)
    _rel(tag + " center grad", ce.grad, g_cen)


# ------------------------------------------------------------------------------------ 3. identities
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES + MORE_SHAPES[2:], ids=_id)
def test_identities_between_the_methods_and_with_the_mean_call(shape, mode, gpu):
    """meanvar[:, :C] is the 'mean' call with variant='gather' under the same options, 'var' is meanvar[:, C:], and the 'var' gradients are
    the 'meanvar' gradients when grad_out's mean half is zero -- all bit for bit (the gradients in deterministic mode)"""
    B, V, C = shape["B"], shape["V"], shape["C"]
    feats, proj, coords = _problem(shape, 1.6, seed=21)
    mask = _mode_mask(mode, B, V, seed=22)
    kw = dict(mask=None if mask is None else torch.from_numpy(mask), visible=mode in ("visible", "both"))
    f, p, c = (_t(x, gpu) for x in (feats, proj, coords))
    with _Deterministic():
        var = _run(f, p, c, "var", **kw)
        go2 = torch.cat([torch.zeros_like(var["go"]), var["go"]], 1)
        both = _run(f, p, c, "meanvar", go=go2, **kw)
        mean = _run(f, p, c, "mean", variant="gather", **kw)
    assert torch.equal(both["out"][:, :C], mean["out"]), "mean half"
    assert torch.equal(both["out"][:, C:], var["out"]), "variance half"
    for k in ("gf", "gp", "gc"):
        assert torch.equal(var[k], both[k]), k
    for variant in ("gather",):                                                            # 'auto' runs the gather family
        assert torch.equal(aggregation.unprojection(f, p, c, "meanvar", variant=variant, view_mask=kw["mask"], visible_only=kw["visible"]), both["out"])


def test_one_view_has_no_variance_and_no_gradient_from_it(gpu):
    shape = MORE_SHAPES[2]
    feats, proj, coords = _problem(shape, 1.6, seed=23)
    f, p, c = (_t(x, gpu) for x in (feats, proj, coords))
    C = shape["C"]
    for visible in (False, True):
        r = _run(f, p, c, "var", visible=visible)
        assert torch.count_nonzero(r["out"]) == 0 and torch.count_nonzero(r["gf"]) == 0
        assert torch.count_nonzero(r["gp"]) == 0 and torch.count_nonzero(r["gc"]) == 0
        b = _run(f, p, c, "meanvar", visible=visible)
        assert torch.count_nonzero(b["out"][:, C:]) == 0 and torch.count_nonzero(b["out"][:, :C]) > 0
        go = b["go"].clone()
        go[:, :C] = 0
        z = _run(f, p, c, "meanvar", visible=visible, go=go)
        assert torch.count_nonzero(z["gf"]) == 0                                           # features.grad from g_v is exactly 0


@pytest.mark.parametrize("method", METHODS)
def test_no_participating_view_gives_exact_zeros_and_unseen_views_are_never_read(method, gpu):
    """a sample with no present view, and voxels no view sees: both halves zero, gradients exact zeros; NaN / Inf planted in every pixel no
    participating voxel-view taps (the oracle's tap_count is zero there; pixel (0, 0), the dummy tap, among them) change no bit"""
    shape = SHAPES[0]
    B, V, C = shape["B"], shape["V"], shape["C"]
    feats, proj, coords = _problem(shape, 4.0, seed=27)
    mask = _mask(B, V, seed=28)                                                            # sample 2 has no views
    f, p, c = (_t(x, gpu) for x in (feats, proj, coords))
    m = torch.from_numpy(mask)
    go = torch.randn((B, (2 if method == "meanvar" else 1) * C) + tuple(shape["vol"]), generator=torch.Generator().manual_seed(7))
    ref = mo.moments_unprojection(feats, proj, coords, go.numpy(), method, mask=mask, visible=True, geometry=False)
    untapped = np.broadcast_to((ref["tap_count"] == 0)[:, :, None], feats.shape)
    assert 0.005 < untapped.mean() < 0.999
    u = torch.from_numpy(untapped.copy()).to(gpu)
    for deterministic in (True, False):
        with _Deterministic(deterministic):
            clean = _run(f, p, c, method, mask=m, visible=True, go=go.to(gpu))
            assert torch.count_nonzero(clean["out"][2]) == 0 and torch.count_nonzero(clean["gf"][2]) == 0
            assert torch.count_nonzero(clean["gp"][2]) == 0 and torch.count_nonzero(clean["gc"][2]) == 0
            nobody = torch.from_numpy((ref["count"] == 0).reshape((B,) + tuple(shape["vol"]))).to(gpu)
            assert nobody[0].any() and torch.count_nonzero(clean["out"].permute(0, 2, 3, 4, 1)[nobody]) == 0
            assert torch.count_nonzero(clean["gc"][nobody]) == 0
            for fill in (float("nan"), float("inf")):
                g = f.clone()
                g[u] = fill
                r = _run(g, p, c, method, mask=m, visible=True, go=go.to(gpu))
                keys = ("out", "gf", "gp", "gc") if deterministic else ("out", "gp", "gc")      # (float atomics: features.grad is not bitwise repeatable)
                for k in keys:
                    assert torch.isfinite(r[k]).all() and torch.equal(r[k], clean[k]), (k, fill)
                assert torch.isfinite(r["gf"]).all()


@pytest.mark.parametrize("method", METHODS)
def test_tensor_and_cuboid_routes_agree_bit_for_bit(method, gpu):
    B, V, C, H, W, S = 3, 4, 8, 24, 20, 16
    feats, proj, _ = _ring_problem(B, V, C, H, W, (S, S, S), seed=24)
    rng = np.random.default_rng(25)
    th = rng.uniform(0, 2 * np.pi, B)
    rot = np.stack([[[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]] for t in th]).astype(np.float32)
    cen = rng.uniform(-100, 100, (B, 3)).astype(np.float32)
    f, p, r, ce = (_t(x, gpu) for x in (feats, proj, rot, cen))
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=4000.0, device=gpu)
    cub = gen.cuboid()
    coords = gen.coord_volumes(r, ce, gpu)
    mask = torch.from_numpy(_mask(B, V, seed=26))
    for kw in (dict(), dict(visible_only=True), dict(view_mask=mask), dict(visible_only=True, view_mask=mask)):
        a = aggregation.unprojection(f, p, coords, method, **kw)
        b = aggregation.unprojection_cuboid(f, p, r, ce, cub.position, cub.sides, (S, S, S), method, **kw)
        assert torch.equal(a, b) and torch.count_nonzero(a) > 0, kw


def test_a_run_time_instance_equals_the_fixed_instances(gpu):
    """12 views with 8 masked, the 4 present ones packed into the first slots of the run-time-V instance, against the same problem as a
    4-view call (the fixed V = 4 instance): the same bits, forward and (deterministic mode) features.grad"""
    shape = MORE_SHAPES[3]
    B, V, C = shape["B"], shape["V"], shape["C"]
    feats, proj, coords = _problem(shape, 1.6, seed=29)
    present = [1, 4, 6, 11]
    mask = np.zeros((B, V), bool)
    mask[:, present] = True
    f, p, c = (_t(x, gpu) for x in (feats, proj, coords))
    idx = torch.tensor(present, device=gpu)
    for method in METHODS:
        for visible in (False, True):
            with _Deterministic():
                a = _run(f, p, c, method, mask=torch.from_numpy(mask), visible=visible)
                b = _run(f[:, idx].contiguous(), p[:, idx].contiguous(), c, method, visible=visible, go=a["go"])
            assert torch.equal(a["out"], b["out"]), (method, visible)
            assert torch.equal(a["gf"][:, idx], b["gf"]), (method, visible)
            for k, x, y in (("proj grad", a["gp"][:, idx], b["gp"]), ("coord grad", a["gc"], b["gc"])):     # (the geometry kernels split the channels
                y = y.double().cpu().numpy()                                                                  # over the lanes by V: fp32 sums in another order)
                record_err("moments run-time vs fixed %s visible=%d %s" % (method, visible, k), _err(x.cpu().numpy(), y), REL * float(np.abs(y).max()))
            assert torch.count_nonzero(a["out"]) > 0 and torch.count_nonzero(a["gf"][:, idx]) > 0


# ------------------------------------------------------------------------------------ 4. deterministic mode
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_deterministic_mode_repeats_bitwise(method, masked, gpu):
    shape = SHAPES[0]
    feats, proj, coords = _problem(shape, 1.6, seed=30)
    mask = _mask(shape["B"], shape["V"], seed=31) if masked else None
    f, p, c = (_t(x, gpu) for x in (feats, proj, coords))
    for visible in (False, True):
        with _Deterministic():
            a = _run(f, p, c, method, mask=None if mask is None else torch.from_numpy(mask), visible=visible)
            b = _run(f, p, c, method, mask=None if mask is None else torch.from_numpy(mask), visible=visible, go=a["go"])
        for k in ("out", "gf", "gp", "gc"):
            assert torch.equal(a[k], b[k]), k
        ref = mo.moments_unprojection(feats, proj, coords, a["go"].cpu().numpy(), method, mask=mask, visible=visible, geometry=False)
        eps = _bound(np.float64(ref["samples_max"]))
        C = shape["C"]
        record_err("moments deterministic bwd %s masked=%d visible=%d" % (method, masked, visible), _err(a["gf"].cpu().numpy(), ref["grad_features"]),
                   grad_bound(ref["grad_features"], eps, float(a["go"][:, -C:].abs().max()), int(ref["tap_count"].max())))


def test_deterministic_scale_bound_carries_the_variance_half(gpu):
    """|ds| <= max|g_m| + 4 max|g_v| Fmax: with the variance half of grad_out at 1e30 (a few binades below the poison limit of fp32, features
    O(1)) a scale chosen from the mean half alone would let the int64 sums wrap.  Finite gradients that repeat bitwise and match the
    oracle to its own relative bar."""
    shape = SHAPES[0]
    B, C = shape["B"], shape["C"]
    feats, proj, coords = _problem(shape, 1.6, seed=32)
    go = torch.randn((B, 2 * C) + tuple(shape["vol"]), generator=torch.Generator().manual_seed(33)).clamp(-4, 4)
    go[:, C:] *= 2.5e29
    ref = mo.moments_unprojection(feats, proj, coords, go.numpy(), "meanvar", visible=True, geometry=False)
    f, p, c = (_t(x, gpu) for x in (feats, proj, coords))
    with _Deterministic():
        a = _run(f, p, c, "meanvar", go=go.to(gpu), geometry=False, visible=True)
        b = _run(f, p, c, "meanvar", go=go.to(gpu), geometry=False, visible=True)
    assert torch.isfinite(a["gf"]).all() and torch.equal(a["gf"], b["gf"]) and torch.count_nonzero(a["gf"]) > 0
    eps = _bound(np.float64(ref["samples_max"]))
    record_err("moments deterministic scale bound", _err(a["gf"].cpu().numpy(), ref["grad_features"]),
               grad_bound(ref["grad_features"], eps, float(go[:, C:].abs().max()), int(ref["tap_count"].max())))


# ------------------------------------------------------------------------------------ 5. storage and plumbing
@pytest.mark.parametrize("storage", ["f16", "bf16vol"])
@pytest.mark.parametrize("method", METHODS)
def test_storage_modes_round_the_fp32_result_once(method, storage, gpu):
    """fp16 features with an fp16 volume against the fp32-volume call on the same fp16 features, fp32 features with a bf16 volume against
    the fp32 call: the stored volume is the fp32 result rounded once to nearest even, both halves"""
    shape = SHAPES[0]
    feats, proj, coords = _problem(shape, 1.6, seed=34)
    f, p, c = (_t(x, gpu) for x in (feats, proj, coords))
    for visible in (False, True):
        if storage == "f16":
            low = aggregation.unprojection(f.half(), p, c, method, visible_only=visible)
            full = aggregation.unprojection(f.half(), p, c, method, visible_only=visible, out_dtype=torch.float32)
            assert low.dtype == torch.float16 and full.dtype == torch.float32 and torch.equal(low, full.half())
        else:
            low = aggregation.unprojection(f, p, c, method, visible_only=visible, out_dtype=torch.bfloat16)
            full = aggregation.unprojection(f, p, c, method, visible_only=visible)
            assert low.dtype == torch.bfloat16 and torch.equal(low, full.bfloat16())
        assert torch.count_nonzero(low) > 0
    # and the backward takes the stored grad_out
    x = (f.half() if storage == "f16" else f).clone().requires_grad_(True)
    out = aggregation.unprojection(x, p, c, method, out_dtype=None if storage == "f16" else torch.bfloat16)
    out.backward(torch.ones_like(out))
    assert x.grad.dtype == x.dtype and torch.isfinite(x.grad).all() and torch.count_nonzero(x.grad) > 0


def test_brick_is_refused_and_auto_runs_the_gather_family(gpu):
    shape = SHAPES[0]
    feats, proj, coords = _problem(shape, 1.6)
    f, p, c = (_t(x, gpu) for x in (feats, proj, coords))
    for method in METHODS:
        with pytest.raises(RuntimeError, match="gather kernels"):
            aggregation.unprojection(f, p, c, method, variant="brick")
        assert torch.equal(aggregation.unprojection(f, p, c, method, variant="auto"), aggregation.unprojection(f, p, c, method, variant="gather"))
        cl = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)   # channels-last features: read as they are
        assert torch.equal(aggregation.unprojection(cl, p, c, method), aggregation.unprojection(f, p, c, method))


def test_forward_graph_capture(gpu):
    shape = SHAPES[0]
    feats, proj, coords = _problem(shape, 1.6, seed=36)
    mask = torch.from_numpy(_mask(shape["B"], shape["V"], seed=37)).to(gpu)
    f, p, c = (_t(x, gpu) for x in (feats, proj, coords))
    for m, visible in ((None, False), (mask, True)):
        eager = aggregation.unprojection(f, p, c, "meanvar", visible_only=visible, view_mask=m)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            aggregation.unprojection(f, p, c, "meanvar", visible_only=visible, view_mask=m)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = aggregation.unprojection(f, p, c, "meanvar", visible_only=visible, view_mask=m)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_volume_generator_meanvar_visible_only_end_to_end(gpu):
    """VolumeGenerator('meanvar', visible_only=True) with a view mask in the batch against the oracle on the generator's own conv output,
    projections and pose; the fused conv route is not taken and volume_channels says what comes back"""
    from test_visible_gpu import _generator_problem
    gen, batch, feats, proj_org = _generator_problem(gpu, True)
    gen.aggregation_method = "meanvar"
    B, V = feats.shape[:2]
    S, C = gen.volume_size, gen.output_channels
    mask = np.ones((B, V), bool)
    mask[1, 2] = False
    batch = dict(batch, view_mask=torch.from_numpy(mask))
    out = gen(feats, proj_org, batch)
    assert gen.volume_channels == 2 * C and tuple(out.shape) == (B, 2 * C, S, S, S)
    conv = gen.process_feature(feats.view(-1, *feats.shape[2:]))
    conv = conv.view(B, V, *conv.shape[1:]).detach()
    proj = aggregation.feature_level_projections_device(batch["cameras_packed"], (96, 96), tuple(feats.shape[-2:])).to(gpu).contiguous()
    rots, centers = gen.volume_pose(batch, proj_org, (96, 96), batch["view_mask"])
    coords = gen.coord_volumes(rots, centers, gpu)
    ref = mo.moments_unprojection(conv.cpu().numpy(), proj.cpu().numpy(), coords.cpu().numpy(), None, "meanvar", mask=mask, visible=True)
    assert (ref["count"] == 0).any() and (ref["count"] == V).any()
    eps = _bound(np.float64(ref["samples_max"]))
    o = out.detach().cpu().numpy()
    record_err("moments volgen mean", _err(o[:, :C], ref["mean"]), _bound(ref["mean"]))
    record_err("moments volgen var", _err(o[:, C:], ref["var"]), var_bound(eps, ref["dev_max"]))
    gen.aggregation_method = "var"
    assert gen.volume_channels == C and torch.equal(gen(feats, proj_org, batch), out[:, C:])
