"""Visibility-aware aggregation (unprojection(visible_only=True), mvhmr_unproject_*_visible) on the device: the reference's
goldens stitched from per-pattern runs, the float64 oracle (tests/visibility_oracle.py) on cuboids that leave the cameras' frames and
reach behind them, the rule exactly at the map's edges and at z = 0, the identities with the plain call, the masked call and the cuboid
route, data only unseen views would tap never read, bitwise repeats and the scale bound in deterministic mode, storage modes,
VolumeGenerator and graph capture."""
import numpy as np
import pytest
import torch

import visibility_oracle as vis
from conftest import golden_cases, load_golden, record_err
from multiviewhmr_amd import aggregation
from test_geometry_grad_gpu import REL
from test_unproject_gpu import _bound, _err, _ring_problem
from test_view_mask_gpu import SHAPES, _mask

pytestmark = pytest.mark.gpu

METHODS = ("softmax", "sum", "mean", "max")
MORE_SHAPES = [
    dict(B=1, V=8, C=300, H=24, W=24, vol=(4, 8, 16)),     # two channel groups
    dict(B=1, V=3, C=20, H=24, W=40, vol=(9, 7, 13)),      # tile tail, non-square map
    dict(B=3, V=2, C=16, H=32, W=32, vol=(8, 8, 8)),       # V = 2
]
SCALES = (1.6, 4.0)                                        # every count populated / voxel-views behind a camera


def _id(s):
    return "V%dC%d" % (s["V"], s["C"])


def _problem(shape, scale, seed=None):
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=shape["V"] if seed is None else seed)
    return feats, proj, (coords * np.float32(scale)).astype(np.float32)


def _run(f, p, c, method, variant="auto", out_dtype=None, go=None, geometry=True, mask=None, visible=True):
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
    def __enter__(self):
        self.was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(True)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.was)


# ------------------------------------------------------------------------------------ 1. the reference's goldens
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("variant", ["auto", "gather"])
@pytest.mark.parametrize("case", golden_cases("visibility"))
def test_goldens_on_the_seeing_views(case, variant, method, gpu):
    d = load_golden("visibility", case)
    f, p, c, go = (torch.from_numpy(d[k]).to(gpu) for k in ("features", "proj", "coords", "grad_out"))
    bits = aggregation.view_visibility(p, c, tuple(f.shape[-2:]))
    assert bits.dtype == torch.int32 and bits.shape == c.shape[:4] and np.array_equal(bits.cpu().numpy(), d["bits"])
    r = _run(f, p, c, method, variant, go=go, geometry=False)
    ref, gref = d["out_" + method], d["gfeat_" + method]
    record_err("visibility golden fwd %s %s %s" % (case, method, variant), _err(r["out"].cpu().numpy(), ref), _bound(ref))
    record_err("visibility golden bwd %s %s %s" % (case, method, variant), _err(r["gf"].cpu().numpy(), gref), _bound(gref))


# ------------------------------------------------------------------------------------ 2. the float64 oracle
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES + MORE_SHAPES, ids=_id)
def test_oracle_parity(shape, scale, method, gpu):
    """A voxel is left out only if one of its views lies within 1e-3 px of a map edge or has |z| < 1e-3 max |z| in float64 (at most 2 % of
    them): its grad_out is zeroed, so it adds nothing to any gradient on either side, and its volume entries are not compared."""
    B, V, C, H, W = (shape[k] for k in "BVCHW")
    feats, proj, coords = _problem(shape, scale)
    edge = vis.edge_voxels(proj, coords, H, W)                                         # (B, N)
    assert edge.mean() <= 0.02, edge.mean()
    keep = torch.from_numpy(~edge).reshape((B, 1) + tuple(shape["vol"]))
    go = torch.randn((B, C) + tuple(shape["vol"]), generator=torch.Generator().manual_seed(7)) * keep
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    r = _run(f, p, c, method, go=go.to(gpu))
    ref = vis.visible_unprojection(feats, proj, coords, go.numpy(), method)
    kept = ~edge.reshape((B,) + tuple(shape["vol"]))
    bits = aggregation.view_visibility(p, c, (H, W)).cpu().numpy()
    assert np.array_equal(bits[kept], ref["bits"][kept])
    counts = np.bincount(ref["seen"].sum(1).ravel(), minlength=V + 1)
    if scale == 1.6:
        assert counts[0] > 0 and counts[V] > 0 and (counts > 0).sum() >= V, counts      # nobody, every view, and all counts between but at most one
    else:
        z = np.einsum("bvj,bnj->bvn", proj[:, :, 2, :3].astype(np.float64), coords.reshape(B, -1, 3).astype(np.float64)) + proj[:, :, 2, 3:4]
        assert (z <= 0).mean() > 0.02, (z <= 0).mean()                                   # voxel-views behind a camera
    tag = "visibility %s x%.1f V%d C%d" % (method, scale, V, C)
    km = np.broadcast_to(kept[:, None], ref["out"].shape)
    record_err(tag + " fwd", _err(r["out"].cpu().numpy()[km], ref["out"][km]), _bound(ref["out"]))
    record_err(tag + " bwd", _err(r["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))
    _rel(tag + " proj grad", r["gp"], ref["grad_proj"])
    _rel(tag + " coord grad", r["gc"], ref["grad_coords"])
    # exact zeros: volume and grad_coords where no view sees the voxel
    unseen = torch.from_numpy((ref["bits"] == 0) & kept).to(gpu)
    assert unseen.any()
    assert torch.count_nonzero(r["out"].permute(0, 2, 3, 4, 1)[unseen]) == 0 and torch.count_nonzero(r["gc"][unseen]) == 0


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=_id)
def test_a_view_that_sees_nothing_gets_exact_zeros(shape, method, gpu):
    """one (b, v) looks the other way (its depth row negated: z < 0 for every voxel it saw): its grad_features and its grad_proj row are
    exact zeros, and the sample is the call without that view"""
    B, V = shape["B"], shape["V"]
    feats, proj, coords = _problem(shape, 1.6, seed=20)
    proj[1, V - 1, 2] *= -1
    blind = ~vis.seen_views(proj, coords, shape["H"], shape["W"]).any(2)
    assert blind[1, V - 1] and blind.sum() == 1
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    r = _run(f, p, c, method)
    assert torch.count_nonzero(r["gf"][1, V - 1]) == 0 and torch.count_nonzero(r["gp"][1, V - 1]) == 0
    assert torch.count_nonzero(r["gf"][1, 0]) > 0 and torch.count_nonzero(r["gp"][1, 0]) > 0
    s = _run(f[1:2, :V - 1], p[1:2, :V - 1], c[1:2], method, go=r["go"][1:2])
    tag = "visibility blind view %s V%d " % (method, V)
    for name, x, y in (("fwd", r["out"][1], s["out"][0]), ("bwd", r["gf"][1, :V - 1], s["gf"][0]), ("coord grad", r["gc"][1], s["gc"][0])):
        y = y.cpu().numpy()
        record_err(tag + name, _err(x.cpu().numpy(), y), _bound(y))


# ------------------------------------------------------------------------------------ 3. the rule at the edge, exactly
@pytest.mark.parametrize("V", [3, 4])
def test_the_rule_at_the_map_edges_and_at_zero_depth(V, gpu):
    """P = rows (1,0,0,0), (0,1,0,0), (0,0,0,1): u = X0, v = X1, z = 1; Hf = Wf = 16, so ix = u * 15 / 16 is exactly 0 at u = 0 and exactly
    Wf - 1 at u = 16: seen, both ends inclusive.  Just outside -- u = -2^-20 and the fp32 successor of 16, the nearest coordinates whose fp32
    ix leaves [0, 15] -- not seen.  View 1 has z = 0 (never seen), view 2 z = the smallest positive normal (u = X0 / z: seen where X0 = X1 =
    0, the quotient overflows elsewhere), view 3 z = -1.  Constant feature maps make the mean volume show the count exactly."""
    H = W = 16
    tiny = np.float32(1.1754943508222875e-38)
    lo, hi = np.float32(-2.0 ** -20), np.nextafter(np.float32(16), np.float32(np.inf))
    axis = np.array([lo, 0, 8, 16, hi], np.float32)
    inside = np.array([False, True, True, True, False])
    coords = np.zeros((1, 5, 5, 1, 3), np.float32)
    coords[0, :, :, 0, 0] = axis[:, None]
    coords[0, :, :, 0, 1] = axis[None, :]
    proj = np.zeros((1, V, 3, 4), np.float32)
    proj[0, :, 0, 0] = proj[0, :, 1, 1] = 1
    for v, z in enumerate((1, 0, tiny, -1)[:V]):
        proj[0, v, 2, 3] = z
    values = (1.0, 64.0, 4.0, 1024.0)[:V]
    feats = np.stack([np.full((4, H, W), x, np.float32) for x in values])[None]
    expect_bits = np.zeros((5, 5), np.int32)
    expect_bits[np.ix_(inside, inside)] |= 1
    expect_bits[1, 1] |= 4                                                  # X0 = X1 = 0 under the tiny depth
    expect_mean = np.select([expect_bits == 5, expect_bits == 1], [np.float32(2.5), np.float32(1.0)], np.float32(0))
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    bits = aggregation.view_visibility(p, c, (H, W)).cpu().numpy()[0, :, :, 0]
    assert np.array_equal(bits, expect_bits), bits
    assert np.array_equal(vis.visibility_bits(proj, coords, H, W)[0, :, :, 0], expect_bits)        # the oracle reads the same rule
    for variant in ("auto", "gather"):
        out = aggregation.unprojection(f, p, c, "mean", variant=variant, visible_only=True).cpu().numpy()[0, :, :, :, 0]
        assert np.array_equal(out, np.broadcast_to(expect_mean, out.shape)), out[0]
    plain = aggregation.unprojection(f, p, c, "mean", variant="gather").cpu().numpy()[0, 0, :, :, 0]
    assert plain[1, 1] == np.float32(5) / np.float32(V) and plain[0, 1] != 0          # the plain call: zeros take part, a partly inside footprint gives a sample


# ------------------------------------------------------------------------------------ 4. identities
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_everything_seen_is_the_plain_gather_call(shape, method, gpu):
    feats, proj, coords = _problem(shape, 0.5, seed=21)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    assert (aggregation.view_visibility(p, c, (shape["H"], shape["W"])) == (1 << shape["V"]) - 1).all()
    a = _run(f, p, c, method, "gather")
    b = _run(f, p, c, method, "gather", go=a["go"], visible=False)
    tag = "visibility all seen %s V%d C%d " % (method, shape["V"], shape["C"])
    for k, name in (("out", "fwd"), ("gf", "bwd"), ("gp", "proj grad"), ("gc", "coord grad")):
        ref = b[k].cpu().numpy()
        record_err(tag + name, _err(a[k].cpu().numpy(), ref), _bound(ref))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=_id)
def test_with_a_view_mask_it_is_the_call_on_the_present_views(shape, method, gpu):
    B, V = shape["B"], shape["V"]
    feats, proj, coords = _problem(shape, 1.6, seed=22)
    mask = _mask(B, V, seed=23)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    m = torch.from_numpy(mask).to(gpu)
    r = _run(f, p, c, method, mask=torch.from_numpy(mask))
    bits = aggregation.view_visibility(p, c, (shape["H"], shape["W"]), view_mask=torch.from_numpy(mask))
    full = aggregation.view_visibility(p, c, (shape["H"], shape["W"]))
    present = torch.from_numpy((mask.astype(np.int64) << np.arange(V)).sum(1).astype(np.int32)).to(gpu)
    assert torch.equal(bits, full & present[:, None, None, None])
    assert torch.count_nonzero(r["gf"][~m]) == 0 and torch.count_nonzero(r["gp"][~m]) == 0
    assert torch.count_nonzero(r["out"][2]) == 0 and torch.count_nonzero(r["gc"][2]) == 0          # sample 2 has no views
    for b in (0, 1, 3):
        P = torch.from_numpy(np.nonzero(mask[b])[0]).to(gpu)
        s = _run(f[b:b + 1, P], p[b:b + 1, P], c[b:b + 1], method, go=r["go"][b:b + 1])
        tag = "visibility masked %s V%d b%d " % (method, V, b)
        for name, x, y in (("fwd", r["out"][b], s["out"][0]), ("bwd", r["gf"][b, P], s["gf"][0]), ("proj grad", r["gp"][b, P], s["gp"][0]),
                           ("coord grad", r["gc"][b], s["gc"][0])):
            y = y.cpu().numpy()
            record_err(tag + name, _err(x.cpu().numpy(), y), _bound(y))


@pytest.mark.parametrize("method", METHODS)
def test_tensor_and_cuboid_routes_agree_bit_for_bit(method, gpu):
    B, V, C, H, W, S = 3, 4, 8, 24, 20, 16
    feats, proj, _ = _ring_problem(B, V, C, H, W, (S, S, S), seed=24)
    rng = np.random.default_rng(25)
    th = rng.uniform(0, 2 * np.pi, B)
    rot = np.stack([[[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]] for t in th]).astype(np.float32)
    cen = rng.uniform(-100, 100, (B, 3)).astype(np.float32)
    f, p, r, ce = (torch.from_numpy(x).to(gpu) for x in (feats, proj, rot, cen))
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=4000.0, device=gpu)
    cub = gen.cuboid()
    coords = gen.coord_volumes(r, ce, gpu)
    a = aggregation.unprojection(f, p, coords, method, visible_only=True)
    b = aggregation.unprojection_cuboid(f, p, r, ce, cub.position, cub.sides, (S, S, S), method, visible_only=True)
    assert torch.equal(a, b)
    ba = aggregation.view_visibility(p, coords, (H, W))
    bb = aggregation.view_visibility_cuboid(p, r, ce, cub.position, cub.sides, (S, S, S), (H, W))
    assert torch.equal(ba, bb) and 0 < int((ba == 0).sum()) < ba.numel()
    mask = torch.from_numpy(_mask(B, V, seed=26))
    assert torch.equal(aggregation.unprojection(f, p, coords, method, visible_only=True, view_mask=mask),
                       aggregation.unprojection_cuboid(f, p, r, ce, cub.position, cub.sides, (S, S, S), method, visible_only=True, view_mask=mask))
    assert torch.equal(aggregation.view_visibility(p, coords, (H, W), mask), aggregation.view_visibility_cuboid(p, r, ce, cub.position, cub.sides, (S, S, S), (H, W), mask))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=_id)
def test_what_only_unseen_views_would_tap_is_never_read(shape, method, gpu):
    """NaN / Inf in every pixel no seeing voxel-view taps (the oracle's `sum` backward of a grad_out of ones leaves exactly those at zero;
    pixel (0, 0), the plain kernels' dummy tap, among them where nobody sees it): the results keep their bits"""
    feats, proj, coords = _problem(shape, 4.0, seed=27)
    ones = np.ones((shape["B"], shape["C"]) + tuple(shape["vol"]), np.float32)
    untapped = vis.visible_unprojection(feats, proj, coords, ones, "sum", geometry=False)["grad_features"] == 0
    assert 0.005 < untapped.mean() < 0.95
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    u = torch.from_numpy(untapped).to(gpu)
    with _Deterministic():                                                   # reproducible feature-gradient bits
        clean = _run(f, p, c, method)
        for fill in (float("nan"), float("inf")):
            g = f.clone()
            g[u] = fill
            r = _run(g, p, c, method, go=clean["go"])
            for k in ("out", "gf", "gp", "gc"):
                assert torch.isfinite(r[k]).all() and torch.equal(r[k], clean[k]), (k, fill)


def test_brick_is_refused_and_auto_runs_the_gather_family(gpu):
    shape = SHAPES[0]
    feats, proj, coords = _problem(shape, 1.6)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    with pytest.raises(RuntimeError, match="gather kernels"):
        aggregation.unprojection(f, p, c, variant="brick", visible_only=True)
    assert torch.equal(aggregation.unprojection(f, p, c, variant="auto", visible_only=True), aggregation.unprojection(f, p, c, variant="gather", visible_only=True))
    cl = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)       # channels-last features: read as they are
    assert torch.equal(aggregation.unprojection(cl, p, c, visible_only=True), aggregation.unprojection(f, p, c, visible_only=True))


# ------------------------------------------------------------------------------------ 5. deterministic mode
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("method", ["softmax", "mean"])
def test_deterministic_mode_repeats_bitwise(method, masked, gpu):
    shape = SHAPES[0]
    feats, proj, coords = _problem(shape, 1.6, seed=28)
    mask = torch.from_numpy(_mask(shape["B"], shape["V"], seed=29)) if masked else None
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    with _Deterministic():
        a = _run(f, p, c, method, mask=mask)
        b = _run(f, p, c, method, mask=mask, go=a["go"])
    for k in ("out", "gf", "gp", "gc"):
        assert torch.equal(a[k], b[k]), k
    ref = vis.visible_unprojection(feats, proj, coords, a["go"].cpu().numpy(), method, mask=None if mask is None else mask.numpy(), geometry=False)
    record_err("visibility deterministic bwd %s masked=%d" % (method, masked), _err(a["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))


def test_deterministic_mean_is_scaled_for_a_voxel_one_view_sees(gpu):
    """mean's ds is g / |S| and |S| can be 1 for a voxel whatever V and the sample's view count are: a scale chosen from g / V would let
    the int64 sums wrap.  |grad_out| up to 1e30; finite gradients that match the oracle."""
    shape = SHAPES[1]                                                        # 8 views
    feats, proj, coords = _problem(shape, 4.0, seed=30)
    go = torch.randn((shape["B"], shape["C"]) + tuple(shape["vol"]), generator=torch.Generator().manual_seed(31)).clamp(-4, 4) * 2.5e29
    ref = vis.visible_unprojection(feats, proj, coords, go.numpy(), "mean", geometry=False)
    assert (ref["seen"].sum(1) == 1).mean() > 0.02                           # voxels seen by exactly one view
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    with _Deterministic():
        a = _run(f, p, c, "mean", go=go.to(gpu), geometry=False)
        b = _run(f, p, c, "mean", go=go.to(gpu), geometry=False)
    assert torch.isfinite(a["gf"]).all() and torch.equal(a["gf"], b["gf"])
    record_err("visibility deterministic mean one view", _err(a["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))


# ------------------------------------------------------------------------------------ 6. storage and plumbing
@pytest.mark.parametrize("storage", ["f16", "bf16vol"])
def test_storage_modes(storage, gpu):
    """against the fp32 oracle on the rounded inputs, with the bound of the existing storage tests (test_view_mask_gpu.py)"""
    shape = SHAPES[0]
    feats, proj, coords = _problem(shape, 1.6, seed=32)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    out_dtype = None
    if storage == "f16":
        f = f.half()
        feats = f.float().cpu().numpy()
    else:
        out_dtype = torch.bfloat16
    r = _run(f, p, c, "softmax", out_dtype=out_dtype, geometry=False)
    assert r["out"].dtype == (torch.float16 if storage == "f16" else torch.bfloat16) and r["gf"].dtype == f.dtype
    ref = vis.visible_unprojection(feats, proj, coords, r["go"].float().cpu().numpy(), "softmax", geometry=False)
    record_err("visibility storage %s fwd" % storage, _err(r["out"].float().cpu().numpy(), ref["out"]), 2e-2)
    record_err("visibility storage %s bwd" % storage, _err(r["gf"].float().cpu().numpy(), ref["grad_features"]), 2e-2)


def _generator_problem(gpu, visible_only):
    B, V, Cin, Cout, Hf, Wf, S, img = 2, 4, 16, 8, 24, 24, 16, 96
    K, Rt = np.zeros((B, V, 3, 3)), np.zeros((B, V, 3, 4))
    for b in range(B):
        for v in range(V):
            az = 2 * np.pi * v / V + 0.3 + 0.1 * b
            eye = np.array([5000 * np.cos(az), 5000 * np.sin(az), 1500.0])
            fwd = -eye / np.linalg.norm(eye)
            right = np.cross(fwd, [0, 0, 1.0])
            right /= np.linalg.norm(right)
            R = np.stack([right, np.cross(fwd, right), fwd])
            K[b, v] = [[160.0, 0, img / 2], [0, 160.0, img / 2], [0, 0, 1]]
            Rt[b, v] = np.hstack([R, (-R @ eye)[:, None]])
    torch.manual_seed(33)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=Cin, output_channels=Cout, cuboid_side=4000.0, device=gpu, visible_only=visible_only)
    gen.eval()
    batch = dict(images=torch.empty((B, V, img, img, 3), device="meta"), cameras_packed=dict(K=torch.from_numpy(K).to(gpu), Rt=torch.from_numpy(Rt).to(gpu)),
                 keypoints_3d=torch.zeros(B, 17, 3))
    feats = torch.randn(B, V, Cin, Hf, Wf, generator=torch.Generator().manual_seed(34)).to(gpu)
    proj_org = torch.from_numpy(np.einsum("bvij,bvjk->bvik", K, Rt).astype(np.float32)).to(gpu)
    return gen, batch, feats, proj_org


def test_volume_generator_passes_visible_only_on(gpu):
    gen, batch, feats, proj_org = _generator_problem(gpu, True)
    x = feats.clone().requires_grad_(True)
    out = gen(x, proj_org, batch)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(35)).to(gpu)
    out.backward(go)
    gw = gen.process_feature[0].weight.grad.clone()
    gen.zero_grad()
    # the same by hand: the conv, then unprojection_cuboid on the generator's own projections and pose
    B, V = feats.shape[:2]
    S = gen.volume_size
    y = feats.clone().requires_grad_(True)
    conv = gen.process_feature(y.view(-1, *y.shape[2:]))
    conv = conv.view(B, V, *conv.shape[1:])
    proj = aggregation.feature_level_projections_device(batch["cameras_packed"], (96, 96), tuple(feats.shape[-2:])).to(gpu).contiguous()
    rots, centers = gen.volume_pose(batch, proj_org, (96, 96))
    cub = gen.cuboid()
    ref = aggregation.unprojection_cuboid(conv, proj, rots, centers, cub.position, cub.sides, (S, S, S), aggregation_method=gen.aggregation_method,
                                          visible_only=True)
    ref.backward(go)
    assert torch.equal(out, ref)
    bits = aggregation.view_visibility_cuboid(proj, rots, centers, cub.position, cub.sides, (S, S, S), tuple(feats.shape[-2:]))
    assert 0 < int((bits == 0).sum()) and int((bits == 15).sum()) > 0
    for name, a, b in (("input grad", x.grad, y.grad), ("weight grad", gw, gen.process_feature[0].weight.grad)):
        b = b.cpu().numpy()
        record_err("visibility volgen " + name, _err(a.cpu().numpy(), b), _bound(b))
    # and it is not the plain generator: the flag reaches the kernels, the fused conv route is not taken
    plain, _, _, _ = _generator_problem(gpu, False)
    plain.load_state_dict(gen.state_dict())
    assert not torch.equal(plain(feats, proj_org, batch), out)


def test_forward_graph_capture(gpu):
    shape = SHAPES[0]
    feats, proj, coords = _problem(shape, 1.6, seed=36)
    mask = torch.from_numpy(_mask(shape["B"], shape["V"], seed=37)).to(gpu)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    for m in (None, mask):
        eager = aggregation.unprojection(f, p, c, visible_only=True, view_mask=m)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            aggregation.unprojection(f, p, c, visible_only=True, view_mask=m)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = aggregation.unprojection(f, p, c, visible_only=True, view_mask=m)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
