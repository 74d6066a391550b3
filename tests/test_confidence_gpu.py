"""Per-pixel view confidence maps (unprojection(view_confidence=...), mvhmr_unproject_*_confidence) on the device: the
reference's goldens (constant integer maps = repeated views), the float64 oracle (tests/confidence_oracle.py) on maps with planted zero,
negative and NaN regions, absent data never read, the identities with the masked and the visible call, scale invariance, bitwise repeats of
every gradient, the scale bound of the deterministic sum, storage modes, the cuboid route, VolumeGenerator and graph capture.

Bounds: volumes and feature gradients use _bound(ref) of test_unproject_gpu.py; gradient tensors of geometry and confidence use REL (1e-4)
times the largest oracle value of the tensor, as test_view_weights_gpu._rel does."""
import numpy as np
import pytest
import torch

import confidence_oracle as co
import visibility_oracle as vis
from conftest import golden_cases, load_golden, record_err
from multiviewhmr_amd import aggregation
from test_geometry_grad_gpu import REL
from test_unproject_gpu import _bound, _err, _ring_problem
from test_view_mask_gpu import SHAPES, _mask
from test_visible_gpu import _Deterministic, _generator_problem

pytestmark = pytest.mark.gpu

METHODS = ("softmax", "sum", "mean")
MORE_SHAPES = [
    dict(B=2, V=1, C=8, H=16, W=16, vol=(8, 8, 8)),        # V = 1
    dict(B=3, V=4, C=8, H=20, W=24, vol=(5, 6, 7)),        # 210 voxels: the tile tail is no multiple of 32
    dict(B=1, V=2, C=260, H=8, W=8, vol=(4, 4, 3)),        # two channel groups
    dict(B=2, V=16, C=4, H=12, W=12, vol=(4, 4, 5)),       # 16 views: the geometry kernel's largest LDS footprint (69 KiB of dynamic LDS)
]
SCALE = 1.6                                                # the cuboid leaves the cameras' frames: every kind of footprint occurs


def _id(s):
    return "V%dC%dN%d" % (s["V"], s["C"], int(np.prod(s["vol"])))


def _problem(shape, scale=SCALE, seed=None):
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=shape["V"] if seed is None else seed)
    return feats, proj, (coords * np.float32(scale)).astype(np.float32)


def _maps(shape, seed, planted=True, nan=True):
    """random maps in [0.05, 4]; planted: a zero half-plane in view 0 of sample 0, a patch of negative and NaN pixels in its view 1, one
    all-zero view in sample 1, sample 2 all zero"""
    B, V, H, W = (shape[k] for k in "BVHW")
    conf = np.random.default_rng(seed).uniform(0.05, 4.0, (B, V, H, W)).astype(np.float32)
    if planted:
        conf[0, 0, :, :W // 2] = 0
        if V > 1:
            conf[0, 1, H // 4:H // 4 + 4, W // 2:W // 2 + 4] = -1
            if nan:
                conf[0, 1, H // 4 + 1:H // 4 + 3, W // 2 + 1:W // 2 + 3] = np.nan
        if B > 1:
            conf[1, V - 1] = 0
        if B > 2:
            conf[2] = 0
    return conf


def _run(f, p, c, conf, method, variant="auto", out_dtype=None, go=None, geometry=True, mask=None, visible=False):
    f = f.detach().clone().requires_grad_(True)
    p = p.detach().clone().requires_grad_(geometry)
    c = c.detach().clone().requires_grad_(geometry)
    k = conf.detach().clone().requires_grad_(True)
    out = aggregation.unprojection(f, p, c, method, variant=variant, out_dtype=out_dtype, view_mask=mask, visible_only=visible, view_confidence=k)
    if go is None:
        go = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(out.device, out.dtype)
    out.backward(go)
    torch.cuda.synchronize()
    return dict(out=out.detach(), gf=f.grad, gp=p.grad, gc=c.grad, gk=k.grad, go=go)


def _rel(name, got, ref):
    scale = float(np.abs(ref).max())
    assert scale > 0, name
    record_err(name, _err(got.double().cpu().numpy(), ref), REL * scale)


def _dev(gpu, *arrays):
    return tuple(torch.from_numpy(x).to(gpu) for x in arrays)


# ------------------------------------------------------------------------------------ 1. the reference's goldens
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("variant", ["auto", "gather"])
@pytest.mark.parametrize("case", golden_cases("confidence"))
def test_goldens_with_constant_maps_as_repeated_views(case, variant, method, gpu):
    d = load_golden("confidence", case)
    f, p, c, k, go = _dev(gpu, *(d[x] for x in ("features", "proj", "coords", "confidence", "grad_out")))
    r = _run(f, p, c, k, method, variant, go=go, geometry=False)
    ref, gref = d["out_" + method], d["gfeat_" + method]
    clean = np.broadcast_to(d["clean"][:, None], ref.shape)
    assert clean.mean() >= 0.70
    record_err("confidence golden fwd %s %s %s" % (case, method, variant), _err(r["out"].cpu().numpy()[clean], ref[clean]), _bound(ref))
    record_err("confidence golden bwd %s %s %s" % (case, method, variant), _err(r["gf"].cpu().numpy(), gref), _bound(gref))


# ------------------------------------------------------------------------------------ 2. the float64 oracle
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES + MORE_SHAPES, ids=_id)
def test_oracle_parity(shape, method, gpu):
    B, V = shape["B"], shape["V"]
    feats, proj, coords = _problem(shape)
    conf = _maps(shape, seed=50 + V)
    go = torch.randn((B, shape["C"]) + tuple(shape["vol"]), generator=torch.Generator().manual_seed(7))
    ref = co.conf_unprojection(feats, proj, coords, conf, go.numpy(), method)
    present = ref["present"]
    assert 0.02 < present.mean() < 0.98, present.mean()                     # absent and present voxel-views both occur
    f, p, c, k = _dev(gpu, feats, proj, coords, conf)
    r = _run(f, p, c, k, method, go=go.to(gpu))
    tag = "confidence %s V%d C%d N%d" % (method, V, shape["C"], int(np.prod(shape["vol"])))
    record_err(tag + " fwd", _err(r["out"].cpu().numpy(), ref["out"]), _bound(ref["out"]))
    record_err(tag + " bwd", _err(r["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))
    if V == 1 and method != "sum":
        # out = s_v whatever a lone view's confidence is: the gradient is identically zero (the oracle's is float64 noise, which gives no
        # scale), and the kernel returns exact zeros for a voxel with a single present view
        assert np.abs(ref["grad_confidence"]).max() <= 1e-12 and torch.count_nonzero(r["gk"]) == 0
    else:
        _rel(tag + " conf grad", r["gk"], ref["grad_confidence"])
    _rel(tag + " proj grad", r["gp"], ref["grad_proj"])
    _rel(tag + " coord grad", r["gc"], ref["grad_coords"])
    # exact zeros where the oracle has none of a view: planted all-zero maps
    if B > 1:
        assert torch.count_nonzero(r["gf"][1, V - 1]) == 0 and torch.count_nonzero(r["gk"][1, V - 1]) == 0 and torch.count_nonzero(r["gp"][1, V - 1]) == 0
    if B > 2:
        assert torch.count_nonzero(r["out"][2]) == 0 and torch.count_nonzero(r["gc"][2]) == 0 and torch.count_nonzero(r["gk"][2]) == 0


# ------------------------------------------------------------------------------------ 3. absent data is never read
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=_id)
def test_a_view_with_an_all_zero_map_is_never_read(shape, method, gpu):
    V = shape["V"]
    feats, proj, coords = _problem(shape, seed=60)
    conf = _maps(shape, seed=61, planted=False)
    conf[0, 1] = 0
    feats[0, 1] = np.nan
    f, p, c, k = _dev(gpu, feats, proj, coords, conf)
    r = _run(f, p, c, k, method)
    for key in ("out", "gf", "gp", "gc", "gk"):
        assert torch.isfinite(r[key]).all(), key
    assert torch.count_nonzero(r["gf"][0, 1]) == 0 and torch.count_nonzero(r["gp"][0, 1]) == 0 and torch.count_nonzero(r["gk"][0, 1]) == 0
    assert torch.count_nonzero(r["gf"][0, 0]) > 0 and torch.count_nonzero(r["gk"][0, 0]) > 0
    keep = [v for v in range(V) if v != 1]
    s = _run(f[:1, keep], p[:1, keep], c[:1], k[:1, keep], method, go=r["go"][:1])
    ref = s["out"][0].cpu().numpy()
    record_err("confidence zero map %s V%d fwd" % (method, V), _err(r["out"][0].cpu().numpy(), ref), _bound(ref))


@pytest.mark.parametrize("method", METHODS)
def test_features_under_a_zero_half_plane_are_never_read(method, gpu):
    """the map of one view is zero on its left half; NaN features in the columns at least 2 px inside that half: a voxel whose footprint
    touches them samples a confidence of exactly 0"""
    shape = SHAPES[0]
    W = shape["W"]
    feats, proj, coords = _problem(shape, seed=62)
    conf = _maps(shape, seed=63, planted=False)
    conf[:, 0, :, :W // 2] = 0
    clean = feats.copy()
    feats[:, 0, :, :, :W // 2 - 2] = np.nan
    f, g, p, c, k = _dev(gpu, feats, clean, proj, coords, conf)
    r = _run(f, p, c, k, method)
    s = _run(g, p, c, k, method, go=r["go"])
    assert torch.isfinite(r["out"]).all() and torch.equal(r["out"], s["out"])
    for key in ("gp", "gc", "gk"):
        assert torch.isfinite(r[key]).all() and torch.equal(r[key], s[key]), key
    assert torch.isfinite(r["gf"]).all()


# ------------------------------------------------------------------------------------ 4. equalities
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=_id)
def test_zero_maps_for_the_views_a_mask_drops_is_the_view_mask_call(shape, method, gpu):
    """the mask is the case of an all-zero map: the call with view_mask (the packed route) against the call whose maps are zeroed for the
    views the mask drops (no mask reaches the library: nothing packed); the views of a sample are summed in slot order there and in view order here, hence bounds"""
    B, V = shape["B"], shape["V"]
    feats, proj, coords = _problem(shape, seed=64)
    mask = _mask(B, V, seed=65)
    conf = _maps(shape, seed=66, planted=False)
    zeroed = conf * mask[:, :, None, None].astype(np.float32)
    f, p, c, k, kz = _dev(gpu, feats, proj, coords, conf, zeroed)
    a = _run(f, p, c, k, method, mask=torch.from_numpy(mask))
    b = _run(f, p, c, kz, method, go=a["go"])
    tag = "confidence mask as zero maps %s V%d " % (method, V)
    for key, name in (("out", "fwd"), ("gf", "bwd")):
        ref = b[key].cpu().numpy()
        record_err(tag + name, _err(a[key].cpu().numpy(), ref), _bound(ref))
    for key, name in (("gk", "conf grad"), ("gp", "proj grad"), ("gc", "coord grad")):
        _rel(tag + name, a[key], b[key].double().cpu().numpy())
    m = ~torch.from_numpy(mask).to(gpu)
    for key in ("gf", "gk", "gp"):
        assert torch.count_nonzero(a[key][m]) == 0 and torch.count_nonzero(b[key][m]) == 0, key
    assert torch.count_nonzero(a["out"][2]) == 0 and torch.count_nonzero(a["gc"][2]) == 0              # sample 2 has no views
    # an all-ones mask (everything packed, in view order) and no mask (the caller's own tensors are read) run the same arithmetic
    full = _run(f, p, c, k, method, mask=torch.ones(B, V, dtype=torch.bool), go=a["go"])
    none = _run(f, p, c, k, method, go=a["go"])
    for key in ("out", "gk", "gp", "gc"):
        assert torch.equal(full[key], none[key]), key


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_constant_maps_with_visible_only_are_weights_over_the_seeing_views(method, masked, gpu):
    shape = SHAPES[0]
    B, V, H, W = (shape[k] for k in "BVHW")
    feats, proj, coords = _problem(shape, seed=66)
    w = np.random.default_rng(67).uniform(0.1, 3.0, (B, V)).astype(np.float32)
    conf = np.broadcast_to(w[:, :, None, None], (B, V, H, W)).copy()
    mask = _mask(B, V, seed=68) if masked else None
    edge = vis.edge_voxels(proj, coords, H, W)
    assert edge.mean() <= 0.02
    keep = torch.from_numpy(~edge).reshape((B, 1) + tuple(shape["vol"]))
    go = torch.randn((B, shape["C"]) + tuple(shape["vol"]), generator=torch.Generator().manual_seed(7)) * keep
    ref = co.conf_unprojection(feats, proj, coords, conf, go.numpy(), method, mask=mask, visible=True)
    seen = vis.seen_views(proj, coords, H, W, mask)
    kept = ~edge
    assert np.array_equal(ref["present"].transpose(0, 2, 1)[kept], seen.transpose(0, 2, 1)[kept])       # S is the seeing set
    f, p, c, k = _dev(gpu, feats, proj, coords, conf)
    r = _run(f, p, c, k, method, go=go.to(gpu), visible=True, mask=None if mask is None else torch.from_numpy(mask))
    km = np.broadcast_to(keep.numpy(), ref["out"].shape)
    tag = "confidence visible %s masked=%d " % (method, masked)
    record_err(tag + "fwd", _err(r["out"].cpu().numpy()[km], ref["out"][km]), _bound(ref["out"]))
    record_err(tag + "bwd", _err(r["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))
    _rel(tag + "conf grad", r["gk"], ref["grad_confidence"])
    _rel(tag + "proj grad", r["gp"], ref["grad_proj"])
    _rel(tag + "coord grad", r["gc"], ref["grad_coords"])


@pytest.mark.parametrize("method", ["mean", "softmax"])
def test_scaling_the_maps_of_a_sample(method, gpu):
    """x 4: volumes and gradients unchanged, grad_confidence / 4; the dot of maps and their gradient vanishes (Euler: out is homogeneous of
    degree 0 in a sample's maps) -- the terms conf * grad_conf cancel, so the dot is held to REL of the sum of their magnitudes, which is
    what a relative error of REL on every term allows (far tighter than entries x max conf x max |grad_conf|, the form of DESIGN.md 5.9's
    test, at V Hf Wf entries); x 1e-6: grad_confidence x 1e6 within REL, which
    needs the measured fixed-point exponent"""
    shape = SHAPES[0]
    V, H, W = (shape[k] for k in "VHW")
    feats, proj, coords = _problem(shape, seed=69)
    conf = _maps(shape, seed=70, nan=False)
    conf[conf < 0] = 0
    f, p, c, k = _dev(gpu, feats, proj, coords, conf)
    a = _run(f, p, c, k, method)
    b = _run(f, p, c, k * 4, method, go=a["go"])
    tag = "confidence scaled %s " % method
    for key, name in (("out", "fwd"), ("gf", "bwd")):
        ref = a[key].cpu().numpy()
        record_err(tag + name, _err(b[key].cpu().numpy(), ref), _bound(ref))
    for key, name in (("gp", "proj grad"), ("gc", "coord grad")):
        _rel(tag + name, b[key], a[key].double().cpu().numpy())
    _rel(tag + "conf grad / 4", b["gk"] * 4, a["gk"].double().cpu().numpy())
    gk = a["gk"].double().cpu().numpy()
    dot = np.abs((conf.astype(np.float64) * gk).sum((1, 2, 3))).max()
    record_err(tag + "orthogonality", dot, REL * float(np.abs(conf.astype(np.float64) * gk).sum((1, 2, 3)).max()))
    s = _run(f, p, c, k * 1e-6, method, go=a["go"])
    _rel(tag + "conf grad x 1e-6", s["gk"] * 1e-6, gk)


# ------------------------------------------------------------------------------------ 5. reproducibility
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_gradients_repeat_bitwise(method, masked, gpu):
    """grad_confidence, grad_proj and grad_coords in default mode; every gradient under torch.use_deterministic_algorithms(True)"""
    shape = SHAPES[0]
    feats, proj, coords = _problem(shape, seed=71)
    conf = _maps(shape, seed=72)
    mask = torch.from_numpy(_mask(shape["B"], shape["V"], seed=73)) if masked else None
    f, p, c, k = _dev(gpu, feats, proj, coords, conf)
    a = _run(f, p, c, k, method, mask=mask)
    b = _run(f, p, c, k, method, mask=mask, go=a["go"])
    for key in ("out", "gk", "gp", "gc"):
        assert torch.equal(a[key], b[key]), key
    with _Deterministic():
        d = _run(f, p, c, k, method, mask=mask, go=a["go"])
        e = _run(f, p, c, k, method, mask=mask, go=a["go"])
    for key in ("out", "gf", "gk", "gp", "gc"):
        assert torch.equal(d[key], e[key]), key
    assert torch.equal(d["gk"], a["gk"])
    ref = a["gf"].cpu().numpy()
    record_err("confidence deterministic bwd %s masked=%d" % (method, masked), _err(d["gf"].cpu().numpy(), ref), _bound(ref))


@pytest.mark.parametrize("masked", [False, True])
def test_deterministic_softmax_with_visible_only(masked, gpu):
    """the scale pass's marks under the seeing test (k_det_mark's visible branch): bitwise repeats, and the oracle's feature gradient"""
    shape = SHAPES[0]
    B, V, H, W = (shape[k] for k in "BVHW")
    feats, proj, coords = _problem(shape, seed=90)
    conf = _maps(shape, seed=91)
    mask = _mask(B, V, seed=92) if masked else None
    edge = vis.edge_voxels(proj, coords, H, W)
    assert edge.mean() <= 0.02
    go = torch.randn((B, shape["C"]) + tuple(shape["vol"]), generator=torch.Generator().manual_seed(7)) * torch.from_numpy(~edge).reshape((B, 1) + tuple(shape["vol"]))
    ref = co.conf_unprojection(feats, proj, coords, conf, go.numpy(), "softmax", mask=mask, visible=True, geometry=False)
    f, p, c, k = _dev(gpu, feats, proj, coords, conf)
    m = None if mask is None else torch.from_numpy(mask)
    with _Deterministic():
        a = _run(f, p, c, k, "softmax", go=go.to(gpu), visible=True, mask=m)
        b = _run(f, p, c, k, "softmax", go=go.to(gpu), visible=True, mask=m)
    for key in ("out", "gf", "gk", "gp", "gc"):
        assert torch.isfinite(a[key]).all() and torch.equal(a[key], b[key]), key
    record_err("confidence deterministic softmax visible masked=%d" % masked, _err(a["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))


def test_deterministic_sum_is_scaled_by_the_confidence(gpu):
    """sum's ds is g c_v: a fixed-point scale chosen from max |g| alone would let the int64 sums wrap with confidences up to 1e4"""
    shape = SHAPES[1]
    feats, proj, coords = _problem(shape, seed=74)
    conf = _maps(shape, seed=75, planted=False) * np.float32(2500.0)
    assert conf.max() > 9000
    go = torch.randn((shape["B"], shape["C"]) + tuple(shape["vol"]), generator=torch.Generator().manual_seed(76))
    ref = co.conf_unprojection(feats, proj, coords, conf, go.numpy(), "sum", geometry=False)
    f, p, c, k = _dev(gpu, feats, proj, coords, conf)
    with _Deterministic():
        a = _run(f, p, c, k, "sum", go=go.to(gpu), geometry=False)
        b = _run(f, p, c, k, "sum", go=go.to(gpu), geometry=False)
    assert torch.isfinite(a["gf"]).all() and torch.equal(a["gf"], b["gf"])
    record_err("confidence deterministic sum 1e4", _err(a["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))


# ------------------------------------------------------------------------------------ 6. storage and plumbing
@pytest.mark.parametrize("storage", ["f16", "bf16vol", "channels_last"])
def test_storage_and_layouts(storage, gpu):
    """against the float64 oracle on the stored inputs, with the rounding bounds of test_view_weights_gpu.test_storage_and_layouts"""
    shape = SHAPES[0]
    feats, proj, coords = _problem(shape, seed=77)
    conf = _maps(shape, seed=78)
    f, p, c, k = _dev(gpu, feats, proj, coords, conf)
    out_dtype = None
    loose = storage != "channels_last"
    if storage == "f16":
        f = f.half()
        feats = f.float().cpu().numpy()
    elif storage == "bf16vol":
        out_dtype = torch.bfloat16
    else:
        f = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    r = _run(f, p, c, k, "softmax", out_dtype=out_dtype)
    assert r["out"].dtype == dict(f16=torch.float16, bf16vol=torch.bfloat16, channels_last=torch.float32)[storage] and r["gf"].dtype == f.dtype
    ref = co.conf_unprojection(feats, proj, coords, conf, r["go"].float().cpu().numpy(), "softmax")
    record_err("confidence storage %s fwd" % storage, _err(r["out"].float().cpu().numpy(), ref["out"]), 2e-2 if loose else _bound(ref["out"]))
    record_err("confidence storage %s bwd" % storage, _err(r["gf"].float().cpu().numpy(), ref["grad_features"]),
               2e-2 if loose else _bound(ref["grad_features"]))
    assert r["gk"].dtype == torch.float32
    _rel("confidence storage %s conf grad" % storage, r["gk"], ref["grad_confidence"])     # (fp32 whatever the storage: the oracle reads the stored values)


@pytest.mark.parametrize("method", METHODS)
def test_tensor_and_cuboid_routes_agree(method, gpu):
    """bit for bit on the materialised coordinates: the volume, grad_confidence and grad_proj (fixed-order sums of bit-equal positions), and
    -- deterministic mode -- the feature gradient; grad_rot and grad_center against the chain rule through coords = R (grid - center) + center
    applied to the tensor route's grad_coords in float64"""
    B, V, C, H, W, S = 3, 4, 8, 24, 20, 16
    feats, proj, _ = _ring_problem(B, V, C, H, W, (S, S, S), seed=79)
    rng = np.random.default_rng(80)
    th = rng.uniform(0, 2 * np.pi, B)
    rot = np.stack([[[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]] for t in th]).astype(np.float32)
    cen = rng.uniform(-100, 100, (B, 3)).astype(np.float32)
    conf = _maps(dict(B=B, V=V, H=H, W=W), seed=81)
    f, p, r, ce, k = _dev(gpu, feats, proj, rot, cen, conf)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=4000.0, device=gpu)
    cub = gen.cuboid()
    coords = gen.coord_volumes(r, ce, gpu)
    with _Deterministic():
        a = _run(f, p, coords, k, method)
        fc, pc, rc, cc, kc = (t.detach().clone().requires_grad_(True) for t in (f, p, r, ce, k))
        out = aggregation.unprojection_cuboid(fc, pc, rc, cc, cub.position, cub.sides, (S, S, S), method, view_confidence=kc)
        out.backward(a["go"])
    assert torch.equal(out, a["out"]) and torch.equal(fc.grad, a["gf"]) and torch.equal(kc.grad, a["gk"]) and torch.equal(pc.grad, a["gp"])
    gX = a["gc"].double().reshape(B, -1, 3)
    R, c0 = r.double(), ce.double()
    d = torch.einsum("bji,bnj->bni", R, coords.double().reshape(B, -1, 3) - c0[:, None])          # grid - center = R^T (X - center)
    g_rot = torch.einsum("bni,bnj->bij", gX, d).cpu().numpy()
    g_cen = (gX.sum(1) - torch.einsum("bji,bj->bi", R, gX.sum(1))).cpu().numpy()
    _rel("confidence cuboid %s rot grad" % method, rc.grad, g_rot)
    _rel("confidence cuboid %s center grad" % method, cc.grad, g_cen)
    # the maps' gradient alone on the cuboid route: no grad_proj, no pose gradients, the same bits
    only = k.detach().clone().requires_grad_(True)
    aggregation.unprojection_cuboid(f, p, r, ce, cub.position, cub.sides, (S, S, S), method, view_confidence=only).backward(a["go"])
    assert torch.equal(only.grad, a["gk"])
    mask = torch.from_numpy(_mask(B, V, seed=82))
    assert torch.equal(aggregation.unprojection(f, p, coords, method, view_confidence=k, view_mask=mask, visible_only=True),
                       aggregation.unprojection_cuboid(f, p, r, ce, cub.position, cub.sides, (S, S, S), method, view_confidence=k, view_mask=mask,
                                                       visible_only=True))


def test_volume_generator_reads_the_maps_from_the_batch(gpu):
    gen, batch, feats, proj_org = _generator_problem(gpu, False)
    B, V, _, Hf, Wf = feats.shape
    conf = torch.from_numpy(_maps(dict(B=B, V=V, H=Hf, W=Wf), seed=83)).to(gpu)
    plain = gen(feats, proj_org, batch)
    batch = dict(batch, view_confidence=conf)
    k = conf.clone().requires_grad_(True)
    x = feats.clone().requires_grad_(True)
    out = gen(x, proj_org, dict(batch, view_confidence=k))
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(84)).to(gpu)
    out.backward(go)
    S = gen.volume_size
    y = feats.clone().requires_grad_(True)
    conv = gen.process_feature(y.view(-1, *y.shape[2:]))
    conv = conv.view(B, V, *conv.shape[1:])
    proj = aggregation.feature_level_projections_device(batch["cameras_packed"], (96, 96), (Hf, Wf)).to(gpu).contiguous()
    rots, centers = gen.volume_pose(batch, proj_org, (96, 96))
    cub = gen.cuboid()
    k2 = conf.clone().requires_grad_(True)
    ref = aggregation.unprojection_cuboid(conv, proj, rots, centers, cub.position, cub.sides, (S, S, S), aggregation_method=gen.aggregation_method,
                                          view_confidence=k2)
    ref.backward(go)
    assert torch.equal(out, ref) and torch.equal(k.grad, k2.grad) and not torch.equal(out, plain)
    b = y.grad.cpu().numpy()
    record_err("confidence volgen input grad", _err(x.grad.cpu().numpy(), b), _bound(b))


def test_forward_graph_capture(gpu):
    shape = SHAPES[0]
    feats, proj, coords = _problem(shape, seed=85)
    conf = _maps(shape, seed=86)
    mask = torch.from_numpy(_mask(shape["B"], shape["V"], seed=87)).to(gpu)
    f, p, c, k = _dev(gpu, feats, proj, coords, conf)
    for m in (None, mask):
        eager = aggregation.unprojection(f, p, c, view_confidence=k, view_mask=m)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            aggregation.unprojection(f, p, c, view_confidence=k, view_mask=m)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = aggregation.unprojection(f, p, c, view_confidence=k, view_mask=m)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_the_gradient_comes_back_in_the_maps_own_dtype_and_device(gpu):
    shape = SHAPES[2]
    feats, proj, coords = _problem(shape, seed=88)
    conf = _maps(shape, seed=89, nan=False)
    f, p, c, k = _dev(gpu, feats, proj, coords, conf)
    base = _run(f, p, c, k, "mean")
    host = torch.from_numpy(conf).double().requires_grad_(True)                # float64 on the CPU
    out = aggregation.unprojection(f, p, c, "mean", view_confidence=host)
    out.backward(base["go"])
    assert host.grad.dtype == torch.float64 and host.grad.device.type == "cpu" and torch.equal(out, base["out"])
    assert torch.equal(host.grad.float(), base["gk"].cpu())
    with pytest.raises(RuntimeError, match="gather kernels"):
        aggregation.unprojection(f, p, c, variant="brick", view_confidence=k)
