"""Per-view confidence weights (unprojection(view_weights=...), mvhmr_unproject_*_weighted) on the device: the reference's
goldens on duplicated views, real weights against the float64 oracle (tests/viewweight_oracle.py) over every voxel, view and sample --
volume and all five gradients, the weights' included --, absent views exactly zero and never read, the {0, 1} and all-ones and scaled
weights against the calls they must equal, bitwise repeats, the deterministic bound under a large weight, storage modes, the cuboid
route, VolumeGenerator, graph capture."""
import numpy as np
import pytest
import torch

import viewweight_oracle as vo
from conftest import golden_cases, load_golden, record_err
from multiviewhmr_amd import aggregation
from test_geometry_grad_gpu import REL
from test_unproject_gpu import _bound, _err, _ring_problem
from test_view_mask_gpu import SHAPES, _mask

pytestmark = pytest.mark.gpu

METHODS = ("softmax", "sum", "mean")


def _weights(B, V, seed):
    """real weights in [0.05, 4] with zeros where test_view_mask_gpu._mask places absences (sample 0 all views, 1 one view, 2 none)"""
    rng = np.random.default_rng(seed + 100)
    return (rng.uniform(0.05, 4.0, (B, V)) * _mask(B, V, seed)).astype(np.float32)


def _run(f, p, c, w, method, variant="auto", out_dtype=None, go=None, geometry=True, mask=None, want_w=True):
    f = f.detach().clone().requires_grad_(True)
    p = p.detach().clone().requires_grad_(geometry)
    c = c.detach().clone().requires_grad_(geometry)
    w = None if w is None else w.detach().clone().requires_grad_(want_w)
    out = aggregation.unprojection(f, p, c, method, variant=variant, out_dtype=out_dtype, view_weights=w, view_mask=mask)
    if go is None:
        go = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(out.device, out.dtype)
    out.backward(go)
    torch.cuda.synchronize()
    return dict(out=out.detach(), gf=f.grad, gp=p.grad, gc=c.grad, gw=None if w is None else w.grad, go=go)


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


# ------------------------------------------------------------------------------------ the reference's goldens
@pytest.mark.parametrize("variant", ["auto", "gather"])
@pytest.mark.parametrize("case", golden_cases("viewweights"))
def test_goldens_on_duplicated_views(case, variant, gpu):
    d = load_golden("viewweights", case)
    f, p, c, w, go = (torch.from_numpy(d[k]).to(gpu) for k in ("features", "proj", "coords", "weights", "grad_out"))
    for method in METHODS:
        r = _run(f, p, c, w, method, variant, go=go, geometry=False)
        ref, gref = d["out_" + method], d["gfeat_" + method]
        record_err("viewweights golden fwd %s %s %s" % (case, method, variant), _err(r["out"].cpu().numpy(), ref), _bound(ref))
        record_err("viewweights golden bwd %s %s %s" % (case, method, variant), _err(r["gf"].cpu().numpy(), gref), _bound(gref))


# ------------------------------------------------------------------------------------ real weights against the oracle
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("variant", ["auto", "gather"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "V%dC%d" % (s["V"], s["C"]))
def test_oracle_parity(shape, variant, method, gpu):
    B, V = shape["B"], shape["V"]
    feats, proj, coords = _ring_problem(B, V, shape["C"], shape["H"], shape["W"], shape["vol"], seed=V)
    wts = _weights(B, V, seed=shape["C"])
    f, p, c, w = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords, wts))
    r = _run(f, p, c, w, method, variant)
    ref = vo.weighted_unprojection(feats, proj, coords, wts, r["go"].cpu().numpy(), method)
    tag = "viewweights %s %s V%d C%d" % (variant, method, V, shape["C"])
    record_err(tag + " fwd", _err(r["out"].cpu().numpy(), ref["out"]), _bound(ref["out"]))
    record_err(tag + " bwd", _err(r["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))
    _rel(tag + " proj grad", r["gp"], ref["grad_proj"])
    _rel(tag + " coord grad", r["gc"], ref["grad_coords"])
    _rel(tag + " weight grad", r["gw"], ref["grad_weights"])
    assert r["gw"].dtype == torch.float32 and r["gw"].shape == w.shape
    # absent views: exactly zero gradients (features, projection rows, weights); the all-absent sample: zeros everywhere
    absent = torch.from_numpy(wts == 0).to(gpu)
    assert absent[2].all() and absent.sum() > V
    for k in ("gf", "gp", "gw"):
        assert torch.count_nonzero(r[k][absent]) == 0, k
    assert torch.count_nonzero(r["out"][2]) == 0 and torch.count_nonzero(r["gc"][2]) == 0


@pytest.mark.parametrize("method", ["mean", "softmax"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "V%dC%d" % (s["V"], s["C"]))
def test_weight_gradient_is_orthogonal_to_the_weights(shape, method, gpu):
    """sum_v w_v grad_w_v vanishes for mean and softmax; on the device: at most V * max w * 1e-4 * max |grad_w|, which is what the parity
    bound on each entry allows the sum to be"""
    B, V = shape["B"], shape["V"]
    feats, proj, coords = _ring_problem(B, V, shape["C"], shape["H"], shape["W"], shape["vol"], seed=20 + V)
    wts = _weights(B, V, seed=21)
    f, p, c, w = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords, wts))
    gw = _run(f, p, c, w, method, geometry=False)["gw"].double().cpu().numpy()
    dot = np.abs((wts.astype(np.float64) * gw).sum(1)).max()
    record_err("viewweights orthogonality %s V%d" % (method, V), dot, V * float(wts.max()) * REL * float(np.abs(gw).max()))


# ------------------------------------------------------------------------------------ the calls it must equal
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "V%dC%d" % (s["V"], s["C"]))
def test_zero_one_weights_are_the_mask_and_ones_the_unweighted_call(shape, method, gpu):
    B, V = shape["B"], shape["V"]
    feats, proj, coords = _ring_problem(B, V, shape["C"], shape["H"], shape["W"], shape["vol"], seed=30 + V)
    mask = _mask(B, V, seed=31)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    tag = "viewweights %s V%d" % (method, V)
    a = _run(f, p, c, torch.from_numpy(mask.astype(np.float32)).to(gpu), method)
    b = _run(f, p, c, None, method, mask=torch.from_numpy(mask), go=a["go"])
    for k in ("out", "gf", "gp", "gc"):
        y = b[k].cpu().numpy()
        record_err(tag + " {0,1} vs mask " + k, _err(a[k].cpu().numpy(), y), _bound(y))
    a = _run(f, p, c, torch.ones(B, V, device=gpu), method, "gather", go=a["go"])
    b = _run(f, p, c, None, method, "gather", go=a["go"])
    for k in ("out", "gf", "gp", "gc"):
        y = b[k].cpu().numpy()
        record_err(tag + " ones vs unweighted " + k, _err(a[k].cpu().numpy(), y), _bound(y))


@pytest.mark.parametrize("method", ["mean", "softmax"])
def test_scaling_the_weights_changes_nothing(method, gpu):
    shape = SHAPES[0]
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=40)
    w = torch.from_numpy(_weights(shape["B"], shape["V"], seed=41)).to(gpu)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    a = _run(f, p, c, w, method)
    b = _run(f, p, c, 4 * w, method, go=a["go"])
    for k in ("out", "gf", "gp", "gc"):
        y = a[k].cpu().numpy()
        record_err("viewweights w vs 4w %s %s" % (method, k), _err(b[k].cpu().numpy(), y), _bound(y))
    y = a["gw"].cpu().numpy()
    record_err("viewweights w vs 4w %s gw" % method, _err(4 * b["gw"].cpu().numpy(), y), _bound(y))


# ------------------------------------------------------------------------------------ absent data is never read
@pytest.mark.parametrize("method", METHODS)
def test_absent_data_is_never_read(method, gpu):
    """test_view_mask_gpu.test_masked_data_is_never_read with the absent views chosen by zero (and one negative, one NaN) weight"""
    shape = SHAPES[0]
    B, V = shape["B"], shape["V"]
    feats, proj, coords = _ring_problem(B, V, shape["C"], shape["H"], shape["W"], shape["vol"], seed=5)
    wts = _weights(B, V, seed=6)
    absent = np.argwhere(wts == 0)
    wts[tuple(absent[0])], wts[tuple(absent[1])] = -2.0, np.nan
    m = torch.from_numpy(wts > 0).to(gpu)
    f, p, c, w = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords, wts))
    runs = []
    with _Deterministic():          # the default feature gradient adds with float atomics: compare reproducible bits
        for fill in (0.0, float("nan"), float("inf")):
            fg, pg = f.clone(), p.clone()
            fg[~m] = fill
            pg[~m] = -fill if fill == float("inf") else fill
            runs.append(_run(fg, pg, c, w, method, go=runs[0]["go"] if runs else None))
    for r in runs[1:]:
        for k in ("out", "gf", "gp", "gc", "gw"):
            assert torch.equal(runs[0][k], r[k]), k
    for k in ("gf", "gp", "gw"):
        assert torch.count_nonzero(runs[0][k][~m]) == 0 and torch.isfinite(runs[0][k]).all(), k


# ------------------------------------------------------------------------------------ reproducible bits
@pytest.mark.parametrize("method", METHODS)
def test_deterministic_mode_repeats_bitwise(method, gpu):
    shape = SHAPES[0]
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=9)
    wts = _weights(shape["B"], shape["V"], seed=10)
    f, p, c, w = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords, wts))
    with _Deterministic():
        a = _run(f, p, c, w, method)
        b = _run(f, p, c, w, method, go=a["go"])
    for k in ("out", "gf", "gp", "gc", "gw"):
        assert torch.equal(a[k], b[k]), k
    ref = vo.weighted_unprojection(feats, proj, coords, wts, a["go"].cpu().numpy(), method, geometry=False)
    record_err("viewweights deterministic bwd %s" % method, _err(a["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))
    # grad_weights (and the other geometry gradients) carry the same bits from run to run in default mode too: no float atomics
    a = _run(f, p, c, w, method)
    b = _run(f, p, c, w, method, go=a["go"])
    for k in ("gp", "gc", "gw"):
        assert torch.equal(a[k], b[k]), k


def test_deterministic_sum_under_a_large_weight(gpu):
    """sum's ds is g w_v: the deterministic scale must carry the sample's largest weight, or the int64 sums wrap (a weight of 1e3 on one
    view, a uniform grad_out of 3e3: every contribution near the bound)"""
    B, V, C, H, W, vol = 3, 8, 8, 12, 12, (16, 16, 16)
    feats, proj, coords = _ring_problem(B, V, C, H, W, vol, seed=13)
    wts = np.ones((B, V), np.float32)
    wts[0, 3] = 1.0e3
    wts[1, [0, 5]] = 0.0
    f, p, c, w = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords, wts))
    go = torch.full((B, C) + vol, 3.0e3, device=gpu)
    with _Deterministic():
        a = _run(f, p, c, w, "sum", go=go, geometry=False)
        b = _run(f, p, c, w, "sum", go=go, geometry=False)
    assert torch.equal(a["gf"], b["gf"])
    ref = vo.weighted_unprojection(feats, proj, coords, wts, go.cpu().numpy(), "sum", geometry=False)
    record_err("viewweights deterministic sum large weight", _err(a["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))


# ------------------------------------------------------------------------------------ storage modes
@pytest.mark.parametrize("storage", ["f16", "bf16vol", "channels_last"])
def test_storage_and_layouts(storage, gpu):
    shape = SHAPES[0]
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=3)
    wts = _weights(shape["B"], shape["V"], seed=4)
    f, p, c, w = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords, wts))
    out_dtype = None
    if storage == "f16":
        f = f.half()
        feats = f.float().cpu().numpy()
    elif storage == "bf16vol":
        out_dtype = torch.bfloat16
    else:
        f = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    r = _run(f, p, c, w, "softmax", out_dtype=out_dtype)
    ref = vo.weighted_unprojection(feats, proj, coords, wts, r["go"].float().cpu().numpy(), "softmax")
    loose = storage != "channels_last"
    record_err("viewweights storage %s fwd" % storage, _err(r["out"].float().cpu().numpy(), ref["out"]), 2e-2 if loose else _bound(ref["out"]))
    record_err("viewweights storage %s bwd" % storage, _err(r["gf"].float().cpu().numpy(), ref["grad_features"]),
               2e-2 if loose else _bound(ref["grad_features"]))
    _rel("viewweights storage %s weight grad" % storage, r["gw"], ref["grad_weights"])      # (fp32 whatever the storage: the oracle reads the stored values)
    assert torch.count_nonzero(r["gf"][torch.from_numpy(wts == 0).to(gpu)]) == 0


def test_weights_of_another_dtype_and_device_get_their_gradient_back(gpu):
    shape = SHAPES[2]
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=50)
    wts = _weights(shape["B"], shape["V"], seed=51)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    w = torch.from_numpy(wts).double().requires_grad_(True)                  # float64, on the host
    out = aggregation.unprojection(f, p, c, "mean", view_weights=w)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(gpu)
    out.backward(go)
    assert w.grad.dtype == torch.float64 and w.grad.device.type == "cpu"
    ref = vo.weighted_unprojection(feats, proj, coords, wts, go.cpu().numpy(), "mean", geometry=False)
    _rel("viewweights host float64 weight grad", w.grad, ref["grad_weights"])
    # the weights' gradient alone (nothing else requires grad): the geometry kernel runs for it
    assert torch.count_nonzero(w.grad[torch.from_numpy(wts == 0)]) == 0


# ------------------------------------------------------------------------------------ cuboid route, VolumeGenerator
@pytest.mark.parametrize("method", METHODS)
def test_cuboid_route_matches_the_tensor_route(method, gpu):
    """unprojection_cuboid against unprojection on the coordinates mvhmr_build_coord_volumes builds: the volume, the feature, projection
    and weight gradients, and the pose gradients against the chain rule through those coordinates"""
    B, V, C, H, W, S = 5, 4, 8, 24, 20, 16
    feats, proj, _ = _ring_problem(B, V, C, H, W, (S, S, S), seed=14)
    wts = _weights(B, V, seed=15)
    rng = np.random.default_rng(16)
    th = rng.uniform(0, 2 * np.pi, B)
    rot = np.stack([[[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]] for t in th]).astype(np.float32)
    cen = rng.uniform(-100, 100, (B, 3)).astype(np.float32)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=2500.0, device=gpu)
    cub = gen.cuboid()
    f, p, r, ce, w = (torch.from_numpy(x).to(gpu).requires_grad_(True) for x in (feats, proj, rot, cen, wts))
    out = aggregation.unprojection_cuboid(f, p, r, ce, cub.position, cub.sides, (S, S, S), method, view_weights=w)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(17)).to(gpu)
    out.backward(go)
    coords = gen.coord_volumes(r.detach(), ce.detach(), gpu)
    t = _run(f, p, coords, w, method, go=go)
    tag = "viewweights cuboid %s " % method
    for name, x, y in (("fwd", out.detach(), t["out"]), ("feat grad", f.grad, t["gf"]), ("proj grad", p.grad, t["gp"]), ("weight grad", w.grad, t["gw"])):
        y = y.cpu().numpy()
        record_err(tag + name, _err(x.cpu().numpy(), y), _bound(y))
    # X = R d + c, d = grid - c: grad_rot = sum gX (x) d, grad_center = sum gX - R^T sum gX, in float64 from the tensor route's grad_coords
    gX = t["gc"].double().reshape(B, -1, 3)
    R, c64 = r.detach().double(), ce.detach().double()
    d = torch.einsum("brk,bnr->bnk", R, coords.double().reshape(B, -1, 3) - c64[:, None])          # R^T (X - c)
    grot = torch.einsum("bnr,bnk->brk", gX, d).cpu().numpy()
    gcen = (gX.sum(1) - torch.einsum("brk,br->bk", R, gX.sum(1))).cpu().numpy()
    _rel(tag + "rot grad", r.grad, grot)
    if np.abs(gcen).max() > 0:
        record_err(tag + "center grad", _err(ce.grad.cpu().numpy(), gcen), REL * float(np.abs(gX.sum(1).cpu().numpy()).max()))
    absent = torch.from_numpy(wts == 0).to(gpu)
    for g in (f.grad, p.grad, w.grad):
        assert torch.count_nonzero(g[absent]) == 0
    assert torch.count_nonzero(out[2]) == 0 and torch.count_nonzero(r.grad[2]) == 0 and torch.count_nonzero(ce.grad[2]) == 0


@pytest.mark.parametrize("case", ["eval_tri_coco", "train_tri_mpii"])
def test_volume_generator_view_weights(case, gpu):
    """batch['view_weights']: the pivot is the weighted DLT on the effective weights, the volume unprojection_cuboid with that pose, and a
    weight tensor that requires grad receives the sum of the DLT's and the aggregate's gradients"""
    from multiviewhmr_amd import multiview
    from test_pose_grad_gpu import _rebuild
    d = load_golden("posegrad", case)
    gen, batch, seed = _rebuild(d, gpu)
    gen.fused_conv = False
    if gen.aggregation_method == "max":
        gen.aggregation_method = "softmax"
    B, V = d["features_in"].shape[:2]
    rng = np.random.default_rng(60)
    wts = rng.uniform(0.05, 4.0, (B, V)).astype(np.float32)
    wts[1, 0] = 0.0                                           # at least two present views per sample (the triangulated pivot)
    mask = np.ones((B, V), bool)
    mask[0, V - 1] = False
    eff = np.where(mask, wts, 0).astype(np.float32)
    f = torch.from_numpy(d["features_in"]).to(gpu)
    P = torch.from_numpy(d["proj_org"]).to(gpu)
    w = torch.from_numpy(wts).to(gpu).requires_grad_(True)
    np.random.seed(seed)
    out = gen(f, P, dict(batch, view_weights=w, view_mask=torch.from_numpy(mask)))
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(61)).to(gpu)
    out.backward(go)
    # the same by hand: pivot, pose, volume
    hw = tuple(batch["images"].shape[2:4])
    centre = (torch.tensor(hw, dtype=torch.float32) / 2).expand(V, 2)
    w2 = torch.from_numpy(eff).to(gpu).requires_grad_(True)
    Pm = torch.where(torch.from_numpy(eff > 0).to(gpu)[:, :, None, None], P, torch.zeros((), device=gpu))
    pivot = multiview.triangulate_points_from_multiple_views_linear_batch(Pm, centre, w2)
    np.random.seed(seed)
    rots, centers = gen.volume_pose(batch, P, hw, torch.from_numpy(mask), w.detach())
    record_err("viewweights volgen pivot %s" % case, _err(centers.detach().cpu().numpy(), pivot.detach().cpu().numpy()), 1e-3)
    feats = gen.process_feature(f.view(-1, *f.shape[2:])).view(B, V, -1, *f.shape[3:])
    proj = aggregation.feature_level_projections(batch["cameras"], hw, tuple(f.shape[-2:]))
    cub, S = gen.cuboid(), gen.volume_size
    ref = aggregation.unprojection_cuboid(feats, torch.from_numpy(proj).to(gpu), rots.to(gpu), pivot, cub.position, cub.sides, (S, S, S),
                                          gen.aggregation_method, view_weights=w2)
    y = ref.detach().cpu().numpy()
    record_err("viewweights volgen volume %s" % case, _err(out.detach().cpu().numpy(), y), _bound(y))
    ref.backward(go)
    y = w2.grad.cpu().numpy()                                 # DLT's grad_conf + the aggregate's grad_weights, on the effective weights
    assert np.abs(y).max() > 0
    record_err("viewweights volgen weight grad %s" % case, _err(w.grad.cpu().numpy(), y), REL * float(np.abs(y).max()))
    assert float(w.grad[0, V - 1]) == 0.0 and float(w.grad[1, 0]) == 0.0


# ------------------------------------------------------------------------------------ graph capture
def test_weighted_forward_graph_capture(gpu):
    shape = SHAPES[0]
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=11)
    w = torch.from_numpy(_weights(shape["B"], shape["V"], seed=12)).to(gpu)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    eager = aggregation.unprojection(f, p, c, view_weights=w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        aggregation.unprojection(f, p, c, view_weights=w)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = aggregation.unprojection(f, p, c, view_weights=w)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
