"""Shared feature maps (unprojection(feature_index=...), mvhmr_unproject_*_shared) on the device: the reference's goldens on
features[idx], the oracle composition (tests/shared_oracle.py) at the smallest shapes of every kernel path, bit equality with the
materialised call, samples named twice, unused samples and invalid entries between NaN-filled neighbours, deterministic mode and the count
in its scale, storage modes, the cuboid route, the geometry gradients, routing, VolumeGenerator and graph capture.

No tolerance of its own: TOL / _bound (feature side) and REL (geometry side) are the project's, the storage bounds those of
test_view_mask_gpu.py (2e-2 for the 16-bit modes, _bound for channels-last)."""
import numpy as np
import pytest
import torch

import shared_oracle as so
from conftest import golden_cases, load_golden, record_err
from multiviewhmr_amd import aggregation
from posegrad_oracle import pose_grad
from test_geometry_grad_gpu import REL
from test_unproject_gpu import TOL, _bound, _err, _far_rig_problem, _ring_problem

pytestmark = pytest.mark.gpu

METHODS = ("softmax", "sum", "mean", "max")
STORAGE_BOUND = 2e-2                                       # the 16-bit storage modes (test_view_mask_gpu.py::test_storage_and_layouts)
# the smallest shapes at which each kernel path can go wrong; the index is ragged and unsorted and repeats a sample wherever B > 1, and
# leaves a sample unused where B = 3 (with B = 2 an unused sample would leave a single one: not unsorted)
SHAPES = [
    dict(B=3, M=5, V=2, C=16, H=32, W=32, vol=(8, 8, 8), index=[2, 0, 2, 2, 0]),          # V = 2
    dict(B=3, M=5, V=4, C=5, H=24, W=40, vol=(9, 7, 13), index=[1, 2, 1, 1, 2]),          # tile tail, C % 4 != 0, non-square map
    dict(B=2, M=6, V=8, C=300, H=24, W=24, vol=(4, 8, 16), index=[1, 0, 1, 1, 0, 1]),     # two channel groups
    dict(B=2, M=4, V=3, C=20, H=16, W=16, vol=(5, 6, 7), index=[1, 0, 1, 1]),             # run-time view loop
    dict(B=1, M=3, V=12, C=8, H=12, W=12, vol=(4, 5, 6), index=[0, 0, 0]),                # more than 8 views
]


def _id(s):
    return "B%dM%dV%dC%d" % (s["B"], s["M"], s["V"], s["C"])


def _coords(M, vol, scale=1.0):
    """one cuboid per volume: _ring_problem's grid, each turned by its own angle and moved by its own offset"""
    X, Y, Z = vol
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).astype(np.float64)
    pts = (-1250.0 + g * (2500.0 / (np.array([X, Y, Z]) - 1))) * scale
    out = []
    for m in range(M):
        ct, st = np.cos(0.3 + 0.25 * m), np.sin(0.3 + 0.25 * m)
        out.append(pts @ np.array([[ct, -st, 0], [st, ct, 0], [0, 0, 1.0]]).T + np.array([70.0 * m, -45.0 * m, 20.0 * m]))
    return np.stack(out).astype(np.float32)


def _problem(shape, seed=None):
    feats, proj, _ = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=shape["V"] if seed is None else seed)
    return feats, proj, _coords(shape["M"], shape["vol"]), np.asarray(shape["index"], np.int64)


def _run(f, p, c, idx, method, variant="auto", out_dtype=None, go=None, geometry=True):
    f = f.detach().clone().requires_grad_(True)
    p = p.detach().clone().requires_grad_(geometry)
    c = c.detach().clone().requires_grad_(geometry)
    out = aggregation.unprojection(f, p, c, method, variant=variant, out_dtype=out_dtype, feature_index=idx)
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
@pytest.mark.parametrize("case", golden_cases("shared"))
def test_goldens(case, variant, method, gpu):
    d = load_golden("shared", case)
    f, p, c, go = (torch.from_numpy(d[k]).to(gpu) for k in ("features", "proj", "coords", "grad_out"))
    r = _run(f, p, c, torch.from_numpy(d["index"]), method, variant, go=go)
    assert r["out"].shape == d["out_" + method].shape and r["gf"].shape == f.shape and r["gp"].shape == p.shape and r["gc"].shape == c.shape
    tag = "shared golden %s %s %s " % (case, method, variant)
    record_err(tag + "fwd", _err(r["out"].cpu().numpy(), d["out_" + method]), _bound(d["out_" + method]))
    record_err(tag + "bwd", _err(r["gf"].cpu().numpy(), d["gfeat_" + method]), _bound(d["gfeat_" + method]))
    _rel(tag + "proj grad", r["gp"], d["gproj_" + method].astype(np.float64))
    _rel(tag + "coord grad", r["gc"], d["gcoords_" + method].astype(np.float64))


# ------------------------------------------------------------------------------------ 2. the oracle composition
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_oracle_parity(shape, method, gpu):
    feats, proj, coords, index = _problem(shape)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    r = _run(f, p, c, torch.from_numpy(index).to(gpu), method)
    ref = so.shared_unprojection(feats, proj, coords, index, r["go"].cpu().numpy(), method)
    tag = "shared %s %s " % (_id(shape), method)
    assert tuple(r["out"].shape) == (shape["M"], shape["C"]) + tuple(shape["vol"])
    record_err(tag + "fwd", _err(r["out"].cpu().numpy(), ref["out"]), TOL)
    record_err(tag + "bwd", _err(r["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))
    _rel(tag + "proj grad", r["gp"], ref["grad_proj"])
    _rel(tag + "coord grad", r["gc"], ref["grad_coords"])
    for b in set(range(shape["B"])) - set(shape["index"]):                  # a sample no volume names: exact zeros, every element written
        assert torch.count_nonzero(r["gf"][b]) == 0 and torch.count_nonzero(r["gp"][b]) == 0


# ------------------------------------------------------------------------------------ 3. the materialised call
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES[:2] + SHAPES[3:4], ids=_id)
def test_it_is_the_materialised_gather_call(shape, method, gpu):
    """the same arithmetic on the same rows: the volume is bit-equal to the gather call on features[idx], proj[idx]; the feature gradient
    equals the index_add of that call's (float atomics arrive in another order: within _bound)"""
    feats, proj, coords, index = _problem(shape, seed=40)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    idx = torch.from_numpy(index).to(gpu)
    a = _run(f, p, c, idx, method)
    fm = f[idx].detach().clone().requires_grad_(True)
    out = aggregation.unprojection(fm, p[idx], c, method, variant="gather")
    assert torch.equal(a["out"], out)
    out.backward(a["go"])
    want = torch.zeros_like(f).index_add_(0, idx, fm.grad).cpu().numpy()
    record_err("shared materialised bwd %s %s" % (_id(shape), method), _err(a["gf"].cpu().numpy(), want), _bound(want))


@pytest.mark.parametrize("method", METHODS)
def test_the_identity_index_is_the_plain_gather_forward(method, gpu):
    shape = dict(SHAPES[1], M=3, index=[0, 1, 2])
    feats, proj, coords, index = _problem(shape, seed=41)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    for idx in (torch.from_numpy(index), torch.from_numpy(index).to(gpu), torch.from_numpy(index).to(gpu, torch.int32), torch.from_numpy(index).to(torch.uint8)):
        assert torch.equal(aggregation.unprojection(f, p, c, method, feature_index=idx), aggregation.unprojection(f, p, c, method, variant="gather"))
    assert aggregation.unprojection(f, p, c[:0], method, feature_index=torch.zeros(0, dtype=torch.long)).shape == (0, shape["C"]) + tuple(shape["vol"])


# ------------------------------------------------------------------------------------ 4. one sample named twice with the same coordinates
@pytest.mark.parametrize("method", METHODS)
def test_a_sample_named_twice_with_the_same_coordinates(method, gpu):
    shape = SHAPES[1]
    feats, proj, coords, _ = _problem(shape, seed=42)
    f, p = (torch.from_numpy(x).to(gpu) for x in (feats[:1], proj[:1]))
    c = torch.from_numpy(coords[:1]).to(gpu)
    go = torch.randn((1, shape["C"]) + tuple(shape["vol"]), generator=torch.Generator().manual_seed(8)).to(gpu)
    two = _run(f, p, c.expand(2, -1, -1, -1, -1).contiguous(), torch.tensor([0, 0]), method, go=go.expand(2, -1, -1, -1, -1).contiguous())
    one = _run(f, p, c, torch.tensor([0]), method, go=go)
    assert torch.equal(two["out"][0], two["out"][1]) and torch.equal(two["out"][0], one["out"][0])
    assert torch.equal(two["gc"][0], two["gc"][1]) and torch.equal(two["gc"][0], one["gc"][0])
    for k, name in (("gf", "bwd"), ("gp", "proj grad")):
        want = 2 * one[k].double().cpu().numpy()
        record_err("shared twice %s %s" % (method, name), _err(two[k].cpu().numpy(), want), _bound(want))


# ------------------------------------------------------------------------------------ 5. an unused sample and invalid entries
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES[:2] + SHAPES[3:4], ids=_id)
def test_invalid_entries_are_no_sample_and_nothing_is_read_through_them(shape, method, gpu):
    """the features and projections are the slice big[1:B+1] of allocations that hold one NaN-filled sample before and one behind: a read
    through -1 or B stays inside live memory and would show up as NaN (the pattern of test_guard_bands_gpu.py)"""
    B, M = 3, 5
    shape = dict(shape, B=B, M=M)
    feats, proj, coords, _ = _problem(dict(shape, index=[0] * M), seed=43)
    index = [1, 0, 1, 1, 0]                                                 # sample 2 is unused
    bigf = torch.full((B + 2,) + feats.shape[1:], float("nan"), device=gpu)
    bigp = torch.full((B + 2,) + proj.shape[1:], float("nan"), device=gpu)
    bigf[1:B + 1] = torch.from_numpy(feats).to(gpu)
    bigp[1:B + 1] = torch.from_numpy(proj).to(gpu)
    f, p = bigf[1:B + 1], bigp[1:B + 1]
    assert f.is_contiguous() and p.is_contiguous() and f.data_ptr() == bigf.data_ptr() + feats[0].size * 4
    c = torch.from_numpy(coords).to(gpu)
    with _Deterministic():                                                  # reproducible feature-gradient bits
        clean = _run(f, p, c, torch.tensor(index, device=gpu), method)
        assert torch.count_nonzero(clean["gf"][2]) == 0 and torch.count_nonzero(clean["gp"][2]) == 0
        assert torch.count_nonzero(clean["gf"][1]) > 0 and torch.count_nonzero(clean["gp"][1]) > 0
        # two invalid volumes among them, as a DEVICE index (nothing is inspected on the host)
        full = [1, -1, 0, 1, B, 1, 0]
        keep = [0, 2, 3, 5, 6]
        c7 = torch.cat([c[0:1], c[4:5], c[1:3], c[0:1], c[3:5]])
        go7 = torch.zeros((7,) + tuple(clean["go"].shape[1:]), device=gpu)
        go7[keep] = clean["go"]
        go7[[1, 4]] = 3.0                                                   # their grad_out must reach nothing
        r = _run(f, p, c7, torch.tensor(full, device=gpu, dtype=torch.int32), method, go=go7)
    for k in ("out", "gf", "gp", "gc"):
        assert torch.isfinite(r[k]).all(), k
    assert torch.count_nonzero(r["out"][[1, 4]]) == 0 and torch.count_nonzero(r["gc"][[1, 4]]) == 0
    assert torch.equal(r["out"][keep], clean["out"]) and torch.equal(r["gc"][keep], clean["gc"])
    assert torch.equal(r["gf"], clean["gf"]) and torch.equal(r["gp"], clean["gp"])


def test_invalid_entries_on_the_cuboid_route(gpu):
    B, V, C, H, W, S = 2, 4, 8, 24, 20, 8
    feats, proj, _ = _ring_problem(B, V, C, H, W, (S, S, S), seed=44)
    f, p = (torch.from_numpy(x).to(gpu) for x in (feats, proj))
    rot = torch.eye(3, device=gpu).repeat(3, 1, 1)
    rot[1] = float("nan")                                                   # the pose of a volume without a sample is not read either
    cen = torch.zeros(3, 3, device=gpu)
    idx = torch.tensor([1, 7, 0], device=gpu)
    f, p, rot, cen = (t.requires_grad_(True) for t in (f, p, rot, cen))
    out = aggregation.unprojection_cuboid(f, p, rot, cen, (-1250.0,) * 3, (2500.0,) * 3, (S, S, S), "softmax", feature_index=idx)
    out.backward(torch.ones_like(out))
    for t in (out, f.grad, p.grad, rot.grad, cen.grad):
        assert torch.isfinite(t).all()
    assert torch.count_nonzero(out[1]) == 0 and torch.count_nonzero(rot.grad[1]) == 0 and torch.count_nonzero(cen.grad[1]) == 0
    assert torch.count_nonzero(out[0]) > 0 and torch.count_nonzero(rot.grad[2]) > 0


# ------------------------------------------------------------------------------------ 6. deterministic mode
@pytest.mark.parametrize("method", METHODS)
def test_deterministic_mode_repeats_bitwise_and_ignores_the_order_of_the_volumes(method, gpu):
    shape = SHAPES[1]
    feats, proj, coords, index = _problem(shape, seed=45)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    idx = torch.from_numpy(index).to(gpu)
    with _Deterministic():
        runs = [_run(f, p, c, idx, method) for _ in range(3)]
        for r in runs[1:]:
            for k in ("out", "gf", "gp", "gc"):
                assert torch.equal(r[k], runs[0][k]), k
        perm = torch.tensor([3, 0, 4, 2, 1], device=gpu)
        q = _run(f, p, c[perm], idx[perm], method, go=runs[0]["go"][perm])
    assert torch.equal(q["gf"], runs[0]["gf"])                              # integer sums: any arrival order, any volume order
    assert torch.equal(q["out"], runs[0]["out"][perm])
    ref = so.shared_unprojection(feats, proj, coords, index, runs[0]["go"].cpu().numpy(), method, geometry=False)
    record_err("shared deterministic bwd %s" % method, _err(runs[0]["gf"].cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))


def test_deterministic_scale_counts_the_volumes_that_share_a_sample(gpu):
    """B = 1, M = 16 identical volumes, `sum`, a camera rig so far away that every voxel projects into one pixel footprint, a constant
    grad_out g just below a power of two.  The per-sample bound N * g * 2^K < 2^62 alone puts g * 2^K just below 2^51 (N = 12^3 = 1728 voxels
    round up to 2^11), and the heaviest pixel of a view collects `heavy` units of tap weight out of M * N = 27648 -- at least a quarter when the
    footprint is one 2 x 2 cell -- so its int64 sum would pass 2^63 and wrap; with cnt[b] = 16 in the bound it stays below 2^59."""
    M, g = 16, float(np.float32(0.999 * 2.0 ** 20))
    shape = dict(B=1, V=4, C=4, H=24, W=24, vol=(12, 12, 12))
    feats, proj, coords = _far_rig_problem(seed=46, radius=400000.0, **shape)
    coords = np.repeat(coords, M, 0)
    index = np.zeros(M, np.int64)
    go = np.full((M, shape["C"]) + shape["vol"], g, np.float32)
    ref = so.shared_unprojection(feats, proj, coords, index, go, "sum", geometry=False)["grad_features"]
    heavy = float(np.abs(ref).max()) / g
    assert heavy * 0.999 * 2.0 ** 51 > 2.0 ** 63, heavy                     # the premise: without the count this sum wraps
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    with _Deterministic():
        a = _run(f, p, c, torch.from_numpy(index).to(gpu), "sum", go=torch.from_numpy(go).to(gpu), geometry=False)
        b = _run(f, p, c, torch.from_numpy(index).to(gpu), "sum", go=torch.from_numpy(go).to(gpu), geometry=False)
    assert torch.isfinite(a["gf"]).all() and torch.equal(a["gf"], b["gf"])
    record_err("shared deterministic scale with 16 volumes on one sample", _err(a["gf"].cpu().numpy(), ref), _bound(ref))


# ------------------------------------------------------------------------------------ 7. storage modes
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("storage", ["f16", "bf16vol", "channels_last"])
def test_storage_modes(storage, deterministic, gpu):
    """against the fp32 oracle on the rounded inputs, with the bounds of the existing storage tests"""
    shape = dict(B=3, M=5, V=4, C=8, H=24, W=20, vol=(8, 8, 16), index=[2, 0, 2, 2, 0])
    feats, proj, coords, index = _problem(shape, seed=47)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    out_dtype = None
    if storage == "f16":
        f = f.half()
        feats = f.float().cpu().numpy()
    elif storage == "bf16vol":
        out_dtype = torch.bfloat16
    else:
        f = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    if deterministic:
        with _Deterministic():
            r = _run(f, p, c, torch.from_numpy(index), "softmax", out_dtype=out_dtype)
    else:
        r = _run(f, p, c, torch.from_numpy(index), "softmax", out_dtype=out_dtype)
    want = {"f16": torch.float16, "bf16vol": torch.bfloat16, "channels_last": torch.float32}[storage]
    assert r["out"].dtype == want and r["gf"].dtype == f.dtype and r["gf"].shape == f.shape and r["gp"].dtype == torch.float32
    ref = so.shared_unprojection(feats, proj, coords, index, r["go"].float().cpu().numpy(), "softmax")
    tag = "shared storage %s det=%d " % (storage, deterministic)
    record_err(tag + "fwd", _err(r["out"].float().cpu().numpy(), ref["out"]), STORAGE_BOUND if storage != "channels_last" else _bound(ref["out"]))
    record_err(tag + "bwd", _err(r["gf"].float().cpu().numpy(), ref["grad_features"]), STORAGE_BOUND if storage != "channels_last" else _bound(ref["grad_features"]))
    assert torch.count_nonzero(r["gf"][1]) == 0 and torch.count_nonzero(r["gp"][1]) == 0
    _rel(tag + "proj grad", r["gp"], ref["grad_proj"])
    _rel(tag + "coord grad", r["gc"], ref["grad_coords"])


# ------------------------------------------------------------------------------------ 8. the cuboid route
@pytest.mark.parametrize("method", METHODS)
def test_cuboid_route(method, gpu):
    B, M, V, C, H, W, S = 3, 5, 4, 8, 24, 20, 12
    index = np.array([2, 0, 2, 2, 0])
    feats, proj, _ = _ring_problem(B, V, C, H, W, (S, S, S), seed=48)
    rng = np.random.default_rng(49)
    th = rng.uniform(0, 2 * np.pi, M)
    rot = np.stack([[[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]] for t in th]).astype(np.float32)
    cen = rng.uniform(-100, 100, (M, 3)).astype(np.float32)
    f, p, r, ce = (torch.from_numpy(x).to(gpu) for x in (feats, proj, rot, cen))
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=4, output_channels=4, cuboid_side=2500.0, device=gpu)
    cub = gen.cuboid()
    coords = gen.coord_volumes(r, ce, gpu)                                  # mvhmr_build_coord_volumes for the M poses
    idx = torch.from_numpy(index)
    a = aggregation.unprojection(f, p, coords, method, feature_index=idx)
    f, p, r, ce = (t.detach().clone().requires_grad_(True) for t in (f, p, r, ce))
    b = aggregation.unprojection_cuboid(f, p, r, ce, cub.position, cub.sides, (S, S, S), method, feature_index=idx)
    assert torch.equal(a, b)
    go = torch.randn(b.shape, generator=torch.Generator().manual_seed(50)).to(gpu)
    b.backward(go)
    assert r.grad.shape == (M, 3, 3) and ce.grad.shape == (M, 3) and p.grad.shape == (B, V, 3, 4)
    gp, gr, gc = pose_grad(feats[index], proj[index], rot, cen, cub.position, cub.sides, (S, S, S), go.cpu().numpy(), method)
    gp_b = np.zeros(proj.shape, np.float64)
    np.add.at(gp_b, index, gp)
    tag = "shared cuboid %s " % method
    _rel(tag + "rot grad", r.grad, gr)
    _rel(tag + "center grad", ce.grad, gc)
    _rel(tag + "proj grad", p.grad, gp_b)
    assert torch.count_nonzero(p.grad[1]) == 0 and torch.count_nonzero(f.grad[1]) == 0
    ref = so.shared_unprojection(feats, proj, coords.cpu().numpy(), index, go.cpu().numpy(), method, geometry=False)
    record_err(tag + "bwd", _err(f.grad.cpu().numpy(), ref["grad_features"]), _bound(ref["grad_features"]))


# ------------------------------------------------------------------------------------ 9. geometry gradients
class _Spy:
    """the extension's namespace, remembering which ops were asked for"""

    def __init__(self, real):
        self.real, self.asked = real, []

    def __getattr__(self, name):
        self.asked.append(name)
        return getattr(self.real, name)


def test_geometry_gradients_repeat_bitwise_and_a_features_only_backward_launches_no_geometry_kernel(gpu, monkeypatch):
    shape = SHAPES[1]
    feats, proj, coords, index = _problem(shape, seed=51)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    idx = torch.from_numpy(index).to(gpu)
    a = _run(f, p, c, idx, "softmax")
    for _ in range(2):                                                      # default mode: no float atomics on the geometry side
        b = _run(f, p, c, idx, "softmax", go=a["go"])
        assert torch.equal(a["gp"], b["gp"]) and torch.equal(a["gc"], b["gc"])
    spy = _Spy(aggregation._native())
    monkeypatch.setattr(aggregation, "_native", lambda: spy)
    r = _run(f, p, c, idx, "softmax", go=a["go"], geometry=False)
    assert r["gp"] is None and r["gc"] is None and spy.asked == ["unprojection", "unprojection_backward"]
    spy.asked.clear()
    _run(f, p, c, idx, "softmax", go=a["go"])
    assert spy.asked == ["unprojection", "unprojection_backward", "unprojection_backward_geometry"]


# ------------------------------------------------------------------------------------ 10. routing
def test_brick_is_refused_and_auto_runs_the_gather_family(gpu):
    shape = dict(B=2, M=3, V=4, C=32, H=24, W=24, vol=(64, 64, 32), index=[1, 1, 0])       # a shape AUTO gates towards the bricks without an index
    feats, proj, coords, index = _problem(shape, seed=52)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    idx = torch.from_numpy(index)
    with pytest.raises(RuntimeError, match="shared feature maps run the gather kernels"):
        aggregation.unprojection(f, p, c, variant="brick", feature_index=idx)
    auto = aggregation.unprojection(f, p, c, variant="auto", feature_index=idx)
    assert torch.equal(auto, aggregation.unprojection(f, p, c, variant="gather", feature_index=idx))
    assert torch.equal(auto, aggregation.unprojection(f[idx.to(gpu)], p[idx.to(gpu)], c, variant="gather"))
    cl = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)       # channels-last features: read as they are
    assert torch.equal(aggregation.unprojection(cl, p, c, feature_index=idx), auto)


# ------------------------------------------------------------------------------------ 11. VolumeGenerator
@pytest.mark.parametrize("triangulate", [False, True])
def test_volume_generator_reads_the_index_from_the_batch(triangulate, gpu):
    from test_visible_gpu import _generator_problem
    gen, batch, feats, proj_org = _generator_problem(gpu, False)
    gen.use_triangulation = triangulate
    gen.train()                                                             # one theta per volume: under theta = 0 the pivot cancels (X = g)
    B, V = feats.shape[:2]
    S = gen.volume_size
    idx = torch.tensor([1, 0, 1])
    kp = torch.zeros(3, 17, 3)
    kp[:, 6] = torch.tensor([[100.0, -50.0, 30.0], [0.0, 0.0, 0.0], [-200.0, 80.0, -60.0]])
    shared = dict(batch, feature_index=idx, keypoints_3d=kp)
    P = proj_org.clone().requires_grad_(True)
    x = feats.clone().requires_grad_(True)
    np.random.seed(55)
    out = gen(x, P, shared)
    assert tuple(out.shape) == (3, gen.process_feature[0].out_channels, S, S, S)
    # the same by hand: the conv, then unprojection_cuboid on the generator's own projections and the volumes' poses
    conv = gen.process_feature(feats.view(-1, *feats.shape[2:]))
    conv = conv.view(B, V, *conv.shape[1:])
    proj = aggregation.feature_level_projections_device(batch["cameras_packed"], (96, 96), tuple(feats.shape[-2:])).to(gpu).contiguous()
    np.random.seed(55)                                                      # the same draws as the call above
    rots, centers = gen.volume_pose(shared, proj_org, (96, 96), feature_index=idx)
    assert tuple(rots.shape) == (3, 3, 3) and tuple(centers.shape) == (3, 3)
    if triangulate:
        per_sample = gen.volume_pose(batch, proj_org, (96, 96))[1]
        assert torch.equal(centers, per_sample[idx.to(per_sample.device)])  # the per-sample DLT pivots, gathered
    else:
        assert torch.equal(centers.cpu(), kp[:, 6])
    cub = gen.cuboid()
    ref = aggregation.unprojection_cuboid(conv, proj, rots, centers, cub.position, cub.sides, (S, S, S), aggregation_method=gen.aggregation_method,
                                          feature_index=idx)
    assert torch.equal(out, ref)
    assert not torch.equal(out[0], out[2])                                  # one pose per volume, also where two volumes share a sample
    out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(53)).to(gpu))
    assert x.grad is not None and torch.count_nonzero(x.grad) > 0
    if triangulate:
        assert P.grad is not None and torch.isfinite(P.grad).all() and torch.count_nonzero(P.grad) > 0      # proj_org.grad reaches the caller
    # the identity index gives the generator's plain unfused result
    gen.fused_conv = False
    np.random.seed(56)
    plain = gen(feats, proj_org, batch)
    np.random.seed(56)                                                      # ... and consumes the global stream as the plain call does (Q6)
    assert torch.equal(gen(feats, proj_org, dict(batch, feature_index=torch.arange(B))), plain)


# ------------------------------------------------------------------------------------ 12. graph capture
def test_forward_graph_capture_follows_the_index(gpu):
    shape = SHAPES[1]
    feats, proj, coords, index = _problem(shape, seed=54)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    idx = torch.from_numpy(index).to(gpu, torch.int32)
    other = torch.tensor([0, 0, 2, 1, 2], device=gpu, dtype=torch.int32)
    eager, eager_other = aggregation.unprojection(f, p, c, feature_index=idx), aggregation.unprojection(f, p, c, feature_index=other)
    assert not torch.equal(eager, eager_other)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        aggregation.unprojection(f, p, c, feature_index=idx)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = aggregation.unprojection(f, p, c, feature_index=idx)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    idx.copy_(other)                                                        # in place: the captured launch reads the index on the device
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_other)


def test_deterministic_sum_takes_more_than_65535_maps(gpu):
    """only the softmax scale pass puts the (sample, view) maps in a grid's y extent: a deterministic `sum` over B * V > 65535 maps
    (channels-last: no layout pass) runs like the default mode does and agrees with it"""
    B, V, C, H, W = 4097, 16, 4, 2, 2
    g = torch.Generator().manual_seed(57)
    f = torch.randn(B, V, H, W, C, generator=g).to(gpu).permute(0, 1, 4, 2, 3)
    p = torch.zeros(B, V, 3, 4, device=gpu)
    p[:, :, 0, 0] = p[:, :, 1, 1] = p[:, :, 2, 3] = 1                       # u = X0, v = X1, z = 1
    c = torch.rand(3, 2, 2, 2, 3, generator=g).to(gpu) * 2
    idx = torch.tensor([4096, 7, 4096], device=gpu)
    a = _run(f, p, c, idx, "sum", geometry=False)
    with _Deterministic():
        d = _run(f, p, c, idx, "sum", go=a["go"], geometry=False)
    want = a["gf"].cpu().numpy()
    assert np.abs(want[4096]).max() > 0 and not want[:7].any()
    record_err("shared deterministic sum, 65552 maps", _err(d["gf"].cpu().numpy(), want), _bound(want))
