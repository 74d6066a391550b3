"""Per-sample view masks (unprojection(view_mask=...), mvhmr_unproject_*_masked) on the device: every sample against the CPU oracle run
on its present views alone, masked data never read, masked gradients exactly zero, empty samples, the all-true mask against the unmasked
gather route, and bitwise repeats in deterministic mode."""
import numpy as np
import pytest
import torch

from conftest import record_err
from multiviewhmr_amd import aggregation
from oracle import cport
from test_unproject_gpu import _bound, _err, _ring_problem

pytestmark = pytest.mark.gpu

METHODS = ("softmax", "sum", "mean", "max")


def _mask(B, V, seed):
    """a different subset per sample: sample 0 all views, sample 1 one view, sample 2 none, the rest random"""
    rng = np.random.default_rng(seed)
    m = rng.random((B, V)) < 0.6
    m[0] = True
    m[1] = False
    m[1, V - 1] = True
    m[2] = False
    return m


def _run(f, p, c, mask, method, variant="auto", out_dtype=None, go=None, geometry=True):
    f = f.detach().clone().requires_grad_(True)
    p = p.detach().clone().requires_grad_(geometry)
    c = c.detach().clone().requires_grad_(geometry)
    out = aggregation.unprojection(f, p, c, method, variant=variant, out_dtype=out_dtype, view_mask=mask)
    if go is None:
        go = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(out.device, out.dtype)
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach(), f.grad, (p.grad if geometry else None), (c.grad if geometry else None), go


def _subset_refs(feats, proj, coords, mask, go, method):
    outs, grads = [], []
    for b in range(feats.shape[0]):
        P = np.nonzero(mask[b])[0]
        C = feats.shape[2]
        if len(P) == 0:
            outs.append(np.zeros((C,) + coords.shape[1:4], np.float32))
            grads.append(np.zeros(feats.shape[1:], np.float32))
            continue
        fb, pb, cb = feats[b:b + 1, P], proj[b:b + 1, P], coords[b:b + 1]
        outs.append(cport.forward(fb, pb, cb, method)[0])
        g = np.zeros(feats.shape[1:], np.float32)
        g[P] = cport.backward(go[b:b + 1], fb, pb, cb, method)[0]
        grads.append(g)
    return np.stack(outs), np.stack(grads)


SHAPES = [
    dict(B=6, V=4, C=8, H=24, W=20, vol=(16, 16, 32)),     # the vector-view gather instances (V = 4)
    dict(B=5, V=8, C=8, H=20, W=16, vol=(8, 8, 16)),       # V = 8
    dict(B=4, V=3, C=6, H=16, W=16, vol=(8, 8, 8)),        # runtime view count, C % 4 != 0
    dict(B=4, V=12, C=4, H=12, W=12, vol=(8, 8, 8)),       # 12 views
]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("variant", ["auto", "gather"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "V%dC%d" % (s["V"], s["C"]))
def test_subset_parity(shape, variant, method, gpu):
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=shape["V"])
    mask = _mask(shape["B"], shape["V"], seed=shape["C"])
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    out, gf, gp, gc, go = _run(f, p, c, torch.from_numpy(mask), method, variant)
    ref, gref = _subset_refs(feats, proj, coords, mask, go.cpu().numpy(), method)
    tag = "mask %s %s V%d C%d" % (variant, method, shape["V"], shape["C"])
    record_err(tag + " fwd", _err(out.cpu().numpy(), ref), _bound(ref))
    record_err(tag + " bwd", _err(gf.cpu().numpy(), gref), _bound(gref))
    # masked views: exactly zero gradients (features and projection rows); an empty sample: a zero volume
    assert torch.count_nonzero(gf[~torch.from_numpy(mask).to(gpu)]) == 0
    assert torch.count_nonzero(gp[~torch.from_numpy(mask).to(gpu)]) == 0
    assert torch.count_nonzero(out[2]) == 0 and torch.count_nonzero(gc[2]) == 0
    # the geometry gradients of every sample match the subset problem's (sample by sample, the unmasked op on the present views)
    for b in (0, 1, 3):
        P = torch.from_numpy(np.nonzero(mask[b])[0]).to(gpu)
        _, _, gp1, gc1, _ = _run(f[b:b + 1, P], p[b:b + 1, P], c[b:b + 1], None, method, "gather", go=go[b:b + 1])
        record_err(tag + " proj grad b%d" % b, _err(gp[b, P].cpu().numpy(), gp1[0].cpu().numpy()), _bound(gp1.cpu().numpy()))
        record_err(tag + " coord grad b%d" % b, _err(gc[b].cpu().numpy(), gc1[0].cpu().numpy()), _bound(gc1.cpu().numpy()))


@pytest.mark.parametrize("storage", ["f16", "bf16vol", "channels_last"])
def test_storage_and_layouts(storage, gpu):
    shape = SHAPES[0]
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=3)
    mask = _mask(shape["B"], shape["V"], seed=4)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    out_dtype = None
    if storage == "f16":
        f = f.half()
        feats = f.float().cpu().numpy()
    elif storage == "bf16vol":
        out_dtype = torch.bfloat16
    else:
        f = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    out, gf, _, _, go = _run(f, p, c, torch.from_numpy(mask), "softmax", out_dtype=out_dtype, geometry=False)
    ref, gref = _subset_refs(feats, proj, coords, mask, go.float().cpu().numpy(), "softmax")
    bound = 2e-2 if storage != "channels_last" else _bound(ref)
    record_err("mask storage %s fwd" % storage, _err(out.float().cpu().numpy(), ref), bound)
    record_err("mask storage %s bwd" % storage, _err(gf.float().cpu().numpy(), gref), 2e-2 if storage != "channels_last" else _bound(gref))
    assert torch.count_nonzero(gf[~torch.from_numpy(mask).to(gpu)]) == 0


@pytest.mark.parametrize("method", METHODS)
def test_masked_data_is_never_read(method, gpu):
    shape = SHAPES[0]
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=5)
    mask = _mask(shape["B"], shape["V"], seed=6)
    m = torch.from_numpy(mask).to(gpu)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    runs = []
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)          # the default feature gradient adds with float atomics: compare reproducible bits
    try:
        for fill in (0.0, float("nan"), float("inf")):
            fg, pg = f.clone(), p.clone()
            fg[~m] = fill
            pg[~m] = -fill if fill == float("inf") else fill
            runs.append(_run(fg, pg, c, m, method, go=runs[0][4] if runs else None))
    finally:
        torch.use_deterministic_algorithms(was)
    for r in runs[1:]:
        for a, b in zip(runs[0][:4], r[:4]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "V%dC%d" % (s["V"], s["C"]))
def test_all_true_mask_is_the_gather_route_bitwise(shape, method, gpu):
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=8)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    f = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) if shape["C"] % 4 == 0 else f   # the scatter backward on both sides
    full = torch.ones(shape["B"], shape["V"], dtype=torch.bool)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)          # reproducible feature-gradient bits on both sides (the default adds with atomics)
    try:
        a = _run(f, p, c, full, method, "gather")
        b = _run(f, p, c, None, method, "gather", go=a[4])
    finally:
        torch.use_deterministic_algorithms(was)
    assert torch.equal(a[0], b[0])
    if shape["C"] % 4 == 0:
        assert torch.equal(a[1], b[1])
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    # and the forward of planar features too
    a = aggregation.unprojection(f.contiguous(), p, c, method, variant="gather", view_mask=full)
    b = aggregation.unprojection(f.contiguous(), p, c, method, variant="gather")
    assert torch.equal(a, b)


def test_deterministic_mode_repeats_bitwise(gpu):
    shape = SHAPES[0]
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=9)
    mask = torch.from_numpy(_mask(shape["B"], shape["V"], seed=10))
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        a = _run(f, p, c, mask, "softmax")
        b = _run(f, p, c, mask, "softmax", go=a[4])
    finally:
        torch.use_deterministic_algorithms(was)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    _, gref = _subset_refs(feats, proj, coords, mask.numpy(), a[4].cpu().numpy(), "softmax")
    record_err("mask deterministic bwd", _err(a[1].cpu().numpy(), gref), _bound(gref))


def test_masked_forward_graph_capture(gpu):
    shape = SHAPES[0]
    feats, proj, coords = _ring_problem(shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"], seed=11)
    mask = torch.from_numpy(_mask(shape["B"], shape["V"], seed=12)).to(gpu)
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    eager = aggregation.unprojection(f, p, c, view_mask=mask)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        aggregation.unprojection(f, p, c, view_mask=mask)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = aggregation.unprojection(f, p, c, view_mask=mask)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_masked_mean_deterministic_with_few_present_views(gpu):
    """mean's ds is g / n_b: the deterministic scale must be chosen from n_b, not V (a single present view of eight here)"""
    B, V, C, H, W, vol = 3, 8, 8, 12, 12, (16, 16, 16)
    feats, proj, coords = _ring_problem(B, V, C, H, W, vol, seed=13)
    mask = np.zeros((B, V), bool)
    mask[0, 3] = True
    mask[1, [0, 5]] = True
    mask[2, :] = True
    f, p, c = (torch.from_numpy(x).to(gpu) for x in (feats, proj, coords))
    go = torch.full((B, C) + vol, 3.0e3, device=gpu)                # large, uniform: every contribution near the bound
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        a = _run(f, p, c, torch.from_numpy(mask), "mean", go=go, geometry=False)
        b = _run(f, p, c, torch.from_numpy(mask), "mean", go=go, geometry=False)
    finally:
        torch.use_deterministic_algorithms(was)
    assert torch.equal(a[1], b[1])
    _, gref = _subset_refs(feats, proj, coords, mask, go.cpu().numpy(), "mean")
    record_err("mask deterministic mean few views", _err(a[1].cpu().numpy(), gref), _bound(gref))


@pytest.mark.parametrize("method", METHODS)
def test_cuboid_route_matches_per_sample_runs(method, gpu):
    B, V, C, H, W, S = 5, 4, 8, 24, 20, 16
    feats, proj, _ = _ring_problem(B, V, C, H, W, (S, S, S), seed=14)
    mask = _mask(B, V, seed=15)
    rng = np.random.default_rng(16)
    th = rng.uniform(0, 2 * np.pi, B)
    rot = np.stack([[[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]] for t in th]).astype(np.float32)
    cen = rng.uniform(-100, 100, (B, 3)).astype(np.float32)
    pos, sides = (-1250.0, -1250.0, -1250.0), (2500.0, 2500.0, 2500.0)
    f, p, r, ce = (torch.from_numpy(x).to(gpu) for x in (feats, proj, rot, cen))

    def run(f, p, r, ce, m, go=None):
        f, p, r, ce = (t.detach().clone().requires_grad_(True) for t in (f, p, r, ce))
        out = aggregation.unprojection_cuboid(f, p, r, ce, pos, sides, (S, S, S), method, view_mask=m)
        if go is None:
            go = torch.randn(out.shape, generator=torch.Generator().manual_seed(17)).to(gpu)
        out.backward(go)
        return out.detach(), f.grad, p.grad, r.grad, ce.grad, go

    out, gf, gp, gr, gc, go = run(f, p, r, ce, torch.from_numpy(mask))
    m = torch.from_numpy(mask).to(gpu)
    assert torch.count_nonzero(gf[~m]) == 0 and torch.count_nonzero(gp[~m]) == 0
    assert torch.count_nonzero(out[2]) == 0 and torch.count_nonzero(gr[2]) == 0 and torch.count_nonzero(gc[2]) == 0
    for b in range(B):
        P = torch.from_numpy(np.nonzero(mask[b])[0]).to(gpu)
        if len(P) == 0:
            continue
        o1, gf1, gp1, gr1, gc1, _ = run(f[b:b + 1, P], p[b:b + 1, P], r[b:b + 1], ce[b:b + 1], None, go[b:b + 1])
        tag = "mask cuboid %s b%d" % (method, b)
        for name, x, y in (("fwd", out[b], o1[0]), ("feat grad", gf[b, P], gf1[0]), ("proj grad", gp[b, P], gp1[0]), ("rot grad", gr[b], gr1[0]),
                           ("center grad", gc[b], gc1[0])):
            y = y.cpu().numpy()
            record_err(tag + " " + name, _err(x.cpu().numpy(), y), _bound(y))


@pytest.mark.parametrize("case", ["eval_tri_coco", "train_tri_mpii"])
@pytest.mark.parametrize("triangulate", [True, False])
def test_volume_generator_view_mask_matches_per_sample_runs(case, triangulate, gpu):
    """batch['view_mask']: every sample equals a run of the generator on its present cameras alone; in training the global numpy stream
    is re-seeded so that both sides draw the same rotation (one draw per sample, in order)"""
    from conftest import load_golden
    from multiviewhmr_amd import multiview
    from test_pose_grad_gpu import _rebuild
    d = load_golden("posegrad", case)
    gen, batch, seed = _rebuild(d, gpu)
    gen.use_triangulation = triangulate
    gen.fused_conv = False
    B, V = d["features_in"].shape[:2]
    mask = np.ones((B, V), bool)
    mask[1, 0] = False                                       # at least two present views per sample (the triangulated pivot)
    f = torch.from_numpy(d["features_in"]).to(gpu)
    P = torch.from_numpy(d["proj_org"]).to(gpu)
    np.random.seed(seed)
    out = gen(f, P, dict(batch, view_mask=torch.from_numpy(mask)))
    for b in range(B):
        pv = list(np.nonzero(mask[b])[0])
        sub = dict(images=batch["images"][b:b + 1][:, pv], cameras=[batch["cameras"][v][b:b + 1] for v in pv],
                   keypoints_3d=[batch["keypoints_3d"][b]])
        np.random.seed(seed)
        if b:
            np.random.uniform(0.0, 2 * np.pi, size=b)         # the draws of the samples before this one (training only reads them)
        ref = gen(f[b:b + 1, pv], P[b:b + 1, pv], sub)
        ref = ref.detach().cpu().numpy()
        record_err("mask volgen %s tri=%d b%d" % (case, triangulate, b), _err(out[b].detach().cpu().numpy(), ref[0]), _bound(ref))
    if triangulate:                                           # the pivot: the DLT on the present views only
        hw = tuple(batch["images"].shape[2:4])
        c = (torch.tensor(hw, dtype=torch.float32) / 2)
        for b in range(B):
            pv = torch.from_numpy(np.nonzero(mask[b])[0]).to(gpu)
            one = multiview.triangulate_points_from_multiple_views_linear_batch(P[b:b + 1, pv], c.expand(len(pv), 2))
            Pm = torch.where(torch.from_numpy(mask).to(gpu)[:, :, None, None], P, torch.zeros((), device=gpu))
            allm = multiview.triangulate_points_from_multiple_views_linear_batch(Pm, c.expand(V, 2), torch.from_numpy(mask).float().to(gpu))
            record_err("mask volgen pivot %s b%d" % (case, b), _err(allm[b].cpu().numpy(), one[0].cpu().numpy()), 1e-3)
