"""Gradients of the cuboid route w.r.t. proj_matricies, rotations and centers (k_bwd_geom's pose epilogue + k_pose_reduce) and of the
DLT triangulation (k_triangulate_dlt_bwd) on the MI355X: against the float64 oracle (tests/posegrad_oracle.py), against the tensor route
fed the same coordinates, against the reference's goldens through VolumeGenerator, bitwise reproducibility, and unchanged feature
gradients and DLT forward.  Errors are asserted through conftest.record_err, which also keeps them."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden_cases, load_golden, record_err
from posegrad_oracle import cuboid_points, dlt_grad, pose_grad
from test_geometry_grad_gpu import _features, _ring
from multiviewhmr_amd import _capi, aggregation, multiview, volumetric

pytestmark = pytest.mark.gpu
REL = 1e-4
POSITION, SIDES = (-1.2, -1.1, -1.3), (2.4, 2.2, 2.6)


def _pose(B, seed, identity=False):
    rng = np.random.default_rng(seed)
    if identity:
        rot = np.tile(np.eye(3, dtype=np.float32), (B, 1, 1))
    else:
        rot = np.stack([volumetric.get_rotation_matrix(rng.normal(size=3), rng.uniform(0, 2 * np.pi)) for _ in range(B)]).astype(np.float32)
    return rot, rng.uniform(-0.2, 0.2, (B, 3)).astype(np.float32)


def _quad(f):
    """the library's quad-planar copy of planar fp32 features (mvhmr_convert_features), as the fused path keeps it"""
    L = _capi.lib()
    desc = aggregation._make_desc(f, (1, 1, 1), 0, torch.float32, _capi.LAYOUT_BVCHW, 0)
    q = torch.empty(L.mvhmr_feature_layout_bytes(ctypes.byref(desc), _capi.LAYOUT_QUAD), dtype=torch.uint8, device=f.device)
    _capi.check(L.mvhmr_convert_features(ctypes.byref(desc), aggregation._ptr(f), _capi.LAYOUT_QUAD, aggregation._ptr(q),
                                         aggregation._stream(f.device)))
    return q


def _cuboid_geometry(f, P, rot, center, go, vol, method, odt=None, layout="planar", want=(True, True, True)):
    """-> grad_proj, grad_rot, grad_center of the cuboid route (None where not asked for), plus the grad_out the kernels read"""
    gpu = f.device
    m = _capi.AGG[method]
    out_dtype = odt or (torch.float16 if f.dtype == torch.float16 else torch.float32)
    g = torch.from_numpy(go).to(gpu, out_dtype)
    p, r, c = (torch.from_numpy(a).to(gpu) for a in (P, rot, center))
    args = ([float(x) for x in POSITION], [float(x) for x in SIDES], list(vol), m, aggregation._dtype_code(out_dtype), 0)
    if layout == "quad":
        B, V, C, H, W = f.shape
        desc = (B, V, C, H, W, m, _capi.F32, aggregation._dtype_code(out_dtype), _capi.LAYOUT_QUAD, 0)
        res = aggregation._native().unprojection_cuboid_backward_geometry(g, _quad(f), p, r, c, *args[:3], *desc, *want)
    else:
        res = torch.ops.mvhmr.unprojection_cuboid_backward_geometry(g, f, p, r, c, *args, *want)
    return tuple(t if w else None for t, w in zip(res, want)), g.float().cpu().numpy()


def _check(name, got, ref, rel=REL):
    scale = float(np.abs(ref).max())
    assert scale > 0, name
    record_err(name, float(np.abs(got.cpu().double().numpy() - ref).max()), rel * scale)


# rows: B, V, C, Hf, Wf, vol, method, layout, feature dtype, volume dtype
ROWS = [
    (2, 1, 5, 11, 16, (5, 4, 6), "softmax", "planar", torch.float32, None),
    (2, 3, 6, 12, 18, (7, 3, 5), "sum", "planar", torch.float32, None),
    (1, 4, 8, 16, 20, (6, 5, 4), "mean", "channels_last", torch.float32, None),
    (2, 4, 12, 16, 16, (5, 5, 5), "max", "quad", torch.float32, None),
    (1, 5, 7, 10, 14, (4, 6, 5), "softmax", "planar", torch.float16, None),
    (1, 8, 16, 12, 12, (5, 4, 5), "softmax", "channels_last", torch.float16, torch.float32),
    (1, 11, 9, 9, 13, (3, 5, 7), "mean", "planar", torch.float32, torch.bfloat16),
    (1, 16, 4, 8, 10, (4, 4, 3), "softmax", "quad", torch.float32, torch.bfloat16),
    (2, 16, 3, 8, 8, (3, 3, 5), "sum", "planar", torch.float32, None),
    (1, 4, 32, 20, 24, (21, 20, 22), "softmax", "planar", torch.float32, None),    # 289 tiles: more than the reduce's 256 threads
]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "b%dv%dc%d_%s_%s_%s_%s" % (r[0], r[1], r[2], r[6], r[7], str(r[8])[6:], str(r[9])[6:]))
def test_pose_gradients_match_the_oracle(row, gpu):
    B, V, C, H, W, vol, method, layout, fdt, odt = row
    rng = np.random.default_rng(V * 100 + C)
    P = _ring(B, V, H, W, seed=V + C)
    rot, center = _pose(B, seed=V * 7 + C)
    feats = rng.standard_normal((B, V, C, H, W)).astype(np.float32)
    go = rng.standard_normal((B, C) + vol).astype(np.float32)
    f = _features(feats, gpu, fdt, layout == "channels_last")
    (gp, gr, gc), go_seen = _cuboid_geometry(f, P, rot, center, go, vol, method, odt, layout)
    op, orot, ocen = pose_grad(f.float().cpu().numpy(), P, rot, center, POSITION, SIDES, vol, go_seen, method)
    tag = "pose grad %s" % (row,)
    _check(tag + " proj", gp, op)
    _check(tag + " rot", gr, orot)
    _check(tag + " center", gc, ocen)


def _torch_route(f, P, rot, center, go, vol, method):
    """coords = R (g - c) + c built in torch from rot / center that require grad, with the values of mvhmr_build_coord_volumes (the
    kernels' bits, so both routes sample the same cells), then the tensor route unprojection()"""
    gpu = f.device
    r = torch.from_numpy(rot).to(gpu).requires_grad_(True)
    c = torch.from_numpy(center).to(gpu).requires_grad_(True)
    p = torch.from_numpy(P).to(gpu).requires_grad_(True)
    _, X32 = cuboid_points(rot, center, POSITION, SIDES, vol)
    B = rot.shape[0]
    grid = cuboid_points(np.tile(np.eye(3, dtype=np.float32), (B, 1, 1)), np.zeros((B, 3), np.float32), POSITION, SIDES, vol)[0].to(gpu)
    Xt = torch.einsum("brk,bxyzk->bxyzr", r, grid - c[:, None, None, None, :]) + c[:, None, None, None, :]
    X = X32.to(gpu) + (Xt - Xt.detach())                    # the kernels' values, torch's derivatives
    out = aggregation.unprojection(f, p, X, aggregation_method=method)
    out.backward(torch.from_numpy(go).to(gpu))
    return p.grad, r.grad, c.grad


def test_cuboid_route_agrees_with_the_tensor_route(gpu):
    B, V, C, H, W, vol = 2, 4, 8, 16, 20, (9, 8, 7)
    rng = np.random.default_rng(5)
    P = _ring(B, V, H, W, seed=5)
    rot, center = _pose(B, seed=5)
    feats = rng.standard_normal((B, V, C, H, W)).astype(np.float32)
    go = rng.standard_normal((B, C) + vol).astype(np.float32)
    f = torch.from_numpy(feats).to(gpu)
    tp, tr, tc = _torch_route(f, P, rot, center, go, vol, "softmax")
    (gp, gr, gc), _ = _cuboid_geometry(f, P, rot, center, go, vol, "softmax")
    for name, a, b in (("rot", gr, tr), ("center", gc, tc)):
        record_err("cuboid vs tensor route: %s" % name, float((a - b).abs().max()), 1e-5 * float(b.abs().max()))
    # grad_proj: bit-equal to the tensor route's on the same coordinates (for this non-cubic volume, the oracle's restatement of the
    # recipe; for a cube, the coordinates mvhmr_build_coord_volumes builds)
    L = _capi.lib()
    coords = cuboid_points(rot, center, POSITION, SIDES, vol)[1].to(gpu)
    gp_t, _ = torch.ops.mvhmr.unprojection_backward_geometry(torch.from_numpy(go).to(gpu), f, torch.from_numpy(P).to(gpu), coords,
                                                             _capi.AGG["softmax"], _capi.F32, 0, True, False)
    assert torch.equal(gp, gp_t)
    S = 8
    go8 = rng.standard_normal((B, C, S, S, S)).astype(np.float32)
    (gp8, _, _), _ = _cuboid_geometry(f, P, rot, center, go8, (S, S, S), "softmax", want=(True, False, False))
    rot_d, cen_d = torch.from_numpy(rot).to(gpu), torch.from_numpy(center).to(gpu)
    built = torch.empty(B, S, S, S, 3, dtype=torch.float32, device=gpu)
    _capi.check(L.mvhmr_build_coord_volumes(aggregation._ptr(built), aggregation._ptr(rot_d), aggregation._ptr(cen_d), B, S,
                                            (ctypes.c_double * 3)(*POSITION), (ctypes.c_double * 3)(*SIDES), aggregation._stream(gpu)))
    gp8_t, _ = torch.ops.mvhmr.unprojection_backward_geometry(torch.from_numpy(go8).to(gpu), f, torch.from_numpy(P).to(gpu), built,
                                                              _capi.AGG["softmax"], _capi.F32, 0, True, False)
    assert torch.equal(gp8, gp8_t)


def test_identity_rotation_gives_an_exactly_zero_center_gradient(gpu):
    B, V, C, H, W, vol = 2, 3, 8, 12, 16, (6, 5, 7)
    rng = np.random.default_rng(8)
    rot, center = _pose(B, seed=8, identity=True)
    (gp, gr, gc), _ = _cuboid_geometry(torch.from_numpy(rng.standard_normal((B, V, C, H, W)).astype(np.float32)).to(gpu), _ring(B, V, H, W, 8),
                                       rot, center, rng.standard_normal((B, C) + vol).astype(np.float32), vol, "softmax")
    assert float(gr.abs().max()) > 0
    assert bool((gc == 0).all())


def test_pose_gradients_are_bitwise_reproducible_and_leave_the_feature_gradient_alone(gpu):
    B, V, C, H, W, vol = 2, 4, 12, 16, 20, (10, 9, 11)
    rng = np.random.default_rng(9)
    P = _ring(B, V, H, W, seed=9)
    rot, center = _pose(B, seed=9)
    feats = rng.standard_normal((B, V, C, H, W)).astype(np.float32)
    go = torch.from_numpy(rng.standard_normal((B, C) + vol).astype(np.float32)).to(gpu)

    def run(pose):
        f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
        p, r, c = (torch.from_numpy(a).to(gpu).requires_grad_(pose) for a in (P, rot, center))
        aggregation.unprojection_cuboid(f, p, r, c, POSITION, SIDES, vol).backward(go)
        return f.grad, p.grad, r.grad, c.grad

    a, b, base = run(True), run(True), run(False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert base[1] is None and base[2] is None and base[3] is None
    assert torch.equal(a[0], base[0])


def test_fused_aggregate_pose_gradients_equal_the_plain_route(gpu):
    B, V, Cin, Cout, H, W, S = 2, 3, 16, 128, 8, 32, 8
    rng = np.random.default_rng(10)
    P = _ring(B, V, H, W, seed=10)
    rot, center = _pose(B, seed=10)
    x = torch.from_numpy(rng.standard_normal((B, V, Cin, H, W)).astype(np.float32)).to(gpu)
    w = torch.from_numpy((rng.standard_normal((Cout, Cin, 1, 1)) * 0.3).astype(np.float32)).to(gpu)
    bias = torch.from_numpy((rng.standard_normal(Cout) * 0.1).astype(np.float32)).to(gpu)
    go = torch.from_numpy(rng.standard_normal((B, Cout, S, S, S)).astype(np.float32)).to(gpu)

    def leaves():
        return [torch.from_numpy(a).to(gpu).requires_grad_(True) for a in (P, rot, center)]

    p, r, c = leaves()
    out = aggregation._FusedAggregate.apply(x, w, bias, p, r, c, POSITION, SIDES, (S, S, S), _capi.AGG["softmax"], torch.float32)
    out.backward(go)
    p2, r2, c2 = leaves()
    y = torch.nn.functional.conv2d(x.view(B * V, Cin, H, W), w, bias).view(B, V, Cout, H, W)
    aggregation.unprojection_cuboid(y, p2, r2, c2, POSITION, SIDES, (S, S, S)).backward(go)
    for name, a, b in (("proj", p.grad, p2.grad), ("rot", r.grad, r2.grad), ("center", c.grad, c2.grad)):
        record_err("fused vs plain route: %s" % name, float((a - b).abs().max()), 1e-5 * float(b.abs().max()))


@pytest.mark.parametrize("V", (2, 3, 4, 8, 16))
@pytest.mark.parametrize("mode", ("shared", "per_sample"))
def test_dlt_backward_matches_the_oracle(V, mode, gpu):
    import bench
    B = 6
    rng = np.random.default_rng(V)
    P = bench.ring_projections(B, V, (96, 96), seed=V)
    X = rng.uniform(-600, 600, (B, 3))
    r = np.einsum("bvij,bj->bvi", P.astype(np.float64), np.concatenate([X, np.ones((B, 1))], 1))
    uv = (r[..., :2] / r[..., 2:3] + rng.normal(0, 1.0, (B, V, 2))).astype(np.float32)
    conf = rng.uniform(0.3, 1.0, (B, V)).astype(np.float32)
    if mode == "shared":
        uv, conf = uv[0], conf[0]
    go = rng.standard_normal((B, 3)).astype(np.float32)
    for cf in (None, conf):
        Pt = torch.from_numpy(P).to(gpu).requires_grad_(True)
        ut = torch.from_numpy(uv).to(gpu).requires_grad_(True)
        ct = None if cf is None else torch.from_numpy(cf).to(gpu).requires_grad_(True)
        out = multiview.triangulate_points_from_multiple_views_linear_batch(Pt, ut, ct)
        out.backward(torch.from_numpy(go).to(gpu))
        oP, oU, oC = dlt_grad(P, uv, cf, go)
        tag = "DLT backward V=%d %s %s" % (V, mode, "weighted" if cf is not None else "unweighted")
        _check(tag + " proj", Pt.grad, oP, 1e-5)
        _check(tag + " points", ut.grad, oU, 1e-5)
        if cf is not None:
            _check(tag + " conf", ct.grad, oC, 1e-5)


def test_dlt_backward_single_view_is_nan(gpu):
    P = torch.from_numpy(_ring(3, 1, 16, 16, seed=1)).to(gpu)
    uv = torch.full((1, 2), 8.0, device=gpu)
    gp, gu, gc = torch.ops.mvhmr.triangulate_dlt_backward(torch.ones(3, 3, device=gpu), P, uv, None)
    assert bool(torch.isnan(gp).all() and torch.isnan(gu).all() and torch.isnan(gc).all())


def _jacobi_dlt(P, uv):
    """k_triangulate_dlt restated in float64 Python, operation for operation (IEEE +, *, /, sqrt): the forward's bits"""
    import math
    V = P.shape[0]
    M = [[0.0] * 4 for _ in range(4)]
    E = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for v in range(V):
        for r in range(2):
            a = [1.0 * (float(uv[v, r]) * float(P[v, 2, k]) - float(P[v, r, k])) for k in range(4)]
            for i in range(4):
                for j in range(4):
                    M[i][j] += a[i] * a[j]
    for _ in range(12):
        off = 0.0
        for i in range(4):
            for j in range(i + 1, 4):
                off += M[i][j] * M[i][j]
        if off == 0.0:
            break
        for p in range(3):
            for q in range(p + 1, 4):
                if M[p][q] == 0.0:
                    continue
                th = (M[q][q] - M[p][p]) / (2.0 * M[p][q])
                t = (1.0 if th >= 0 else -1.0) / (abs(th) + math.sqrt(th * th + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                sn = t * c
                for k in range(4):
                    mkp, mkq = M[k][p], M[k][q]
                    M[k][p] = c * mkp - sn * mkq; M[k][q] = sn * mkp + c * mkq
                for k in range(4):
                    mpk, mqk = M[p][k], M[q][k]
                    M[p][k] = c * mpk - sn * mqk; M[q][k] = sn * mpk + c * mqk
                    ekp, ekq = E[k][p], E[k][q]
                    E[k][p] = c * ekp - sn * ekq; E[k][q] = sn * ekp + c * ekq
    m = 0
    for k in range(1, 4):
        m = k if M[k][k] < M[m][m] else m
    h = [E[i][m] for i in range(4)]
    return np.array([h[0] / h[3], h[1] / h[3], h[2] / h[3]]).astype(np.float32)


def test_dlt_forward_is_bitwise_unchanged(gpu):
    import bench
    P = bench.ring_projections(5, 4, (96, 96), seed=3)
    uv = np.array([[48.0, 48.0]] * 4, np.float32)
    got = multiview.triangulate_points_from_multiple_views_linear_batch(torch.from_numpy(P).to(gpu), torch.from_numpy(uv).to(gpu)).cpu().numpy()
    want = np.stack([_jacobi_dlt(P[b], uv) for b in range(5)])
    assert np.array_equal(got, want), np.abs(got - want).max()


def _rebuild(d, gpu):
    B, V, C_in, C_out, S = (int(x) for x in d["meta"][:5])
    cams = [[multiview.Camera(d["R"][v, b], d["t"][v, b], d["K"][v, b]) for b in range(B)] for v in range(V)]
    batch = dict(images=np.zeros((B, V, int(d["image_hw"][0]), int(d["image_hw"][1]), 3), dtype=np.uint8), cameras=cams,
                 keypoints_3d=[k for k in d["keypoints"]])
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=C_in, output_channels=C_out, cuboid_side=2500.0,
                                      aggregation_method=str(d["method"]), use_triangulation=True, kind=str(d["kind"]), device=gpu)
    gen.load_state_dict({"process_feature.0.weight": torch.from_numpy(d["weight"]), "process_feature.0.bias": torch.from_numpy(d["bias"])})
    gen.train(bool(int(d["meta"][5])))
    return gen, batch, int(d["meta"][7])


@pytest.mark.parametrize("fused", (True, False))
@pytest.mark.parametrize("case", [c for c in golden_cases("posegrad") if not c.startswith("dlt")])
def test_volume_generator_gradients_match_the_reference(case, fused, gpu):
    """proj_org.grad through the triangulated pivot against the reference.  The bound is twice the distance between the reference and
    the float64 oracle: the reference's own fp32 error, mostly that of its fp32 pivot, which moves voxels across cells.  With R = I
    (eval) both are exactly zero.  The feature and conv gradients depend on the cells too: they are compared in a second run whose pivot
    is pinned to the reference's own (stored in the golden), at 1e-4 of their scale."""
    d = load_golden("posegrad", case)
    gen, batch, seed = _rebuild(d, gpu)
    gen.fused_conv = fused

    def run():
        np.random.seed(seed)
        f = torch.from_numpy(d["features_in"]).to(gpu).requires_grad_(True)
        P = torch.from_numpy(d["proj_org"]).to(gpu).requires_grad_(True)
        gen.zero_grad()
        (gen(f, P, batch) * torch.from_numpy(d["grad_out"]).to(gpu)).sum().backward()
        return f.grad, P.grad

    _, gP = run()
    assert gP is not None
    tag = "volgen pose grad %s fused=%d" % (case, fused)
    ref, orc = d["gproj_org"], d["oracle_gproj_org"]
    got = gP.cpu().double().numpy()
    if np.abs(orc).max() == 0:
        assert (got == 0).all()
    else:
        record_err(tag + " proj_org (vs reference)", float(np.abs(got - ref).max()), 2.0 * float(np.abs(ref - orc).max()))
        record_err(tag + " proj_org (vs float64 oracle)", float(np.abs(got - orc).max()), 2.0 * float(np.abs(ref - orc).max()))
    real = gen.volume_pose
    gen.volume_pose = lambda b, p, shape: (real(b, p, shape)[0], torch.from_numpy(d["ref_center"]).to(gpu))
    gf, _ = run()
    for name, mine, want in (("features", gf, d["gfeatures"]), ("weight", gen.process_feature[0].weight.grad, d["gweight"]),
                             ("bias", gen.process_feature[0].bias.grad, d["gbias"])):
        record_err(tag + " " + name + " (reference's pivot)", float(np.abs(mine.cpu().double().numpy() - want).max()),
                   1e-4 * float(np.abs(want).max()))


def test_north_star_shape_matches_the_torch_coords_route(gpu):
    """B 32, 64^3, C 256, V 4, 96 x 96, softmax: the cuboid op's rot / center gradients against the chain rule applied in float64 to the
    tensor route's grad_coords on the same coordinates, and its grad_proj bit-equal to the tensor route's"""
    import bench
    B, V, C, H, W, S = 32, 4, 256, 96, 96, 64
    gen = torch.Generator(device=gpu).manual_seed(0)
    f = torch.randn(B, V, C, H, W, device=gpu, generator=gen)
    go = torch.randn(B, C, S, S, S, device=gpu, generator=gen)
    P = torch.from_numpy(bench.ring_projections(B, V, (H, W), seed=1)).to(gpu)
    rot_np, cen_np = _pose(B, seed=11)
    cen_np = (cen_np * 1000.0).astype(np.float32)
    rot, cen = torch.from_numpy(rot_np).to(gpu), torch.from_numpy(cen_np).to(gpu)
    pos, sides = (-1250.0,) * 3, (2500.0,) * 3
    L = _capi.lib()
    coords = torch.empty(B, S, S, S, 3, dtype=torch.float32, device=gpu)
    _capi.check(L.mvhmr_build_coord_volumes(aggregation._ptr(coords), aggregation._ptr(rot), aggregation._ptr(cen), B, S,
                                            (ctypes.c_double * 3)(*pos), (ctypes.c_double * 3)(*sides), aggregation._stream(gpu)))
    m = _capi.AGG["softmax"]
    gp_t, gX = torch.ops.mvhmr.unprojection_backward_geometry(go, f, P, coords, m, _capi.F32, 0, True, True)
    gp, gr, gc = torch.ops.mvhmr.unprojection_cuboid_backward_geometry(go, f, P, rot, cen, list(pos), list(sides), [S, S, S], m, _capi.F32, 0)
    assert torch.equal(gp, gp_t)
    step = torch.tensor(np.float32(2500.0 / (S - 1)), device=gpu)
    ax = torch.tensor(np.float32(-1250.0), device=gpu) + step * torch.arange(S, device=gpu, dtype=torch.float32)
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(1, -1, 3)
    d = (grid - cen[:, None, :]).double()                                            # fp32 d, then float64
    gX = gX.reshape(B, -1, 3).double()
    want_r = torch.einsum("bnr,bnk->brk", gX, d)
    s_g = gX.sum(1)
    want_c = s_g - torch.einsum("brk,br->bk", rot.double(), s_g)
    record_err("north star: rot vs torch-coords route", float((gr.double() - want_r).abs().max()), 1e-5 * float(want_r.abs().max()))
    record_err("north star: center vs torch-coords route", float((gc.double() - want_c).abs().max()), 1e-5 * float(want_c.abs().max()))
