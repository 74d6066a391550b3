"""Gradients of unprojection w.r.t. proj_matricies and coord_volumes on the MI355X (k_bwd_geom + k_geom_reduce): autograd through
aggregation.unprojection against the float64 oracle (tests/geomgrad_oracle.py) and the reference's own goldens, bitwise
reproducibility, and the feature gradient unchanged when the geometry asks for gradients too.  Every bound is 1e-4 of the largest
oracle value of that tensor, asserted through conftest.record_err, which also keeps the observed errors."""
import numpy as np
import pytest
import torch

from conftest import golden_cases, load_golden, record_err
from geomgrad_oracle import geometry_grad
from multiviewhmr_amd import aggregation

pytestmark = pytest.mark.gpu
MODES = ("softmax", "sum", "mean", "max")
REL = 1e-4


def _ring(B, V, H, W, seed):
    """cameras on a ring around a unit-scale volume; view 0 close enough that some voxels fall behind it or outside its frame"""
    rng = np.random.default_rng(seed)
    P = np.zeros((B, V, 3, 4), np.float32)
    for b in range(B):
        for v in range(V):
            az = 2 * np.pi * v / V + 0.4 * b + 0.1
            eye = np.array([np.cos(az), np.sin(az), 0.3]) * (1.6 if v == 0 else rng.uniform(3.5, 4.5))
            fwd = -eye / np.linalg.norm(eye)
            right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
            R = np.stack([right, np.cross(fwd, right), fwd])
            K = np.array([[1.3 * H, 0, H / 2 + rng.uniform(-1, 1)], [0, 1.3 * W, W / 2 + rng.uniform(-1, 1)], [0, 0, 1]])
            P[b, v] = K @ np.hstack([R, (-R @ eye)[:, None]])
    return P


def _problem(B, V, C, H, W, vol, seed):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.linspace(-1.2, 1.2, n) for n in vol], indexing="ij"), -1)
    coords = (g[None] + rng.uniform(-0.05, 0.05, (B,) + tuple(vol) + (3,))).astype(np.float32)
    feats = rng.standard_normal((B, V, C, H, W)).astype(np.float32)
    go = rng.standard_normal((B, C) + tuple(vol)).astype(np.float32)
    return feats, _ring(B, V, H, W, seed), coords, go


def _features(feats, gpu, fdt, channels_last):
    f = torch.from_numpy(feats).to(gpu, fdt)
    if channels_last:
        f = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)          # physically (B,V,H,W,C)
    return f


def _run(feats, P, coords, go, gpu, method, fdt=torch.float32, odt=None, channels_last=False, want_features=False):
    f = _features(feats, gpu, fdt, channels_last).requires_grad_(want_features)
    p = torch.from_numpy(P).to(gpu).requires_grad_(True)
    c = torch.from_numpy(coords).to(gpu).requires_grad_(True)
    out = aggregation.unprojection(f, p, c, aggregation_method=method, out_dtype=odt)
    g = torch.from_numpy(go).to(gpu, out.dtype)
    out.backward(g)
    # what the kernels saw: features and grad_out in their storage types
    return p.grad, c.grad, (f.grad if want_features else None), f.detach().float().cpu().numpy(), g.float().cpu().numpy()


def _check(name, got, ref):
    scale = float(np.abs(ref).max())
    assert scale > 0, name
    assert torch.isfinite(got).all(), name
    record_err(name, float(np.abs(got.double().cpu().numpy() - ref).max()), REL * scale)


# (V, C, layout, feature dtype, volume dtype, volume): every method for each row; the rows cover 1 ... 16 views, C % 4 != 0, planar and
# channels-last features, fp16 features (fp16 and fp32 volumes), a bf16 volume, non-square maps and odd extents; the last row has more
# blocks per sample than k_geom_reduce has threads
SWEEP = [
    (1, 4, "planar", "f32", "f32", (5, 6, 7)),
    (2, 7, "planar", "f16", "f16", (7, 5, 3)),
    (4, 256, "channels_last", "f32", "f32", (3, 5, 4)),
    (4, 7, "planar", "f32", "bf16", (6, 5, 7)),
    (8, 4, "channels_last", "f16", "f16", (5, 5, 5)),
    (8, 256, "planar", "f16", "f32", (3, 3, 5)),
    (12, 7, "planar", "f32", "f32", (5, 7, 3)),
    (12, 4, "channels_last", "f32", "bf16", (4, 5, 6)),
    (16, 4, "planar", "f32", "f32", (5, 3, 7)),
    (16, 256, "channels_last", "f16", "f16", (3, 3, 3)),
    (3, 4, "planar", "f32", "f32", (17, 33, 19)),
]
_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.mark.parametrize("row", range(len(SWEEP)))
def test_geometry_gradients_match_the_oracle(row, gpu):
    V, C, layout, fdt, odt, vol = SWEEP[row]
    feats, P, coords, go = _problem(2, V, C, 11, 14, vol, seed=100 + row)
    for method in MODES:
        gp, gc, _, f_seen, g_seen = _run(feats, P, coords, go, gpu, method, _DT[fdt], _DT[odt], layout == "channels_last")
        rp, rc = geometry_grad(f_seen, P, coords, g_seen, method)
        tag = "geomgrad V%d C%d %s %s/%s %s %s" % (V, C, layout, fdt, odt, "x".join(map(str, vol)), method)
        _check(tag + " proj", gp, rp)
        _check(tag + " coords", gc, rc)


@pytest.mark.parametrize("case", golden_cases("geomgrad"))
def test_geometry_gradients_match_reference_goldens(case, gpu):
    d = load_golden("geomgrad", case)
    for method in MODES:
        gp, gc, _, _, _ = _run(d["features"], d["proj"], d["coords"], d["grad_out"], gpu, method)
        _check("geomgrad golden %s %s proj" % (case, method), gp, d["gproj_" + method])
        _check("geomgrad golden %s %s coords" % (case, method), gc, d["gcoords_" + method])


def test_geometry_gradients_are_bitwise_reproducible(gpu):
    feats, P, coords, go = _problem(2, 4, 64, 24, 20, (16, 12, 20), seed=7)
    a = _run(feats, P, coords, go, gpu, "softmax")
    b = _run(feats, P, coords, go, gpu, "softmax")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_feature_gradient_unchanged_when_geometry_requires_grad(gpu):
    feats, P, coords, go = _problem(2, 4, 16, 24, 20, (8, 8, 8), seed=8)
    f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
    out = aggregation.unprojection(f, torch.from_numpy(P).to(gpu), torch.from_numpy(coords).to(gpu), aggregation_method="softmax")
    out.backward(torch.from_numpy(go).to(gpu))
    _, _, g_all, _, _ = _run(feats, P, coords, go, gpu, "softmax", want_features=True)
    ref = f.grad.double().cpu().numpy()
    m = float(np.abs(ref).max())
    record_err("geomgrad feature grad unchanged", float(np.abs(g_all.double().cpu().numpy() - ref).max()), 1e-4 if m <= 16.0 else max(1e-4, 8e-6 * m))


def test_geometry_grad_dtypes_follow_the_caller(gpu):
    """float64 proj / coords get float64 gradients (autograd casts back through .to(float32))"""
    feats, P, coords, go = _problem(1, 2, 4, 9, 12, (3, 4, 5), seed=9)
    p = torch.from_numpy(P).to(gpu, torch.float64).requires_grad_(True)
    c = torch.from_numpy(coords).to(gpu, torch.float64).requires_grad_(True)
    out = aggregation.unprojection(torch.from_numpy(feats).to(gpu), p, c, aggregation_method="mean")
    assert out.grad_fn is not None
    out.backward(torch.from_numpy(go).to(gpu))
    assert p.grad.dtype == torch.float64 and c.grad.dtype == torch.float64 and c.grad.shape == c.shape


def test_full_size_softmax_against_the_oracle_on_a_voxel_subset(gpu):
    """64^3 voxels, 256 channels, 4 views, batch 32, softmax, the benchmark's cameras (grad_out holds more than 2^31 elements):
    grad_coords of a seeded voxel subset against the oracle -- each voxel's gradient is its own.  grad_proj sums every voxel, so here
    it is only checked to be finite; the sweep above pins its values."""
    from bench import cuboid_volume, ring_projections
    B, S, C, V, HW = 32, 64, 256, 4, 96
    torch.manual_seed(0)
    f = torch.randn(B, V, C, HW, HW, device=gpu)
    P = ring_projections(B, V, (HW, HW), seed=0)
    coords = torch.from_numpy(cuboid_volume(1, S)).to(gpu).expand(B, S, S, S, 3).contiguous().requires_grad_(True)
    p = torch.from_numpy(P).to(gpu).requires_grad_(True)
    out = aggregation.unprojection(f, p, coords, aggregation_method="softmax")
    g = torch.randn_like(out)
    out.backward(g)
    gc = coords.grad
    assert torch.isfinite(gc).all() and torch.isfinite(p.grad).all()
    rng = np.random.default_rng(0)
    N = S ** 3
    idx = torch.from_numpy(rng.choice(B * N, size=512, replace=False))
    bs, ns = (idx // N), (idx % N)
    for b in sorted(set(bs.tolist()))[:8]:
        sel = ns[bs == b]
        pts = coords.detach()[b].reshape(N, 3)[sel.to(gpu)].cpu()
        gsel = g[b].reshape(C, N)[:, sel.to(gpu)].cpu()
        _, rc = geometry_grad(f[b:b + 1].cpu(), P[b:b + 1], pts.reshape(1, -1, 1, 1, 3), gsel.reshape(1, C, -1, 1, 1), "softmax")
        got = gc[b].reshape(N, 3)[sel.to(gpu)]
        _check("geomgrad full size sample %d coords" % b, got, rc.reshape(-1, 3))
