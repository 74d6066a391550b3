"""Deterministic mode of the feature-gradient backward on the GPU (torch.use_deterministic_algorithms(True) at backward time): the
gradient against the float64 oracle at the existing bounds and bitwise equal across runs on every route, bit-equal to the default on
the plane route, equivariant under a permutation of the batch, non-finite wherever the default is, and a fused VolumeGenerator train
step whose every gradient repeats bit for bit."""
import numpy as np
import pytest
import torch

from conftest import golden_cases, load_golden, record_err
from multiviewhmr_amd import _capi, aggregation
from oracle import cport
from test_unproject_gpu import _bound, _err, _ring_problem

pytestmark = pytest.mark.gpu
MODES = ("softmax", "sum", "mean", "max")


@pytest.fixture
def deterministic():
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(was)


def _grad(f, p, c, go, mode, variant="auto", out_dtype=None, det=True):
    f = f.detach().requires_grad_(True)
    out = aggregation.unprojection(f, p, c, aggregation_method=mode, variant=variant, out_dtype=out_dtype)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(det)
    try:
        out.backward(go)
    finally:
        torch.use_deterministic_algorithms(was)
    return f.grad


SHAPES = [
    dict(B=2, V=1, C=16, H=40, W=40, vol=(8, 8, 16)),          # 1 view
    dict(B=2, V=3, C=32, H=48, W=48, vol=(8, 16, 16)),         # 3 views (brick shapes by default)
    dict(B=2, V=4, C=64, H=48, W=48, vol=(16, 16, 32)),        # 4 views
    dict(B=1, V=5, C=20, H=24, W=40, vol=(9, 7, 13)),          # 5 views, run-time view count
    dict(B=1, V=8, C=300, H=24, W=24, vol=(4, 8, 16)),         # 8 views, two channel groups
    dict(B=1, V=3, C=6, H=16, W=16, vol=(5, 5, 5)),            # C % 4 != 0 (the default's tail)
    dict(B=1, V=4, C=8, H=256, W=256, vol=(16, 16, 32), close=True),   # windows that do not fit (the default's slow path / gate)
    dict(B=1, V=12, C=8, H=16, W=16, vol=(4, 4, 8)),           # 9 ... 16 views
    dict(B=1, V=16, C=12, H=12, W=20, vol=(4, 6, 8)),
    dict(B=1, V=4, C=16, H=200, W=200, vol=(8, 8, 16)),        # maps too large for the plane kernels
    dict(B=2, V=4, C=16, H=24, W=24, vol=(8, 8, 8)),           # plane shapes
    dict(B=1, V=8, C=8, H=32, W=32, vol=(8, 8, 8)),
]


def _problem(shape, seed):
    kw = {k: v for k, v in shape.items() if k != "close"}
    feats, proj, coords = _ring_problem(seed=seed, **kw)
    if shape.get("close"):
        coords = coords * np.float32(3.0)                          # a wide volume: windows overflow LDS
    return feats, proj, coords


@pytest.mark.parametrize("variant", ["auto", "gather"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "V%d_C%d_%dx%d_vol%s" % (s["V"], s["C"], s["H"], s["W"], "x".join(map(str, s["vol"]))))
@pytest.mark.parametrize("mode", MODES)
def test_deterministic_backward_vs_oracle_and_repeats(shape, mode, variant, gpu):
    feats, proj, coords = _problem(shape, seed=MODES.index(mode) * 100 + shape["C"])
    f, p, c = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    go_np = np.random.default_rng(5).standard_normal((shape["B"], shape["C"]) + shape["vol"], dtype=np.float32)
    go = torch.from_numpy(go_np).to(gpu)
    runs = [_grad(f, p, c, go, mode, variant) for _ in range(3)]
    gref = cport.backward(go_np, feats, proj, coords, mode)
    record_err("det %s %s V%d C%d %dx%d vol%s" % (variant, mode, shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"]),
               _err(runs[0].cpu().numpy(), gref), _bound(gref))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("variant", ["auto", "gather"])                   # 3 views: the plane kernels refuse them -> brick / gather fixed point
@pytest.mark.parametrize("storage", ["f32_f32", "f16_f16", "f16_f32", "f32_bf16", "channels_last", "channels_last_f16"])
@pytest.mark.parametrize("mode", MODES)
def test_deterministic_backward_storage_and_layouts(storage, mode, variant, gpu):
    B, V, C, H, W, vol = 2, 3, 32, 40, 40, (8, 16, 16)
    feats, proj, coords = _ring_problem(B, V, C, H, W, vol, seed=7 + MODES.index(mode))
    f = torch.from_numpy(feats).to(gpu)
    p, c = torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    go32 = np.random.default_rng(9).standard_normal((B, C) + vol, dtype=np.float32)
    out_dtype, ftol = None, 0.0
    if storage.endswith("f16") and not storage.startswith("channels"):
        f, out_dtype = f.half(), torch.float16
    elif storage == "f16_f32":
        f, out_dtype = f.half(), torch.float32
    elif storage == "f32_bf16":
        out_dtype = torch.bfloat16
    elif storage.startswith("channels_last"):
        f = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)      # physically (B, V, H, W, C)
        if storage.endswith("f16"):
            f, out_dtype = f.half(), torch.float16
            f = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    go = torch.from_numpy(go32).to(gpu, dtype=out_dtype or torch.float32)
    runs = [_grad(f, p, c, go, mode, variant, out_dtype=out_dtype) for _ in range(3)]
    assert runs[0].dtype == f.dtype
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    gref = cport.backward(go.float().cpu().numpy(), f.float().cpu().numpy(), proj, coords, mode)
    bound = _bound(gref)
    if f.dtype == torch.float16:
        bound += float(np.abs(gref).max()) * 2.0 ** -10                   # one fp16 ulp of the largest gradient (storage)
    record_err("det storage %s %s %s" % (storage, mode, variant), _err(runs[0].float().cpu().numpy(), gref), bound)
    # the default route on the same inputs, at the same bound
    dflt = _grad(f, p, c, go, mode, variant, out_dtype=out_dtype, det=False)
    record_err("det vs default storage %s %s %s" % (storage, mode, variant), _err(runs[0].float().cpu().numpy(), dflt.float().cpu().numpy()), bound)


@pytest.mark.parametrize("shape", [dict(B=2, V=4, C=16, H=24, W=24, vol=(8, 8, 8)), dict(B=1, V=8, C=8, H=32, W=32, vol=(8, 8, 8)),
                                   dict(B=3, V=2, C=16, H=32, W=32, vol=(8, 8, 8))])
@pytest.mark.parametrize("mode", MODES)
def test_plane_route_is_unchanged_by_the_flag(shape, mode, gpu):
    feats, proj, coords = _ring_problem(seed=3, **shape)
    f, p, c = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    go = torch.randn((shape["B"], shape["C"]) + shape["vol"], device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
    on = _grad(f, p, c, go, mode, "gather", det=True)
    off = _grad(f, p, c, go, mode, "gather", det=False)
    assert torch.equal(on, off)


@pytest.mark.parametrize("variant,shape", [("brick", dict(V=4, C=32, H=120, W=120, vol=(8, 16, 32))),       # k_bwd_brick (fixed-point flush)
                                           ("brick", dict(V=3, C=6, H=40, W=40, vol=(8, 8, 16))),          # + k_bwd_tail (C % 4 != 0)
                                           ("gather", dict(V=3, C=24, H=40, W=40, vol=(8, 8, 16))),        # k_bwd_gather_det
                                           ("gather", dict(V=4, C=16, H=24, W=24, vol=(8, 8, 8)))])        # plane kernels
@pytest.mark.parametrize("mode", ["softmax", "max"])
def test_batch_permutation_permutes_the_gradient_bitwise(variant, shape, mode, gpu):
    feats, proj, coords = _ring_problem(B=6, seed=21, **shape)
    for b in range(6):                                                    # distinct samples, distinct scales
        feats[b] *= np.float32(1.0 + 3.0 * b)
    f, p, c = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    go = torch.randn((6, shape["C"]) + shape["vol"], device=gpu, generator=torch.Generator(device=gpu).manual_seed(2))
    go = go * torch.arange(1, 7, device=gpu, dtype=torch.float32).view(6, 1, 1, 1, 1) ** 2
    g = _grad(f, p, c, go, mode, variant)
    perm = torch.tensor([4, 0, 5, 2, 1, 3], device=gpu)
    gp = _grad(f[perm].contiguous(), p[perm].contiguous(), c[perm].contiguous(), go[perm].contiguous(), mode, variant)
    assert torch.equal(gp, g[perm])


@pytest.mark.parametrize("variant", ["auto", "gather"])
@pytest.mark.parametrize("mode", MODES)
def test_non_finite_inputs_give_non_finite_gradients_where_the_default_does(mode, variant, gpu):
    B, V, C, H, W, vol = 2, 3, 8, 32, 32, (8, 8, 16)
    feats, proj, coords = _ring_problem(B, V, C, H, W, vol, seed=31)
    f, p, c = torch.from_numpy(feats).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(coords).to(gpu)
    f[0, 1, 2, 16, 16] = float("inf")
    go = torch.randn((B, C) + vol, device=gpu, generator=torch.Generator(device=gpu).manual_seed(3))
    go[1, 5, 4, 4, 8] = float("nan")
    det = _grad(f, p, c, go, mode, variant)
    dflt = _grad(f, p, c, go, mode, variant, det=False)
    bad_d, bad = ~torch.isfinite(dflt), ~torch.isfinite(det)
    assert bad_d.any()
    assert bool((bad | ~bad_d).all()), "a non-finite default element is finite in deterministic mode"
    # channels the non-finite inputs cannot reach agree with the default
    ok = ~(bad | bad_d)
    assert float((det[ok] - dflt[ok]).abs().max()) <= _bound(dflt[ok].cpu().numpy())


def _fused_generator(gpu):
    from test_pose_grad_gpu import _rebuild
    d = load_golden("posegrad", [c for c in golden_cases("posegrad") if "fusedshape" in c][0])
    gen0, batch, seed = _rebuild(d, gpu)
    torch.manual_seed(0)
    S = gen0.volume_size if hasattr(gen0, "volume_size") else int(d["meta"][4])
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=128, output_channels=128, cuboid_side=2500.0,
                                      aggregation_method=str(d["method"]), use_triangulation=True, kind=str(d["kind"]), device=gpu)
    gen.train(True)
    gen.fused_conv = True
    return gen, batch, seed, d


def test_fused_volume_generator_train_step_repeats_bitwise(gpu):
    gen, batch, seed, d = _fused_generator(gpu)
    B, V, _, H, W = d["features_in"].shape
    g = torch.Generator(device=gpu).manual_seed(4)
    feats = torch.randn(B, V, 128, H, W, device=gpu, generator=g)
    P0 = torch.from_numpy(d["proj_org"]).to(gpu)
    assert gen._fused_path_applies(feats, gen.volume_size if hasattr(gen, "volume_size") else int(d["meta"][4]))

    def step(det):
        np.random.seed(seed)
        f = feats.clone().requires_grad_(True)
        P = P0.clone().requires_grad_(True)
        gen.zero_grad()
        out = gen(f, P, batch)
        go = torch.randn(out.shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(5))
        was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(det)
        try:
            rec = _Rec()
            with rec:
                (out * go).sum().backward()
        finally:
            torch.use_deterministic_algorithms(was)
        conv = gen.process_feature[0]
        return [f.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone(), P.grad.clone()], rec

    # the extension's feature backward takes the mode as its `deterministic` argument (it selects mvhmr_unproject_backward_cuboid_deterministic)
    native_bwd = "mvhmr_native.unprojection_cuboid_backward.default"
    a, rec_on = step(True)
    assert (native_bwd, True) in rec_on.modes and (native_bwd, False) not in rec_on.modes, (rec_on.modes, rec_on.names)
    b, _ = step(True)
    for name, x, y in zip(("features", "weight", "bias", "proj_org"), a, b):
        assert torch.equal(x, y), name
    c, rec_off = step(False)
    assert not any("_deterministic" in n for n in rec_off.names), rec_off.names
    assert (native_bwd, False) in rec_off.modes and (native_bwd, True) not in rec_off.modes, (rec_off.modes, rec_off.names)
    for name, x, y in zip(("features", "weight", "bias", "proj_org"), a, c):
        ref = y.double().cpu().numpy()
        record_err("fused det step %s vs default" % name, _err(x.cpu().numpy(), ref), _bound(ref) if name != "proj_org"
                   else max(_bound(ref), 1e-4 * float(np.abs(ref).max())))


class _Rec(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []
        self.modes = []                 # (op, value of its `deterministic` argument) of every op that has one

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        schema = [a.name for a in func._schema.arguments]
        if "deterministic" in schema:   # (an argument at its default, False, may be left out of args)
            i = schema.index("deterministic")
            self.modes.append((str(func), bool(args[i] if i < len(args) else (kwargs or {}).get("deterministic", False))))
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("bias", [True, False])
def test_deterministic_wgrad_vs_float64_and_repeats(bias, gpu):
    import ctypes
    L = _capi.lib()
    BV, Cin, Cout, HW = 12, 256, 128, 48 * 64
    g = torch.Generator(device=gpu).manual_seed(6)
    gy = torch.randn(BV, Cout, HW, device=gpu, generator=g)
    x = torch.randn(BV, Cin, HW, device=gpu, generator=g)
    n = L.mvhmr_conv1x1_wgrad_deterministic_workspace_bytes(BV, Cin, Cout, HW)
    ws = torch.empty(n, dtype=torch.uint8, device=gpu)
    outs = []
    for _ in range(3):
        gw = torch.full((Cout, Cin), float("nan"), device=gpu)
        gb = torch.full((Cout,), float("nan"), device=gpu)
        _capi.check(L.mvhmr_conv1x1_wgrad_deterministic(aggregation._ptr(gy), aggregation._ptr(x), aggregation._ptr(gw),
                                                        aggregation._ptr(gb) if bias else ctypes.c_void_p(0), BV, Cin, Cout, HW,
                                                        aggregation._ptr(ws), n, aggregation._stream(gpu)))
        outs.append((gw, gb))
    torch.cuda.synchronize()
    want = torch.einsum("nop,nip->oi", gy.double(), x.double()).cpu().numpy()
    record_err("det wgrad weight", _err(outs[0][0].cpu().numpy(), want), 1e-5 * float(np.abs(want).max()) + 1e-4)
    if bias:
        wb = gy.double().sum(dim=(0, 2)).cpu().numpy()
        record_err("det wgrad bias", _err(outs[0][1].cpu().numpy(), wb), 1e-5 * float(np.abs(wb).max()) + 1e-4)
    else:
        assert torch.isnan(outs[0][1]).all()                              # no bias pointer: nothing written
    for gw, gb in outs[1:]:
        assert torch.equal(gw, outs[0][0])
        if bias:
            assert torch.equal(gb, outs[0][1])


def test_north_star_deterministic_against_default(gpu):
    import bench
    B, V, C, H, W, S = 32, 4, 256, 96, 96, 64
    gen = torch.Generator(device=gpu).manual_seed(0)
    f = torch.randn(B, V, C, H, W, device=gpu, generator=gen)
    go = torch.randn(B, C, S, S, S, device=gpu, generator=gen)
    P = torch.from_numpy(bench.ring_projections(B, V, (H, W), seed=1)).to(gpu)
    ax = torch.linspace(-1000.0, 1000.0, S, device=gpu)
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
    c = grid[None].expand(B, S, S, S, 3).contiguous()
    det = _grad(f, P, c, go, "softmax", det=True)
    dflt = _grad(f, P, c, go, "softmax", det=False)
    del go
    ref = dflt.cpu().numpy()
    record_err("north star det vs default", _err(det.cpu().numpy(), ref), _bound(ref))
