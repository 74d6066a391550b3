"""Lens-distortion-aware un-projection (unprojection(lens=), mvhmr_unproject_*_lens) without a GPU: the argument checks, the
C ABI's refusals and workspace queries, feature_level_lens, the fold-back guard, the shard / cfg plumbing, and the premises of the GPU tests
(tests/test_lens_gpu.py): the exact rig, the fold-back rig, the coverage of the parity rigs and the oracle's anchor to the plain oracles."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lattice_rig
import lens_oracle
from conftest import GOLDEN, golden_cases, load_golden
from geomgrad_oracle import geometry_grad, sample_cells
from multiviewhmr_amd import _capi, aggregation, multiview, sharding
from oracle import cport

DP = ctypes.c_void_p
POS = (ctypes.c_double * 3)(-1.0, -1.0, -1.0)
SIDES = (ctypes.c_double * 3)(2.0, 2.0, 2.0)
NAMES = ("forward", "forward_cuboid", "backward", "backward_cuboid", "backward_deterministic", "backward_cuboid_deterministic", "backward_geometry",
         "backward_geometry_cuboid")
PLAIN = {"forward": "forward", "forward_cuboid": "forward", "backward": "backward", "backward_cuboid": "backward",
         "backward_deterministic": "backward_deterministic", "backward_cuboid_deterministic": "backward_deterministic",
         "backward_geometry": "backward_geometry", "backward_geometry_cuboid": "backward_geometry_cuboid"}


# ------------------------------------------------------------------------------------ the C ABI
def _desc(**kw):
    d = _capi.Desc()
    d.abi_version = _capi.ABI_VERSION
    d.batch, d.views, d.channels, d.feat_h, d.feat_w = 2, 4, 32, 24, 20
    d.vol_x, d.vol_y, d.vol_z = 8, 6, 5
    d.method = _capi.AGG["softmax"]
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _ptrs(null=()):
    dummy, zero = DP(256), DP(0)
    return {k: (zero if k in null else dummy) for k in ("features", "proj", "coords", "lens", "index", "out", "grad", "mask", "weights", "conf")}


NONE = ("mask", "weights", "conf", "index")


def _calls(L, d, ptr, ws=DP(0), wsb=0, only=None, visible=0):
    """every lens entry point with its arguments; the pointers are dummies the validation never dereferences"""
    zero, a = DP(0), ctypes.byref(d)
    la = (ptr["lens"], ptr["mask"], ptr["weights"], ptr["conf"], visible, ptr["index"])
    cub = (ptr["coords"], ptr["coords"], POS, SIDES)
    fn = lambda name: getattr(L, "mvhmr_unproject_%s_lens" % name)          # noqa: E731
    calls = {
        "forward": lambda: fn("forward")(a, ptr["features"], ptr["proj"], ptr["coords"], *la, ptr["out"], ws, wsb, zero),
        "forward_cuboid": lambda: fn("forward_cuboid")(a, ptr["features"], ptr["proj"], *cub, *la, ptr["out"], ws, wsb, zero),
        "backward": lambda: fn("backward")(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], *la, ptr["grad"], ws, wsb, zero),
        "backward_cuboid": lambda: fn("backward_cuboid")(a, ptr["out"], ptr["features"], ptr["proj"], *cub, *la, ptr["grad"], ws, wsb, zero),
        "backward_deterministic": lambda: fn("backward_deterministic")(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], *la, ptr["grad"], ws, wsb, zero),
        "backward_cuboid_deterministic": lambda: fn("backward_cuboid_deterministic")(a, ptr["out"], ptr["features"], ptr["proj"], *cub, *la, ptr["grad"], ws, wsb,
                                                                                     zero),
        "backward_geometry": lambda: fn("backward_geometry")(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], *la, ptr["grad"], ptr["grad"], ws, wsb, zero),
        "backward_geometry_cuboid": lambda: fn("backward_geometry_cuboid")(a, ptr["out"], ptr["features"], ptr["proj"], *cub, *la, ptr["grad"], ptr["grad"],
                                                                           ptr["grad"], ws, wsb, zero),
    }
    return {k: f() for k, f in calls.items() if only is None or k in only}


def _query(L, name, d):
    return getattr(L, "mvhmr_unproject_%s_lens_workspace_bytes" % name)(ctypes.byref(d))


def _plain_query(L, name, d):
    f = getattr(L, "mvhmr_unproject_%s_workspace_bytes" % PLAIN[name])
    f.argtypes, f.restype = [ctypes.POINTER(_capi.Desc)], ctypes.c_size_t
    return f(ctypes.byref(d))


def test_the_lens_family_is_exported_and_declared():
    L = _capi.lib()
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mvhmr_unproject.h")).read()
    for name in NAMES:
        for sym in ("mvhmr_unproject_%s_lens" % name, "mvhmr_unproject_%s_lens_workspace_bytes" % name):
            assert sym in _capi.EXPORTS and hasattr(L, sym) and sym + "(" in header, sym
    assert L.mvhmr_abi_version() == 4                                       # additive within ABI 4


@pytest.mark.parametrize("kw", [dict(), dict(feat_layout=_capi.LAYOUT_BVHWC), dict(feat_dtype=_capi.F16, out_dtype=_capi.F16), dict(out_dtype=_capi.BF16),
                                dict(method=_capi.AGG["mean"], views=3, channels=6), dict(batch=3, vol_x=64, vol_y=64, vol_z=32),
                                dict(views=8, channels=260, feat_h=9, feat_w=13, vol_x=3, vol_y=5, vol_z=7)],
                         ids=["planar", "channels_last", "f16", "bf16", "v3c6", "auto_would_gate", "v8c260"])
def test_workspace_is_the_plain_gather_calls_and_covers_the_plain_call(kw):
    """no region is added: every *_lens query equals the plain variant='gather' query (a lens call whose plain twin takes the plane backward
    therefore has the plane kernels' tap table) unless the plain call as the descriptor has it needs more, which the total covers too"""
    L = _capi.lib()
    d = _desc(**kw)
    gather = _desc(**dict(kw, variant=_capi.VARIANT["gather"]))
    for name in NAMES:
        q = _query(L, name, d)
        assert q == max(_plain_query(L, name, gather), _plain_query(L, name, d)), name
        assert _query(L, name, gather) == _plain_query(L, name, gather), name


@pytest.mark.parametrize("kw,text", [(dict(feat_layout=_capi.LAYOUT_QUAD), b"lens distortion runs the gather kernels"),
                                     (dict(feat_layout=_capi.LAYOUT_QUAD_LOG2E), b"lens distortion runs the gather kernels"),
                                     (dict(variant=_capi.VARIANT["brick"]), b"lens distortion runs the gather kernels")])
def test_quad_layouts_and_the_brick_variant_are_unsupported(kw, text):
    L = _capi.lib()
    for ptr in (_ptrs(NONE), _ptrs(NONE + ("lens",))):                      # with and without a lens
        for name, rc in _calls(L, _desc(**kw), ptr).items():
            assert rc == _capi.ERR_UNSUPPORTED, (name, kw, rc)
            assert text in L.mvhmr_last_error()
    for name in NAMES:
        assert _query(L, name, _desc(**kw)) == 0


@pytest.mark.parametrize("given,visible,text", [("mask", 0, b"lens distortion with a view mask is not built yet"),
                                                ("weights", 0, b"lens distortion with view weights is not built yet"),
                                                (None, 1, b"lens distortion with visibility-aware aggregation is not built yet"),
                                                ("conf", 0, b"lens distortion with view confidence maps is not built yet"),
                                                ("index", 0, b"lens distortion with a feature_index is not built yet")])
def test_the_selections_do_not_compose_yet(given, visible, text):
    L = _capi.lib()
    null = tuple(k for k in NONE if k != given)
    for ptr in (_ptrs(null), _ptrs(null + ("lens",))):
        for name, rc in _calls(L, _desc(), ptr, visible=visible).items():
            assert rc == _capi.ERR_UNSUPPORTED, (name, given, rc)
            assert text in L.mvhmr_last_error()


@pytest.mark.parametrize("null", ["features", "proj", "coords", "out"])
def test_null_pointers_are_refused_before_anything_else(null):
    L = _capi.lib()
    for d in (_desc(), _desc(variant=_capi.VARIANT["brick"])):
        for name, rc in _calls(L, d, _ptrs((null,) + NONE)).items():
            if null == "out" and "geometry" in name:
                continue
            assert rc == _capi.ERR_INVALID_ARGUMENT, (name, null, rc)
    assert _calls(L, _desc(abi_version=3), _ptrs(NONE))["forward"] == _capi.ERR_INVALID_ARGUMENT
    geo = ("backward_geometry", "backward_geometry_cuboid")
    for name, rc in _calls(L, _desc(), _ptrs(("grad",) + NONE), only=geo).items():        # every output null
        assert rc == _capi.ERR_INVALID_ARGUMENT and b"nothing to compute" in L.mvhmr_last_error(), (name, rc)


def test_a_served_call_reports_the_missing_workspace():
    """every storage mode and view count of the plain gather call, with a lens and with a null one (the plain gather call)"""
    L = _capi.lib()
    for kw in (dict(), dict(method=_capi.AGG["max"]), dict(views=12), dict(feat_dtype=_capi.F16, out_dtype=_capi.F16), dict(out_dtype=_capi.BF16)):
        for ptr in (_ptrs(NONE), _ptrs(NONE + ("lens",))):
            for name, rc in _calls(L, _desc(**kw), ptr).items():
                assert rc == _capi.ERR_WORKSPACE, (kw, name, rc, L.mvhmr_last_error())


def test_existing_host_answers_are_untouched_by_the_new_plan():
    """Pack::Lens adds no region and changes no plan: the plain queries answer as the parent's did (tests/golden/host_answers_abi4.json is
    checked by test_host_answers_cpu.py; here the twin relation that makes the lens backward take the plane route where the plain one does)"""
    L = _capi.lib()
    d = _desc(variant=_capi.VARIANT["gather"], views=4, channels=16, feat_h=9, feat_w=13, vol_x=3, vol_y=5, vol_z=7)
    plane = _plain_query(L, "backward", d)
    tab = 2 * 4 * 105                                                        # B V N table entries: 16 B of weights, 4 B of coordinates each
    assert plane >= tab * 20 and _query(L, "backward", d) == plane and _query(L, "backward_deterministic", d) == _plain_query(L, "backward_deterministic", d)


# ------------------------------------------------------------------------------------ Python
def test_argument_errors():
    f, p = torch.zeros(2, 3, 4, 5, 6), torch.zeros(2, 3, 3, 4)
    c = torch.zeros(2, 4, 4, 4, 3)
    r, ce = torch.zeros(2, 3, 3), torch.zeros(2, 3)
    cuboid = ((0, 0, 0), (1, 1, 1), (4, 4, 4))
    lens = torch.zeros(2, 3, 10)
    for bad in (torch.zeros(2, 3, 9), torch.zeros(3, 2, 10), torch.zeros(2, 3, 10, 1), torch.zeros(60)):
        with pytest.raises(RuntimeError, match=r"lens must be \(B, V, 10\)"):
            aggregation.unprojection(f, p, c, lens=bad)
        with pytest.raises(RuntimeError, match=r"lens must be \(B, V, 10\)"):
            aggregation.unprojection_cuboid(f, p, r, ce, *cuboid, lens=bad)
    for bad in (lens.long(), lens.bool()):
        with pytest.raises(TypeError, match="floating dtype"):
            aggregation.unprojection(f, p, c, lens=bad)
    with pytest.raises(TypeError):
        aggregation.unprojection(f, p, c, lens=np.zeros((2, 3, 10), np.float32))
    with pytest.raises(TypeError):                                          # keyword-only, placed after feature_index
        aggregation.unprojection(f, p, c, "softmax", None, "auto", None, None, False, None, None, lens)
    import inspect
    for fn in (aggregation.unprojection, aggregation.unprojection_cuboid):
        params = list(inspect.signature(fn).parameters.values())
        assert [q.name for q in params][-2:] == ["feature_index", "lens"] and params[-1].kind is inspect.Parameter.KEYWORD_ONLY and params[-1].default is None
    with pytest.raises(ValueError, match="not differentiable"):
        aggregation.unprojection(f, p, c, lens=lens.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="not differentiable"):
        aggregation.unprojection_cuboid(f, p, r, ce, *cuboid, lens=lens.clone().requires_grad_(True))
    combos = (dict(view_mask=torch.ones(2, 3, dtype=torch.bool)), dict(view_weights=torch.ones(2, 3)), dict(visible_only=True),
              dict(view_confidence=torch.ones(2, 3, 5, 6)), dict(feature_index=torch.tensor([0, 1])))
    for kw in combos:
        with pytest.raises(ValueError, match="not built yet"):
            aggregation.unprojection(f, p, c, lens=lens, **kw)
        with pytest.raises(ValueError, match="not built yet"):
            aggregation.unprojection_cuboid(f, p, r, ce, *cuboid, lens=lens, **kw)
    for dt in (torch.float32, torch.float64, torch.float16):                # any floating dtype passes the checks: no CPU path, as for every call
        with pytest.raises(RuntimeError, match="HIP device"):
            aggregation.unprojection(f, p, c, lens=lens.to(dt))
        with pytest.raises(RuntimeError, match="HIP device"):
            aggregation.unprojection_cuboid(f, p, r, ce, *cuboid, lens=lens.to(dt))
    with pytest.raises(ValueError, match="Unknown aggregation_method"):
        aggregation.unprojection(f, p, c, "median", lens=lens)


def test_lens_ops_have_shape_functions_and_the_lens_is_not_differentiable():
    from torch._subclasses.fake_tensor import FakeTensorMode
    ops = torch.ops.mvhmr
    with FakeTensorMode():
        f, p, c, lens = torch.empty(2, 3, 4, 5, 6), torch.empty(2, 3, 3, 4), torch.empty(2, 4, 5, 6, 3), torch.empty(2, 3, 10)
        out = ops.unprojection_lens(f, p, c, lens, 0, _capi.F32, 1)
        assert tuple(out.shape) == (2, 4, 4, 5, 6) and out.dtype == torch.float32
        assert ops.unprojection_lens(f, p, c, lens, 0, _capi.BF16, 1).dtype == torch.bfloat16
        assert ops.unprojection_lens_backward(out, f, p, c, lens, 0, _capi.F32, 1).shape == f.shape
        assert ops.unprojection_lens_backward_deterministic(out, f, p, c, lens, 0, _capi.F32, 1).shape == f.shape
        gp, gc = ops.unprojection_lens_backward_geometry(out, f, p, c, lens, 0, _capi.F32, 1, True, True)
        assert gp.shape == p.shape and gc.shape == c.shape and gp.dtype == torch.float32
        gp, gc = ops.unprojection_lens_backward_geometry(out, f, p, c, lens, 0, _capi.F32, 1, False, True)
        assert gp.numel() == 0 and gc.shape == c.shape
        r, ce = torch.empty(2, 3, 3), torch.empty(2, 3)
        out = ops.unprojection_cuboid_lens(f, p, r, ce, lens, [0.0] * 3, [1.0] * 3, [4, 4, 4], 2, _capi.F32, 1)
        assert tuple(out.shape) == (2, 4, 4, 4, 4)
        assert ops.unprojection_cuboid_lens_backward(out, f, p, r, ce, lens, [0.0] * 3, [1.0] * 3, [4, 4, 4], 2, _capi.F32, 1).shape == f.shape
        gp, gr, gce = ops.unprojection_cuboid_lens_backward_geometry(out, f, p, r, ce, lens, [0.0] * 3, [1.0] * 3, [4, 4, 4], 2, _capi.F32, 1, True, True, False)
        assert gp.shape == p.shape and gr.shape == r.shape and gce.numel() == 0
    schema = torch.ops.mvhmr.unprojection_lens.default._schema
    assert [a.name for a in schema.arguments][:4] == ["features", "proj", "coords", "lens"]
    schema = torch.ops.mvhmr.unprojection_cuboid_lens.default._schema
    assert [a.name for a in schema.arguments][:5] == ["features", "proj", "rot", "center", "lens"]
    fam = aggregation._OPS["unprojection_lens"]
    assert fam.grads == ("proj", "coords") and fam.tensors[-1] == "lens" and fam.lens and not fam.masked and not fam.shared
    assert aggregation._lens_variant("auto") == _capi.VARIANT["gather"] and aggregation._lens_variant("brick") == _capi.VARIANT["brick"]


def test_the_extension_ops_take_lens_as_one_more_trailing_argument():
    """the set of op names stays; `lens` is the last, defaulted argument of the six un-projection ops"""
    aggregation._native()
    names = ("unprojection", "unprojection_backward", "unprojection_backward_geometry", "unprojection_cuboid", "unprojection_cuboid_backward",
             "unprojection_cuboid_backward_geometry")
    for n in names:
        args = getattr(torch.ops.mvhmr_native, n).default._schema.arguments
        assert args[-1].name == "lens" and args[-2].name == "feature_index" and args[-1].has_default_value() and args[-1].default_value is None, n


# ------------------------------------------------------------------------------------ feature_level_lens, r2max
def _cameras(B, V, dists, skew=0.0, seed=3):
    rng = np.random.default_rng(seed)
    cams = [[None] * B for _ in range(V)]
    for b in range(B):
        for v in range(V):
            q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
            K = [[1145.0 + 10 * v, skew, 512.3 + b], [0, 1140.0 - 7 * b, 498.7 - v], [0, 0, 1]]
            cam = multiview.Camera(q, rng.standard_normal(3) * 1000, K, dist=dists[(b * V + v) % len(dists)])
            cam.update_after_crop((150 + 3 * v, 140, 850, 860))
            cams[v][b] = cam
    return cams


def test_feature_level_lens_agrees_with_feature_level_projections():
    dists = ((-0.2, 0.05, 0.001, -0.002, 0.01), None, (0.1, 0.0, 0.0, 0.0))
    B, V = 2, 3
    cams = _cameras(B, V, dists)
    images_shape, features_shape = (720, 700), (9, 13)
    P = aggregation.feature_level_projections(cams, images_shape, features_shape)
    L = aggregation.feature_level_lens(cams, images_shape, features_shape)
    assert L.shape == (B, V, 10) and L.dtype == np.float32 and P.dtype == np.float32
    for b in range(B):
        for v in range(V):
            cam = cams[v][b]
            fx, fy, cx, cy = (float(x) for x in L[b, v, :4])
            Rt = np.hstack([cam.R, cam.t])
            K = np.array([[fx, 0, cx], [0, fy, cy]])
            want = K @ Rt[:, :3] if False else K[:, :2] @ Rt[:2, :3] + K[:, 2:3] * Rt[2:3, :3]
            # P[:2, :3] is reproduced from the returned intrinsics and Rt to fp32 rounding (the intrinsics are the float64 ones rounded once)
            assert np.abs(P[b, v, :2, :3] - want).max() <= 2.0 ** -22 * np.abs(want).max()
            sx, sy = features_shape[0] / images_shape[1], features_shape[1] / images_shape[0]   # quirk Q3: (Hf, Wf) read as (width, height)
            assert (fx, fy, cx, cy) == tuple(float(np.float32(x)) for x in (cam.K[0, 0] * sx, cam.K[1, 1] * sy, cam.K[0, 2] * sx, cam.K[1, 2] * sy))
            d = dists[(b * V + v) % len(dists)]
            coef = np.zeros(5, np.float32) if d is None else np.float32(list(d) + [0.0] * (5 - len(d)))
            assert np.array_equal(L[b, v, 4:9], coef)
            assert L[b, v, 9] == aggregation.lens_r2max(coef[0], coef[1], coef[4])
    assert L[0, 1, 9] == np.finfo(np.float32).max                           # no coefficients: no guard
    for row in cams:                                                        # the cameras are not modified
        for cam in row:
            assert cam.K[0, 0] > 1000
    with pytest.raises(ValueError, match="skew"):
        aggregation.feature_level_lens(_cameras(1, 2, (None,), skew=0.5), images_shape, features_shape)
    with pytest.raises(ValueError, match="4 or 5 coefficients"):
        aggregation.feature_level_lens(_cameras(1, 1, ((0.1, 0.2, 0.3),)), images_shape, features_shape)


@pytest.mark.parametrize("name,k", [("barrel", (-0.2, 0.0, 0.0)), ("barrel strong", (-0.45, 0.0, 0.0)), ("pincushion", (0.15, 0.02, 0.0)),
                                    ("mixed", (-0.3, 0.12, -0.02)), ("mixed two roots", (-0.5, 0.08, 0.0)), ("oracle barrel", (-0.2, 0.05, 0.0)),
                                    ("k3 only", (0.0, 0.0, -0.01)), ("none", (0.0, 0.0, 0.0))])
def test_r2max_against_a_brute_force_scan(name, k):
    """r rad(r^2) is strictly increasing on [0, sqrt(r2max)) and turns there: a scan of 2 * 10^6 radii finds the first turning point"""
    k1, k2, k3 = k
    got = float(aggregation.lens_r2max(k1, k2, k3))
    r = np.linspace(0.0, 20.0, 2_000_001)
    r2 = r * r
    g = r * (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3)))
    down = np.nonzero(np.diff(g) <= 0)[0]
    if len(down) == 0:
        assert got == float(np.finfo(np.float32).max), (name, got)
        return
    lo, hi = r[down[0] - 1] ** 2, r[down[0] + 1] ** 2                       # the first turning point lies between these samples
    assert lo <= got <= hi, (name, got, lo, hi)
    poly = 1 + 3 * k1 * got + 5 * k2 * got ** 2 + 7 * k3 * got ** 3         # and it is a root of the pinned polynomial, from the inside
    assert abs(poly) <= 1e-5 and 1 + 3 * k1 * (got * 0.999) + 5 * k2 * (got * 0.999) ** 2 + 7 * k3 * (got * 0.999) ** 3 > 0


# ------------------------------------------------------------------------------------ plumbing
def test_shard_batch_dict_slices_the_lens():
    B, V = 5, 2
    lens = torch.arange(B * V * 10, dtype=torch.float32).reshape(B, V, 10)
    batch = dict(images=torch.zeros(B, V, 8, 8, 3), cameras=[[(v, b) for b in range(B)] for v in range(V)], keypoints_3d=list(range(B)), lens=lens)
    seen = []
    for rank in range(3):
        part = sharding.shard_batch_dict(batch, world_size=3, rank=rank)
        lo, hi = sharding.shard_bounds(B, 3, rank)
        assert torch.equal(part["lens"], lens[lo:hi]) and part["images"].shape[0] == hi - lo
        seen += part["keypoints_3d"]
    assert seen == list(range(B))
    plain = {k: v for k, v in batch.items() if k != "lens"}
    assert "lens" not in sharding.shard_batch_dict(plain, world_size=2, rank=0)


class _Node(dict):
    __getattr__ = dict.__getitem__


def _cfg(**agg):
    return _Node(MODEL=_Node(BACKBONE=_Node(DECONV_FILTERS=[8], DECONV_LAYERS=1),
                             AGGREGATION=_Node(dict(VOLUME_SIZE=4, OUTPUT_CHANNELS=4, CUBOID_SIDE=2500.0, USE_TRIANGULATION=False, METHOD="softmax", **agg))),
                 DATASET=_Node(KIND="mpii", TYPE="human36m"))


def test_the_cfg_key_and_the_generator_checks():
    import unittest.mock as mock
    with mock.patch.object(aggregation.VolumeGenerator, "to", lambda self, *a, **k: self):   # no HIP device here
        assert aggregation.build_volume_generator(_cfg()).lens_distortion is False           # absent = off
        assert aggregation.build_volume_generator(_cfg(LENS_DISTORTION=True)).lens_distortion is True
        assert aggregation.build_volume_generator(_cfg(LENS_DISTORTION=False)).lens_distortion is False
        assert aggregation.VolumeGenerator(volume_size=4, input_channels=4, output_channels=4).lens_distortion is False
        gen = aggregation.VolumeGenerator(volume_size=4, input_channels=4, output_channels=4, lens_distortion=True)
    assert "use_triangulation pivot is unchanged" in aggregation.VolumeGenerator.__doc__ and "second order" in aggregation.VolumeGenerator.__doc__
    batch = dict(images=torch.empty((2, 3, 32, 32, 3), device="meta"),
                 cameras_packed=dict(K=torch.eye(3).repeat(2, 3, 1, 1).double(), Rt=torch.eye(3, 4).repeat(2, 3, 1, 1).double()),
                 keypoints_3d=torch.zeros(2, 17, 3), lens=torch.zeros(2, 3, 10))
    feats, proj = torch.zeros(2, 3, 4, 5, 6), torch.zeros(2, 3, 3, 4)
    with pytest.raises(RuntimeError, match=r"lens must be \(B, V, 10\)"):
        gen(feats, proj, dict(batch, lens=torch.zeros(2, 3, 9)))
    with pytest.raises(ValueError, match="not built yet"):
        gen(feats, proj, dict(batch, view_mask=torch.ones(2, 3, dtype=torch.bool)))
    with pytest.raises(RuntimeError, match="HIP device"):                   # the checks pass; there is no CPU path
        gen(feats, proj, batch)


# ------------------------------------------------------------------------------------ the premises of the GPU tests
def _f32_taps(ix, iy, H, W):
    """make_taps' four weights from fp32 positions, in numpy float32 and in float64"""
    res = []
    for F in (np.float32, np.float64):
        x, y = ix.astype(F), iy.astype(F)
        fx0, fy0 = np.floor(x), np.floor(y)
        wx1, wx0 = x - fx0, (fx0 + F(1)) - x
        wy1, wy0 = y - fy0, (fy0 + F(1)) - y
        res.append(np.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1]))
    return res


def test_the_exact_rigs_precondition():
    """every intermediate of the lens step, the Q1 normalisation and the four tap weights are identical in float32 and float64 on the exact
    rig, the sums the kernels form stay within the 2^24 budget of tests/lattice_rig.py -- so the float64 oracle's bits ARE the fp32 result's --
    and the rig exercises the lens: distorted taps with fractional weights, rays past the guard, a plain view, views behind the camera"""
    feats, proj, coords, grad, lens = lens_oracle.exact_rig()
    B, V, C, H, W = feats.shape
    assert H & (H - 1) == 0 and W & (W - 1) == 0
    moved = frac = guarded = plain = behind = 0
    wq = np.inf
    for b in range(B):
        pts = torch.from_numpy(coords[b].reshape(-1, 3))
        for v in range(V):
            L = lens[b, v]
            assert np.log2(L[0]) % 1 == 0 and np.log2(L[1]) % 1 == 0 and L[2] % 1 == 0 and L[3] % 1 == 0 and not L[5:9].any()
            assert L[4] == 0 or np.log2(abs(L[4])) % 1 == 0
            a, bb, z, _, _ = (t.numpy() for t in sample_cells(torch.from_numpy(proj[b, v]), pts, H, W))
            front = z > 0
            behind += int((~front).sum())
            u32, v32 = (a[front] / z[front]).astype(np.float32), (bb[front] / z[front]).astype(np.float32)
            u64, v64 = a[front].astype(np.float64) / z[front], bb[front].astype(np.float64) / z[front]
            assert np.array_equal(u32.astype(np.float64), u64) and np.array_equal(v32.astype(np.float64), v64)
            if lens_oracle.is_plain(L):
                plain += 1
                ud32, vd32, ud64, vd64, ok = u32, v32, u64, v64, np.ones(u32.shape, bool)
            else:
                s32, s64 = lens_oracle.lens_step32(L, u32, v32), lens_oracle.lens_step64(L, u64, v64)
                for key in s32:
                    assert np.array_equal(np.asarray(s32[key], np.float64), np.asarray(s64[key], np.float64)), (b, v, key)
                ud32, vd32, ud64, vd64, ok = s32["ud"], s32["vd"], s64["ud"], s64["vd"], s32["ok"]
                guarded += int((~ok).sum())
                moved += int(((ud32 != u32) | (vd32 != v32))[ok].sum())
            pos = []
            for F, (uu, vv) in ((np.float32, (ud32, vd32)), (np.float64, (ud64, vd64))):
                gx = F(2) * (uu.astype(F) / F(H) - F(0.5))
                gy = F(2) * (vv.astype(F) / F(W) - F(0.5))
                pos.append((((gx + F(1)) * F(0.5)) * F(W - 1), ((gy + F(1)) * F(0.5)) * F(H - 1)))
            (ix32, iy32), (ix64, iy64) = pos
            assert ix32.dtype == np.float32 and np.array_equal(ix32.astype(np.float64), ix64) and np.array_equal(iy32.astype(np.float64), iy64)
            inside = ok & (ix32 > -1) & (ix32 < W) & (iy32 > -1) & (iy32 < H)
            w32, w64 = _f32_taps(ix32[inside], iy32[inside], H, W)
            assert w32.dtype == np.float32 and np.array_equal(w32.astype(np.float64), w64)
            if not lens_oracle.is_plain(L) and inside.any():
                frac += int(((w64 > 0) & (w64 < 1)).any(0).sum())
                wq = min(wq, float(lattice_rig.lowbit(w64[w64 > 0]).min()))
    assert moved >= 40 and frac >= 20 and guarded >= 10 and plain >= 2 and behind >= 48, (moved, frac, guarded, plain, behind)
    # the budget: every term is a whole feature (or grad_out) times a weight that is a multiple of wq; sums of |terms| / wq must stay below 2^24
    N = coords[0].reshape(-1, 3).shape[0]
    fwd = V * np.abs(feats).max() / wq                                       # a sample's weights sum to at most 1, V views are summed
    bwd = N * np.abs(grad).max() / wq                                        # a pixel receives at most one tap of weight <= 1 per voxel of a view
    assert fwd < lattice_rig.LIMIT and bwd < lattice_rig.LIMIT, (wq, fwd, bwd)


def test_the_fold_back_rig():
    """voxel-views with r2 > r2max that the raw polynomial would land INSIDE the map (what the guard exists for), next to enough live ones"""
    feats, proj, coords, lens = lens_oracle.foldback_rig()
    B, V, C, H, W = feats.shape
    folded = live = 0
    for b in range(B):
        pts = torch.from_numpy(coords[b].reshape(-1, 3))
        for v in range(V):
            assert lens[b, v, 4] < 0 and abs(lens[b, v, 9] - 1 / 0.9) < 1e-6
            z, ix, iy, ok = (t.numpy() for t in lens_oracle.raw_positions(torch.from_numpy(proj[b, v]), lens[b, v], pts, H, W))
            inside = (z > 0) & (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
            folded += int((inside & ~ok).sum())
            live += int((inside & ok).sum())
    assert folded >= 8 and live >= 8, (folded, live)


RIGS = [dict(B=2, V=2, C=6, H=9, W=13, vol=(3, 5, 7)), dict(B=2, V=3, C=16, H=9, W=13, vol=(4, 4, 3)), dict(B=2, V=4, C=16, H=9, W=13, vol=(3, 5, 7)),
        dict(B=2, V=8, C=260, H=9, W=13, vol=(4, 4, 3))]


@pytest.mark.parametrize("kind", sorted(lens_oracle.LENSES))
@pytest.mark.parametrize("shape", RIGS, ids=lambda s: "v%dc%d" % (s["V"], s["C"]))
def test_the_parity_rigs_cover_the_frame(kind, shape):
    """at least a third of the voxel-views inside the frame and inside r2max (asserted again where the GPU tests use the rigs), and the lens
    moves the positions by a visible fraction of a pixel"""
    feats, proj, coords, lens = lens_oracle.ring_rig(seed=5, dists=lens_oracle.LENSES[kind], **shape)
    B, V, C, H, W = feats.shape
    live = total = 0
    shift = 0.0
    for b in range(B):
        pts = torch.from_numpy(coords[b].reshape(-1, 3))
        for v in range(V):
            _, _, z, ix, iy, ok = lens_oracle.lens_cells(torch.from_numpy(proj[b, v]), lens[b, v], pts, H, W)
            _, _, _, px, py = sample_cells(torch.from_numpy(proj[b, v]), pts, H, W)
            inside = (z > 0) & ok & (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
            live += int(inside.sum())
            total += len(z)
            if inside.any():
                shift = max(shift, float(torch.hypot(ix - px, iy - py)[inside].max()))
    assert 3 * live >= total, (live, total)
    assert shift > 0.02, shift


@pytest.mark.parametrize("method", ["softmax", "sum", "mean", "max"])
def test_the_oracle_on_zero_coefficients_is_the_plain_oracle(method):
    """arbitrary intrinsics, zero coefficients: the positions are geomgrad_oracle.sample_cells' and the geometry gradients geometry_grad's, bit
    for bit; the volume and the feature gradient (float64 here) agree with the fp32 C oracle to its rounding"""
    d = load_golden("unproj", "nonsquare_v3c5")
    f, p, c, go = d["features"], d["proj"], d["coords"], d["grad_out"]
    B, V, C, H, W = f.shape
    rng = np.random.default_rng(1)
    lens = np.zeros((B, V, 10), np.float32)
    lens[..., :4] = rng.uniform(-50, 50, (B, V, 4))
    lens[..., 9] = rng.uniform(0, 1e-3, (B, V))                             # not even the guard is read
    lens[0, 1, 4:9] = -0.0
    for b in range(B):
        pts = torch.from_numpy(c[b].reshape(-1, 3))
        for v in range(V):
            got = lens_oracle.lens_cells(torch.from_numpy(p[b, v]), lens[b, v], pts, H, W)
            want = sample_cells(torch.from_numpy(p[b, v]), pts, H, W)
            for g, w in zip(got[:5], want):
                assert torch.equal(g, w) or (torch.isnan(g) == torch.isnan(w)).all() and torch.equal(torch.nan_to_num(g), torch.nan_to_num(w))
            assert bool(got[5].all())
    res = lens_oracle.lens_unprojection(f, p, c, lens, go, method)
    gp, gc = geometry_grad(f, p, c, go, method)
    assert np.array_equal(res["grad_proj"], gp) and np.array_equal(res["grad_coords"], gc)
    ref, gref = cport.forward(f, p, c, method), cport.backward(go, f, p, c, method)
    assert np.abs(res["out"] - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    assert np.abs(res["grad_features"] - gref).max() <= 1e-5 * max(1.0, np.abs(gref).max())


def test_the_goldens_the_gpu_file_reads_exist():
    assert {"tiny_b2v2c4", "nonsquare_v3c5", "tiles_v4c16", "eight_views_c7", "adversarial_v4c6"} <= set(golden_cases("unproj"))
