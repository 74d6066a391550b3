"""Per-view confidence weights without a GPU: the float64 oracle (tests/viewweight_oracle.py) against the reference's goldens on duplicated
views, the scale invariance of its weight gradient, unprojection(view_weights=...)'s argument errors, the C ABI's argument checks of the
*_weighted entry points and their workspace queries, the weighted ops' shape functions and shard_batch_dict."""
import ctypes

import numpy as np
import pytest
import torch

import viewweight_oracle as vo
from conftest import golden_cases, load_golden
from multiviewhmr_amd import _capi, aggregation
from test_unproject_gpu import _bound, _err

DP = ctypes.c_void_p
SZ = ctypes.c_size_t
NAMES = ("forward", "forward_cuboid", "backward", "backward_cuboid", "backward_deterministic", "backward_cuboid_deterministic",
         "backward_geometry", "backward_geometry_cuboid")


# ------------------------------------------------------------------------------------ the oracle against the reference
@pytest.mark.parametrize("method", vo.METHODS)
@pytest.mark.parametrize("case", golden_cases("viewweights"))
def test_oracle_matches_the_reference_on_duplicated_views(case, method):
    """an integer weight k is the reference run on a sample that holds the view k times (tests/golden/make_golden_viewweights.py)"""
    d = load_golden("viewweights", case)
    w = d["weights"]
    assert w.min() == 0 and w.max() == 3 and (w.sum(1) == 0).any() and ((w > 0).sum(1) == 1).any() and w.sum(1).max() <= 8
    r = vo.weighted_unprojection(d["features"], d["proj"], d["coords"], w, d["grad_out"], method, geometry=False)
    ref, gref = d["out_" + method], d["gfeat_" + method]
    fwd, bwd = _err(r["out"], ref), _err(r["grad_features"], gref)
    print("viewweights oracle %s %s: fwd %.3g (bound %.3g), bwd %.3g (bound %.3g)" % (case, method, fwd, _bound(ref), bwd, _bound(gref)))
    assert fwd <= _bound(ref) and bwd <= _bound(gref)


@pytest.mark.parametrize("method", ["mean", "softmax"])
@pytest.mark.parametrize("case", golden_cases("viewweights"))
def test_oracle_weight_gradient_is_orthogonal_to_the_weights(case, method):
    """mean and softmax do not change when a sample's weights are scaled: sum_v w_v grad_w_v == 0 (float64: 1e-12 of sum |w_v grad_w_v|).
    A sample with ONE present view has a single term, which is itself zero up to the rounding of s - out: there the term is held to 1e-12
    of the products that cancel in it, sum |g| |s| / w (an upper bound of them: the `sum` oracle on |features| and |grad_out|)."""
    d = load_golden("viewweights", case)
    rng = np.random.default_rng(3)
    w = d["weights"] * rng.uniform(0.05, 4.0, d["weights"].shape)          # real weights, the goldens' absences
    r = vo.weighted_unprojection(d["features"], d["proj"], d["coords"], w, d["grad_out"], method, geometry=False)
    dot, mag = (w * r["grad_weights"]).sum(1), np.abs(w * r["grad_weights"]).sum(1)
    several = (w > 0).sum(1) >= 2
    assert several.any() and (np.abs(dot[several]) <= 1e-12 * mag[several]).all(), (dot, mag)
    cancel = vo.weighted_unprojection(np.abs(d["features"]), d["proj"], d["coords"], w, np.abs(d["grad_out"]), "sum", geometry=False)["grad_weights"]
    single = ((w > 0).sum(1) == 1)[:, None] & (w > 0)
    assert single.any() and (np.abs(r["grad_weights"][single]) <= 1e-12 * cancel[single] / w[single]).all()
    assert (r["grad_weights"][w == 0] == 0).all() and mag.max() > 0


@pytest.mark.parametrize("method", vo.METHODS)
def test_oracle_gradient_columns_agree_with_autograd(method):
    """the ds_v and dw_v columns of the table (weighted_agg_grad) against float64 autograd through the `out` column"""
    g = torch.Generator().manual_seed(5)
    S = torch.randn(4, 3, 11, generator=g, dtype=torch.float64).requires_grad_(True)
    w = (torch.rand(4, generator=g, dtype=torch.float64) * 4 + 0.05).requires_grad_(True)
    go = torch.randn(3, 11, generator=g, dtype=torch.float64)
    gs, gw = torch.autograd.grad((vo.weighted_out(S, w, method) * go).sum(), (S, w))
    ds, dw = vo.weighted_agg_grad(S.detach(), w.detach(), go, method)
    assert float((ds - gs).abs().max()) <= 1e-12 * float(gs.abs().max())
    assert float((dw.sum((1, 2)) - gw).abs().max()) <= 1e-12 * float(gw.abs().max())


def test_oracle_absent_views_are_never_touched():
    d = load_golden("viewweights", "v4c5")
    w = d["weights"].copy()
    w[0, 1], w[3, 0] = -1.0, np.nan                                          # negative and NaN weights are absent too
    f, p = d["features"].copy(), d["proj"].copy()
    a = vo.weighted_unprojection(f, p, d["coords"], w, d["grad_out"], "softmax")
    f[~vo.present_views(w)] = np.nan
    p[~vo.present_views(w)] = np.inf
    b = vo.weighted_unprojection(f, p, d["coords"], w, d["grad_out"], "softmax")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not a["grad_weights"][~vo.present_views(w)].any() and not a["out"][1].any()


# ------------------------------------------------------------------------------------ Python argument errors
def test_view_weights_argument_errors():
    f, p, c = torch.zeros(2, 3, 4, 5, 5), torch.zeros(2, 3, 3, 4), torch.zeros(2, 4, 4, 4, 3)
    with pytest.raises(RuntimeError):
        aggregation.unprojection(f, p, c, view_weights=torch.ones(2, 4))
    with pytest.raises(RuntimeError):
        aggregation.unprojection(f, p, c, view_weights=torch.ones(3))
    with pytest.raises(TypeError):
        aggregation.unprojection(f, p, c, view_weights=torch.ones(2, 3, dtype=torch.bool))
    with pytest.raises(TypeError):
        aggregation.unprojection(f, p, c, view_weights=torch.ones(2, 3, dtype=torch.int64))
    with pytest.raises(TypeError):
        aggregation.unprojection(f, p, c, view_weights=[[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]])
    with pytest.raises(ValueError, match="max"):
        aggregation.unprojection(f, p, c, "max", view_weights=torch.ones(2, 3))
    with pytest.raises(TypeError):                      # view_mask keeps refusing float tensors
        aggregation.unprojection(f, p, c, view_mask=torch.ones(2, 3), view_weights=torch.ones(2, 3))


def test_cuboid_view_weights_argument_errors():
    f, p = torch.zeros(2, 3, 4, 5, 5), torch.zeros(2, 3, 3, 4)
    r, c = torch.zeros(2, 3, 3), torch.zeros(2, 3)
    geo = ((0, 0, 0), (1, 1, 1), (4, 4, 4))
    with pytest.raises(RuntimeError):
        aggregation.unprojection_cuboid(f, p, r, c, *geo, view_weights=torch.ones(3, 3))
    with pytest.raises(TypeError):
        aggregation.unprojection_cuboid(f, p, r, c, *geo, view_weights=torch.ones(2, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="max"):
        aggregation.unprojection_cuboid(f, p, r, c, *geo, "max", view_weights=torch.ones(2, 3))


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
    return {k: (zero if k in null else dummy) for k in ("features", "proj", "coords", "mask", "weights", "out", "grad", "grad_weights")}


POS, SIDES = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1)


def _calls(L, d, ptr, ws=DP(0), wsb=0, only=None):
    """every weighted entry point with its arguments; the pointers are dummies the validation never dereferences"""
    zero, a, m, w = DP(0), ctypes.byref(d), ptr["mask"], ptr["weights"]
    cub = (ptr["coords"], ptr["coords"], POS, SIDES)
    calls = {
        "forward": lambda: L.mvhmr_unproject_forward_weighted(a, ptr["features"], ptr["proj"], ptr["coords"], m, w, ptr["out"], ws, wsb, zero),
        "forward_cuboid": lambda: L.mvhmr_unproject_forward_cuboid_weighted(a, ptr["features"], ptr["proj"], *cub, m, w, ptr["out"], ws, wsb, zero),
        "backward": lambda: L.mvhmr_unproject_backward_weighted(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], m, w, ptr["grad"], ws, wsb, zero),
        "backward_cuboid": lambda: L.mvhmr_unproject_backward_cuboid_weighted(a, ptr["out"], ptr["features"], ptr["proj"], *cub, m, w, ptr["grad"], ws, wsb,
                                                                              zero),
        "backward_deterministic": lambda: L.mvhmr_unproject_backward_deterministic_weighted(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], m, w,
                                                                                            ptr["grad"], ws, wsb, zero),
        "backward_cuboid_deterministic": lambda: L.mvhmr_unproject_backward_cuboid_deterministic_weighted(a, ptr["out"], ptr["features"], ptr["proj"], *cub,
                                                                                                          m, w, ptr["grad"], ws, wsb, zero),
        "backward_geometry": lambda: L.mvhmr_unproject_backward_geometry_weighted(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], m, w,
                                                                                  ptr["grad"], ptr["grad"], ptr["grad_weights"], ws, wsb, zero),
        "backward_geometry_cuboid": lambda: L.mvhmr_unproject_backward_geometry_cuboid_weighted(a, ptr["out"], ptr["features"], ptr["proj"], *cub, m, w,
                                                                                                ptr["grad"], ptr["grad"], ptr["grad"], ptr["grad_weights"],
                                                                                                ws, wsb, zero),
    }
    return {k: f() for k, f in calls.items() if only is None or k in only}


def _query(L, name, d, tag="weighted"):
    f = getattr(L, "mvhmr_unproject_%s_%s_workspace_bytes" % (name, tag) if tag else "mvhmr_unproject_%s_workspace_bytes" % name)
    f.argtypes, f.restype = [ctypes.POINTER(_capi.Desc)], SZ
    return f(ctypes.byref(d))


def test_the_weighted_family_is_exported_and_declared():
    L = _capi.lib()
    for name in NAMES:
        assert "mvhmr_unproject_%s_weighted" % name in _capi.EXPORTS and "mvhmr_unproject_%s_weighted_workspace_bytes" % name in _capi.EXPORTS
        assert hasattr(L, "mvhmr_unproject_%s_weighted" % name)
    assert L.mvhmr_abi_version() == 4


@pytest.mark.parametrize("null", ["features", "proj", "coords", "out"])
def test_null_pointers_are_invalid_arguments(null):
    for name, rc in _calls(_capi.lib(), _desc(), _ptrs((null,))).items():
        if null == "out" and "geometry" in name:
            continue                        # grad_out is "out" here: still non-null outputs, so covered by the other cases
        assert rc == _capi.ERR_INVALID_ARGUMENT, (name, null, rc)


def test_geometry_without_any_output_is_invalid_and_weights_alone_are_served():
    L = _capi.lib()
    geo = ("backward_geometry", "backward_geometry_cuboid")
    for name, rc in _calls(L, _desc(), _ptrs(("grad", "grad_weights")), only=geo).items():
        assert rc == _capi.ERR_INVALID_ARGUMENT and b"nothing to compute" in L.mvhmr_last_error(), (name, rc)
    for name, rc in _calls(L, _desc(), _ptrs(("grad",)), only=geo).items():        # grad_weights alone: gets as far as the workspace check
        assert rc == _capi.ERR_WORKSPACE, (name, rc)
    for name, rc in _calls(L, _desc(), _ptrs(("weights",)), only=geo).items():     # grad_weights needs view_weights
        assert rc == _capi.ERR_INVALID_ARGUMENT and b"grad_weights" in L.mvhmr_last_error(), (name, rc)


def test_bad_descriptors_are_refused():
    L = _capi.lib()
    for kw in (dict(abi_version=3), dict(batch=0), dict(method=7), dict(views=17)):
        for name, rc in _calls(L, _desc(**kw), _ptrs()).items():
            assert rc in (_capi.ERR_INVALID_ARGUMENT, _capi.ERR_UNSUPPORTED), (name, kw, rc)
        for name in NAMES:
            assert _query(L, name, _desc(**kw)) == 0


@pytest.mark.parametrize("kw", [dict(feat_layout=_capi.LAYOUT_QUAD), dict(feat_layout=_capi.LAYOUT_QUAD_LOG2E), dict(variant=_capi.VARIANT["brick"]),
                                dict(method=_capi.AGG["max"])])
def test_quad_layouts_the_brick_variant_and_max_are_unsupported_with_weights(kw):
    L = _capi.lib()
    for name, rc in _calls(L, _desc(**kw), _ptrs()).items():
        assert rc == _capi.ERR_UNSUPPORTED, (name, kw, rc)
    for name, rc in _calls(L, _desc(**kw), _ptrs(("mask",))).items():               # weights without a mask: the same
        assert rc == _capi.ERR_UNSUPPORTED, (name, kw, rc)
    for name in NAMES:
        assert _query(L, name, _desc(**kw)) == 0


def test_max_with_null_weights_is_the_masked_call():
    """null weights: exactly the *_masked entry point, which serves max -- it gets as far as the workspace check"""
    L = _capi.lib()
    for name, rc in _calls(L, _desc(method=_capi.AGG["max"]), _ptrs(("weights", "grad_weights"))).items():
        assert rc == _capi.ERR_WORKSPACE, (name, rc)


def test_missing_workspace_is_reported():
    L = _capi.lib()
    for ptr in (_ptrs(), _ptrs(("mask",))):
        for name, rc in _calls(L, _desc(), ptr).items():
            assert rc == _capi.ERR_WORKSPACE, (name, rc)


@pytest.mark.parametrize("kw", [dict(), dict(feat_layout=_capi.LAYOUT_BVHWC), dict(feat_dtype=_capi.F16, out_dtype=_capi.F16), dict(views=12),
                                dict(channels=6), dict(vol_x=64, vol_y=64, vol_z=64), dict(method=_capi.AGG["sum"])])
def test_weighted_workspace_covers_the_masked_and_the_unmasked_call(kw):
    L = _capi.lib()
    d = _desc(**kw)
    for name in NAMES:
        plain = name.replace("backward_cuboid_deterministic", "backward_deterministic")
        plain = plain if "geometry" in plain else plain.replace("_cuboid", "")      # (the unmasked cuboid calls share the tensor calls' queries)
        weighted, masked, unmasked = _query(L, name, d), _query(L, name, d, "masked"), _query(L, plain, d, "")
        assert weighted >= masked >= unmasked and weighted > 0, (name, weighted, masked, unmasked)
    # a null-weights call needs the masked bytes only: one byte less than that is refused, the masked size passes the workspace check
    need = _query(L, "forward", d, "masked")
    ptr = _ptrs(("weights",))
    a = ctypes.byref(d)
    assert L.mvhmr_unproject_forward_weighted(a, ptr["features"], ptr["proj"], ptr["coords"], ptr["mask"], ptr["weights"], ptr["out"], DP(256),
                                              need - 1, DP(0)) == _capi.ERR_WORKSPACE


# ------------------------------------------------------------------------------------ shape functions of the new ops
def test_fake_shapes_of_the_weighted_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty(3, 4, 8, 6, 5)
        p, c, m, w = torch.empty(3, 4, 3, 4), torch.empty(3, 7, 6, 5, 3), torch.empty(3, 4, dtype=torch.uint8), torch.empty(3, 4)
        out = torch.ops.mvhmr.unprojection_weighted(f, p, c, m, w, 0, _capi.F32, 0)
        assert out.shape == (3, 8, 7, 6, 5) and out.dtype == torch.float32
        g = torch.ops.mvhmr.unprojection_weighted_backward(out, f, p, c, m, w, 0, _capi.F32, 0)
        assert g.shape == f.shape and g.dtype == f.dtype
        g = torch.ops.mvhmr.unprojection_weighted_backward_deterministic(out, f, p, c, m, w, 0, _capi.F32, 0)
        assert g.shape == f.shape
        gp, gc, gw = torch.ops.mvhmr.unprojection_weighted_backward_geometry(out, f, p, c, m, w, 0, _capi.F32, 0)
        assert gp.shape == p.shape and gc.shape == c.shape and gw.shape == w.shape and gw.dtype == torch.float32
        gp, gc, gw = torch.ops.mvhmr.unprojection_weighted_backward_geometry(out, f, p, c, m, w, 0, _capi.F32, 0, False, False, True)
        assert gp.shape == (0,) and gc.shape == (0,) and gw.shape == w.shape
        out16 = torch.ops.mvhmr.unprojection_weighted(f.half(), p, c, m, w, 0, _capi.F16, 0)
        assert out16.dtype == torch.float16


def test_fake_shapes_of_the_weighted_cuboid_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty(3, 4, 8, 6, 5)
        p, r, c = torch.empty(3, 4, 3, 4), torch.empty(3, 3, 3), torch.empty(3, 3)
        m, w = torch.empty(3, 4, dtype=torch.uint8), torch.empty(3, 4)
        args = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [7, 6, 5], 0, _capi.F32, 0)
        out = torch.ops.mvhmr.unprojection_cuboid_weighted(f, p, r, c, m, w, *args)
        assert out.shape == (3, 8, 7, 6, 5)
        assert torch.ops.mvhmr.unprojection_cuboid_weighted_backward(out, f, p, r, c, m, w, *args).shape == f.shape
        assert torch.ops.mvhmr.unprojection_cuboid_weighted_backward_deterministic(out, f, p, r, c, m, w, *args).shape == f.shape
        gp, gr, gc, gw = torch.ops.mvhmr.unprojection_cuboid_weighted_backward_geometry(out, f, p, r, c, m, w, *args)
        assert gp.shape == p.shape and gr.shape == r.shape and gc.shape == c.shape and gw.shape == w.shape


def test_the_weighted_ops_differentiate_the_weights_under_fake_tensors():
    """autograd through the registered formula: view_weights gets a gradient of its shape, view_mask none"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty(2, 3, 4, 6, 5, requires_grad=True)
        p, c = torch.empty(2, 3, 3, 4, requires_grad=True), torch.empty(2, 4, 4, 4, 3)
        m, w = torch.empty(2, 3, dtype=torch.uint8), torch.empty(2, 3, requires_grad=True)
        out = torch.ops.mvhmr.unprojection_weighted(f, p, c, m, w, 1, _capi.F32, 0)
        out.sum().backward()
        assert f.grad.shape == f.shape and p.grad.shape == p.shape and w.grad.shape == w.shape and c.grad is None


def test_shard_batch_dict_slices_the_view_weights():
    from multiviewhmr_amd import sharding
    B, V = 5, 3
    weights = torch.arange(B * V, dtype=torch.float32).reshape(B, V)
    batch = dict(images=torch.zeros(B, V, 4, 4, 3), cameras=[list(range(B)) for _ in range(V)], keypoints_3d=list(range(B)), view_weights=weights)
    parts = [sharding.shard_batch_dict(batch, world_size=2, rank=r) for r in range(2)]
    assert torch.equal(torch.cat([s["view_weights"] for s in parts]), weights)
    for s in parts:
        assert s["view_weights"].shape[0] == len(s["keypoints_3d"])
    plain = dict(batch)
    del plain["view_weights"]
    assert "view_weights" not in sharding.shard_batch_dict(plain, world_size=2, rank=0)
    both = sharding.shard_batch_dict(dict(batch, view_mask=weights > 3), world_size=2, rank=1)
    assert both["view_mask"].shape == both["view_weights"].shape
