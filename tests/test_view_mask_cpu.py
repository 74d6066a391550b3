"""Per-sample view masks without a GPU: the C ABI's argument checks of the *_masked entry points, their workspace queries, the masked
ops' shape functions and unprojection(view_mask=...)'s argument errors."""
import ctypes

import pytest
import torch

from multiviewhmr_amd import _capi, aggregation

DP = ctypes.c_void_p
SZ = ctypes.c_size_t


def _lib():
    L = _capi.lib()
    for name in ("forward", "forward_cuboid", "backward", "backward_cuboid", "backward_deterministic", "backward_cuboid_deterministic",
                 "backward_geometry", "backward_geometry_cuboid"):
        f = getattr(L, "mvhmr_unproject_%s_masked_workspace_bytes" % name)
        f.argtypes, f.restype = [DP], SZ
    return L


def _desc(**kw):
    d = _capi.Desc()
    d.abi_version = _capi.ABI_VERSION
    d.batch, d.views, d.channels, d.feat_h, d.feat_w = 2, 4, 32, 24, 20
    d.vol_x, d.vol_y, d.vol_z = 8, 6, 5
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _calls(L, d, ptr, pos, sides, ws, wsb):
    """every masked entry point with its arguments; the pointers are dummies the validation never dereferences"""
    zero = DP(0)
    a = ctypes.byref(d)
    return {
        "forward": L.mvhmr_unproject_forward_masked(a, ptr["features"], ptr["proj"], ptr["coords"], ptr["mask"], ptr["out"], ws, SZ(wsb), zero),
        "forward_cuboid": L.mvhmr_unproject_forward_cuboid_masked(a, ptr["features"], ptr["proj"], ptr["coords"], ptr["coords"], pos, sides,
                                                                  ptr["mask"], ptr["out"], ws, SZ(wsb), zero),
        "backward": L.mvhmr_unproject_backward_masked(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], ptr["mask"], ptr["grad"], ws,
                                                      SZ(wsb), zero),
        "backward_cuboid": L.mvhmr_unproject_backward_cuboid_masked(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], ptr["coords"], pos,
                                                                    sides, ptr["mask"], ptr["grad"], ws, SZ(wsb), zero),
        "backward_deterministic": L.mvhmr_unproject_backward_deterministic_masked(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"],
                                                                                  ptr["mask"], ptr["grad"], ws, SZ(wsb), zero),
        "backward_cuboid_deterministic": L.mvhmr_unproject_backward_cuboid_deterministic_masked(
            a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], ptr["coords"], pos, sides, ptr["mask"], ptr["grad"], ws, SZ(wsb), zero),
        "backward_geometry": L.mvhmr_unproject_backward_geometry_masked(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], ptr["mask"],
                                                                        ptr["grad"], ptr["grad"], ws, SZ(wsb), zero),
        "backward_geometry_cuboid": L.mvhmr_unproject_backward_geometry_cuboid_masked(
            a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], ptr["coords"], pos, sides, ptr["mask"], ptr["grad"], ptr["grad"], ptr["grad"],
            ws, SZ(wsb), zero),
    }


def _ptrs(null=None):
    dummy, zero = DP(256), DP(0)
    return {k: (zero if k == null else dummy) for k in ("features", "proj", "coords", "mask", "out", "grad")}


POS, SIDES = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1)


@pytest.mark.parametrize("null", ["features", "proj", "coords", "out"])
def test_null_pointers_are_invalid_arguments(null):
    L = _lib()
    rcs = _calls(L, _desc(), _ptrs(null), POS, SIDES, DP(0), 0)
    for name, rc in rcs.items():
        if null == "out" and "geometry" in name:
            continue                        # grad_out is "out" here: still non-null outputs, so covered by the other cases
        assert rc == _capi.ERR_INVALID_ARGUMENT, (name, null, rc)


def test_bad_descriptors_are_refused():
    L = _lib()
    for kw in (dict(abi_version=3), dict(batch=0), dict(method=7), dict(views=17)):
        for name, rc in _calls(L, _desc(**kw), _ptrs(), POS, SIDES, DP(0), 0).items():
            assert rc in (_capi.ERR_INVALID_ARGUMENT, _capi.ERR_UNSUPPORTED), (name, kw, rc)
        for name in ("forward", "backward", "backward_deterministic", "backward_geometry"):
            assert getattr(L, "mvhmr_unproject_%s_masked_workspace_bytes" % name)(ctypes.byref(_desc(**kw))) == 0


@pytest.mark.parametrize("kw", [dict(feat_layout=_capi.LAYOUT_QUAD), dict(feat_layout=_capi.LAYOUT_QUAD + 1), dict(variant=_capi.VARIANT["brick"])])
def test_quad_layouts_and_the_brick_variant_are_unsupported_with_a_mask(kw):
    """the documented decision: a non-null mask needs planar or channels-last features and a gather-capable variant"""
    L = _lib()
    for name, rc in _calls(L, _desc(**kw), _ptrs(), POS, SIDES, DP(0), 0).items():
        assert rc == _capi.ERR_UNSUPPORTED, (name, kw, rc)


def test_missing_workspace_is_reported():
    L = _lib()
    for name, rc in _calls(L, _desc(), _ptrs(), POS, SIDES, DP(0), 0).items():
        assert rc == _capi.ERR_WORKSPACE, (name, rc)


@pytest.mark.parametrize("kw", [dict(), dict(feat_layout=_capi.LAYOUT_BVHWC), dict(feat_dtype=_capi.F16, out_dtype=_capi.F16), dict(views=12),
                                dict(channels=6), dict(vol_x=64, vol_y=64, vol_z=64)])
def test_masked_workspace_covers_the_unmasked_call(kw):
    """a null mask is the unmasked entry point: the masked query must cover its workspace too"""
    L = _lib()
    d = ctypes.byref(_desc(**kw))
    assert L.mvhmr_unproject_forward_masked_workspace_bytes(d) >= L.mvhmr_unproject_forward_workspace_bytes(d)
    assert L.mvhmr_unproject_backward_masked_workspace_bytes(d) >= L.mvhmr_unproject_backward_workspace_bytes(d)
    assert L.mvhmr_unproject_backward_deterministic_masked_workspace_bytes(d) >= L.mvhmr_unproject_backward_deterministic_workspace_bytes(d)
    assert L.mvhmr_unproject_backward_geometry_masked_workspace_bytes(d) >= L.mvhmr_unproject_backward_geometry_workspace_bytes(d)
    assert L.mvhmr_unproject_forward_masked_workspace_bytes(d) > 0


def test_fake_shapes_of_the_masked_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty(3, 4, 8, 6, 5)
        p, c, m = torch.empty(3, 4, 3, 4), torch.empty(3, 7, 6, 5, 3), torch.empty(3, 4, dtype=torch.uint8)
        out = torch.ops.mvhmr.unprojection_masked(f, p, c, m, 0, _capi.F32, 0)
        assert out.shape == (3, 8, 7, 6, 5) and out.dtype == torch.float32
        g = torch.ops.mvhmr.unprojection_masked_backward(out, f, p, c, m, 0, _capi.F32, 0)
        assert g.shape == f.shape
        g = torch.ops.mvhmr.unprojection_masked_backward_deterministic(out, f, p, c, m, 0, _capi.F32, 0)
        assert g.shape == f.shape
        gp, gc = torch.ops.mvhmr.unprojection_masked_backward_geometry(out, f, p, c, m, 0, _capi.F32, 0)
        assert gp.shape == p.shape and gc.shape == c.shape
        out16 = torch.ops.mvhmr.unprojection_masked(f.half(), p, c, m, 0, _capi.F16, 0)
        assert out16.dtype == torch.float16


def test_view_mask_argument_errors():
    f, p, c = torch.zeros(2, 3, 4, 5, 5), torch.zeros(2, 3, 3, 4), torch.zeros(2, 4, 4, 4, 3)
    with pytest.raises(RuntimeError):
        aggregation.unprojection(f, p, c, view_mask=torch.ones(2, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError):
        aggregation.unprojection(f, p, c, view_mask=torch.ones(3, dtype=torch.bool))
    with pytest.raises(TypeError):
        aggregation.unprojection(f, p, c, view_mask=torch.ones(2, 3))
    with pytest.raises(TypeError):
        aggregation.unprojection(f, p, c, view_mask=[[1, 1, 1], [1, 1, 1]])


def test_fake_shapes_of_the_masked_cuboid_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty(3, 4, 8, 6, 5)
        p, r, c, m = torch.empty(3, 4, 3, 4), torch.empty(3, 3, 3), torch.empty(3, 3), torch.empty(3, 4, dtype=torch.uint8)
        args = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [7, 6, 5], 0, _capi.F32, 0)
        out = torch.ops.mvhmr.unprojection_cuboid_masked(f, p, r, c, m, *args)
        assert out.shape == (3, 8, 7, 6, 5)
        assert torch.ops.mvhmr.unprojection_cuboid_masked_backward(out, f, p, r, c, m, *args).shape == f.shape
        assert torch.ops.mvhmr.unprojection_cuboid_masked_backward_deterministic(out, f, p, r, c, m, *args).shape == f.shape
        gp, gr, gc = torch.ops.mvhmr.unprojection_cuboid_masked_backward_geometry(out, f, p, r, c, m, *args)
        assert gp.shape == p.shape and gr.shape == r.shape and gc.shape == c.shape


def test_cuboid_view_mask_argument_errors():
    f, p = torch.zeros(2, 3, 4, 5, 5), torch.zeros(2, 3, 3, 4)
    r, c = torch.zeros(2, 3, 3), torch.zeros(2, 3)
    with pytest.raises(RuntimeError):
        aggregation.unprojection_cuboid(f, p, r, c, (0, 0, 0), (1, 1, 1), (4, 4, 4), view_mask=torch.ones(3, 3, dtype=torch.bool))
    with pytest.raises(TypeError):
        aggregation.unprojection_cuboid(f, p, r, c, (0, 0, 0), (1, 1, 1), (4, 4, 4), view_mask=torch.ones(2, 3))


def test_shard_batch_dict_slices_the_view_mask():
    from multiviewhmr_amd import sharding
    B, V = 5, 3
    mask = torch.arange(B * V).reshape(B, V) % 2 == 0
    batch = dict(images=torch.zeros(B, V, 4, 4, 3), cameras=[list(range(B)) for _ in range(V)], keypoints_3d=list(range(B)), view_mask=mask)
    parts = [sharding.shard_batch_dict(batch, world_size=2, rank=r) for r in range(2)]
    assert torch.equal(torch.cat([s["view_mask"] for s in parts]), mask)
    for s in parts:
        assert s["view_mask"].shape[0] == len(s["keypoints_3d"])
    no_mask = dict(batch)
    del no_mask["view_mask"]
    assert "view_mask" not in sharding.shard_batch_dict(no_mask, world_size=2, rank=0)
