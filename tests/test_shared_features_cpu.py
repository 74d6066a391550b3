"""Shared feature maps (unprojection(feature_index=...), mvhmr_unproject_*_shared) without a GPU: the reference's goldens
against the float64 oracle composition (tests/shared_oracle.py), the C ABI's exports, workspace queries, refusals and argument checks of the
*_shared entry points through ctypes, the Python argument errors, the fake shapes of the op families and the sharding of the batch key."""
import ctypes
import os

import numpy as np
import pytest
import torch

import shared_oracle as so
from conftest import GOLDEN, golden_cases, load_golden
from multiviewhmr_amd import _capi, aggregation, sharding
from test_geometry_grad_gpu import REL
from test_unproject_gpu import _bound, _err

DP = ctypes.c_void_p
NAMES = ("forward", "forward_cuboid", "backward", "backward_cuboid", "backward_deterministic", "backward_cuboid_deterministic",
         "backward_geometry", "backward_geometry_cuboid")
PLAIN = {"forward": "forward", "forward_cuboid": "forward", "backward": "backward", "backward_cuboid": "backward",
         "backward_deterministic": "backward_deterministic", "backward_cuboid_deterministic": "backward_deterministic",
         "backward_geometry": "backward_geometry", "backward_geometry_cuboid": "backward_geometry_cuboid"}     # the plain queries (one per kind)
METHODS = ("softmax", "sum", "mean", "max")
POS, SIDES = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1)
CASES = {"b3m5v4c5": [1, 0, 1, 1, 0], "b2m4v3c6_nonsquare": [1, 1, 0, 1], "b1m3v8c4_behind": [0, 0, 0]}


# ------------------------------------------------------------------------------------ the oracle composition against the reference
def test_the_goldens_cover_what_they_were_made_for():
    assert golden_cases("shared") == sorted(CASES)
    for case, index in CASES.items():
        d = load_golden("shared", case)
        B, M = d["features"].shape[0], d["coords"].shape[0]
        assert d["index"].tolist() == index and d["index"].dtype == np.int32 and M == len(index) and d["grad_out"].shape[0] == M
        assert os.path.getsize(os.path.join(GOLDEN, "shared_%s.npz" % case)) < 500 * 1000
        for b in set(range(B)) - set(index):                                # an unused sample: exact zeros from the reference's autograd too
            assert not d["gfeat_softmax"][b].any() and not d["gproj_softmax"][b].any()
    assert set(range(3)) - set(CASES["b3m5v4c5"]) == {2}
    d = load_golden("shared", "b1m3v8c4_behind")
    z = np.einsum("mvj,mnj->mvn", d["proj"][d["index"]][:, :, 2, :3].astype(np.float64), d["coords"].reshape(3, -1, 3).astype(np.float64))
    assert ((z + d["proj"][d["index"]][:, :, 2, 3:4]) <= 0).mean() > 0.02         # voxel-views behind a camera


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_composition_matches_the_reference(case, method):
    """the existing oracles on features[idx], proj[idx], then np.add.at over the index: every voxel, within the bounds of the golden tests"""
    d = load_golden("shared", case)
    r = so.shared_unprojection(d["features"], d["proj"], d["coords"], d["index"], d["grad_out"], method)
    for name, got, ref, bound in (("fwd", r["out"], d["out_" + method], None), ("bwd", r["grad_features"], d["gfeat_" + method], None),
                                  ("proj grad", r["grad_proj"], d["gproj_" + method], REL), ("coord grad", r["grad_coords"], d["gcoords_" + method], REL)):
        bound = _bound(ref) if bound is None else bound * float(np.abs(ref).max())
        err = _err(got, ref.astype(np.float64))
        print("shared oracle %s %s %s: %.3g (bound %.3g)" % (case, method, name, err, bound))
        assert err <= bound, (case, method, name, err, bound)


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
    return {k: (zero if k in null else dummy) for k in ("features", "proj", "coords", "index", "out", "grad", "mask", "weights", "conf")}


def _calls(L, d, ptr, volumes, ws=DP(0), wsb=0, only=None, visible=0):
    """every shared entry point with its arguments; the pointers are dummies the validation never dereferences"""
    zero, a = DP(0), ctypes.byref(d)
    sh = (volumes, ptr["index"], ptr["mask"], ptr["weights"], ptr["conf"], visible)
    cub = (ptr["coords"], ptr["coords"], POS, SIDES)
    fn = lambda name: getattr(L, "mvhmr_unproject_%s_shared" % name)          # noqa: E731
    calls = {
        "forward": lambda: fn("forward")(a, ptr["features"], ptr["proj"], ptr["coords"], *sh, ptr["out"], ws, wsb, zero),
        "forward_cuboid": lambda: fn("forward_cuboid")(a, ptr["features"], ptr["proj"], *cub, *sh, ptr["out"], ws, wsb, zero),
        "backward": lambda: fn("backward")(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], *sh, ptr["grad"], ws, wsb, zero),
        "backward_cuboid": lambda: fn("backward_cuboid")(a, ptr["out"], ptr["features"], ptr["proj"], *cub, *sh, ptr["grad"], ws, wsb, zero),
        "backward_deterministic": lambda: fn("backward_deterministic")(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], *sh, ptr["grad"], ws, wsb, zero),
        "backward_cuboid_deterministic": lambda: fn("backward_cuboid_deterministic")(a, ptr["out"], ptr["features"], ptr["proj"], *cub, *sh, ptr["grad"], ws, wsb,
                                                                                     zero),
        "backward_geometry": lambda: fn("backward_geometry")(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], *sh, ptr["grad"], ptr["grad"], ws, wsb, zero),
        "backward_geometry_cuboid": lambda: fn("backward_geometry_cuboid")(a, ptr["out"], ptr["features"], ptr["proj"], *cub, *sh, ptr["grad"], ptr["grad"],
                                                                           ptr["grad"], ws, wsb, zero),
    }
    return {k: f() for k, f in calls.items() if only is None or k in only}


def _query(L, name, d, volumes):
    return getattr(L, "mvhmr_unproject_%s_shared_workspace_bytes" % name)(ctypes.byref(d), volumes)


def _plain_query(L, name, d):
    f = getattr(L, "mvhmr_unproject_%s_workspace_bytes" % PLAIN[name])
    f.argtypes, f.restype = [ctypes.POINTER(_capi.Desc)], ctypes.c_size_t
    return f(ctypes.byref(d))


def test_the_shared_family_is_exported_and_declared():
    L = _capi.lib()
    for name in NAMES:
        assert "mvhmr_unproject_%s_shared" % name in _capi.EXPORTS and "mvhmr_unproject_%s_shared_workspace_bytes" % name in _capi.EXPORTS
        assert hasattr(L, "mvhmr_unproject_%s_shared" % name) and hasattr(L, "mvhmr_unproject_%s_shared_workspace_bytes" % name)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mvhmr_unproject.h")).read()
    for name in NAMES:
        assert "mvhmr_unproject_%s_shared(" % name in header and "mvhmr_unproject_%s_shared_workspace_bytes(" % name in header
    assert L.mvhmr_abi_version() == 4


def _align(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("kw", [dict(), dict(feat_layout=_capi.LAYOUT_BVHWC), dict(feat_dtype=_capi.F16, out_dtype=_capi.F16), dict(method=_capi.AGG["mean"], views=3, channels=6),
                                dict(batch=3, vol_x=64, vol_y=64, vol_z=32, variant=_capi.VARIANT["gather"])],
                         ids=["planar", "channels_last", "f16", "v3c6", "auto_would_gate"])
def test_workspace_is_sized_by_the_feature_samples(kw):
    """forward and feature backward: the same total for M = B and M = 4 B (every region is feature-sized); geometry: it grows by the per-volume
    partials alone -- (M, tiles, V, 12) fp32 of grad_proj and (M, tiles, 12) of the pose, 32 voxels per tile, each region rounded up to 256
    bytes; every total covers the plain gather call's (what a null index runs)"""
    L = _capi.lib()
    d = _desc(**kw)
    B, V = d.batch, d.views
    tiles = (d.vol_x * d.vol_y * d.vol_z + 31) // 32
    gather = _desc(**dict(kw, variant=_capi.VARIANT["gather"]))
    for name in NAMES:
        one, four = _query(L, name, d, B), _query(L, name, d, 4 * B)
        assert one >= _plain_query(L, name, gather) and one >= _plain_query(L, name, d), name
        if "geometry" not in name:
            assert one == four, (name, one, four)
            assert one > 0 or d.feat_layout == _capi.LAYOUT_BVHWC, name
            continue
        part = lambda M: _align(M * tiles * V * 12 * 4) + (_align(M * tiles * 12 * 4) if "cuboid" in name else 0)      # noqa: E731
        assert four - one == part(4 * B) - part(B), (name, one, four)
        assert one - part(B) == _plain_query(L, name, gather) - part(B), name        # and at M = B it is the plain call's
    # the deterministic accumulator is int64 over the B samples, with the B x C exponent tables and the B-word histogram behind it
    det, dflt = _query(L, "backward_deterministic", d, 4 * B), _query(L, "backward", d, 4 * B)
    assert det >= dflt and det >= B * V * d.feat_h * d.feat_w * d.channels * 8 + _align(3 * B * d.channels * 4 + B * 4)


@pytest.mark.parametrize("kw,text", [(dict(feat_layout=_capi.LAYOUT_QUAD), b"shared feature maps need planar or channels-last"),
                                     (dict(feat_layout=_capi.LAYOUT_QUAD_LOG2E), b"shared feature maps need planar or channels-last"),
                                     (dict(variant=_capi.VARIANT["brick"]), b"shared feature maps run the gather kernels")])
def test_quad_layouts_and_the_brick_variant_are_unsupported(kw, text):
    L = _capi.lib()
    for name, rc in _calls(L, _desc(**kw), _ptrs(("mask", "weights", "conf")), 5).items():
        assert rc == _capi.ERR_UNSUPPORTED, (name, kw, rc)
        assert text in L.mvhmr_last_error()
    for name in NAMES:
        assert _query(L, name, _desc(**kw), 5) == 0


def test_the_volume_count_is_checked():
    L = _capi.lib()
    none = ("mask", "weights", "conf")
    for name, rc in _calls(L, _desc(), _ptrs(none), 65536).items():
        assert rc == _capi.ERR_UNSUPPORTED and b"at most 65535 volumes" in L.mvhmr_last_error(), (name, rc)
    for name, rc in _calls(L, _desc(), _ptrs(none), 0).items():
        assert rc == _capi.ERR_INVALID_ARGUMENT and b"volumes must be >= 1" in L.mvhmr_last_error(), (name, rc)
    for name, rc in _calls(L, _desc(), _ptrs(none), 65535).items():          # the largest count is served: only the workspace is missing
        assert rc == _capi.ERR_WORKSPACE, (name, rc)
    for name in NAMES:
        assert _query(L, name, _desc(), 65536) == 0 and _query(L, name, _desc(), 0) == 0
    # a null index is the plain call: volumes must be the batch
    for name, rc in _calls(L, _desc(), _ptrs(none + ("index",)), 5).items():
        assert rc == _capi.ERR_INVALID_ARGUMENT and b"a null feature_index is the plain call: volumes (5) must equal batch (2)" in L.mvhmr_last_error(), (name, rc)
    for name, rc in _calls(L, _desc(), _ptrs(none + ("index",)), 2).items():
        assert rc == _capi.ERR_WORKSPACE, (name, rc)
    d = _desc(feat_layout=_capi.LAYOUT_BVHWC)                               # channels-last fp32: the plain gather forward needs no workspace at all ...
    assert _query(L, "forward", d, 2) == 0
    assert _calls(L, d, _ptrs(none + ("index",)), 2, only=("backward_geometry",))["backward_geometry"] == _capi.ERR_WORKSPACE


@pytest.mark.parametrize("given,visible,text", [("mask", 0, b"feature_index with a view mask is not built yet"),
                                                ("weights", 0, b"feature_index with view weights is not built yet"),
                                                (None, 1, b"feature_index with visibility-aware aggregation is not built yet"),
                                                ("conf", 0, b"feature_index with view confidence maps is not built yet")])
def test_the_view_selections_do_not_compose_yet(given, visible, text):
    L = _capi.lib()
    null = tuple(k for k in ("mask", "weights", "conf") if k != given)
    for ptr in (_ptrs(null), _ptrs(null + ("index",))):                     # with and without an index
        for name, rc in _calls(L, _desc(), ptr, 2, visible=visible).items():
            assert rc == _capi.ERR_UNSUPPORTED, (name, given, rc)
            assert text in L.mvhmr_last_error()


@pytest.mark.parametrize("null", ["features", "proj", "coords", "out"])
def test_null_pointers_are_refused_before_anything_else(null):
    L = _capi.lib()
    for d in (_desc(), _desc(variant=_capi.VARIANT["brick"])):
        for name, rc in _calls(L, d, _ptrs((null, "mask", "weights", "conf")), 5).items():
            if null == "out" and "geometry" in name:
                continue
            assert rc == _capi.ERR_INVALID_ARGUMENT, (name, null, rc)
    assert _calls(L, _desc(abi_version=3), _ptrs(("mask", "weights", "conf")), 5)["forward"] == _capi.ERR_INVALID_ARGUMENT
    geo = ("backward_geometry", "backward_geometry_cuboid")
    for name, rc in _calls(L, _desc(), _ptrs(("grad", "mask", "weights", "conf")), 5, only=geo).items():      # every output null
        assert rc == _capi.ERR_INVALID_ARGUMENT and b"nothing to compute" in L.mvhmr_last_error(), (name, rc)


def test_a_served_call_reports_the_missing_workspace():
    L = _capi.lib()
    for kw in (dict(), dict(method=_capi.AGG["max"]), dict(views=12), dict(feat_dtype=_capi.F16, out_dtype=_capi.F16), dict(out_dtype=_capi.BF16)):
        for name, rc in _calls(L, _desc(**kw), _ptrs(("mask", "weights", "conf")), 7).items():
            assert rc == _capi.ERR_WORKSPACE, (kw, name, rc, L.mvhmr_last_error())


# ------------------------------------------------------------------------------------ Python
def test_argument_errors():
    f, p = torch.zeros(2, 3, 4, 5, 6), torch.zeros(2, 3, 3, 4)
    idx = torch.tensor([1, 0, 1, 1, 0])
    c = torch.zeros(5, 4, 4, 4, 3)
    r, ce = torch.zeros(5, 3, 3), torch.zeros(5, 3)
    cuboid = ((0, 0, 0), (1, 1, 1), (4, 4, 4))
    for bad in (torch.zeros(5, 1, dtype=torch.long), torch.tensor(1)):
        with pytest.raises(RuntimeError, match=r"feature_index must be \(M,\)"):
            aggregation.unprojection(f, p, c, feature_index=bad)
    for bad in (idx.float(), idx.bool()):
        with pytest.raises(TypeError, match="integer dtype"):
            aggregation.unprojection(f, p, c, feature_index=bad)
    with pytest.raises(TypeError):
        aggregation.unprojection(f, p, c, feature_index=[1, 0, 1, 1, 0])
    with pytest.raises(TypeError):                                          # keyword-only
        aggregation.unprojection(f, p, c, "softmax", None, "auto", None, None, False, None, idx)
    for bad in (torch.tensor([1, 0, 2, 1, 0]), torch.tensor([1, 0, -1, 1, 0]), torch.tensor([1, 0, 1, 1, 0], dtype=torch.int8) - 2):
        with pytest.raises(IndexError, match=r"outside \[0, 2\)"):
            aggregation.unprojection(f, p, c, feature_index=bad)
        with pytest.raises(IndexError, match=r"outside \[0, 2\)"):
            aggregation.unprojection_cuboid(f, p, r, ce, *cuboid, feature_index=bad)
    with pytest.raises(RuntimeError, match=r"coord_volumes must be \(5, X, Y, Z, 3\)"):     # the leading dimension is M, not B
        aggregation.unprojection(f, p, torch.zeros(2, 4, 4, 4, 3), feature_index=idx)
    with pytest.raises(RuntimeError, match=r"rotations must be \(5, 3, 3\) and centers \(5, 3\)"):
        aggregation.unprojection_cuboid(f, p, torch.zeros(2, 3, 3), torch.zeros(2, 3), *cuboid, feature_index=idx)
    with pytest.raises(RuntimeError, match=r"rotations must be \(5, 3, 3\) and centers \(5, 3\)"):
        aggregation.unprojection_cuboid(f, p, r, torch.zeros(2, 3), *cuboid, feature_index=idx)
    combos = (dict(view_mask=torch.ones(2, 3, dtype=torch.bool)), dict(view_weights=torch.ones(2, 3)), dict(visible_only=True), dict(view_confidence=torch.ones(2, 3, 5, 6)))
    for kw in combos:
        with pytest.raises(ValueError, match="not built yet"):
            aggregation.unprojection(f, p, c, feature_index=idx, **kw)
        with pytest.raises(ValueError, match="not built yet"):
            aggregation.unprojection_cuboid(f, p, r, ce, *cuboid, feature_index=idx, **kw)
    big = torch.zeros(65536, dtype=torch.int32)
    with pytest.raises(ValueError, match="at most 65535"):
        aggregation.unprojection(f, p, torch.zeros(65536, 1, 1, 1, 3), feature_index=big)
    with pytest.raises(RuntimeError, match="HIP device"):                   # no CPU path, as for every other call
        aggregation.unprojection(f, p, c, feature_index=idx)
    with pytest.raises(RuntimeError, match="HIP device"):
        aggregation.unprojection_cuboid(f, p, r, ce, *cuboid, feature_index=idx.to(torch.int16))


def test_shared_ops_have_shape_functions():
    """the fake registrations: the forward returns M volumes, the feature gradient has B samples, grad_proj B and the placing gradients M"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    ops = torch.ops.mvhmr
    with FakeTensorMode():
        f, p = torch.empty(2, 3, 4, 5, 6), torch.empty(2, 3, 3, 4)
        idx, c = torch.empty(7, dtype=torch.int32), torch.empty(7, 4, 5, 6, 3)
        out = ops.unprojection_shared(f, p, c, idx, 0, _capi.F32, 0)
        assert tuple(out.shape) == (7, 4, 4, 5, 6) and out.dtype == torch.float32
        assert ops.unprojection_shared(f, p, c, idx, 0, _capi.BF16, 0).dtype == torch.bfloat16
        assert ops.unprojection_shared_backward(out, f, p, c, idx, 0, _capi.F32, 0).shape == f.shape
        assert ops.unprojection_shared_backward_deterministic(out, f, p, c, idx, 0, _capi.F32, 0).shape == f.shape
        gp, gc = ops.unprojection_shared_backward_geometry(out, f, p, c, idx, 0, _capi.F32, 0, True, True)
        assert gp.shape == p.shape and gc.shape == c.shape and gp.dtype == torch.float32
        gp, gc = ops.unprojection_shared_backward_geometry(out, f, p, c, idx, 0, _capi.F32, 0, False, True)
        assert gp.numel() == 0 and gc.shape == c.shape
        r, ce = torch.empty(7, 3, 3), torch.empty(7, 3)
        out = ops.unprojection_cuboid_shared(f, p, r, ce, idx, [0.0] * 3, [1.0] * 3, [4, 4, 4], 2, _capi.F32, 0)
        assert tuple(out.shape) == (7, 4, 4, 4, 4)
        assert ops.unprojection_cuboid_shared_backward(out, f, p, r, ce, idx, [0.0] * 3, [1.0] * 3, [4, 4, 4], 2, _capi.F32, 0).shape == f.shape
        gp, gr, gce = ops.unprojection_cuboid_shared_backward_geometry(out, f, p, r, ce, idx, [0.0] * 3, [1.0] * 3, [4, 4, 4], 2, _capi.F32, 0, True, True, False)
        assert gp.shape == p.shape and gr.shape == r.shape and gce.numel() == 0
    with torch.device("meta"):                                              # meta tensors: the same shapes
        f, p = torch.empty(2, 3, 4, 5, 6), torch.empty(2, 3, 3, 4)
        idx, c = torch.empty(7, dtype=torch.int32), torch.empty(7, 4, 5, 6, 3)
        assert tuple(ops.unprojection_shared(f, p, c, idx, 0, _capi.F32, 0).shape) == (7, 4, 4, 5, 6)


def test_the_index_is_not_differentiable_and_the_autograd_formula_is_registered():
    schema = torch.ops.mvhmr.unprojection_shared.default._schema
    assert [a.name for a in schema.arguments][:4] == ["features", "proj", "coords", "feature_index"]
    schema = torch.ops.mvhmr.unprojection_cuboid_shared.default._schema
    assert [a.name for a in schema.arguments][:5] == ["features", "proj", "rot", "center", "feature_index"]
    fam = aggregation._OPS["unprojection_shared"]
    assert fam.grads == ("proj", "coords") and fam.tensors[-1] == "feature_index" and fam.shared and not fam.masked


def test_shard_batch_dict_follows_the_samples_of_a_ragged_index():
    B, V = 5, 2
    index = torch.tensor([3, 0, 0, 4, 1, 0, 3, 1])                          # ragged, unsorted; sample 2 is unused
    M = len(index)
    kp = torch.arange(M * 17 * 3, dtype=torch.float32).reshape(M, 17, 3)
    batch = dict(images=torch.arange(B).reshape(B, 1, 1, 1, 1).expand(B, V, 8, 8, 3).clone(), cameras=[[(v, b) for b in range(B)] for v in range(V)],
                 keypoints_3d=kp, feature_index=index)
    for world in (2, 3):
        seen = []
        for rank in range(world):
            part = sharding.shard_batch_dict(batch, world_size=world, rank=rank)
            lo, hi = sharding.shard_bounds(B, world, rank)
            assert part["images"].shape[0] == hi - lo and [len(row) for row in part["cameras"]] == [hi - lo] * V
            keep = [m for m in range(M) if lo <= index[m] < hi]
            assert part["feature_index"].tolist() == [int(index[m]) - lo for m in keep]          # rebased, in the volumes' order
            assert torch.equal(part["keypoints_3d"], kp[keep])
            assert all(0 <= i < hi - lo for i in part["feature_index"].tolist())
            # the rank's volumes read the samples they read in the whole batch
            assert [int(part["images"][i, 0, 0, 0, 0]) for i in part["feature_index"].tolist()] == [int(index[m]) for m in keep]
            seen += keep
        assert sorted(seen) == list(range(M))                               # the union of the shards is the batch
    # a rank without volumes gets M = 0; list keypoints are selected the same way
    lone = dict(batch, feature_index=torch.tensor([0, 0, 1]), keypoints_3d=["a", "b", "c"])
    parts = [sharding.shard_batch_dict(lone, world_size=3, rank=r) for r in range(3)]
    assert [p["feature_index"].tolist() for p in parts] == [[0, 0, 1], [], []] and [p["keypoints_3d"] for p in parts] == [["a", "b", "c"], [], []]
    assert parts[2]["images"].shape[0] == 1 and parts[2]["feature_index"].shape == (0,)
    # without an index: exactly as before (the sample count comes from keypoints_3d)
    plain = {k: v for k, v in batch.items() if k != "feature_index"}
    plain["keypoints_3d"] = list(range(B))
    part = sharding.shard_batch_dict(plain, world_size=2, rank=1)
    assert part["keypoints_3d"] == [3, 4] and "feature_index" not in part and part["images"].shape[0] == 2


def test_volume_generator_checks_the_index_before_anything_runs():
    import unittest.mock as mock
    with mock.patch.object(aggregation.VolumeGenerator, "to", lambda self, *a, **k: self):   # no HIP device here
        gen = aggregation.VolumeGenerator(volume_size=8, input_channels=4, output_channels=4)
    batch = dict(images=torch.empty((2, 3, 32, 32, 3), device="meta"), cameras_packed=dict(K=torch.eye(3).repeat(2, 3, 1, 1).double(),
                                                                                           Rt=torch.eye(3, 4).repeat(2, 3, 1, 1).double()),
                 keypoints_3d=torch.zeros(5, 17, 3), feature_index=torch.tensor([1, 0, 1, 1, 0]))
    feats, proj = torch.zeros(2, 3, 4, 5, 6), torch.zeros(2, 3, 3, 4)
    with pytest.raises(IndexError, match=r"outside \[0, 2\)"):
        gen(feats, proj, dict(batch, feature_index=torch.tensor([1, 0, 2, 1, 0])))
    with pytest.raises(ValueError, match="not built yet"):
        gen(feats, proj, dict(batch, view_mask=torch.ones(2, 3, dtype=torch.bool)))
    with pytest.raises(TypeError, match="integer dtype"):
        gen(feats, proj, dict(batch, feature_index=torch.tensor([1.0, 0.0])))
    # one pose per volume: M draws in order from the global stream -- the identity index consumes it as no index does
    gen.train()
    np.random.seed(5)
    r5, c5 = gen.volume_pose(batch, proj, (32, 32), feature_index=batch["feature_index"])
    assert tuple(r5.shape) == (5, 3, 3) and tuple(c5.shape) == (5, 3)
    np.random.seed(5)
    same = np.random.uniform(0.0, 2 * np.pi, size=5)
    assert np.allclose(r5[:, 0, 0].numpy(), np.cos(same).astype(np.float32))
    two = dict(batch, keypoints_3d=torch.zeros(2, 17, 3))
    np.random.seed(5)
    ra, _ = gen.volume_pose(two, proj, (32, 32), feature_index=torch.tensor([0, 1]))
    np.random.seed(5)
    rb, _ = gen.volume_pose(two, proj, (32, 32))
    assert torch.equal(ra, rb)
