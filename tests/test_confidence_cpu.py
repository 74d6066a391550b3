"""Per-pixel view confidence maps (unprojection(view_confidence=...), mvhmr_unproject_*_confidence) without a GPU: the
float64 oracle (tests/confidence_oracle.py) against the reference's goldens (constant integer maps = repeated views), its own identities,
the C ABI's workspace queries, refusals and argument checks of the *_confidence entry points through ctypes, the Python argument errors, the
fake shapes of the op families and the sharding of the batch key."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import confidence_oracle as co
import visibility_oracle as vis
from conftest import GOLDEN, golden_cases, load_golden
from multiviewhmr_amd import _capi, aggregation, sharding
from test_unproject_gpu import _bound, _err

sys.path.insert(0, GOLDEN)
import make_host_answers as mha  # noqa: E402  (the descriptor sweep the host answers of ABI 4 are recorded over)

DP = ctypes.c_void_p
SZ = ctypes.c_size_t
NAMES = ("forward", "forward_cuboid", "backward", "backward_cuboid", "backward_deterministic", "backward_cuboid_deterministic",
         "backward_geometry", "backward_geometry_cuboid")
POS, SIDES = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1)


# ------------------------------------------------------------------------------------ the oracle against the reference
def test_the_goldens_cover_what_they_were_made_for():
    cases = golden_cases("confidence")
    assert len(cases) == 3
    for case in cases:
        d = load_golden("confidence", case)
        B, V, _, H, W = d["features"].shape
        clean = d["clean"].reshape(B, -1)
        assert (clean.mean(1) >= 0.70).all(), (case, clean.mean(1))
        k = d["confidence"]
        assert (k == k[:, :, :1, :1]).all() and set(np.unique(k)) <= {1.0, 2.0, 3.0}     # constant integer maps
        counts = np.bincount(vis.seen_views(d["proj"], d["coords"], H, W).sum(1)[clean], minlength=V + 1)
        if V in (3, 4):
            assert (counts > 0).all(), (case, counts)                       # every seeing count 0 ... V occurs among the clean voxels
        assert not d["grad_out"][~np.broadcast_to(d["clean"][:, None], d["grad_out"].shape)].any()
        assert os.path.getsize(os.path.join(GOLDEN, "confidence_%s.npz" % case)) < 500 * 1000


@pytest.mark.parametrize("method", co.METHODS)
@pytest.mark.parametrize("case", golden_cases("confidence"))
def test_oracle_matches_the_reference_with_repeated_views(case, method):
    """on a clean voxel whose seeing views are S the result is the reference run on S with view v present k_v times
    (tests/golden/make_golden_confidence.py)"""
    d = load_golden("confidence", case)
    r = co.conf_unprojection(d["features"], d["proj"], d["coords"], d["confidence"], d["grad_out"], method, geometry=False)
    ref, gref = d["out_" + method], d["gfeat_" + method]
    clean = np.broadcast_to(d["clean"][:, None], ref.shape)
    fwd, bwd = _err(r["out"][clean], ref[clean]), _err(r["grad_features"], gref)
    print("confidence oracle %s %s: fwd %.3g (bound %.3g), bwd %.3g (bound %.3g)" % (case, method, fwd, _bound(ref), bwd, _bound(gref)))
    assert fwd <= _bound(ref) and bwd <= _bound(gref)


@pytest.mark.parametrize("method", co.METHODS)
def test_oracle_identities(method):
    """a constant map is a per-view weight where the footprint is inside; scaling a sample's maps leaves mean and softmax alone and divides
    their map gradient; zero, negative and NaN pixels make a view absent; an absent view's features are never read"""
    d = load_golden("confidence", "v3c6_nonsquare")
    f, p, c, go = d["features"], d["proj"], d["coords"], d["grad_out"]
    B, V, _, H, W = f.shape
    conf = np.random.default_rng(1).uniform(0.05, 4.0, (B, V, H, W)).astype(np.float32)
    conf[0, 0, :, :W // 2] = 0
    conf[0, 1, 2:6, 12:16] = -1
    conf[0, 1, 3:5, 13:15] = np.nan
    conf[1, 2] = 0
    a = co.conf_unprojection(f, p, c, conf, go, method)
    assert np.isfinite(a["out"]).all() and np.isfinite(a["grad_confidence"]).all() and np.isfinite(a["grad_proj"]).all()
    assert not a["present"][1, 2].any() and not a["grad_features"][1, 2].any() and not a["grad_confidence"][1, 2].any() and not a["grad_proj"][1, 2].any()
    assert not a["grad_confidence"][0, 1, 3:5, 13:15].any()                  # nothing flows into a NaN pixel: every view touching it is absent
    g = f.copy()
    g[1, 2] = np.nan                                                        # an all-zero map: the view's features are never read
    b = co.conf_unprojection(g, p, c, conf, go, method)
    for k in ("out", "grad_confidence", "grad_proj", "grad_coords"):
        assert np.array_equal(a[k], b[k]), k
    if method != "sum":
        s = co.conf_unprojection(f, p, c, conf * np.float32(4), go, method)
        assert _err(s["out"], a["out"]) <= 1e-12 and _err(s["grad_confidence"] * 4, a["grad_confidence"]) <= 1e-10 * np.abs(a["grad_confidence"]).max()
        clean = np.where(np.isnan(conf), 0, conf).astype(np.float64)
        assert np.abs((clean * a["grad_confidence"]).sum((1, 2, 3))).max() <= 1e-10 * np.abs(a["grad_confidence"]).max() * clean.max()


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
    return {k: (zero if k in null else dummy) for k in ("features", "proj", "coords", "mask", "conf", "out", "grad", "gconf")}


def _calls(L, d, ptr, ws=DP(0), wsb=0, only=None, visible=0, family="confidence"):
    """every confidence entry point with its arguments (family: the masked / visible twin, without the map); the pointers are dummies the
    validation never dereferences"""
    zero, a = DP(0), ctypes.byref(d)
    v = (ptr["mask"], ptr["conf"], visible) if family == "confidence" else (ptr["mask"],)
    gk = (ptr["gconf"],) if family == "confidence" else ()
    cub = (ptr["coords"], ptr["coords"], POS, SIDES)
    fn = lambda name: getattr(L, "mvhmr_unproject_%s_%s" % (name, family))          # noqa: E731
    calls = {
        "forward": lambda: fn("forward")(a, ptr["features"], ptr["proj"], ptr["coords"], *v, ptr["out"], ws, wsb, zero),
        "forward_cuboid": lambda: fn("forward_cuboid")(a, ptr["features"], ptr["proj"], *cub, *v, ptr["out"], ws, wsb, zero),
        "backward": lambda: fn("backward")(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], *v, ptr["grad"], ws, wsb, zero),
        "backward_cuboid": lambda: fn("backward_cuboid")(a, ptr["out"], ptr["features"], ptr["proj"], *cub, *v, ptr["grad"], ws, wsb, zero),
        "backward_deterministic": lambda: fn("backward_deterministic")(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], *v, ptr["grad"], ws, wsb, zero),
        "backward_cuboid_deterministic": lambda: fn("backward_cuboid_deterministic")(a, ptr["out"], ptr["features"], ptr["proj"], *cub, *v, ptr["grad"], ws, wsb,
                                                                                     zero),
        "backward_geometry": lambda: fn("backward_geometry")(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], *v, ptr["grad"], ptr["grad"], *gk, ws,
                                                             wsb, zero),
        "backward_geometry_cuboid": lambda: fn("backward_geometry_cuboid")(a, ptr["out"], ptr["features"], ptr["proj"], *cub, *v, ptr["grad"], ptr["grad"],
                                                                           ptr["grad"], *gk, ws, wsb, zero),
    }
    return {k: f() for k, f in calls.items() if only is None or k in only}


def _query(L, name, d, tag="confidence"):
    f = getattr(L, "mvhmr_unproject_%s_%s_workspace_bytes" % (name, tag))
    f.argtypes, f.restype = [ctypes.POINTER(_capi.Desc)], SZ
    return f(ctypes.byref(d))


def test_the_confidence_family_is_exported_and_declared():
    L = _capi.lib()
    for name in NAMES:
        assert "mvhmr_unproject_%s_confidence" % name in _capi.EXPORTS and "mvhmr_unproject_%s_confidence_workspace_bytes" % name in _capi.EXPORTS
        assert hasattr(L, "mvhmr_unproject_%s_confidence" % name) and hasattr(L, "mvhmr_unproject_%s_confidence_workspace_bytes" % name)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mvhmr_unproject.h")).read()
    for name in NAMES:
        assert "mvhmr_unproject_%s_confidence(" % name in header and "mvhmr_unproject_%s_confidence_workspace_bytes(" % name in header
    assert L.mvhmr_abi_version() == 4


def test_confidence_workspace_is_never_less_than_the_masked_or_visible_one_over_the_host_answers_sweep():
    L = _capi.lib()
    served = 0
    for shape, (fd, od), layout, variant, method in itertools.product(mha.SHAPES, mha.STORAGE, mha.LAYOUTS, mha.VARIANTS, mha.METHODS):
        d = mha._desc(shape, method, fd, od, layout, variant)
        for name in NAMES:
            v = _query(L, name, d)
            if method == _capi.AGG["max"]:
                assert v == 0, (shape, name)                                # refused outright: no workspace
                continue
            m, s = _query(L, name, d, "masked"), _query(L, name, d, "visible")
            assert v >= m and v >= s, (shape, fd, od, layout, variant, method, name, v, m, s)
            served += v > 0
    assert served > 700                                                     # the sweep is not one of refusals only


@pytest.mark.parametrize("kw,text", [(dict(feat_layout=_capi.LAYOUT_QUAD), b"confidence maps"), (dict(feat_layout=_capi.LAYOUT_QUAD_LOG2E), b"confidence maps"),
                                     (dict(variant=_capi.VARIANT["brick"]), b"confidence maps"), (dict(method=_capi.AGG["max"]), b"no weighted form")])
def test_quad_layouts_the_brick_variant_and_max_are_unsupported(kw, text):
    L = _capi.lib()
    for ptr in (_ptrs(), _ptrs(("mask",))):                                 # with and without a mask
        for name, rc in _calls(L, _desc(**kw), ptr).items():
            assert rc == _capi.ERR_UNSUPPORTED, (name, kw, rc)
            assert text in L.mvhmr_last_error()
    for name in NAMES:
        assert _query(L, name, _desc(**kw)) == 0


@pytest.mark.parametrize("null", ["features", "proj", "coords", "out"])
def test_null_pointers_are_refused_before_anything_else(null):
    L = _capi.lib()
    for d in (_desc(), _desc(variant=_capi.VARIANT["brick"])):
        for name, rc in _calls(L, d, _ptrs((null,))).items():
            if null == "out" and "geometry" in name:
                continue
            assert rc == _capi.ERR_INVALID_ARGUMENT, (name, null, rc)
    assert _calls(L, _desc(abi_version=3), _ptrs())["forward"] == _capi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("visible", [0, 1])
def test_a_null_map_is_the_masked_or_visible_calls_answer(visible):
    """status and message over a small descriptor sweep, with and without a mask: the call without a map is the masked (visible = 0) or
    the visible (visible = 1) call"""
    L = _capi.lib()
    twin = "visible" if visible else "masked"
    for kw in (dict(), dict(variant=_capi.VARIANT["brick"]), dict(feat_layout=_capi.LAYOUT_QUAD), dict(method=_capi.AGG["max"]),
               dict(channels=6, feat_layout=_capi.LAYOUT_BVHWC), dict(views=17)):      # (every one is answered before a launch)
        for null in (("conf", "gconf"), ("conf", "gconf", "mask"), ("conf", "gconf", "features")):
            for name in NAMES:
                got = _calls(L, _desc(**kw), _ptrs(null), only=(name,), visible=visible)[name]
                said = L.mvhmr_last_error()
                want = _calls(L, _desc(**kw), _ptrs(null), only=(name,), family=twin)[name]
                assert (got, said) == (want, L.mvhmr_last_error()), (kw, null, name)
                assert got != _capi.OK


def test_a_null_mask_is_served_and_the_missing_workspace_is_reported():
    L = _capi.lib()
    for visible in (0, 1):
        for ptr in (_ptrs(), _ptrs(("mask",)), _ptrs(("gconf",))):
            for name, rc in _calls(L, _desc(), ptr, visible=visible).items():
                assert rc == _capi.ERR_WORKSPACE, (name, rc)


def test_geometry_outputs():
    L = _capi.lib()
    geo = ("backward_geometry", "backward_geometry_cuboid")
    for name, rc in _calls(L, _desc(), _ptrs(("grad", "gconf")), only=geo).items():      # every output null
        assert rc == _capi.ERR_INVALID_ARGUMENT and b"grad_confidence are all null: nothing to compute" in L.mvhmr_last_error(), (name, rc)
    for name, rc in _calls(L, _desc(), _ptrs(("grad",)), only=geo).items():               # grad_confidence may be the only output
        assert rc == _capi.ERR_WORKSPACE, (name, rc)
    for name, rc in _calls(L, _desc(), _ptrs(("conf",)), only=geo).items():               # grad_confidence without view_confidence
        assert rc == _capi.ERR_INVALID_ARGUMENT and b"grad_confidence without view_confidence" in L.mvhmr_last_error(), (name, rc)


# ------------------------------------------------------------------------------------ Python
def test_argument_errors():
    f, p, c = torch.zeros(2, 3, 4, 5, 6), torch.zeros(2, 3, 3, 4), torch.zeros(2, 4, 4, 4, 3)
    k = torch.ones(2, 3, 5, 6)
    r, ce = torch.zeros(2, 3, 3), torch.zeros(2, 3)
    cuboid = (r, ce, (0, 0, 0), (1, 1, 1), (4, 4, 4))
    with pytest.raises(ValueError, match="no weighted form"):
        aggregation.unprojection(f, p, c, "max", view_confidence=k)
    with pytest.raises(ValueError, match="no weighted form"):
        aggregation.unprojection_cuboid(f, p, *cuboid, "max", view_confidence=k)
    with pytest.raises(ValueError, match="multiply the maps by the weights"):
        aggregation.unprojection(f, p, c, view_weights=torch.ones(2, 3), view_confidence=k)
    with pytest.raises(ValueError, match="multiply the maps by the weights"):
        aggregation.unprojection_cuboid(f, p, *cuboid, view_weights=torch.ones(2, 3), view_confidence=k)
    with pytest.raises(ValueError, match="visible_only"):                   # the pinned refusal stays
        aggregation.unprojection(f, p, c, view_weights=torch.ones(2, 3), visible_only=True)
    for bad in (torch.ones(2, 3, 6, 5), torch.ones(2, 3), torch.ones(2, 3, 1, 5, 6)):
        with pytest.raises(RuntimeError, match="view_confidence must be"):
            aggregation.unprojection(f, p, c, view_confidence=bad)
    with pytest.raises(TypeError, match="floating"):
        aggregation.unprojection(f, p, c, view_confidence=torch.ones(2, 3, 5, 6, dtype=torch.int32))
    with pytest.raises(TypeError):
        aggregation.unprojection(f, p, c, view_confidence=np.ones((2, 3, 5, 6), np.float32))
    with pytest.raises(TypeError):                                          # keyword-only
        aggregation.unprojection(f, p, c, "softmax", None, "auto", None, None, False, k)
    for kw in (dict(), dict(visible_only=True), dict(view_mask=torch.ones(2, 3, dtype=torch.bool))):
        with pytest.raises(RuntimeError, match="HIP device"):               # no CPU path, as for every other call
            aggregation.unprojection(f, p, c, view_confidence=k, **kw)
        with pytest.raises(RuntimeError, match="HIP device"):
            aggregation.unprojection_cuboid(f, p, *cuboid, view_confidence=k.double(), **kw)


def test_confidence_ops_have_shape_functions():
    """the fake registrations: FakeTensor calls of the confidence families give the shapes of the real ones"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f, p, c = torch.empty(2, 3, 4, 5, 6), torch.empty(2, 3, 3, 4), torch.empty(2, 4, 5, 6, 3)
        m, k = torch.empty(2, 3, dtype=torch.uint8), torch.empty(2, 3, 5, 6)
        for tag in ("", "_visible"):
            ops = torch.ops.mvhmr
            out = getattr(ops, "unprojection_confidence" + tag)(f, p, c, m, k, 0, _capi.F32, 0)
            assert tuple(out.shape) == (2, 4, 4, 5, 6)
            assert tuple(getattr(ops, "unprojection_confidence" + tag)(f, p, c, None, k, 0, _capi.F32, 0).shape) == (2, 4, 4, 5, 6)   # no mask
            assert getattr(ops, "unprojection_confidence%s_backward" % tag)(out, f, p, c, None, k, 0, _capi.F32, 0).shape == f.shape
            g = getattr(ops, "unprojection_confidence%s_backward_deterministic" % tag)(out, f, p, c, m, k, 0, _capi.F32, 0)
            assert g.shape == f.shape
            gp, gc, gk = getattr(ops, "unprojection_confidence%s_backward_geometry" % tag)(out, f, p, c, m, k, 0, _capi.F32, 0, True, False, True)
            assert gp.shape == p.shape and gc.numel() == 0 and gk.shape == k.shape and gk.dtype == torch.float32
            r, ce = torch.empty(2, 3, 3), torch.empty(2, 3)
            out = getattr(ops, "unprojection_cuboid_confidence" + tag)(f, p, r, ce, m, k, [0.0] * 3, [1.0] * 3, [4, 4, 4], 2, _capi.F32, 0)
            assert tuple(out.shape) == (2, 4, 4, 4, 4)
            gp, gr, gce, gk = getattr(ops, "unprojection_cuboid_confidence%s_backward_geometry" % tag)(out, f, p, r, ce, m, k, [0.0] * 3, [1.0] * 3, [4, 4, 4],
                                                                                                      2, _capi.F32, 0, False, True, True, False)
            assert gp.numel() == 0 and gr.shape == r.shape and gce.shape == ce.shape and gk.numel() == 0


def test_shard_batch_dict_slices_the_maps():
    B, V = 6, 3
    batch = dict(images=torch.zeros(B, V, 8, 8, 3), cameras=[[(v, b) for b in range(B)] for v in range(V)], keypoints_3d=list(range(B)),
                 view_confidence=torch.arange(B * V * 4 * 5, dtype=torch.float32).reshape(B, V, 4, 5))
    for rank in range(3):
        part = sharding.shard_batch_dict(batch, world_size=3, rank=rank)
        lo, hi = sharding.shard_bounds(B, 3, rank)
        assert torch.equal(part["view_confidence"], batch["view_confidence"][lo:hi]) and part["images"].shape[0] == hi - lo
    assert "view_confidence" not in sharding.shard_batch_dict({k: v for k, v in batch.items() if k != "view_confidence"}, world_size=3, rank=0)


def test_volume_generator_checks_the_maps_before_anything_runs():
    import unittest.mock as mock
    with mock.patch.object(aggregation.VolumeGenerator, "to", lambda self, *a, **k: self):   # no HIP device here
        gen = aggregation.VolumeGenerator(volume_size=8, input_channels=4, output_channels=4, aggregation_method="max")
    batch = dict(images=torch.empty((2, 3, 32, 32, 3), device="meta"), cameras_packed=dict(K=torch.eye(3).repeat(2, 3, 1, 1).double(),
                                                                                           Rt=torch.eye(3, 4).repeat(2, 3, 1, 1).double()),
                 keypoints_3d=torch.zeros(2, 17, 3), view_confidence=torch.ones(2, 3, 5, 6))
    feats, proj = torch.zeros(2, 3, 4, 5, 6), torch.zeros(2, 3, 3, 4)
    with pytest.raises(ValueError, match="no weighted form"):
        gen(feats, proj, batch)
    gen.aggregation_method = "softmax"
    with pytest.raises(RuntimeError, match="view_confidence must be"):
        gen(feats, proj, dict(batch, view_confidence=torch.ones(2, 3, 6, 5)))
    with pytest.raises(ValueError, match="multiply the maps by the weights"):
        gen(feats, proj, dict(batch, view_weights=torch.ones(2, 3)))
