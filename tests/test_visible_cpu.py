"""Visibility-aware aggregation (unprojection(visible_only=True), mvhmr_unproject_*_visible) without a GPU: the float64
oracle (tests/visibility_oracle.py) against the reference's goldens stitched from per-pattern runs, its gradient columns against
autograd, the C ABI's workspace queries and refusals of the *_visible entry points through ctypes, and the Python argument errors and
cfg wiring."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import visibility_oracle as vis
from conftest import GOLDEN, golden_cases, load_golden
from multiviewhmr_amd import _capi, aggregation
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
    cases = golden_cases("visibility")
    assert len(cases) == 3
    for case in cases:
        d = load_golden("visibility", case)
        V = d["features"].shape[1]
        counts = np.bincount(np.array([bin(int(x)).count("1") for x in d["bits"].ravel()]), minlength=V + 1)
        if V in (3, 4):
            assert (counts > 0).all(), (case, counts)                       # every count 0 ... V occurs
        assert os.path.getsize(os.path.join(GOLDEN, "visibility_%s.npz" % case)) < 500 * 1000
    d = load_golden("visibility", "v8c4_behind")
    z = np.einsum("bvj,bnj->bvn", d["proj"][:, :, 2, :3].astype(np.float64), d["coords"].reshape(2, -1, 3).astype(np.float64)) + d["proj"][:, :, 2, 3:4]
    assert (z <= 0).mean() > 0.01                                           # voxel-views behind a camera


@pytest.mark.parametrize("method", vis.METHODS)
@pytest.mark.parametrize("case", golden_cases("visibility"))
def test_oracle_matches_the_reference_on_the_seeing_views(case, method):
    """on the voxels whose seeing views are S the result is the reference run on views S alone (tests/golden/make_golden_visibility.py)"""
    d = load_golden("visibility", case)
    r = vis.visible_unprojection(d["features"], d["proj"], d["coords"], d["grad_out"], method, geometry=False)
    assert np.array_equal(r["bits"], d["bits"]) and r["bits"].dtype == np.int32
    H, W = d["features"].shape[3:]
    assert np.array_equal(vis.visibility_bits(d["proj"], d["coords"], H, W), d["bits"])
    ref, gref = d["out_" + method], d["gfeat_" + method]
    fwd, bwd = _err(r["out"], ref), _err(r["grad_features"], gref)
    print("visibility oracle %s %s: fwd %.3g (bound %.3g), bwd %.3g (bound %.3g)" % (case, method, fwd, _bound(ref), bwd, _bound(gref)))
    assert fwd <= _bound(ref) and bwd <= _bound(gref)
    unseen = d["bits"] == 0
    assert unseen.any() and not r["out"][np.broadcast_to(unseen[:, None], r["out"].shape)].any()


@pytest.mark.parametrize("method", vis.METHODS)
def test_oracle_gradient_column_agrees_with_autograd(method):
    """the ds_v column of the table (seen_agg_grad) against float64 autograd through the `out` column, slot 0 absent for some voxels and a
    voxel nobody sees among them"""
    g = torch.Generator().manual_seed(5)
    S = torch.randn(4, 3, 16, generator=g, dtype=torch.float64).requires_grad_(True)
    seen = torch.tensor([[(n >> v) & 1 for n in range(16)] for v in range(4)], dtype=torch.bool)     # every pattern of 4 views
    go = torch.randn(3, 16, generator=g, dtype=torch.float64)
    (gs,) = torch.autograd.grad((vis.seen_out(S, seen, method) * go).sum(), (S,))
    ds = vis.seen_agg_grad(S.detach(), seen, go, method)
    assert float((ds - gs).abs().max()) <= 1e-12 * float(gs.abs().max())
    assert not ds[~seen[:, None, :].expand_as(ds)].any() and not vis.seen_out(S, seen, method)[:, 0].any()


def test_oracle_is_the_plain_oracle_where_every_view_sees_every_voxel():
    """geometry gradients: on a problem every view sees entirely, the visible oracle is geomgrad_oracle's (the existing chain rule)"""
    import geomgrad_oracle as go_
    d = load_golden("visibility", "v4c5")
    coords = (d["coords"] * np.float32(0.25)).astype(np.float32)
    r = vis.visible_unprojection(d["features"], d["proj"], coords, d["grad_out"], "softmax")
    assert (r["bits"] == 15).all()
    gp, gc = go_.geometry_grad(d["features"], d["proj"], coords, d["grad_out"], "softmax")
    assert _err(r["grad_proj"], gp) <= 1e-9 * np.abs(gp).max() and _err(r["grad_coords"], gc) <= 1e-9 * np.abs(gc).max()


def test_oracle_never_reads_what_only_unseen_views_tap():
    d = load_golden("visibility", "v4c5")
    f = d["features"].copy()
    a = vis.visible_unprojection(f, d["proj"], d["coords"], d["grad_out"], "softmax")
    untouched = a["grad_features"] == 0
    mean = vis.visible_unprojection(f, d["proj"], d["coords"], np.ones_like(d["grad_out"]), "sum", geometry=False)["grad_features"]
    untapped = mean == 0                                                    # pixels no seeing voxel-view taps (sum, g = 1: every tap weight adds up)
    assert untapped.any() and untouched[untapped].all()
    f[untapped] = np.nan
    b = vis.visible_unprojection(f, d["proj"], d["coords"], d["grad_out"], "softmax")
    for k in ("out", "grad_proj", "grad_coords"):
        assert np.isfinite(b[k]).all() and np.array_equal(a[k], b[k]), k


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
    return {k: (zero if k in null else dummy) for k in ("features", "proj", "coords", "mask", "out", "grad", "bits")}


def _calls(L, d, ptr, ws=DP(0), wsb=0, only=None):
    """every visible entry point with its arguments; the pointers are dummies the validation never dereferences"""
    zero, a, m = DP(0), ctypes.byref(d), ptr["mask"]
    cub = (ptr["coords"], ptr["coords"], POS, SIDES)
    calls = {
        "forward": lambda: L.mvhmr_unproject_forward_visible(a, ptr["features"], ptr["proj"], ptr["coords"], m, ptr["out"], ws, wsb, zero),
        "forward_cuboid": lambda: L.mvhmr_unproject_forward_cuboid_visible(a, ptr["features"], ptr["proj"], *cub, m, ptr["out"], ws, wsb, zero),
        "backward": lambda: L.mvhmr_unproject_backward_visible(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], m, ptr["grad"], ws, wsb, zero),
        "backward_cuboid": lambda: L.mvhmr_unproject_backward_cuboid_visible(a, ptr["out"], ptr["features"], ptr["proj"], *cub, m, ptr["grad"], ws, wsb, zero),
        "backward_deterministic": lambda: L.mvhmr_unproject_backward_deterministic_visible(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], m,
                                                                                           ptr["grad"], ws, wsb, zero),
        "backward_cuboid_deterministic": lambda: L.mvhmr_unproject_backward_cuboid_deterministic_visible(a, ptr["out"], ptr["features"], ptr["proj"], *cub, m,
                                                                                                         ptr["grad"], ws, wsb, zero),
        "backward_geometry": lambda: L.mvhmr_unproject_backward_geometry_visible(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], m, ptr["grad"],
                                                                                 ptr["grad"], ws, wsb, zero),
        "backward_geometry_cuboid": lambda: L.mvhmr_unproject_backward_geometry_cuboid_visible(a, ptr["out"], ptr["features"], ptr["proj"], *cub, m,
                                                                                               ptr["grad"], ptr["grad"], ptr["grad"], ws, wsb, zero),
        "visibility": lambda: L.mvhmr_unproject_visibility(a, ptr["proj"], ptr["coords"], m, ptr["bits"], zero),
        "visibility_cuboid": lambda: L.mvhmr_unproject_visibility_cuboid(a, ptr["proj"], *cub, m, ptr["bits"], zero),
    }
    return {k: f() for k, f in calls.items() if only is None or k in only}


def _query(L, name, d, tag="visible"):
    f = getattr(L, "mvhmr_unproject_%s_%s_workspace_bytes" % (name, tag))
    f.argtypes, f.restype = [ctypes.POINTER(_capi.Desc)], SZ
    return f(ctypes.byref(d))


def test_the_visible_family_is_exported_and_declared():
    L = _capi.lib()
    for name in NAMES:
        assert "mvhmr_unproject_%s_visible" % name in _capi.EXPORTS and "mvhmr_unproject_%s_visible_workspace_bytes" % name in _capi.EXPORTS
        assert hasattr(L, "mvhmr_unproject_%s_visible" % name) and hasattr(L, "mvhmr_unproject_%s_visible_workspace_bytes" % name)
    for name in ("mvhmr_unproject_visibility", "mvhmr_unproject_visibility_cuboid"):
        assert name in _capi.EXPORTS and hasattr(L, name)
    assert L.mvhmr_abi_version() == 4


def test_visible_workspace_is_never_less_than_the_masked_one_over_the_host_answers_sweep():
    L = _capi.lib()
    served = 0
    for shape, (fd, od), layout, variant, method in itertools.product(mha.SHAPES, mha.STORAGE, mha.LAYOUTS, mha.VARIANTS, mha.METHODS):
        d = mha._desc(shape, method, fd, od, layout, variant)
        for name in NAMES:
            v, m = _query(L, name, d), _query(L, name, d, "masked")
            assert v >= m, (shape, fd, od, layout, variant, method, name, v, m)
            served += v > 0
    assert served > 1000                                                    # the sweep is not one of refusals only


@pytest.mark.parametrize("kw", [dict(feat_layout=_capi.LAYOUT_QUAD), dict(feat_layout=_capi.LAYOUT_QUAD_LOG2E), dict(variant=_capi.VARIANT["brick"])])
def test_quad_layouts_and_the_brick_variant_are_unsupported(kw):
    L = _capi.lib()
    for ptr in (_ptrs(), _ptrs(("mask",))):                                 # with and without a mask
        for name, rc in _calls(L, _desc(**kw), ptr).items():
            assert rc == _capi.ERR_UNSUPPORTED, (name, kw, rc)
            assert b"visibility-aware" in L.mvhmr_last_error()
    for name in NAMES:
        assert _query(L, name, _desc(**kw)) == 0


@pytest.mark.parametrize("null", ["features", "proj", "coords", "out", "bits"])
def test_null_pointers_are_refused_before_anything_else(null):
    """also on a descriptor the call would refuse for its variant: the pointers come first"""
    L = _capi.lib()
    for d in (_desc(), _desc(variant=_capi.VARIANT["brick"])):
        for name, rc in _calls(L, d, _ptrs((null,))).items():
            uses = {"features": "visibility" not in name, "out": "visibility" not in name and "geometry" not in name, "bits": "visibility" in name}
            if not uses.get(null, True):
                continue
            assert rc == _capi.ERR_INVALID_ARGUMENT, (name, null, rc)
    assert _calls(L, _desc(abi_version=3), _ptrs())["forward"] == _capi.ERR_INVALID_ARGUMENT
    f = L.mvhmr_unproject_forward_visible
    assert f(None, DP(256), DP(256), DP(256), DP(0), DP(256), DP(0), 0, DP(0)) == _capi.ERR_INVALID_ARGUMENT       # a null descriptor


def test_a_null_mask_is_served_and_the_missing_workspace_is_reported():
    L = _capi.lib()
    for ptr in (_ptrs(), _ptrs(("mask",))):
        for name, rc in _calls(L, _desc(), ptr, only=NAMES).items():
            assert rc == _capi.ERR_WORKSPACE, (name, rc)


def test_geometry_without_any_output_is_invalid():
    L = _capi.lib()
    for name, rc in _calls(L, _desc(), _ptrs(("grad",)), only=("backward_geometry", "backward_geometry_cuboid")).items():
        assert rc == _capi.ERR_INVALID_ARGUMENT and b"nothing to compute" in L.mvhmr_last_error(), (name, rc)


# ------------------------------------------------------------------------------------ Python
def test_visible_only_with_view_weights_raises_value_error():
    f, p, c = torch.zeros(2, 3, 4, 5, 5), torch.zeros(2, 3, 3, 4), torch.zeros(2, 4, 4, 4, 3)
    with pytest.raises(ValueError, match="visible_only"):
        aggregation.unprojection(f, p, c, view_weights=torch.ones(2, 3), visible_only=True)
    r, ce = torch.zeros(2, 3, 3), torch.zeros(2, 3)
    with pytest.raises(ValueError, match="visible_only"):
        aggregation.unprojection_cuboid(f, p, r, ce, (0, 0, 0), (1, 1, 1), (4, 4, 4), view_weights=torch.ones(2, 3), visible_only=True)
    with pytest.raises(TypeError):                                          # keyword-only
        aggregation.unprojection(f, p, c, "softmax", True)
    with pytest.raises(RuntimeError, match="HIP device"):                   # no CPU path, as for every other call
        aggregation.unprojection(f, p, c, visible_only=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        aggregation.view_visibility(p, c, (5, 5))
    with pytest.raises(RuntimeError):
        aggregation.view_visibility(torch.zeros(2, 3, 4, 4), c, (5, 5))


class _Node(dict):
    __getattr__ = dict.__getitem__


def test_build_volume_generator_reads_visible_only_when_the_cfg_has_it():
    import unittest.mock as mock

    def cfg(**agg):
        return _Node(MODEL=_Node(BACKBONE=_Node(DECONV_FILTERS=[256, 256, 64], DECONV_LAYERS=3),
                                 AGGREGATION=_Node(VOLUME_SIZE=16, OUTPUT_CHANNELS=8, CUBOID_SIDE=2000.0, USE_TRIANGULATION=False, METHOD="mean", **agg)),
                     DATASET=_Node(KIND="coco", TYPE="human36m"))
    with mock.patch.object(aggregation.VolumeGenerator, "to", lambda self, *a, **k: self):   # no HIP device here
        assert aggregation.build_volume_generator(cfg()).visible_only is False
        assert aggregation.build_volume_generator(cfg(VISIBLE_ONLY=True)).visible_only is True
        assert aggregation.build_volume_generator(cfg(VISIBLE_ONLY=False)).visible_only is False
        assert aggregation.VolumeGenerator(volume_size=8, input_channels=4, output_channels=4).visible_only is False
        assert aggregation.VolumeGenerator(volume_size=8, input_channels=4, output_channels=4, visible_only=True).visible_only is True


def test_visible_ops_have_shape_functions():
    """the fake registrations: FakeTensor calls of the visible families give the shapes of the real ones"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f, p, c = torch.empty(2, 3, 4, 5, 6), torch.empty(2, 3, 3, 4), torch.empty(2, 4, 5, 6, 3)
        m = torch.empty(2, 3, dtype=torch.uint8)
        out = torch.ops.mvhmr.unprojection_visible(f, p, c, m, 0, _capi.F32, 0)
        assert tuple(out.shape) == (2, 4, 4, 5, 6)
        g = torch.ops.mvhmr.unprojection_visible_backward_deterministic(out, f, p, c, m, 0, _capi.F32, 0)
        assert g.shape == f.shape
        gp, gc = torch.ops.mvhmr.unprojection_visible_backward_geometry(out, f, p, c, m, 0, _capi.F32, 0, True, False)
        assert gp.shape == p.shape and gc.numel() == 0
        r, ce = torch.empty(2, 3, 3), torch.empty(2, 3)
        out = torch.ops.mvhmr.unprojection_cuboid_visible(f, p, r, ce, m, [0.0] * 3, [1.0] * 3, [4, 4, 4], 2, _capi.F32, 0)
        assert tuple(out.shape) == (2, 4, 4, 4, 4)
