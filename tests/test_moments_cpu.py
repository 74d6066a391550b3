"""The cross-view variance aggregates ('var' / 'meanvar', mvhmr_unproject_*_moments) without a GPU: the float64 oracle
(tests/moments_oracle.py) against the goldens combined from the reference's per-view volumes, the C ABI's workspace queries and refusals
of the *_moments entry points through ctypes, the Python argument errors, the fake-tensor shapes of the new ops, VolumeGenerator's
volume_channels, and the premise of the exact lattice rig the GPU file holds to bit equality."""
import ctypes
import itertools
import sys

import numpy as np
import pytest
import torch

import lattice_rig
import moments_oracle as mo
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
MEAN = _capi.AGG["mean"]

# the rig of the bit-equality tests (the issue's arguments, lattice_rig.lattice_problem called directly) and its V = 2 companion
LATTICE = dict(B=3, V=4, C=5, H=13, W=9, vol=(9, 7, 34), seed=73, fmax=2, gmax=2, depths=(2,))
LATTICE_V2 = dict(B=3, V=2, C=5, H=6, W=5, vol=(4, 4, 5), seed=72, fmax=2, gmax=2, depths=(2,), half_steps=False)


def var_bound(eps, D):
    """The project's bar for a sample, propagated through the variance.  Every s_v is off by at most eps = _bound(samples), hence mu by at
    most eps and d_v = s_v - mu by at most 2 eps; d_v^2 is then off by at most 2 |d_v| (2 eps) + (2 eps)^2 <= 4 eps D + 4 eps^2 with
    D = max |s_v - mu|, and so is their mean over the participating views."""
    return 4 * eps * D + 4 * eps * eps


# ------------------------------------------------------------------------------------ the oracle against the reference
def test_the_goldens_sit_on_the_visibility_geometries():
    cases = golden_cases("moments")
    assert cases == golden_cases("visibility") and len(cases) == 3
    import os
    for case in cases:
        d, v = load_golden("moments", case), load_golden("visibility", case)
        for k in ("features", "proj", "coords", "bits"):
            assert np.array_equal(d[k], v[k]), (case, k)
        assert os.path.getsize(os.path.join(GOLDEN, "moments_%s.npz" % case)) <= os.path.getsize(os.path.join(GOLDEN, "visibility_%s.npz" % case))
        assert d["var_plain"].min() >= 0 and d["var_visible"].min() >= 0 and d["var_plain"].max() > 0.1


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("case", golden_cases("moments"))
def test_oracle_reproduces_the_goldens_at_every_voxel(case, visible):
    """the goldens are the reference's own per-view volumes (one `sum` run per view) combined in float64; the oracle samples in float64 at the
    fp32 positions.  Every voxel is compared: the mean to _bound, the variance to the same bar propagated (var_bound)."""
    d = load_golden("moments", case)
    r = mo.moments_unprojection(d["features"], d["proj"], d["coords"], None, "meanvar", visible=visible)
    tag = "visible" if visible else "plain"
    mean, var = d["mean_" + tag], d["var_" + tag]
    C = d["features"].shape[2]
    assert r["out"].shape[1] == 2 * C and np.array_equal(r["out"][:, :C], r["mean"]) and np.array_equal(r["out"][:, C:], r["var"])
    if visible:
        seen = np.stack([(d["bits"].reshape(d["bits"].shape[0], -1) >> v & 1).astype(bool) for v in range(d["features"].shape[1])], 1)
        assert np.array_equal(r["part"], seen)
        nobody = np.broadcast_to((d["bits"] == 0)[:, None], r["mean"].shape)
        assert nobody.any() and not r["mean"][nobody].any() and not r["var"][nobody].any()
    eps = _bound(d["samples"])
    D = max(r["dev_max"], float(np.abs(d["samples"].astype(np.float64)).max()))       # (a bound on max |s_v - mu| that does not lean on the oracle alone)
    e_m, e_v = _err(r["mean"], mean), _err(r["var"], var)
    print("moments oracle %s %s: mean %.3g (bound %.3g), var %.3g (bound %.3g)" % (case, tag, e_m, _bound(mean), e_v, var_bound(eps, D)))
    assert e_m <= _bound(mean) and e_v <= var_bound(eps, D)
    v1 = mo.moments_unprojection(d["features"], d["proj"], d["coords"], None, "var", visible=visible)["out"]
    assert np.array_equal(v1, r["var"])


def test_oracle_edge_counts_and_gradient_identities():
    """n = 1 gives variance exactly 0 and no gradient from g_v; n = 0 gives zeros and exact-zero gradients; the gradient through mu vanishes:
    autograd's ds_v equals (2 g_v / n)(s_v - mu) + g_m / n (the formula the kernels restate)"""
    g = torch.Generator().manual_seed(5)
    S = torch.randn(4, 3, 16, generator=g, dtype=torch.float64).requires_grad_(True)
    part = torch.tensor([[(n >> v) & 1 for n in range(16)] for v in range(4)], dtype=torch.bool)     # every pattern of 4 views
    gm, gv = torch.randn(3, 16, generator=g, dtype=torch.float64), torch.randn(3, 16, generator=g, dtype=torch.float64)
    mu, var = mo.moments(S, part)
    (ds,) = torch.autograd.grad((mu * gm).sum() + (var * gv).sum(), (S,))
    n = part.sum(0).clamp(min=1).double()
    formula = torch.where(part[:, None, :], 2 * gv[None] / n * (S.detach() - mu.detach()[None]) + gm[None] / n, torch.zeros((), dtype=torch.float64))
    assert float((ds - formula).abs().max()) <= 1e-12 * float(formula.abs().max())
    assert not ds[~part[:, None, :].expand_as(ds)].any()
    one = part.sum(0) == 1
    assert one.sum() == 4 and not var.detach()[:, one].any() and not mu.detach()[:, 0].any() and not var.detach()[:, 0].any()
    assert float(var.detach().min()) >= 0


# ------------------------------------------------------------------------------------ the C ABI
def _desc(shape=mha.SHAPES[0], method=MEAN, **kw):
    d = mha._desc(shape, method, _capi.F32, _capi.F32, _capi.LAYOUT_BVCHW, _capi.VARIANT["auto"])
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _ptrs(null=()):
    dummy, zero = DP(256), DP(0)
    return {k: (zero if k in null else dummy) for k in ("features", "proj", "coords", "mask", "out", "grad")}


def _calls(L, d, ptr, visible=0, moments=_capi.MOMENTS_MEANVAR, ws=DP(0), wsb=0, only=None):
    """every moments entry point with its arguments; the pointers are dummies the validation never dereferences"""
    zero, a, m = DP(0), ctypes.byref(d), ptr["mask"]
    cub = (ptr["coords"], ptr["coords"], POS, SIDES)
    tail = (m, visible, moments)
    calls = {
        "forward": lambda: L.mvhmr_unproject_forward_moments(a, ptr["features"], ptr["proj"], ptr["coords"], *tail, ptr["out"], ws, wsb, zero),
        "forward_cuboid": lambda: L.mvhmr_unproject_forward_cuboid_moments(a, ptr["features"], ptr["proj"], *cub, *tail, ptr["out"], ws, wsb, zero),
        "backward": lambda: L.mvhmr_unproject_backward_moments(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], *tail, ptr["grad"], ws, wsb, zero),
        "backward_cuboid": lambda: L.mvhmr_unproject_backward_cuboid_moments(a, ptr["out"], ptr["features"], ptr["proj"], *cub, *tail, ptr["grad"], ws, wsb, zero),
        "backward_deterministic": lambda: L.mvhmr_unproject_backward_deterministic_moments(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], *tail,
                                                                                           ptr["grad"], ws, wsb, zero),
        "backward_cuboid_deterministic": lambda: L.mvhmr_unproject_backward_cuboid_deterministic_moments(a, ptr["out"], ptr["features"], ptr["proj"], *cub, *tail,
                                                                                                         ptr["grad"], ws, wsb, zero),
        "backward_geometry": lambda: L.mvhmr_unproject_backward_geometry_moments(a, ptr["out"], ptr["features"], ptr["proj"], ptr["coords"], *tail, ptr["grad"],
                                                                                 ptr["grad"], ws, wsb, zero),
        "backward_geometry_cuboid": lambda: L.mvhmr_unproject_backward_geometry_cuboid_moments(a, ptr["out"], ptr["features"], ptr["proj"], *cub, *tail,
                                                                                               ptr["grad"], ptr["grad"], ptr["grad"], ws, wsb, zero),
    }
    return {k: f() for k, f in calls.items() if only is None or k in only}


def _query(L, name, d, tag="moments"):
    f = getattr(L, "mvhmr_unproject_%s_%s_workspace_bytes" % (name, tag))
    f.argtypes, f.restype = [ctypes.POINTER(_capi.Desc)], SZ
    return f(ctypes.byref(d))


def test_the_moments_family_is_exported_and_declared():
    L = _capi.lib()
    header = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "mvhmr_unproject.h")).read()
    for name in NAMES:
        for sym in ("mvhmr_unproject_%s_moments" % name, "mvhmr_unproject_%s_moments_workspace_bytes" % name):
            assert sym in _capi.EXPORTS and hasattr(L, sym) and sym + "(" in header, sym
    assert "MVHMR_MOMENTS_VAR = 1" in header and "MVHMR_MOMENTS_MEANVAR = 2" in header
    assert (_capi.MOMENTS_VAR, _capi.MOMENTS_MEANVAR) == (1, 2) and L.mvhmr_abi_version() == 4


@pytest.mark.parametrize("shape", mha.SHAPES[:2], ids=["small", "north_star"])
def test_every_query_and_call_on_the_host_answers_descriptors(shape):
    """every query is positive and covers its visible twin; every call reaches the workspace check (null workspace, and one byte short)"""
    L = _capi.lib()
    d = _desc(shape)
    for name in NAMES:
        q = _query(L, name, d)
        assert q > 0 and q >= _query(L, name, d, "visible") >= _query(L, name, d, "masked"), name
    for visible, moments, ptr in itertools.product((0, 1), (_capi.MOMENTS_VAR, _capi.MOMENTS_MEANVAR), (_ptrs(), _ptrs(("mask",)))):
        for name, rc in _calls(L, d, ptr, visible, moments).items():
            assert rc == _capi.ERR_WORKSPACE and b"workspace is null" in L.mvhmr_last_error(), (name, visible, moments, rc)
        for name, rc in _calls(L, d, ptr, visible, moments, ws=DP(256), wsb=255).items():
            assert rc == _capi.ERR_WORKSPACE and b"are required" in L.mvhmr_last_error(), (name, rc)


def test_moments_workspace_covers_the_visible_one_over_the_host_answers_sweep():
    L = _capi.lib()
    served = 0
    for shape, (fd, od), layout, variant in itertools.product(mha.SHAPES, mha.STORAGE, mha.LAYOUTS, mha.VARIANTS):
        d = mha._desc(shape, MEAN, fd, od, layout, variant)
        for name in NAMES:
            m, v = _query(L, name, d), _query(L, name, d, "visible")
            assert m >= v, (shape, fd, od, layout, variant, name, m, v)
            served += m > 0
    assert served > 250                                                     # the sweep is not one of refusals only


@pytest.mark.parametrize("moments", [0, 3, -1])
def test_an_unknown_moments_value_is_an_invalid_argument(moments):
    L = _capi.lib()
    for name, rc in _calls(L, _desc(), _ptrs(), 1, moments).items():
        assert rc == _capi.ERR_INVALID_ARGUMENT and b"MVHMR_MOMENTS_VAR" in L.mvhmr_last_error(), (name, rc)


@pytest.mark.parametrize("method", ["softmax", "sum", "max"])
def test_the_variance_is_taken_around_the_mean_only(method):
    L = _capi.lib()
    d = _desc(method=_capi.AGG[method])
    for name, rc in _calls(L, d, _ptrs()).items():
        assert rc == _capi.ERR_UNSUPPORTED and b"around the mean" in L.mvhmr_last_error(), (name, rc)
    for name in NAMES:
        assert _query(L, name, d) == 0


@pytest.mark.parametrize("kw", [dict(feat_layout=_capi.LAYOUT_QUAD), dict(feat_layout=_capi.LAYOUT_QUAD_LOG2E), dict(variant=_capi.VARIANT["brick"])])
def test_quad_layouts_and_the_brick_variant_are_unsupported(kw):
    L = _capi.lib()
    for ptr in (_ptrs(), _ptrs(("mask",))):                                 # with and without a mask
        for name, rc in _calls(L, _desc(**kw), ptr).items():
            assert rc == _capi.ERR_UNSUPPORTED, (name, kw, rc)
            assert b"cross-view variance" in L.mvhmr_last_error() and (b"gather kernels" in L.mvhmr_last_error() or b"planar" in L.mvhmr_last_error())
    for name in NAMES:
        assert _query(L, name, _desc(**kw)) == 0


@pytest.mark.parametrize("null", ["features", "proj", "coords", "out"])
def test_null_pointers_are_refused_before_anything_else(null):
    L = _capi.lib()
    for d in (_desc(), _desc(variant=_capi.VARIANT["brick"])):
        for name, rc in _calls(L, d, _ptrs((null,))).items():
            if null == "out" and "geometry" in name:                        # (their outputs are the `grad` pointers)
                continue
            assert rc == _capi.ERR_INVALID_ARGUMENT, (name, null, rc)
    assert _calls(L, _desc(abi_version=3), _ptrs())["forward"] == _capi.ERR_INVALID_ARGUMENT
    f = L.mvhmr_unproject_forward_moments
    assert f(None, DP(256), DP(256), DP(256), DP(0), 0, 2, DP(256), DP(0), 0, DP(0)) == _capi.ERR_INVALID_ARGUMENT       # a null descriptor


def test_geometry_without_any_output_is_invalid():
    L = _capi.lib()
    for name, rc in _calls(L, _desc(), _ptrs(("grad",)), only=("backward_geometry", "backward_geometry_cuboid")).items():
        assert rc == _capi.ERR_INVALID_ARGUMENT and b"nothing to compute" in L.mvhmr_last_error(), (name, rc)


# ------------------------------------------------------------------------------------ Python
def _cpu_args():
    return torch.zeros(2, 3, 4, 5, 5), torch.zeros(2, 3, 3, 4), torch.zeros(2, 4, 4, 4, 3), torch.zeros(2, 3, 3), torch.zeros(2, 3)


@pytest.mark.parametrize("method", ["var", "meanvar"])
def test_the_combinations_that_are_not_built_yet_raise_value_error(method):
    f, p, c, r, ce = _cpu_args()
    options = dict(view_weights=torch.ones(2, 3), view_confidence=torch.ones(2, 3, 5, 5), feature_index=torch.tensor([0, 1]), lens=torch.zeros(2, 3, 10))
    for key, value in options.items():
        with pytest.raises(ValueError, match=r"aggregation_method='%s' with %s is not built yet" % (method, key)):
            aggregation.unprojection(f, p, c, method, **{key: value})
        with pytest.raises(ValueError, match=r"aggregation_method='%s' with %s is not built yet" % (method, key)):
            aggregation.unprojection_cuboid(f, p, r, ce, (0, 0, 0), (1, 1, 1), (4, 4, 4), method, **{key: value})
    # the methods themselves are known: what is refused on the CPU is the device, as for every other call
    for kw in (dict(), dict(visible_only=True), dict(view_mask=torch.ones(2, 3, dtype=torch.bool)), dict(variant="gather")):
        with pytest.raises(RuntimeError, match="HIP device"):
            aggregation.unprojection(f, p, c, method, **kw)
        with pytest.raises(RuntimeError, match="HIP device"):
            aggregation.unprojection_cuboid(f, p, r, ce, (0, 0, 0), (1, 1, 1), (4, 4, 4), method, **kw)


@pytest.mark.parametrize("method", ["median", "variance", "VAR", "mean_var", None, 2])
def test_every_other_name_is_still_unknown(method):
    f, p, c, r, ce = _cpu_args()
    with pytest.raises(ValueError, match="Unknown aggregation_method: %s" % method):
        aggregation.unprojection(f, p, c, method)
    with pytest.raises(ValueError, match="Unknown aggregation_method: %s" % method):
        aggregation.unprojection_cuboid(f, p, r, ce, (0, 0, 0), (1, 1, 1), (4, 4, 4), method)
    with pytest.raises(ValueError, match="Unknown aggregation_method"):    # and beside an option: the name comes first
        aggregation.unprojection(f, p, c, method, visible_only=True)


def test_moments_ops_have_shape_functions():
    """the fake registrations: FakeTensor calls of the moments families give the shapes and dtypes of the real ones"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f, p, c = torch.empty(2, 3, 4, 5, 6), torch.empty(2, 3, 3, 4), torch.empty(2, 4, 5, 6, 3)
        m = torch.empty(2, 3, dtype=torch.uint8)
        for mask in (m, None):
            var = torch.ops.mvhmr.unprojection_moments(f, p, c, mask, True, 1, MEAN, _capi.F32, 0)
            both = torch.ops.mvhmr.unprojection_moments(f, p, c, mask, False, 2, MEAN, _capi.BF16, 0)
            assert tuple(var.shape) == (2, 4, 4, 5, 6) and var.dtype == torch.float32
            assert tuple(both.shape) == (2, 8, 4, 5, 6) and both.dtype == torch.bfloat16
            for op in (torch.ops.mvhmr.unprojection_moments_backward, torch.ops.mvhmr.unprojection_moments_backward_deterministic):
                g = op(both, f, p, c, mask, False, 2, MEAN, _capi.BF16, 0)
                assert g.shape == f.shape and g.dtype == f.dtype            # the feature gradient has C channels
            gp, gc = torch.ops.mvhmr.unprojection_moments_backward_geometry(both, f, p, c, mask, False, 2, MEAN, _capi.BF16, 0, True, False)
            assert gp.shape == p.shape and gp.dtype == torch.float32 and gc.numel() == 0
        r, ce = torch.empty(2, 3, 3), torch.empty(2, 3)
        out = torch.ops.mvhmr.unprojection_cuboid_moments(f.half(), p, r, ce, m, [0.0] * 3, [1.0] * 3, [4, 4, 4], True, 2, MEAN, _capi.F16, 0)
        assert tuple(out.shape) == (2, 8, 4, 4, 4) and out.dtype == torch.float16
        gp, gr, gce = torch.ops.mvhmr.unprojection_cuboid_moments_backward_geometry(out, f.half(), p, r, ce, m, [0.0] * 3, [1.0] * 3, [4, 4, 4], True, 2, MEAN,
                                                                                    _capi.F16, 0, False, True, True)
        assert gp.numel() == 0 and gr.shape == r.shape and gce.shape == ce.shape


def test_volume_generator_reports_its_volume_channels():
    import unittest.mock as mock
    with mock.patch.object(aggregation.VolumeGenerator, "to", lambda self, *a, **k: self):   # no HIP device here
        for method, channels in (("softmax", 8), ("mean", 8), ("var", 8), ("meanvar", 16)):
            gen = aggregation.VolumeGenerator(volume_size=8, input_channels=4, output_channels=8, aggregation_method=method)
            assert gen.volume_channels == channels and gen.aggregation_method == method
            with pytest.raises(AttributeError):
                gen.volume_channels = 3                                     # read-only
        assert aggregation.VolumeGenerator(volume_size=8, input_channels=4).volume_channels == 32
        gen = aggregation.VolumeGenerator(volume_size=8, input_channels=4, output_channels=8, aggregation_method="meanvar")
        assert sorted(gen.state_dict()) == ["process_feature.0.bias", "process_feature.0.weight"]           # the reference's checkpoint keys, nothing more


# ------------------------------------------------------------------------------------ the premise of the exact lattice rig
def lattice_mask(B, V):
    """sample 0 full, sample 1 a single view, sample 2 empty (lattice_rig's own masks)"""
    mask = np.ones((B, V), np.uint8)
    mask[1] = 0
    mask[1, 1] = 1
    mask[2] = 0
    return mask


def lattice_cases(B, V):
    return (("plain", dict()), ("mask", dict(view_mask=lattice_mask(B, V))), ("visible", dict(visible_only=True)))


def lattice_reference(cfg, method, kw):
    """-> (the rig's arrays, grad_out as the test must feed it (zero where not compared), the oracle's dict); budgets asserted"""
    feats, proj, coords, grad = lattice_rig.lattice_problem(**cfg)
    C = feats.shape[2]
    if method == "meanvar":                                                  # the second half: the rig's own grad_out, its channels in reverse
        grad = np.concatenate([grad, grad[:, ::-1]], 1)
    cmp_ = mo.lattice_moments(feats, proj, coords, None, method, **kw)["compared"]
    grad = np.where(cmp_[:, None], grad, np.float32(0)).astype(np.float32)
    res = mo.lattice_moments(feats, proj, coords, grad, method, **kw)
    assert grad.shape[1] == (2 * C if method == "meanvar" else C)
    lattice_rig.assert_budget(res, "moments %s" % method)
    return (feats, proj, coords), grad, res


@pytest.mark.parametrize("method", ["var", "meanvar"])
@pytest.mark.parametrize("cfg", [LATTICE, LATTICE_V2], ids=["v4", "v2"])
def test_lattice_premise(cfg, method):
    """The budgets, forward and backward, stay below 2^24 (lattice_rig.assert_budget), every count 0 ... V occurs under visible_only, and at
    least half of the voxels are compared there (n a power of two); in the plain mode every voxel is."""
    V = cfg["V"]
    for tag, kw in lattice_cases(cfg["B"], V):
        _, grad, res = lattice_reference(cfg, method, kw)
        print("lattice %s V%d %s: fwd budget %.4g * 2^24, bwd budget %.4g * 2^24, compared %.3f, counts %s"
              % (method, V, tag, res["fwd_budget"] / lattice_rig.LIMIT, res["bwd_budget"] / lattice_rig.LIMIT, res["compared"].mean(),
                 np.bincount(res["count"].ravel(), minlength=V + 1).tolist()))
        assert res["fwd_budget"] < lattice_rig.LIMIT and res["bwd_budget"] < lattice_rig.LIMIT
        assert np.abs(res["grad_features"]).max() > 0 and res["out"].min() >= 0 if method == "var" else True
        if tag == "plain":
            assert res["compared"].all() and (res["count"] == V).all()
        if tag == "visible":
            assert (np.bincount(res["count"].ravel(), minlength=V + 1) > 0).all()
            assert res["compared"].mean() >= 0.5
        if tag == "mask":
            assert sorted(set(res["count"].ravel().tolist())) == [0, 1, V]
        assert not grad[np.broadcast_to(~res["compared"][:, None], grad.shape)].any()


def test_lattice_fp32_emulation_of_the_pinned_order_carries_the_float64_bits():
    """a numpy fp32 restatement of the pinned arithmetic (acc = 0; acc += s_v in view order; / n; d = s - mu; acc = fma(d, d, acc); / n --
    the fma emulated in float64 and rounded once) on the rig's exact samples equals the float64 oracle cast once, wherever n is a power of two"""
    feats, proj, coords, _ = lattice_rig.lattice_problem(**LATTICE)
    B, V, C, H, W = feats.shape
    N = int(np.prod(coords.shape[1:4]))
    for tag, kw in lattice_cases(B, V):
        ref = mo.lattice_moments(feats, proj, coords, None, "meanvar", **kw)
        cmp_ = np.broadcast_to(ref["compared"].reshape(B, 1, N), (B, C, N))
        for b in range(B):
            pts = coords[b].reshape(-1, 3)
            T = [lattice_rig.taps64(proj[b, v], pts, H, W) for v in range(V)]
            S = [np.float32(sum(feats[b, v].reshape(C, H * W).astype(np.float64)[:, T[v]["off"][k]] * T[v]["w"][k][None] for k in range(4))) for v in range(V)]
            P = []
            for v in range(V):
                t = T[v]
                seen = (t["z"] > 0) & (t["ix"] >= 0) & (t["ix"] <= W - 1) & (t["iy"] >= 0) & (t["iy"] <= H - 1)
                present = np.full(N, True if "view_mask" not in kw else bool(kw["view_mask"][b, v]))
                P.append(present & (seen if kw.get("visible_only") else True))
            n = np.float32(np.maximum(np.sum(P, 0), 1))
            acc = np.zeros((C, N), np.float32)
            for v in range(V):
                acc = np.where(P[v][None], acc + S[v], acc).astype(np.float32)
            mu = (acc / n[None]).astype(np.float32)
            acc = np.zeros((C, N), np.float32)
            for v in range(V):
                d = (S[v] - mu).astype(np.float32)
                acc = np.where(P[v][None], np.float32(d.astype(np.float64) * d.astype(np.float64) + acc.astype(np.float64)), acc)
            var = (acc / n[None]).astype(np.float32)
            want = ref["out"][b].reshape(2 * C, N).astype(np.float32)
            assert np.array_equal(mu[cmp_[b]], want[:C][cmp_[b]]) and np.array_equal(var[cmp_[b]], want[C:][cmp_[b]]), (tag, b)


# ------------------------------------------------------------------------------------ the lattice case's geometry gradients
# the same construction on power-of-two maps, on which kx = (W - 1) / H and ky = (H - 1) / W are dyadic (lattice_rig.GEO_RIGS)
LATTICE_GEO = dict(B=3, V=4, C=5, H=8, W=8, vol=(3, 4, 5), seed=74, fmax=1, gmax=1, depths=(2,))   # (5, 4, 7) or fmax = 2 break grad_proj's budget


def lattice_geometry_reference(method, kw, cfg=LATTICE_GEO):
    """-> (the rig's arrays, grad_out as the test must feed it, lattice_rig.geo_oracle's dict) for 'var' / 'meanvar' at the voxels whose
    participating count n is a power of two (grad_out is zero elsewhere).  ds is restated from the README's definition in float64 --
    var = (1 / n) sum_S (s_v - mu)^2, so ds_v = (2 g_v / n)(s_v - mu) + g_m / n for v in S, 0 outside -- on lattice_rig.geotaps64's samples
    and handed to the geometry oracle; S = every view (a view that misses the map takes part with its sample of zero), the present ones
    under view_mask, the seeing ones under visible_only.  The geometry budget is asserted."""
    (feats, proj, coords), grad, res = lattice_reference(cfg, method, kw)
    B, V, C, H, W = feats.shape
    N = int(np.prod(coords.shape[1:4]))
    g = grad.reshape(B, -1, N).astype(np.float64)
    g_m, g_v = (g[:, :C], g[:, C:]) if method == "meanvar" else (np.zeros((B, C, N)), g)
    ds = np.zeros((B, V, C, N))
    for b in range(B):
        T = [lattice_rig.geotaps64(proj[b, v], coords[b].reshape(-1, 3), feats[b, v].reshape(C, H * W), H, W) for v in range(V)]
        part = np.stack([np.full(N, True if "view_mask" not in kw else bool(kw["view_mask"][b, v])) & (T[v]["seen"] if kw.get("visible_only") else True)
                         for v in range(V)])
        n = part.sum(0)
        assert np.array_equal(n, res["count"][b].ravel())
        S = np.stack([t["s"] for t in T])
        mu = np.where(part[:, None], S, 0.0).sum(0) / np.maximum(n, 1)
        ds[b] = np.where(part[:, None], (2 * g_v[b] / np.maximum(n, 1))[None] * (S - mu[None]) + (g_m[b] / np.maximum(n, 1))[None], 0.0)
    geo = lattice_rig.geo_oracle(feats, proj, coords, None, "given", ds=ds)
    lattice_rig.assert_geo_budget(geo, "moments geometry %s" % method)
    return (feats, proj, coords), grad, geo


@pytest.mark.parametrize("method", ["var", "meanvar"])
def test_lattice_geometry_premise(method):
    """budget < 2^24, and the float64 restatement equals tests/moments_oracle.py's independent autograd oracle exactly on the rig"""
    for tag, kw in lattice_cases(LATTICE_GEO["B"], LATTICE_GEO["V"]):
        (feats, proj, coords), grad, geo = lattice_geometry_reference(method, kw)
        assert 0 < geo["geo_budget"] < lattice_rig.LIMIT
        ref = mo.moments_unprojection(feats, proj, coords, grad, method, mask=kw.get("view_mask"), visible=kw.get("visible_only", False))
        assert np.array_equal(ref["grad_proj"], geo["grad_proj"]) and np.array_equal(ref["grad_coords"], geo["grad_coords"]), (tag, method)
        assert (geo["grad_coords"] != 0).mean() >= (0.1 if tag == "mask" else 0.3) and (geo["grad_proj"] != 0).any(), (tag, method)
