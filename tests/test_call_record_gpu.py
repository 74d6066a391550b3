"""The call record on the GPU (mvhmr_unproject_*_call): every family's named entry point and the record that spells the same
call, both through raw ctypes on the same inputs, must leave the same bits -- forward, deterministic feature backward and geometry backward
(every family's geometry gradients repeat bitwise from run to run: no float atomics), tensor and cuboid placing.  Tiny shapes: B = 2, V = 3,
C = 4, 8 x 12 maps, an 8^3 volume, fp32, method sum (mean for the moments)."""
import ctypes

import pytest
import torch

import bench
from multiviewhmr_amd import _capi

pytestmark = pytest.mark.gpu

B, V, C, H, W, S = 2, 3, 4, 8, 12, 8
POS = (ctypes.c_double * 3)(-1250.0, -1250.0, -1250.0)
SIDES = (ctypes.c_double * 3)(2500.0, 2500.0, 2500.0)
vp, sz = ctypes.c_void_p, ctypes.c_size_t

# family, then what the case hands over: mask (one absent view in sample 1), weights, maps, visible, index, lens, moments
CASES = {
    "plain": dict(family="plain"),
    "masked": dict(family="masked", mask=True),
    "weighted": dict(family="weighted", mask=True, weights=True),
    "visible": dict(family="visible"),
    "confidence": dict(family="confidence", mask=True, conf=True, visible=1),
    "shared": dict(family="shared", index=[1, 0, 1]),
    "shared null index": dict(family="shared", index=None),                 # the plain call with the gather variant forced
    "lens": dict(family="lens", lens=True),
    "lens null lens": dict(family="lens", lens=False),                      # the plain gather call
    "moments": dict(family="moments", mask=True, visible=1, moments=_capi.MOMENTS_MEANVAR, method="mean"),
}


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _inputs(case, gpu):
    """the device tensors of one case; M volumes (B without an index)"""
    g = torch.Generator().manual_seed(7)
    index = case.get("index")
    M = len(index) if index else B
    t = {"features": torch.randn(B, V, C, H, W, generator=g), "proj": torch.from_numpy(bench.ring_projections(B, V, (H, W))),
         "coords": torch.from_numpy(bench.cuboid_volume(M, S)), "rot": torch.eye(3).repeat(M, 1, 1), "center": torch.zeros(M, 3),
         "grad_out": torch.randn(M, C * (2 if case.get("moments") == _capi.MOMENTS_MEANVAR else 1), S, S, S, generator=g)}
    if case.get("mask"):
        m = torch.ones(B, V, dtype=torch.uint8)
        m[1, 2] = 0
        t["mask"] = m
    if case.get("weights"):
        t["weights"] = torch.rand(B, V, generator=g) + 0.25
    if case.get("conf"):
        t["conf"] = torch.rand(B, V, H, W, generator=g) + 0.05
    if index:
        t["index"] = torch.tensor(index, dtype=torch.int32)
    if case.get("lens"):
        rec = torch.tensor([20.0, 20.0, W / 2, H / 2, 0.05, 0.0, 0.0, 0.0, 0.0, 4.0])    # fx fy cx cy | k1 k2 p1 p2 k3 | r2max
        t["lens"] = rec.repeat(B, V, 1)
    return {k: v.to(gpu).contiguous() for k, v in t.items()}, M


def _middle(case, t, M):
    """the family's arguments behind the placing, as its named entry points take them, and the same as record fields"""
    fam, mask, visible = case["family"], vp(_ptr(t.get("mask"))), case.get("visible", 0)
    fields = dict(view_mask=_ptr(t.get("mask")), view_weights=_ptr(t.get("weights")), view_confidence=_ptr(t.get("conf")),
                  feature_index=_ptr(t.get("index")), lens=_ptr(t.get("lens")), visible=visible, moments=case.get("moments", 0),
                  volumes=M if fam == "shared" else 0)
    args = {"plain": [], "masked": [mask], "weighted": [mask, vp(_ptr(t.get("weights")))], "visible": [mask],
            "confidence": [mask, vp(_ptr(t.get("conf"))), visible], "shared": [M, vp(_ptr(t.get("index"))), vp(0), vp(0), vp(0), 0],
            "lens": [vp(_ptr(t.get("lens"))), vp(0), vp(0), vp(0), 0, vp(0)], "moments": [mask, visible, case.get("moments", 0)]}[fam]
    return args, fields


def _workspace(n, gpu):
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device=gpu)


def _both_ways(L, d, name, fam, kind, lead, place, middle, outs, rec, gpu):
    """one call by its name and once more by its record; outs: {record field: tensor shape}.  Returns the two sets of outputs."""
    sfx = "" if fam == "plain" else "_" + fam
    # (the plain family has five queries: the forward and feature-backward ones serve both placings)
    qname = name.replace("_cuboid", "") if fam == "plain" and not name.startswith("backward_geometry") else name
    q = getattr(L, "mvhmr_unproject_%s%s_workspace_bytes" % (qname, sfx))
    need = q(ctypes.byref(d), *([rec.volumes] if fam == "shared" else []))
    assert need == L.mvhmr_unproject_call_workspace_bytes(ctypes.byref(d), ctypes.byref(rec), kind), (name, fam)
    results = []
    for by_record in (False, True):
        got = {k: torch.full(shape, float("nan"), device=gpu) for k, shape in outs.items()}
        ws = _workspace(need, gpu)
        if by_record:
            for k, v in got.items():
                setattr(rec, k, v.data_ptr())
            fn = getattr(L, "mvhmr_unproject_%s_call" % ("forward" if kind == _capi.CALL_FORWARD else "backward" if kind == _capi.CALL_BACKWARD else "backward_geometry"))
            status = fn(ctypes.byref(d), ctypes.byref(rec), vp(ws.data_ptr() if need else 0), need, vp(0))
        else:
            status = getattr(L, "mvhmr_unproject_%s%s" % (name, sfx))(ctypes.byref(d), *lead, *place, *middle, *[vp(v.data_ptr()) for v in got.values()],
                                                                      vp(ws.data_ptr() if need else 0), sz(need), vp(0))
        assert status == _capi.OK, (name, fam, by_record, L.mvhmr_last_error())
        torch.cuda.synchronize()
        results.append(got)
    return results


@pytest.mark.parametrize("name", list(CASES))
def test_named_call_and_record_leave_the_same_bits(name, gpu):
    case = CASES[name]
    fam = case["family"]
    L = _capi.lib()
    t, M = _inputs(case, gpu)
    d = _capi.Desc(abi_version=_capi.ABI_VERSION, batch=B, views=V, channels=C, feat_h=H, feat_w=W, vol_x=S, vol_y=S, vol_z=S,
                   method=_capi.AGG[case.get("method", "sum")])
    middle, fields = _middle(case, t, M)
    f, p, g = vp(t["features"].data_ptr()), vp(t["proj"].data_ptr()), vp(t["grad_out"].data_ptr())
    halves = t["grad_out"].shape[1] // C
    for cub, placing, place, pf in (
            ("", _capi.PLACING_TENSOR, [vp(t["coords"].data_ptr())], dict(coords=t["coords"].data_ptr())),
            ("_cuboid", _capi.PLACING_CUBOID, [vp(t["rot"].data_ptr()), vp(t["center"].data_ptr()), POS, SIDES],
             dict(rot=t["rot"].data_ptr(), center=t["center"].data_ptr(), position=ctypes.addressof(POS), sides=ctypes.addressof(SIDES)))):
        def rec(**more):
            return _capi.record(fam, placing, features=t["features"].data_ptr(), proj=t["proj"].data_ptr(), **pf, **fields, **more)

        a, b = _both_ways(L, d, "forward" + cub, fam, _capi.CALL_FORWARD, [f, p], place, middle, {"out": (M, C * halves, S, S, S)}, rec(), gpu)
        assert torch.isfinite(a["out"]).all() and a["out"].abs().max() > 0
        assert torch.equal(a["out"], b["out"]), (name, cub, "forward")

        a, b = _both_ways(L, d, "backward%s_deterministic" % cub, fam, _capi.CALL_BACKWARD, [g, f, p], place, middle,
                          {"grad_features": (B, V, C, H, W)}, rec(grad_out=t["grad_out"].data_ptr(), deterministic=1), gpu)
        assert torch.isfinite(a["grad_features"]).all() and a["grad_features"].abs().max() > 0
        assert torch.equal(a["grad_features"], b["grad_features"]), (name, cub, "deterministic backward")

        outs = {"grad_proj": (B, V, 3, 4)}
        outs.update({"grad_rot": (M, 3, 3), "grad_center": (M, 3)} if cub else {"grad_coords": (M, S, S, S, 3)})
        if t.get("weights") is not None:
            outs["grad_weights"] = (B, V)
        if t.get("conf") is not None:
            outs["grad_confidence"] = (B, V, H, W)
        a, b = _both_ways(L, d, "backward_geometry" + cub, fam, _capi.CALL_GEOMETRY, [g, f, p], place, middle, outs,
                          rec(grad_out=t["grad_out"].data_ptr()), gpu)
        for k in outs:
            assert torch.isfinite(a[k]).all(), (name, cub, k)
            assert torch.equal(a[k], b[k]), (name, cub, k)
        assert a["grad_proj"].abs().max() > 0
