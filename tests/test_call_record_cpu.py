"""The call record without a GPU (mvhmr_unproject_call, mvhmr_unproject_*_call): every named entry point is a shim over the
record, so for every family x placing x kind the record's workspace query must answer what the named query answers, and where a call is
refused before any launch -- descriptor, null pointers, the family's own refusals, the workspace check -- status and text must be the
same by either way in.  Nothing is launched: every launching call here is one the library refuses."""
import ctypes
import itertools

import pytest

from multiviewhmr_amd import _capi

DP = ctypes.c_void_p
POS = (ctypes.c_double * 3)(-1.0, -1.0, -1.0)
SIDES = (ctypes.c_double * 3)(2.0, 2.0, 2.0)
DUMMY = 256                                                # a pointer the validation never dereferences
KINDS = (("forward", _capi.CALL_FORWARD, 0), ("backward", _capi.CALL_BACKWARD, 0), ("backward deterministic", _capi.CALL_BACKWARD, 1),
         ("geometry", _capi.CALL_GEOMETRY, 0))
FAMILIES = tuple(_capi.FAMILY)


def _desc(volumes, **kw):
    d = _capi.Desc(abi_version=_capi.ABI_VERSION, batch=2, views=4, channels=4, feat_h=24, feat_w=20, vol_x=8, vol_y=6, vol_z=5)
    for k, v in kw.items():
        setattr(d, k, v)
    return d, volumes


# the four methods, C = 4 and 5, the planar / channels-last / quad layouts, AUTO / GATHER / BRICK, `volumes` of 1, 3 and 65536; the large
# volume is the shape whose AUTO forward is gated (both variants planned)
DESCS = {
    "softmax planar auto": _desc(1, method=_capi.AGG["softmax"]),
    "sum c5 planar gather": _desc(3, method=_capi.AGG["sum"], channels=5, variant=_capi.VARIANT["gather"]),
    "mean channels-last auto": _desc(3, method=_capi.AGG["mean"], feat_layout=_capi.LAYOUT_BVHWC),
    "max quad auto": _desc(1, method=_capi.AGG["max"], feat_layout=_capi.LAYOUT_QUAD),
    "mean planar brick": _desc(3, method=_capi.AGG["mean"], variant=_capi.VARIANT["brick"]),
    "softmax c32 planar auto 64^3": _desc(65536, method=_capi.AGG["softmax"], channels=32, vol_x=64, vol_y=64, vol_z=64),
    "sum c5 channels-last": _desc(2, method=_capi.AGG["sum"], channels=5, feat_layout=_capi.LAYOUT_BVHWC),
}
# what the family's own arguments hold: everything it takes, nothing (the degradations), or a selection it carries only to refuse
FILLS = ("full", "null", "refused")


def _named(family, placing, kind_name):
    cub = "_cuboid" if placing == _capi.PLACING_CUBOID else ""
    stem = {"forward": "forward" + cub, "backward": "backward" + cub, "backward deterministic": "backward%s_deterministic" % cub,
            "geometry": "backward_geometry" + cub}[kind_name]
    return "mvhmr_unproject_" + stem + ("" if family == "plain" else "_" + family)


def _named_query(L, family, placing, kind_name):
    if family == "plain":                                   # five queries: the forward and feature-backward ones serve both placings
        name = _named(family, placing if kind_name == "geometry" else _capi.PLACING_TENSOR, kind_name)
    else:
        name = _named(family, placing, kind_name)
    return getattr(L, name + "_workspace_bytes")


def _fields(family, fill, volumes):
    """the record's optional inputs, and the same as the arguments behind the placing of the family's named entry points"""
    on = DUMMY if fill != "null" else 0
    stray = DUMMY if fill == "refused" else 0
    f = dict(view_mask=0, view_weights=0, view_confidence=0, visible=0, feature_index=0, lens=0, moments=0, volumes=0)
    if family in ("masked", "weighted", "visible", "confidence", "moments"):
        f["view_mask"] = on
    if family == "weighted":
        f["view_weights"] = on
    if family == "confidence":
        f.update(view_confidence=on, visible=1 if on else 0)
    if family == "moments":
        f.update(visible=1 if on else 0, moments=_capi.MOMENTS_MEANVAR if on else 0)
    if family == "shared":
        f.update(volumes=volumes, feature_index=on, view_mask=stray)
    if family == "lens":
        f.update(lens=on, feature_index=stray)
    p = lambda k: DP(f[k])                                  # noqa: E731
    args = {"plain": [], "masked": [p("view_mask")], "weighted": [p("view_mask"), p("view_weights")], "visible": [p("view_mask")],
            "confidence": [p("view_mask"), p("view_confidence"), f["visible"]],
            "shared": [f["volumes"], p("feature_index"), p("view_mask"), p("view_weights"), p("view_confidence"), f["visible"]],
            "lens": [p("lens"), p("view_mask"), p("view_weights"), p("view_confidence"), f["visible"], p("feature_index")],
            "moments": [p("view_mask"), f["visible"], f["moments"]]}[family]
    return f, args


def _sentinel(L):
    """leaves a known text in mvhmr_last_error(): a query that refuses says why there, one that answers leaves it alone"""
    assert L.mvhmr_unproject_call_workspace_bytes(None, None, 0) == 0
    return L.mvhmr_last_error()


def _launch_both(L, d, family, placing, kind_name, kind, det, fields, args, null_features):
    """the named launching entry point and the record, dummy pointers, no workspace -> [(status, text)] * 2"""
    feat = 0 if null_features else DUMMY
    place_args = [DP(DUMMY), DP(DUMMY), POS, SIDES] if placing == _capi.PLACING_CUBOID else [DP(DUMMY)]
    place_fields = (dict(rot=DUMMY, center=DUMMY, position=ctypes.addressof(POS), sides=ctypes.addressof(SIDES)) if placing == _capi.PLACING_CUBOID
                    else dict(coords=DUMMY))
    rec = _capi.record(family, placing, features=feat, proj=DUMMY, deterministic=det, **place_fields, **fields)
    if kind == _capi.CALL_FORWARD:
        lead, outs = [DP(feat), DP(DUMMY)], ["out"]
    else:
        lead = [DP(DUMMY), DP(feat), DP(DUMMY)]
        rec.grad_out = DUMMY
        outs = ["grad_features"] if kind == _capi.CALL_BACKWARD else (
            ["grad_proj", "grad_rot", "grad_center"] if placing == _capi.PLACING_CUBOID else ["grad_proj", "grad_coords"]) + (
            ["grad_weights"] if family == "weighted" else ["grad_confidence"] if family == "confidence" else [])
    for k in outs:
        setattr(rec, k, DUMMY)
    by_name = getattr(L, _named(family, placing, kind_name))(ctypes.byref(d), *lead, *place_args, *args, *[DP(DUMMY)] * len(outs), DP(0), 0, DP(0))
    t_name = L.mvhmr_last_error()
    fn = {_capi.CALL_FORWARD: L.mvhmr_unproject_forward_call, _capi.CALL_BACKWARD: L.mvhmr_unproject_backward_call,
          _capi.CALL_GEOMETRY: L.mvhmr_unproject_backward_geometry_call}[kind]
    by_record = fn(ctypes.byref(d), ctypes.byref(rec), DP(0), 0, DP(0))
    return (by_name, t_name), (by_record, L.mvhmr_last_error())


@pytest.mark.parametrize("label", list(DESCS))
def test_record_answers_what_the_names_answer(label):
    L = _capi.lib()
    d, volumes = DESCS[label]
    refused = answered = compared = 0
    blank = _sentinel(L)
    L.mvhmr_unproject_forward_workspace_bytes(ctypes.byref(d))
    desc_refused = L.mvhmr_last_error() != blank
    for family, placing, (kind_name, kind, det) in itertools.product(FAMILIES, (_capi.PLACING_TENSOR, _capi.PLACING_CUBOID), KINDS):
        where = (label, family, placing, kind_name)
        # the workspace query: the same bytes and, where it refuses, the same text
        blank = _sentinel(L)
        need = _named_query(L, family, placing, kind_name)(ctypes.byref(d), *([volumes] if family == "shared" else []))
        said = L.mvhmr_last_error()
        assert _sentinel(L) == blank
        rec = _capi.record(family, placing, deterministic=det, volumes=volumes)          # no pointer: the query reads none
        assert L.mvhmr_unproject_call_workspace_bytes(ctypes.byref(d), ctypes.byref(rec), kind) == need, where
        assert L.mvhmr_last_error() == said, where
        query_refused = said != blank
        assert not (query_refused and need), where
        refused += query_refused
        answered += need > 0
        # the launching call.  Null features are refused before anything else the call says.  With dummy pointers and no workspace only
        # calls that cannot launch are made: the descriptor is refused, or the plain call of this kind needs a workspace -- every family's
        # plan, and every plan a family degrades to, holds the plain plan's regions, so the call is refused at the workspace check at
        # the latest.  Status and text must be the same by either way in.
        cannot_launch = desc_refused or _named_query(L, "plain", placing, kind_name)(ctypes.byref(d)) > 0
        for fill in FILLS:
            if fill == "refused" and family not in ("shared", "lens"):
                continue
            fields, args = _fields(family, fill, volumes)
            for null_features in (True, False):
                if not null_features and not cannot_launch:
                    continue
                if not null_features and family == "shared" and fill == "null" and volumes == d.batch:
                    continue                                # (the plain call with the gather variant forced: another plan)
                a, b = _launch_both(L, d, family, placing, kind_name, kind, det, fields, args, null_features)
                assert a == b, (where, fill, null_features, a, b)
                assert a[0] != _capi.OK, (where, fill, null_features)
                compared += 1
    assert (answered or refused) and compared >= 2 * 8 * 2 * 4


def test_the_cases_cover_refusals_and_plans():
    """the descriptors above reach what they are there for: refused families, a gated forward, volumes past the limit"""
    L = _capi.lib()
    q = lambda label, family, kind, **kw: L.mvhmr_unproject_call_workspace_bytes(      # noqa: E731
        ctypes.byref(DESCS[label][0]), ctypes.byref(_capi.record(family, volumes=DESCS[label][1], **kw)), kind)
    assert q("softmax planar auto", "plain", _capi.CALL_FORWARD) > 0
    assert q("softmax planar auto", "masked", _capi.CALL_BACKWARD, deterministic=1) > q("softmax planar auto", "plain", _capi.CALL_BACKWARD)
    assert q("max quad auto", "masked", _capi.CALL_FORWARD) == 0 and b"quad-planar" in L.mvhmr_last_error()
    assert q("mean planar brick", "lens", _capi.CALL_GEOMETRY) == 0 and b"MVHMR_VARIANT_BRICK" in L.mvhmr_last_error()
    assert q("max quad auto", "moments", _capi.CALL_FORWARD) == 0 and b"MVHMR_AGG_MEAN" in L.mvhmr_last_error()
    assert q("softmax c32 planar auto 64^3", "shared", _capi.CALL_FORWARD) == 0 and b"volumes per call" in L.mvhmr_last_error()
    assert q("softmax c32 planar auto 64^3", "plain", _capi.CALL_FORWARD) > 0
    assert q("sum c5 channels-last", "plain", _capi.CALL_FORWARD) == 0 and b"C % 4" in L.mvhmr_last_error()
    assert q("sum c5 planar gather", "shared", _capi.CALL_GEOMETRY) > q("sum c5 planar gather", "plain", _capi.CALL_GEOMETRY)


def test_a_malformed_record_is_refused():
    L = _capi.lib()
    d = ctypes.byref(DESCS["softmax planar auto"][0])
    ways = ((L.mvhmr_unproject_forward_call, _capi.ERR_INVALID_ARGUMENT), (L.mvhmr_unproject_backward_call, _capi.ERR_INVALID_ARGUMENT),
            (L.mvhmr_unproject_backward_geometry_call, _capi.ERR_INVALID_ARGUMENT))

    def refused(rec, text):
        for fn, status in ways:
            assert fn(d, ctypes.byref(rec), DP(0), 0, DP(0)) == status
            assert text in L.mvhmr_last_error(), L.mvhmr_last_error()

    good = dict(features=DUMMY, proj=DUMMY, coords=DUMMY, out=DUMMY)
    for size in (0, ctypes.sizeof(_capi.Call) - 8, ctypes.sizeof(_capi.Call) + 8):
        rec = _capi.record("plain", **good)
        rec.struct_size = size
        refused(rec, b"struct_size")
        assert L.mvhmr_unproject_call_workspace_bytes(d, ctypes.byref(rec), _capi.CALL_FORWARD) == 0 and b"struct_size" in L.mvhmr_last_error()
    for family in (-1, 8, 1000):
        rec = _capi.record("plain", **good)
        rec.family = family
        refused(rec, b"unknown call family")
        assert L.mvhmr_unproject_call_workspace_bytes(d, ctypes.byref(rec), _capi.CALL_FORWARD) == 0 and b"unknown call family" in L.mvhmr_last_error()
    rec = _capi.record("plain", placing=2, **good)
    refused(rec, b"unknown placing")
    # an optional input the family's name has no argument for: refused, not ignored
    refused(_capi.record("plain", view_mask=DUMMY, **good), b"takes none of the optional inputs")
    refused(_capi.record("masked", view_mask=DUMMY, lens=DUMMY, **good), b"takes none of the optional inputs")
    refused(_capi.record("shared", volumes=2, moments=1, **good), b"takes none of the optional inputs")
    rec = _capi.record("plain")
    assert L.mvhmr_unproject_call_workspace_bytes(d, ctypes.byref(rec), 3) == 0 and b"unknown call kind" in L.mvhmr_last_error()
    for fn, status in ways:
        assert fn(d, None, DP(0), 0, DP(0)) == status and b"call record is null" in L.mvhmr_last_error()
