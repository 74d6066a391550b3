"""The deterministic scale pass without a GPU: the testing hook mvhmr_internal_det_exponent_table answers from the plan alone
-- for every family and placing the exponent table lies inside the workspace the library itself asks for, and the plane route, which has no
scale pass, says so -- and every rig of test_detscale_gpu.py satisfies the oracle's own condition: the pixels its voxel-views surely tap and
those they possibly tap give the same K for every (b, c), so the comparison on the GPU needs no tolerance."""
import ctypes

import numpy as np
import pytest

import detscale_oracle as oracle
from multiviewhmr_amd import _capi

RIGS = oracle.rigs()
FAKE = 4096                      # a non-null address: the hook and the queries read no device pointer


def _pointers():
    pos = (ctypes.c_double * 3)(-500.0, -500.0, -500.0)
    p = {k: FAKE for k in ("features", "proj", "grad_out", "grad_features", "coords", "mask", "weights", "conf", "index", "lens", "rot", "center")}
    p.update(position=ctypes.addressof(pos), sides=ctypes.addressof(pos), _keep=pos)
    return p


def _table(d, call):
    off, cnt = ctypes.c_size_t(~0 & 0xFFFF), ctypes.c_size_t(0)
    rc = _capi.lib().mvhmr_internal_det_exponent_table(ctypes.byref(d), ctypes.byref(call), ctypes.byref(off), ctypes.byref(cnt))
    return rc, off.value, cnt.value


@pytest.mark.parametrize("placing", [_capi.PLACING_TENSOR, _capi.PLACING_CUBOID])
@pytest.mark.parametrize("name", list(RIGS))
def test_the_exponent_table_lies_inside_the_workspace_the_library_asks_for(name, placing):
    rig = RIGS[name]
    L = _capi.lib()
    d, call = oracle.call_of(rig, _pointers(), placing)
    need = L.mvhmr_unproject_call_workspace_bytes(ctypes.byref(d), ctypes.byref(call), _capi.CALL_BACKWARD)
    rc, off, cnt = _table(d, call)
    assert rc == _capi.OK, L.mvhmr_last_error()
    B, _, C = rig["features"].shape[:3]
    assert cnt == B * C and off % 4 == 0
    assert off + 4 * cnt <= need, (off, cnt, need)


@pytest.mark.parametrize("family", ["plain", "lens"])
def test_the_plane_route_has_no_exponent_table(family):
    L = _capi.lib()
    # the plane kernels serve 2 / 4 / 8 views whose maps fit LDS: test_plane_route_is_unchanged_by_the_flag's shape
    d = _capi.Desc(abi_version=_capi.ABI_VERSION, batch=2, views=4, channels=16, feat_h=24, feat_w=24, vol_x=8, vol_y=8, vol_z=8,
                   method=_capi.AGG["softmax"], variant=_capi.VARIANT["gather"])
    call = _capi.record(family, deterministic=1, features=FAKE, proj=FAKE, grad_out=FAKE, grad_features=FAKE, coords=FAKE,
                        **({"lens": FAKE} if family == "lens" else {}))
    rc, off, cnt = _table(d, call)
    assert rc == _capi.ERR_UNSUPPORTED and b"no scale pass" in L.mvhmr_last_error()
    assert cnt == 0                                                       # nothing was answered


def test_the_hook_wants_a_deterministic_backward_record():
    L = _capi.lib()
    d, call = oracle.call_of(RIGS["plain softmax"], _pointers())
    call.deterministic = 0
    assert _table(d, call)[0] == _capi.ERR_INVALID_ARGUMENT and b"deterministic" in L.mvhmr_last_error()
    call.deterministic, call.view_mask = 1, FAKE                         # a plain record takes no mask: refused as the call itself would be
    assert _table(d, call)[0] == _capi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", list(RIGS))
def test_sure_and_possible_taps_give_the_same_exponents(name):
    """the oracle's own condition, for every (b, c) of every rig: no exemption"""
    sure, poss = oracle.k_table(RIGS[name])
    assert np.array_equal(sure, poss), (name, np.argwhere(sure != poss))


def test_the_rigs_can_tell_a_wrong_pass_from_a_right_one():
    """what each rig is there for, read off the oracle's K"""
    K = {n: oracle.k_table(r)[0] for n, r in RIGS.items()}
    P = oracle.POISON
    assert (K["plain sum N=64"] - K["plain sum N=65"] == 1).all()                              # ceil log2 N: 6 against 7
    for m in oracle.METHODS:
        assert np.array_equal(K["lens %s" % m], K["plain %s" % m])
    # n_b = 3: the mean divides by 3 (one or two more bits); n_b = 1 and n_b = 0 (divisor max(n_b, 1)): the sum's exponents
    assert ((K["masked mean"][0] - K["masked sum"][0] >= 1) & (K["masked mean"][0] - K["masked sum"][0] <= 2)).all()
    assert np.array_equal(K["masked mean"][1:], K["masked sum"][1:])
    masked = RIGS["masked softmax"]
    assert np.array_equal(K["masked softmax"][2], oracle._k(dict(masked, features=masked["features"] * 0), None)[2])    # no view present: F = 0
    assert (K["weighted inf sum"][0] == P).all() and (K["weighted inf sum"][1] != P).all()
    assert (K["weighted inf mean"] != P).all() and (K["weighted inf softmax"] != P).all()
    assert not np.array_equal(K["weighted sum"], K["weighted mean"])
    for n, r in RIGS.items():
        if oracle.uses_marks(r):
            if r.get("visible") or r.get("conf") is not None:
                assert r["hidden"], n                                                          # a pixel only left-out voxel-views tap exists
            every = oracle._k(r, None)                                                         # a pass that ignored the marks
            named = every != K[n]
            assert named.any(), n
            if "inf outside" in n:
                assert (every == P).all() and (K[n] != P).all()
    conf = K["confidence softmax"]
    assert (conf[1] == oracle._k(dict(RIGS["confidence softmax"], features=RIGS["confidence softmax"]["features"] * 0), None)[1]).all()   # all maps <= 0: F = 0
    assert (K["confidence sum"][1] == 0).all()                                                 # cmax = 0: the bound is 0
    assert (K["shared M=3 softmax"][0] == 0).all() and (K["shared M=2 nobody"][1] == 0).all()
    assert (K["shared M=2 nobody"][0] != 0).all() and (K["shared M=2 nobody"][0] != P).all()
    assert (K["plain softmax inf grad"][1, 2] == P) and (K["plain softmax inf grad"] == P).sum() == 1
    assert (K["plain softmax nan feature"][0, 3] == P) and (K["plain sum nan feature"] != P).all()
    assert K["visible softmax nan tapped"][0, 3] == P and (K["visible softmax nan tapped"] == P).sum() == 1
