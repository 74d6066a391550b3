"""The deterministic scale pass on the GPU: the exponent table K[b][c] that a deterministic feature backward leaves in its
workspace, read through the testing hook mvhmr_internal_det_exponent_table, equals detscale_oracle's K as integers -- poison included --
for every family, method, storage type and selection the pass serves.  The rigs are detscale_oracle.rigs(); test_detscale_cpu.py proves
without a GPU that each satisfies the oracle's condition, which is asserted here once more before the comparison."""
import ctypes

import numpy as np
import pytest
import torch

import detscale_oracle as oracle
from multiviewhmr_amd import _capi

pytestmark = pytest.mark.gpu

RIGS = oracle.rigs()
POS = (ctypes.c_double * 3)(-500.0, -500.0, -500.0)


def _device_inputs(rig, gpu):
    B, V = rig["features"].shape[:2]
    t = {"features": torch.from_numpy(rig["features"]).to(rig["feat_dtype"]), "grad_out": torch.from_numpy(rig["grad_out"]).to(rig["out_dtype"]),
         "proj": torch.from_numpy(rig["proj"]), "coords": torch.from_numpy(rig["coords"])}
    assert np.array_equal(t["features"].float().numpy(), rig["features"], equal_nan=True)          # the storage type keeps the rig's values
    assert np.array_equal(t["grad_out"].float().numpy(), rig["grad_out"], equal_nan=True)
    for key, dtype in (("mask", torch.uint8), ("weights", torch.float32), ("conf", torch.float32), ("index", torch.int32)):
        if rig.get(key) is not None:
            t[key] = torch.as_tensor(np.asarray(rig[key])).to(dtype)
    if rig.get("lens"):
        H, W = rig["features"].shape[3:]
        t["lens"] = torch.tensor([20.0, 20.0, W / 2, H / 2, 0.05, 0.0, 0.0, 0.0, 0.0, 4.0]).repeat(B, V, 1)     # fx fy cx cy | k1 k2 p1 p2 k3 | r2max
    t["grad_features"] = torch.zeros(rig["features"].shape, dtype=rig["feat_dtype"])
    return {k: v.to(gpu).contiguous() for k, v in t.items()}


@pytest.mark.parametrize("name", list(RIGS))
def test_the_exponent_table_equals_the_oracle(name, gpu):
    rig = RIGS[name]
    sure, possible = oracle.k_table(rig)
    assert np.array_equal(sure, possible), "the rig breaks the oracle's condition: see test_detscale_cpu.py"
    L = _capi.lib()
    t = _device_inputs(rig, gpu)
    d, call = oracle.call_of(rig, {k: v.data_ptr() for k, v in t.items()})
    need = L.mvhmr_unproject_call_workspace_bytes(ctypes.byref(d), ctypes.byref(call), _capi.CALL_BACKWARD)
    off, cnt = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.mvhmr_internal_det_exponent_table(ctypes.byref(d), ctypes.byref(call), ctypes.byref(off), ctypes.byref(cnt)) == _capi.OK, L.mvhmr_last_error()
    assert off.value + 4 * cnt.value <= need
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=gpu)            # test-owned: K must be written, not found
    status = L.mvhmr_unproject_backward_call(ctypes.byref(d), ctypes.byref(call), ctypes.c_void_p(ws.data_ptr()), need, ctypes.c_void_p(0))
    assert status == _capi.OK, L.mvhmr_last_error()
    torch.cuda.synchronize()
    got = ws[off.value:off.value + 4 * cnt.value].cpu().numpy().view(np.int32).astype(np.int64).reshape(sure.shape)
    print("%s: K oracle\n%s\nK device\n%s" % (name, sure, got))
    assert np.array_equal(got, sure), (name, np.argwhere(got != sure))
    # the gradient of a poisoned (b, c) is NaN
    grad = t["grad_features"].float().cpu().numpy()
    poisoned = np.broadcast_to((sure == oracle.POISON)[:, None, :, None, None], grad.shape)
    if rig.get("mask") is not None or rig.get("weights") is not None:
        with np.errstate(invalid="ignore"):
            absent = ~oracle._present(rig)
        poisoned = poisoned & ~absent[:, :, None, None, None]               # an absent view's gradient is zero-filled
    assert np.isnan(grad[poisoned]).all()
