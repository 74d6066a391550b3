"""Deterministic mode of the feature-gradient backward, without a GPU: which op autograd dispatches with
torch.use_deterministic_algorithms on and off, the new ops' shape functions, the C ABI's argument checks of the deterministic entry
points against the default ones, and the gfx950 ISA of the deterministic kernel instances (no float atomics)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from multiviewhmr_amd import _capi, aggregation  # noqa: F401  (registers the ops)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multiviewhmr_amd", "csrc")


class _OpNames(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


class _deterministic:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(self.on)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.was)


def _recorded_backward(cuboid, deterministic):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty(1, 2, 4, 6, 6, requires_grad=True)
        p = torch.empty(1, 2, 3, 4)
        if cuboid:
            o = torch.ops.mvhmr.unprojection_cuboid(f, p, torch.empty(1, 3, 3), torch.empty(1, 3), [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [3, 3, 3],
                                                    0, _capi.F32, 0)
        else:
            o = torch.ops.mvhmr.unprojection(f, p, torch.empty(1, 3, 3, 3, 3), 0, _capi.F32, 0)
        rec = _OpNames()
        with _deterministic(deterministic), rec:
            o.sum().backward()
    return rec.names


@pytest.mark.parametrize("cuboid", [False, True])
def test_backward_dispatch_follows_the_deterministic_flag(cuboid):
    default = "mvhmr.unprojection_cuboid_backward." if cuboid else "mvhmr.unprojection_backward."
    det = "mvhmr.unprojection_cuboid_backward_deterministic." if cuboid else "mvhmr.unprojection_backward_deterministic."
    off = _recorded_backward(cuboid, False)
    assert any(default in n for n in off), off
    assert not any("_deterministic" in n for n in off), off
    on = _recorded_backward(cuboid, True)
    assert any(det in n for n in on), on
    assert not any(default in n for n in on), on
    assert not torch.are_deterministic_algorithms_enabled()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_fake_shapes_of_the_deterministic_ops(dtype):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty(2, 3, 8, 5, 7, dtype=dtype)
        p = torch.empty(2, 3, 3, 4)
        go = torch.empty(2, 8, 4, 3, 2, dtype=dtype)
        g = torch.ops.mvhmr.unprojection_backward_deterministic(go, f, p, torch.empty(2, 4, 3, 2, 3), 1, _capi.F32, 0)
        assert g.shape == f.shape and g.dtype == dtype
        g = torch.ops.mvhmr.unprojection_cuboid_backward_deterministic(go, f, p, torch.empty(2, 3, 3), torch.empty(2, 3), [0.0] * 3, [1.0] * 3,
                                                                       [4, 3, 2], 1, _capi.F32, 0)
        assert g.shape == f.shape and g.dtype == dtype


def _desc(**kw):
    d = _capi.Desc()
    d.abi_version = _capi.ABI_VERSION
    d.batch, d.views, d.channels, d.feat_h, d.feat_w = 2, 4, 32, 24, 20
    d.vol_x, d.vol_y, d.vol_z = 8, 6, 5
    for k, v in kw.items():
        setattr(d, k, v)
    return d


_CASES = [
    dict(),                                                               # valid: no workspace -> ERR_WORKSPACE
    dict(abi_version=3), dict(batch=0), dict(views=17), dict(method=7), dict(feat_dtype=_capi.BF16),
    dict(feat_dtype=_capi.F32, out_dtype=_capi.F16), dict(feat_layout=_capi.LAYOUT_QUAD_LOG2E), dict(feat_layout=9), dict(variant=5),
    dict(feat_layout=_capi.LAYOUT_BVHWC, channels=6), dict(feat_layout=_capi.LAYOUT_QUAD, channels=6),
    dict(variant=_capi.VARIANT["brick"], views=12), dict(feat_layout=_capi.LAYOUT_QUAD, feat_dtype=_capi.F16, channels=4096),
]


@pytest.mark.parametrize("null", [None, "grad_out", "features", "proj", "coords", "grad_features"])
@pytest.mark.parametrize("kw", _CASES, ids=[str(k) for k in _CASES])
def test_c_abi_validation_matches_the_default_entry_points(kw, null):
    """the validation paths return before anything touches the (dummy, never dereferenced) pointers"""
    L = _capi.lib()
    dummy, zero = ctypes.c_void_p(256), ctypes.c_void_p(0)
    ptr = {k: (zero if k == null else dummy) for k in ("grad_out", "features", "proj", "coords", "grad_features")}
    d = _desc(**kw)
    a = (ctypes.byref(d), ptr["grad_out"], ptr["features"], ptr["proj"])
    tail = (ptr["grad_features"], zero, 0, zero)
    pos, sides = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1)
    rc = L.mvhmr_unproject_backward(*a, ptr["coords"], *tail)
    rc_det = L.mvhmr_unproject_backward_deterministic(*a, ptr["coords"], *tail)
    assert rc == rc_det, (kw, null, rc, rc_det)
    rc = L.mvhmr_unproject_backward_cuboid(*a, ptr["coords"], ptr["coords"], pos, sides, *tail)
    rc_det = L.mvhmr_unproject_backward_cuboid_deterministic(*a, ptr["coords"], ptr["coords"], pos, sides, *tail)
    assert rc == rc_det, (kw, null, rc, rc_det)
    if not kw and null is None:
        assert rc_det == _capi.ERR_WORKSPACE


@pytest.mark.parametrize("kw", [dict(), dict(feat_layout=_capi.LAYOUT_BVHWC), dict(feat_layout=_capi.LAYOUT_QUAD), dict(feat_dtype=_capi.F16,
                                out_dtype=_capi.F16), dict(feat_h=200, feat_w=200), dict(channels=6), dict(views=12), dict(vol_x=64, vol_y=64, vol_z=64),
                                dict(variant=_capi.VARIANT["gather"]), dict(variant=_capi.VARIANT["brick"])])
def test_deterministic_workspace_is_at_least_the_default(kw):
    L = _capi.lib()
    d = _desc(**kw)
    det = L.mvhmr_unproject_backward_deterministic_workspace_bytes(ctypes.byref(d))
    assert det >= L.mvhmr_unproject_backward_workspace_bytes(ctypes.byref(d))
    assert det > 0


def test_conv_wgrad_deterministic_validation_and_workspace():
    L = _capi.lib()
    dummy, zero = ctypes.c_void_p(256), ctypes.c_void_p(0)
    assert L.mvhmr_conv1x1_wgrad_deterministic(zero, dummy, dummy, zero, 4, 128, 128, 64, dummy, 1 << 30, zero) == _capi.ERR_INVALID_ARGUMENT
    assert L.mvhmr_conv1x1_wgrad_deterministic(dummy, dummy, dummy, zero, 0, 128, 128, 64, dummy, 1 << 30, zero) == _capi.ERR_INVALID_ARGUMENT
    assert L.mvhmr_conv1x1_wgrad_deterministic(dummy, dummy, dummy, zero, 4, 96, 128, 64, dummy, 1 << 30, zero) == _capi.ERR_UNSUPPORTED
    assert L.mvhmr_conv1x1_wgrad_deterministic(dummy, dummy, dummy, zero, 4, 128, 128, 64, zero, 0, zero) == _capi.ERR_WORKSPACE
    # at most 2048 partial 128 x 128 tiles (+ bias partials)
    n = L.mvhmr_conv1x1_wgrad_deterministic_workspace_bytes(128, 256, 256, 96 * 96)
    assert 0 < n <= 2048 * (128 * 128 + 128) * 4
    assert L.mvhmr_conv1x1_wgrad_deterministic_workspace_bytes(4, 96, 128, 64) == 0


def _kernels(path, prefix):
    """{mangled name: [instructions]} of every function whose name contains prefix"""
    out, name = {}, None
    for line in open(path):
        ls = line.strip()
        m = re.match(r"^(_Z\S+):", ls)
        if m:
            name = m.group(1) if prefix in m.group(1) else None
            if name:
                out[name] = []
            continue
        if ls.startswith(".Lfunc_end"):
            name = None
        elif name and ls and not ls.startswith((";", ".")):
            out[name].append(ls)
    return out


def _asm(tmp_path, unit):
    asm = tmp_path / (unit + ".s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(CSRC, unit + ".hip")], stderr=subprocess.DEVNULL)
    return str(asm)


_FLOAT_ATOMIC = re.compile(r"_atomic_(add_f32|pk_add_\w+|add_f64)\b")


def test_deterministic_kernels_have_no_float_atomics_in_their_isa(tmp_path):
    gather = _kernels(_asm(tmp_path, "unproject_gather"), "k_bwd_gather_det")
    # 3 storage pairings (+ bf16 volume) x 4 methods x 4 view paths
    assert len(gather) == 4 * 4 * 4, sorted(gather)
    for name, ins in gather.items():
        assert not any(_FLOAT_ATOMIC.search(i) for i in ins), name
        assert sum(i.startswith(("global_atomic_add_x2", "buffer_atomic_add_x2", "flat_atomic_add_x2")) for i in ins) >= 4, name
    conv = _kernels(_asm(tmp_path, "conv1x1_quad"), "k_conv1x1_wgrad_")
    assert len(conv) == 2, sorted(conv)                                    # k_conv1x1_wgrad_det + k_conv1x1_wgrad_reduce
    for name, ins in conv.items():
        assert not any("atomic" in i for i in ins), name
    brick = _kernels(_asm(tmp_path, "unproject_brick_bwd"), "mvhmr")
    # deterministic instances: the trailing `const int *kexp` pack (JPKiE in the mangled name); default ones have the empty pack (JEE)
    det_brick = {k: v for k, v in brick.items() if "k_bwd_brick" in k and "JPKiE" in k}
    det_tail = {k: v for k, v in brick.items() if "k_bwd_tail" in k and "JPKiE" in k}
    det_slow = {k: v for k, v in brick.items() if "bwd_brick_slow" in k and "JPKiE" in k}
    assert len(det_brick) == 4 * 3 * 3 * 2, sorted(det_brick)              # 4 methods x 2 / 4 / 8 views x 3 grad_out types x 2 brick depths
    assert len(det_tail) == 4 * 3 * 3, sorted(det_tail)
    assert len(det_slow) >= 4 * 3 * 3, sorted(det_slow)
    for name, ins in list(det_brick.items()) + list(det_tail.items()) + list(det_slow.items()):
        assert not any(_FLOAT_ATOMIC.search(i) for i in ins), name
    for name, ins in det_brick.items():                                   # the flush: u64 buffer atomics
        assert sum(i.startswith("buffer_atomic_add_x2") for i in ins) >= 4, name
    for name, ins in det_slow.items():
        assert sum("_atomic_add_x2" in i for i in ins) >= 4, name
    # and the default instances still flush with f32 atomics (the check above is not vacuous)
    assert any(i.startswith("buffer_atomic_add_f32") for k, v in brick.items() if "k_bwd_brick" in k and "JEE" in k for i in v)
    det = _kernels(_asm(tmp_path, "unproject_det"), "k_det_")
    assert len(det) >= 7, sorted(det)
    for name, ins in det.items():
        assert not any(_FLOAT_ATOMIC.search(i) for i in ins), name
