"""The host side of the four fused 1x1-conv GEMM entry points (csrc/conv1x1_quad.hip behind include/mvhmr_unproject.h), without a GPU:
the support predicates and the deterministic workspace size against independent restatements of the header's rules, and the argument
checks (null and misaligned pointers, non-positive extents, unsupported shapes, n_maps above the grid limit) with their documented
error codes.  Every call here has exactly one defect and returns before anything touches its (dummy, never dereferenced) pointers: no
call in this file is valid as a whole, so none reaches a kernel launch."""
import ctypes
import itertools

import pytest
import torch

from multiviewhmr_amd import _capi, aggregation

DIMS = (1, 4, 15, 16, 17, 31, 32, 96, 127, 128, 129, 256, 2048)
MAX_MAPS = 65535                     # the header's limit for to_quad / planar: n_maps is the grid's z extent
# (BV, Cin, Cout, HW) of the exact-arithmetic weight-gradient tests (tests/test_conv1x1_gemm_gpu.py)
WGRAD_SHAPES = ((1, 128, 128, 32), (2, 256, 128, 64), (1, 128, 256, 9216), (40, 256, 256, 1024), (600, 128, 128, 64), (3000, 128, 128, 64),
                (2, 2048, 256, 1024))


# ---- the header's rules, restated
def quad_rule(c_in, c_out, h, w):
    return c_in % 16 == 0 and c_out % 128 == 0 and h % 4 == 0 and w % 32 == 0


def planar_rule(c_in, c_out, pixels):
    return c_in % 16 == 0 and c_out % 128 == 0 and pixels % 128 == 0


def wgrad_rule(c_in, c_out, pixels):
    return c_in % 128 == 0 and c_out % 128 == 0 and pixels % 32 == 0


def slices_per_map_rule(n_maps, c_in, c_out, pixels):
    """the largest divisor c of pixels / 32 with n_maps * c * (c_out / 128) * (c_in / 128) <= 2048, else 1"""
    chunks, tiles = pixels // 32, (c_out // 128) * (c_in // 128)
    fits = [c for c in range(1, chunks + 1) if chunks % c == 0 and n_maps * c * tiles <= 2048]
    return max(fits) if fits else 1


def workspace_rule(n_maps, c_in, c_out, pixels):
    if n_maps <= 0 or not wgrad_rule(c_in, c_out, pixels):
        return 0
    return n_maps * slices_per_map_rule(n_maps, c_in, c_out, pixels) * (c_out * c_in + c_out) * 4


def test_support_predicates_follow_the_header():
    L = _capi.lib()
    for c_in, c_out, h, w in itertools.product(DIMS, repeat=4):
        assert L.mvhmr_conv1x1_to_quad_supported(c_in, c_out, h, w) == int(quad_rule(c_in, c_out, h, w)), (c_in, c_out, h, w)
    for c_in, c_out, px in itertools.product(DIMS, repeat=3):
        assert L.mvhmr_conv1x1_planar_supported(c_in, c_out, px) == int(planar_rule(c_in, c_out, px)), (c_in, c_out, px)
        assert L.mvhmr_conv1x1_wgrad_supported(c_in, c_out, px) == int(wgrad_rule(c_in, c_out, px)), (c_in, c_out, px)
    # the sweep holds both answers of every predicate, and shapes on which the three differ
    assert L.mvhmr_conv1x1_to_quad_supported(16, 128, 4, 32) == 1 and L.mvhmr_conv1x1_planar_supported(16, 128, 128) == 1
    assert L.mvhmr_conv1x1_wgrad_supported(16, 128, 128) == 0 and L.mvhmr_conv1x1_wgrad_supported(128, 128, 32) == 1
    assert L.mvhmr_conv1x1_planar_supported(128, 128, 32) == 0


def test_deterministic_workspace_bytes_follow_the_header():
    L = _capi.lib()
    q = L.mvhmr_conv1x1_wgrad_deterministic_workspace_bytes
    for shape in WGRAD_SHAPES + ((257, 512, 512, 128 * 128), (128, 256, 256, 96 * 96)):
        assert q(*shape) == workspace_rule(*shape) > 0, shape
    seen = set()
    for n_maps in (-1, 0, 1, 2, 3, 7, 8, 9, 16, 17, 64, 100, 127, 128, 129, 511, 512, 513, 1000, 2047, 2048, 2049, 4096, 65535, 65536, 100000):
        for c_in, c_out in itertools.product((64, 96, 128, 256, 384, 2048), repeat=2):
            for px in (16, 32, 48, 64, 96, 128, 160, 224, 640, 1024, 1536, 3072, 9216, 16384):
                want = workspace_rule(n_maps, c_in, c_out, px)
                assert q(n_maps, c_in, c_out, px) == want, (n_maps, c_in, c_out, px)
                if want:
                    spm, chunks = slices_per_map_rule(n_maps, c_in, c_out, px), px // 32
                    seen.add("one" if spm == 1 else "all" if spm == chunks else "some")
    assert seen == {"one", "some", "all"}
    # at most 2048 partial tiles of 128 x 128 wherever the maps alone do not exceed that
    assert q(128, 256, 256, 96 * 96) <= 2048 * (128 * 128 + 128) * 4


# ---- argument checks: (entry point, pointer arguments, extents of a supported shape, shapes the header rules out, 16-byte pointers)
_ENTRIES = {
    "to_quad": dict(fn="mvhmr_conv1x1_to_quad", ptrs=("x", "weight", "bias", "dst"), optional=("bias",), aligned=("x", "weight", "bias", "dst"),
                    dims=dict(n_maps=4, c_in=32, c_out=128, feat_h=8, feat_w=64),
                    unsupported=(dict(c_in=24), dict(c_out=64), dict(c_out=132), dict(feat_h=6), dict(feat_w=48), dict(n_maps=MAX_MAPS + 1))),
    "planar": dict(fn="mvhmr_conv1x1_planar", ptrs=("x", "weight", "bias", "dst"), optional=("bias",), aligned=("x", "weight", "bias", "dst"),
                   dims=dict(n_maps=4, c_in=32, c_out=128, pixels=256),
                   unsupported=(dict(c_in=24), dict(c_out=64), dict(pixels=192), dict(pixels=32), dict(n_maps=MAX_MAPS + 1))),
    "wgrad": dict(fn="mvhmr_conv1x1_wgrad", ptrs=("grad_y", "x", "grad_weight", "grad_bias"), optional=("grad_bias",), aligned=("grad_y", "x"),
                  dims=dict(n_maps=4, c_in=128, c_out=256, pixels=64),
                  unsupported=(dict(c_in=64), dict(c_in=144), dict(c_out=192), dict(pixels=48))),
    "wgrad_deterministic": dict(fn="mvhmr_conv1x1_wgrad_deterministic", ptrs=("grad_y", "x", "grad_weight", "grad_bias"), optional=("grad_bias",),
                                aligned=("grad_y", "x"), dims=dict(n_maps=4, c_in=128, c_out=256, pixels=64), workspace=True,
                                unsupported=(dict(c_in=64), dict(c_in=144), dict(c_out=192), dict(pixels=48))),
}


def _call(entry, ptr=None, dim=None):
    """the entry point on dummy pointers (address 256), with the given pointers / extents replaced"""
    e = _ENTRIES[entry]
    ptrs = dict.fromkeys(e["ptrs"], 256)
    ptrs.update(ptr or {})
    dims = dict(e["dims"])
    dims.update(dim or {})
    assert ptr or dim, "a call with no defect would launch a kernel on dummy pointers"
    args = [ctypes.c_void_p(ptrs[k]) for k in e["ptrs"]] + [dims[k] for k in e["dims"]]
    if e.get("workspace"):
        args += [ctypes.c_void_p(256), 1 << 40]
    return getattr(_capi.lib(), e["fn"])(*args, ctypes.c_void_p(0))


def _cases(key):
    return [(name, v) for name, e in _ENTRIES.items() for v in e[key]]


@pytest.mark.parametrize("entry,name", [(n, p) for n, e in _ENTRIES.items() for p in e["ptrs"] if p not in e["optional"]])
def test_null_pointer_is_an_invalid_argument(entry, name):
    assert _call(entry, ptr={name: 0}) == _capi.ERR_INVALID_ARGUMENT
    assert _capi.lib().mvhmr_last_error()


@pytest.mark.parametrize("value", (0, -1, -128))
@pytest.mark.parametrize("entry,name", [(n, d) for n, e in _ENTRIES.items() for d in e["dims"]])
def test_non_positive_extent_is_an_invalid_argument(entry, name, value):
    assert _call(entry, dim={name: value}) == _capi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("entry,dim", _cases("unsupported"), ids=lambda v: str(v))
def test_unsupported_shape_has_its_own_code(entry, dim):
    assert _call(entry, dim=dim) == _capi.ERR_UNSUPPORTED
    assert _capi.lib().mvhmr_last_error()


@pytest.mark.parametrize("offset", (4, 8, 12))
@pytest.mark.parametrize("entry,name", _cases("aligned"))
def test_pointer_off_a_16_byte_boundary_is_an_invalid_argument(entry, name, offset):
    assert _call(entry, ptr={name: 256 + offset}) == _capi.ERR_INVALID_ARGUMENT
    assert b"16" in _capi.lib().mvhmr_last_error()


def test_defects_are_reported_in_the_documented_order():
    """invalid arguments (null, extents, alignment) before unsupported shapes; an unsupported shape before the workspace check"""
    assert _call("to_quad", ptr={"x": 0}, dim={"c_in": 24}) == _capi.ERR_INVALID_ARGUMENT
    assert _call("to_quad", ptr={"dst": 260}, dim={"n_maps": MAX_MAPS + 1}) == _capi.ERR_INVALID_ARGUMENT
    assert _call("planar", dim={"n_maps": 0, "pixels": 192}) == _capi.ERR_INVALID_ARGUMENT
    assert _call("wgrad", ptr={"grad_y": 264}, dim={"c_in": 64}) == _capi.ERR_INVALID_ARGUMENT
    L = _capi.lib()
    dummy, zero = ctypes.c_void_p(256), ctypes.c_void_p(0)
    assert L.mvhmr_conv1x1_wgrad_deterministic(dummy, dummy, dummy, zero, 4, 64, 128, 64, zero, 0, zero) == _capi.ERR_UNSUPPORTED
    assert L.mvhmr_conv1x1_wgrad_deterministic(dummy, ctypes.c_void_p(260), dummy, zero, 4, 128, 128, 64, zero, 0, zero) == _capi.ERR_INVALID_ARGUMENT
    assert L.mvhmr_conv1x1_wgrad_deterministic(dummy, dummy, dummy, zero, 4, 128, 128, 64, zero, 0, zero) == _capi.ERR_WORKSPACE


class _Features:
    """what VolumeGenerator._fused_path_applies reads of its features argument, without device memory"""
    is_cuda, dtype, device = True, torch.float32, torch.device("cpu")

    def __init__(self, shape, address=256, contiguous=True):
        self.shape, self._address, self._contiguous = shape, address, contiguous

    def data_ptr(self):
        return self._address

    def is_contiguous(self):
        return self._contiguous


def _generator(c_in=128, c_out=128):
    return aggregation.VolumeGenerator(volume_size=32, input_channels=c_in, output_channels=c_out, device="cpu")


def test_fused_path_is_refused_above_the_grid_limit():
    gen = _generator()
    assert gen._fused_path_applies(_Features((2, 4, 128, 32, 32)), 32)
    assert gen._fused_path_applies(_Features((13107, 5, 128, 32, 32)), 32)                   # 65535 maps
    assert not gen._fused_path_applies(_Features((8192, 8, 128, 32, 32)), 32)                # 65536 maps
    assert not gen._fused_path_applies(_Features((MAX_MAPS + 1, 1, 128, 32, 32)), 32)


def test_fused_path_is_refused_for_pointers_off_a_16_byte_boundary():
    gen = _generator()
    shape = (2, 4, 128, 32, 32)
    assert gen._fused_path_applies(_Features(shape), 32)
    for offset in (4, 8, 12):
        assert not gen._fused_path_applies(_Features(shape, 256 + offset), 32)
    # a strided view is copied by the fused route (a fresh, aligned allocation) before any kernel reads it
    assert gen._fused_path_applies(_Features(shape, 260, contiguous=False), 32)
    for name in ("weight", "bias"):
        gen = _generator()
        conv = gen.process_feature[0]
        p = getattr(conv, name)
        big = torch.zeros(p.numel() + 1)
        assert big.data_ptr() % 16 == 0
        big[1:].view_as(p).copy_(p.detach())
        getattr(conv, name).data = big[1:].view_as(p)                                        # contiguous, one float off the boundary
        assert getattr(conv, name).data_ptr() % 16 == 4 and getattr(conv, name).is_contiguous()
        assert not gen._fused_path_applies(_Features(shape), 32), name
