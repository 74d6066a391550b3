"""Guard bands and poison through the C ABI: every buffer a call touches is owned by the test.

The numeric tests compare output values, and two kinds of bug leave those right on the day of the test: bytes read outside a tensor
(fresh allocator memory is usually zero or finite leftovers) and bytes that are never written (an output the allocator happened to
zero).  Here every caller buffer -- inputs, outputs, the workspace at exactly its *_workspace_bytes size -- is a view into a larger
allocation with a 4 MiB guard on each side (start offsets multiples of 4 KiB).  Guards of float inputs and of the mask hold 0xFF
bytes (NaN in fp32 / fp16 / bf16; "present" for the mask), so a stray read times a zero weight turns the output NaN.  Outputs and the
workspace are filled with 0xFF (NaN) before the call, then again with 0x7F (a large finite value): an element that is never written,
or a workspace byte read before it is written, shows up against the oracle, and the forward, the deterministic backward and the
geometry backward must give the same bits under both fills.  After each call every guard byte must be unchanged and every input
bitwise intact."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import record_err
from geomgrad_oracle import geometry_grad
from multiviewhmr_amd import _capi, volumetric
from oracle import cport
from posegrad_oracle import cuboid_points, pose_grad
from test_unproject_gpu import TOL, _bound, _err, _ring_problem

pytestmark = pytest.mark.gpu

GUARD = 4 << 20
PAGE = 4096
POISONS = (0xFF, 0x7F)
REL = 1e-4                                  # geometry gradients: 1e-4 of the largest oracle value (test_geometry_grad_gpu.py)
vp, sz = ctypes.c_void_p, ctypes.c_size_t


def _lib():
    L = ctypes.CDLL(_capi.LIB_PATH)
    for n in _capi.EXPORTS:
        if n.endswith("_workspace_bytes") or n == "mvhmr_feature_layout_bytes":
            getattr(L, n).restype = ctypes.c_size_t
    L.mvhmr_unproject_forward_kernel_name.restype = ctypes.c_char_p
    L.mvhmr_last_error.restype = ctypes.c_char_p
    return L


class Buf:
    """nbytes at a 4-KiB-aligned offset GUARD into an allocation of GUARD + round_up(nbytes, 4 KiB) + GUARD bytes, all `fill`"""

    def __init__(self, gpu, nbytes, fill):
        self.n, self.fill = int(nbytes), fill
        span = (self.n + PAGE - 1) // PAGE * PAGE
        self.arena = torch.full((2 * GUARD + span,), fill, dtype=torch.uint8, device=gpu)
        assert (self.arena.data_ptr() + GUARD) % 256 == 0

    @property
    def ptr(self):
        return vp(self.arena.data_ptr() + GUARD)

    def bytes(self):
        return self.arena[GUARD:GUARD + self.n]

    def view(self, dtype, shape):
        return self.bytes().view(dtype).view(shape)

    def guards_intact(self):
        return bool((self.arena[:GUARD] == self.fill).all()) and bool((self.arena[GUARD + self.n:] == self.fill).all())


def _raw(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _guarded(gpu, inputs, outputs, ws_bytes, poison, launch):
    """inputs {name: device tensor in its storage layout}, outputs {name: (dtype, shape)}; launch(p) makes the call with p[name] the
    address of each buffer (p['ws'] the workspace, p['ws_bytes'] its size) and returns its status -> {name: output tensor}"""
    bufs = {}
    for k, t in inputs.items():
        b = Buf(gpu, t.numel() * t.element_size(), 0xFF)
        b.bytes().copy_(_raw(t))
        bufs[k] = b
    for k, (dt, shape) in outputs.items():
        bufs[k] = Buf(gpu, int(np.prod(shape)) * torch.empty((), dtype=dt).element_size(), poison)
    bufs["ws"] = Buf(gpu, ws_bytes, poison)
    p = {k: b.ptr for k, b in bufs.items()}
    p["ws_bytes"] = sz(ws_bytes)
    p["stream"] = vp(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    st = launch(p)
    torch.cuda.synchronize()
    assert st == 0, (st, _lib().mvhmr_last_error())
    for k, b in bufs.items():
        assert b.guards_intact(), "bytes outside `%s` changed (poison 0x%02X)" % (k, poison)
    for k, t in inputs.items():
        assert torch.equal(bufs[k].bytes(), _raw(t)), "input `%s` was written" % k
    return {k: bufs[k].view(dt, shape).clone() for k, (dt, shape) in outputs.items()}


def _both(gpu, inputs, outputs, ws_bytes, launch):
    return [_guarded(gpu, inputs, outputs, ws_bytes, poison, launch) for poison in POISONS]


def _bitwise(name, a, b):
    for k in a:
        assert torch.equal(_raw(a[k]), _raw(b[k])), "%s: `%s` depends on what the buffers held before the call" % (name, k)


def _desc(B, V, C, H, W, vol, method="softmax", fdt=_capi.F32, odt=_capi.F32, layout=_capi.LAYOUT_BVCHW, variant="auto"):
    d = _capi.Desc()
    d.abi_version = _capi.ABI_VERSION
    d.batch, d.views, d.channels, d.feat_h, d.feat_w = B, V, C, H, W
    d.vol_x, d.vol_y, d.vol_z = vol
    d.method, d.feat_dtype, d.out_dtype, d.feat_layout, d.variant = _capi.AGG[method], fdt, odt, layout, _capi.VARIANT[variant]
    return d


def _cl(f):
    return f.permute(0, 1, 3, 4, 2).contiguous()                                  # (B,V,H,W,C) storage


def _problem(gpu, shape, seed, theta=0.3):
    feats, proj, coords = _ring_problem(seed=seed, theta=theta, **shape)
    X, Y, Z = shape["vol"]
    go = np.random.default_rng(seed + 1).standard_normal((shape["B"], shape["C"], X, Y, Z), dtype=np.float32)
    t = lambda a: torch.from_numpy(a).to(gpu)
    return feats, proj, coords, go, t(feats), t(proj), t(coords), t(go)


def _fwd_bwd(gpu, name, shape, variant, layout, kernels, method="softmax", seed=3, geometry=True):
    """forward, default backward, deterministic backward and geometry backward of one tensor-route problem"""
    L = _lib()
    B, V, C, H, W, vol = shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"]
    feats, proj, coords, go, f, p, c, g = _problem(gpu, shape, seed)
    fin = _cl(f) if layout == _capi.LAYOUT_BVHWC else f
    d = _desc(B, V, C, H, W, vol, method, layout=layout, variant=variant)
    D = ctypes.byref(d)
    if kernels:
        assert L.mvhmr_unproject_forward_kernel_name(D).decode() in kernels
    out_shape = (B, C) + tuple(vol)
    ref = cport.forward(feats, proj, coords, method)
    fw = _both(gpu, {"f": fin, "p": p, "c": c}, {"out": (torch.float32, out_shape)}, L.mvhmr_unproject_forward_workspace_bytes(D),
               lambda q: L.mvhmr_unproject_forward(D, q["f"], q["p"], q["c"], q["out"], q["ws"], q["ws_bytes"], q["stream"]))
    for k, r in enumerate(fw):
        record_err("guard %s fwd poison %d" % (name, k), _err(r["out"].cpu().numpy(), ref), _bound(ref))
    _bitwise(name + " fwd", *fw)

    gref = cport.backward(go, feats, proj, coords, method)
    gshape = (B, V, C, H, W) if layout != _capi.LAYOUT_BVHWC else (B, V, H, W, C)
    unl = (lambda t: t.permute(0, 1, 4, 2, 3)) if layout == _capi.LAYOUT_BVHWC else (lambda t: t)
    bw = _both(gpu, {"g": g, "f": fin, "p": p, "c": c}, {"gf": (torch.float32, gshape)}, L.mvhmr_unproject_backward_workspace_bytes(D),
               lambda q: L.mvhmr_unproject_backward(D, q["g"], q["f"], q["p"], q["c"], q["gf"], q["ws"], q["ws_bytes"], q["stream"]))
    for k, r in enumerate(bw):                                                     # float atomics: within the oracle's bound
        record_err("guard %s bwd poison %d" % (name, k), _err(unl(r["gf"]).cpu().numpy(), gref), _bound(gref))
    dt = _both(gpu, {"g": g, "f": fin, "p": p, "c": c}, {"gf": (torch.float32, gshape)},
               L.mvhmr_unproject_backward_deterministic_workspace_bytes(D),
               lambda q: L.mvhmr_unproject_backward_deterministic(D, q["g"], q["f"], q["p"], q["c"], q["gf"], q["ws"], q["ws_bytes"], q["stream"]))
    for k, r in enumerate(dt):
        record_err("guard %s det bwd poison %d" % (name, k), _err(unl(r["gf"]).cpu().numpy(), gref), _bound(gref))
    _bitwise(name + " det bwd", *dt)
    if not geometry:
        return
    gp_ref, gc_ref = geometry_grad(feats, proj, coords, go, method)
    ge = _both(gpu, {"g": g, "f": fin, "p": p, "c": c}, {"gp": (torch.float32, (B, V, 3, 4)), "gc": (torch.float32, (B,) + tuple(vol) + (3,))},
               L.mvhmr_unproject_backward_geometry_workspace_bytes(D),
               lambda q: L.mvhmr_unproject_backward_geometry(D, q["g"], q["f"], q["p"], q["c"], q["gp"], q["gc"], q["ws"], q["ws_bytes"], q["stream"]))
    for k, r in enumerate(ge):
        record_err("guard %s geom proj poison %d" % (name, k), _err(r["gp"].cpu().numpy(), gp_ref), REL * float(np.abs(gp_ref).max()))
        record_err("guard %s geom coords poison %d" % (name, k), _err(r["gc"].cpu().numpy(), gc_ref.reshape(r["gc"].shape)),
                   REL * float(np.abs(gc_ref).max()))
    _bitwise(name + " geom", *ge)


def test_gather_family_planar_and_channels_last(gpu):
    """k_fwd_gather with C % 4 != 0 on a ragged volume; its backward is the plane kernel for planar features and the per-tap scatter
    for channels-last ones"""
    shape = dict(B=2, V=3, C=6, H=24, W=40, vol=(9, 7, 13))
    _fwd_bwd(gpu, "gather planar", shape, "gather", _capi.LAYOUT_BVCHW, ("k_fwd_gather",))
    shape["C"] = 8                                                                 # channels-last features need C % 4 == 0
    _fwd_bwd(gpu, "gather channels-last", shape, "gather", _capi.LAYOUT_BVHWC, None, seed=5)   # (the kernel-name query takes planar / quad descriptors)


@pytest.mark.parametrize("method", ("softmax", "max"))
def test_brick_kernels_on_a_ragged_volume(method, gpu):
    """k_fwd_brick / k_fwd_brick_groups below 256 bricks (30 here), 3 views (one absent slot), C % 4 != 0 (the tail kernels), and k_bwd_brick"""
    shape = dict(B=1, V=3, C=6, H=24, W=24, vol=(20, 36, 44))
    _fwd_bwd(gpu, "brick %s" % method, shape, "brick", _capi.LAYOUT_BVCHW, ("k_fwd_brick", "k_fwd_brick_groups"), method=method, seed=11,
             geometry=False)


def test_plane_backward_at_the_shipped_config(gpu):
    """the reference's shipped 16^3 volume on 12 x 12 maps: gather forward, plane backward"""
    shape = dict(B=2, V=4, C=8, H=12, W=12, vol=(16, 16, 16))
    _fwd_bwd(gpu, "shipped 16^3 12x12", shape, "auto", _capi.LAYOUT_BVCHW, None, seed=13, geometry=False)


@pytest.mark.parametrize("shape,odt", [
    (dict(B=16, V=4, C=8, H=48, W=48, vol=(32, 32, 32)), _capi.F32),               # the north star's kernel at a small batch
    (dict(B=9, V=4, C=8, H=40, W=56, vol=(20, 35, 40)), _capi.F16),                # ragged, 16-bit volume
    (dict(B=9, V=4, C=8, H=40, W=56, vol=(20, 35, 40)), _capi.BF16),
    (dict(B=4, V=4, C=4, H=400, W=400, vol=(64, 64, 32)), _capi.F32),              # no window fits: the compute waves' global path
])
def test_wave_specialised_forward(shape, odt, gpu):
    L = _lib()
    B, V, C, H, W, vol = shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"]
    feats, proj, coords, go, f, p, c, g = _problem(gpu, shape, seed=17)
    fdt = _capi.F16 if odt == _capi.F16 else _capi.F32                              # an fp16 volume goes with fp16 features
    if fdt == _capi.F16:
        feats = feats.astype(np.float16).astype(np.float32)
        f = f.half()
    d = _desc(B, V, C, H, W, vol, fdt=fdt, odt=odt, variant="brick")
    D = ctypes.byref(d)
    assert L.mvhmr_unproject_forward_kernel_name(D).decode() == "k_fwd_ws"
    tdt = {_capi.F32: torch.float32, _capi.F16: torch.float16, _capi.BF16: torch.bfloat16}[odt]
    ref = cport.forward(feats, proj, coords, "softmax")
    fw = _both(gpu, {"f": f, "p": p, "c": c}, {"out": (tdt, (B, C) + tuple(vol))}, L.mvhmr_unproject_forward_workspace_bytes(D),
               lambda q: L.mvhmr_unproject_forward(D, q["f"], q["p"], q["c"], q["out"], q["ws"], q["ws_bytes"], q["stream"]))
    rnd = {_capi.F32: 0.0, _capi.F16: 2.0 ** -11, _capi.BF16: 2.0 ** -8}[odt]
    for k, r in enumerate(fw):
        record_err("guard k_fwd_ws %dx%d vol%s dtype %d poison %d" % (H, W, vol, odt, k), _err(r["out"].float().cpu().numpy(), ref),
                   _bound(ref) + rnd * float(np.abs(ref).max()))
    _bitwise("k_fwd_ws", *fw)


def test_quad_planar_input_forward_and_backward(gpu):
    """mvhmr_convert_features' output (itself written into a guarded, poisoned buffer) handed to the forward and the backward"""
    L = _lib()
    shape = dict(B=16, V=4, C=8, H=48, W=48, vol=(32, 32, 32))
    B, V, C, H, W, vol = shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"]
    feats, proj, coords, go, f, p, c, g = _problem(gpu, shape, seed=19)
    ref, gref = cport.forward(feats, proj, coords, "softmax"), cport.backward(go, feats, proj, coords, "softmax")
    for lay in (_capi.LAYOUT_QUAD_LOG2E, _capi.LAYOUT_QUAD):
        d_pl = _desc(B, V, C, H, W, vol)
        nq = L.mvhmr_feature_layout_bytes(ctypes.byref(d_pl), lay)
        cv = _both(gpu, {"f": f}, {"q": (torch.uint8, (nq,))}, 0,
                   lambda q: L.mvhmr_convert_features(ctypes.byref(d_pl), q["f"], lay, q["q"], q["stream"]))
        _bitwise("convert layout %d" % lay, *cv)
        quad = cv[0]["q"]
        d = _desc(B, V, C, H, W, vol, layout=lay)
        D = ctypes.byref(d)
        fw = _both(gpu, {"f": quad, "p": p, "c": c}, {"out": (torch.float32, (B, C) + tuple(vol))}, L.mvhmr_unproject_forward_workspace_bytes(D),
                   lambda q: L.mvhmr_unproject_forward(D, q["f"], q["p"], q["c"], q["out"], q["ws"], q["ws_bytes"], q["stream"]))
        for k, r in enumerate(fw):
            record_err("guard quad layout %d fwd poison %d" % (lay, k), _err(r["out"].cpu().numpy(), ref), _bound(ref))
        _bitwise("quad fwd", *fw)
        if lay == _capi.LAYOUT_QUAD_LOG2E:
            continue                                                               # forward only
        bw = _both(gpu, {"g": g, "f": quad, "p": p, "c": c}, {"gf": (torch.float32, (B, V, C, H, W))}, L.mvhmr_unproject_backward_workspace_bytes(D),
                   lambda q: L.mvhmr_unproject_backward(D, q["g"], q["f"], q["p"], q["c"], q["gf"], q["ws"], q["ws_bytes"], q["stream"]))
        for k, r in enumerate(bw):
            record_err("guard quad bwd poison %d" % k, _err(r["gf"].cpu().numpy(), gref), _bound(gref))


def _pose(B, seed):
    rng = np.random.default_rng(seed)
    rot = np.stack([volumetric.get_rotation_matrix(rng.normal(size=3), rng.uniform(0, 2 * np.pi)) for _ in range(B)]).astype(np.float32)
    return rot, rng.uniform(-200.0, 200.0, (B, 3)).astype(np.float32)


def test_cuboid_route(gpu):
    """forward, backward, deterministic backward and geometry backward of the cuboid recipe: rotated, a pivot per sample"""
    L = _lib()
    B, V, C, H, W, S = 2, 4, 8, 32, 32, 16
    vol = (S, S, S)
    feats, proj, _ = _ring_problem(B=B, V=V, C=C, H=H, W=W, vol=vol, seed=23)
    go = np.random.default_rng(24).standard_normal((B, C) + vol, dtype=np.float32)
    rot, center = _pose(B, 25)
    pos, sides = (-1250.0, -1250.0, -1250.0), (2500.0, 2500.0, 2500.0)
    P3, S3 = (ctypes.c_double * 3)(*pos), (ctypes.c_double * 3)(*sides)
    coords = cuboid_points(rot, center, pos, sides, vol)[1].numpy()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    f, p, r, ce, g = t(feats), t(proj), t(rot), t(center), t(go)
    d = _desc(B, V, C, H, W, vol)
    D = ctypes.byref(d)
    ins = {"f": f, "p": p, "r": r, "ce": ce}
    ref = cport.forward(feats, proj, coords, "softmax")
    fw = _both(gpu, ins, {"out": (torch.float32, (B, C) + vol)}, L.mvhmr_unproject_forward_workspace_bytes(D),
               lambda q: L.mvhmr_unproject_forward_cuboid(D, q["f"], q["p"], q["r"], q["ce"], P3, S3, q["out"], q["ws"], q["ws_bytes"], q["stream"]))
    for k, res in enumerate(fw):
        record_err("guard cuboid fwd poison %d" % k, _err(res["out"].cpu().numpy(), ref), _bound(ref))
    _bitwise("cuboid fwd", *fw)
    gref = cport.backward(go, feats, proj, coords, "softmax")
    ins_g = dict(ins, g=g)
    bw = _both(gpu, ins_g, {"gf": (torch.float32, (B, V, C, H, W))}, L.mvhmr_unproject_backward_workspace_bytes(D),
               lambda q: L.mvhmr_unproject_backward_cuboid(D, q["g"], q["f"], q["p"], q["r"], q["ce"], P3, S3, q["gf"], q["ws"], q["ws_bytes"],
                                                           q["stream"]))
    for k, res in enumerate(bw):
        record_err("guard cuboid bwd poison %d" % k, _err(res["gf"].cpu().numpy(), gref), _bound(gref))
    dt = _both(gpu, ins_g, {"gf": (torch.float32, (B, V, C, H, W))}, L.mvhmr_unproject_backward_deterministic_workspace_bytes(D),
               lambda q: L.mvhmr_unproject_backward_cuboid_deterministic(D, q["g"], q["f"], q["p"], q["r"], q["ce"], P3, S3, q["gf"], q["ws"],
                                                                         q["ws_bytes"], q["stream"]))
    for k, res in enumerate(dt):
        record_err("guard cuboid det bwd poison %d" % k, _err(res["gf"].cpu().numpy(), gref), _bound(gref))
    _bitwise("cuboid det bwd", *dt)
    gp_ref, gr_ref, gc_ref = pose_grad(feats, proj, rot, center, pos, sides, vol, go, "softmax")
    ge = _both(gpu, ins_g, {"gp": (torch.float32, (B, V, 3, 4)), "gr": (torch.float32, (B, 3, 3)), "gc": (torch.float32, (B, 3))},
               L.mvhmr_unproject_backward_geometry_cuboid_workspace_bytes(D),
               lambda q: L.mvhmr_unproject_backward_geometry_cuboid(D, q["g"], q["f"], q["p"], q["r"], q["ce"], P3, S3, q["gp"], q["gr"], q["gc"],
                                                                    q["ws"], q["ws_bytes"], q["stream"]))
    for k, res in enumerate(ge):
        for key, gref_k in (("gp", gp_ref), ("gr", gr_ref), ("gc", gc_ref)):
            record_err("guard cuboid geom %s poison %d" % (key, k), _err(res[key].cpu().numpy(), gref_k), REL * float(np.abs(gref_k).max()))
    _bitwise("cuboid geom", *ge)


def test_masked_entry_points(gpu):
    """a full, a single-view and an empty sample: masked views' features and cameras are NaN (never read), their gradients exact
    zeros, the empty sample's volume and gradients exact zeros"""
    L = _lib()
    shape = dict(B=3, V=4, C=8, H=24, W=24, vol=(9, 7, 13))
    B, V, C, H, W, vol = shape["B"], shape["V"], shape["C"], shape["H"], shape["W"], shape["vol"]
    feats, proj, coords, go, _, _, c, g = _problem(gpu, shape, seed=29)
    mask = np.array([[1, 1, 1, 1], [0, 0, 1, 0], [0, 0, 0, 0]], np.uint8)
    fz, pz = feats.copy(), proj.copy()
    fz[mask == 0] = np.nan
    pz[mask == 0] = np.nan
    f, p, m = torch.from_numpy(fz).to(gpu), torch.from_numpy(pz).to(gpu), torch.from_numpy(mask).to(gpu)
    ref = np.zeros((B, C) + vol, np.float32)
    gref = np.zeros_like(feats)
    gp_ref, gc_ref = np.zeros((B, V, 3, 4)), np.zeros((B,) + vol + (3,))
    for b in range(B):
        pres = np.flatnonzero(mask[b])
        if len(pres):
            sl = (slice(b, b + 1), pres)
            ref[b] = cport.forward(feats[sl], proj[sl], coords[b:b + 1], "softmax")[0]
            gref[b, pres] = cport.backward(go[b:b + 1], feats[sl], proj[sl], coords[b:b + 1], "softmax")[0]
            gpb, gcb = geometry_grad(feats[sl], proj[sl], coords[b:b + 1], go[b:b + 1], "softmax")
            gp_ref[b, pres], gc_ref[b] = gpb[0], gcb.reshape((1,) + vol + (3,))[0]
    absent = torch.from_numpy(mask == 0)
    for lay in (_capi.LAYOUT_BVCHW, _capi.LAYOUT_BVHWC):
        d = _desc(B, V, C, H, W, vol, layout=lay)
        D = ctypes.byref(d)
        fin = _cl(f) if lay == _capi.LAYOUT_BVHWC else f
        unl = (lambda t: t.permute(0, 1, 4, 2, 3)) if lay == _capi.LAYOUT_BVHWC else (lambda t: t)
        gshape = (B, V, C, H, W) if lay == _capi.LAYOUT_BVCHW else (B, V, H, W, C)
        ins = {"f": fin, "p": p, "c": c, "m": m}
        fw = _both(gpu, ins, {"out": (torch.float32, (B, C) + vol)}, L.mvhmr_unproject_forward_masked_workspace_bytes(D),
                   lambda q: L.mvhmr_unproject_forward_masked(D, q["f"], q["p"], q["c"], q["m"], q["out"], q["ws"], q["ws_bytes"], q["stream"]))
        for k, r in enumerate(fw):
            record_err("guard masked layout %d fwd poison %d" % (lay, k), _err(r["out"].cpu().numpy(), ref), _bound(ref))
            assert int(torch.count_nonzero(_raw(r["out"][2]))) == 0                  # the empty sample: +0.0 everywhere
        _bitwise("masked fwd", *fw)
        ins_g = dict(ins, g=g)
        for det in (False, True):
            fn = L.mvhmr_unproject_backward_deterministic_masked if det else L.mvhmr_unproject_backward_masked
            wsq = L.mvhmr_unproject_backward_deterministic_masked_workspace_bytes if det else L.mvhmr_unproject_backward_masked_workspace_bytes
            bw = _both(gpu, ins_g, {"gf": (torch.float32, gshape)}, wsq(D),
                       lambda q: fn(D, q["g"], q["f"], q["p"], q["c"], q["m"], q["gf"], q["ws"], q["ws_bytes"], q["stream"]))
            for k, r in enumerate(bw):
                gf = unl(r["gf"]).cpu()
                record_err("guard masked layout %d det %d bwd poison %d" % (lay, det, k), _err(gf.numpy(), gref), _bound(gref))
                assert int(torch.count_nonzero(_raw(gf[absent].contiguous()))) == 0    # masked views: exact +0.0
            if det:
                _bitwise("masked det bwd", *bw)
        ge = _both(gpu, ins_g, {"gp": (torch.float32, (B, V, 3, 4)), "gc": (torch.float32, (B,) + vol + (3,))},
                   L.mvhmr_unproject_backward_geometry_masked_workspace_bytes(D),
                   lambda q: L.mvhmr_unproject_backward_geometry_masked(D, q["g"], q["f"], q["p"], q["c"], q["m"], q["gp"], q["gc"], q["ws"],
                                                                        q["ws_bytes"], q["stream"]))
        for k, r in enumerate(ge):
            record_err("guard masked geom proj poison %d" % k, _err(r["gp"].cpu().numpy(), gp_ref), REL * float(np.abs(gp_ref).max()))
            record_err("guard masked geom coords poison %d" % k, _err(r["gc"].cpu().numpy(), gc_ref), REL * float(np.abs(gc_ref).max()))
            assert int(torch.count_nonzero(_raw(r["gp"].cpu()[absent].contiguous()))) == 0
            assert int(torch.count_nonzero(_raw(r["gc"][2]))) == 0
        _bitwise("masked geom", *ge)
