"""CPU oracle of the deterministic scale pass (csrc/det_scale.h, unproject_det.hip): the exponent table K[b][c] itself, as an
integer, from the inputs of a deterministic feature backward -- and the rigs test_detscale_gpu.py runs, which test_detscale_cpu.py proves
sound without a GPU.

TEST INFRASTRUCTURE ONLY.  numpy float64 throughout, by det_scale.h's definition: with g = max |grad_out| of the (b, c) row, F = max |feature|
of (b, c) over the pixels the bound ranges over, N the voxels per sample and log2n = ceil log2 N,

    K = 62 - log2n - e,   bound < 2^e (frexp),   0 when the bound is 0,   kDetPoison when it is not < FLT_MAX or an input it reads is not finite

with the bound of every selection as DESIGN.md 5.7 tabulates it.  The maxima are exact in any arithmetic and the bound is a handful of IEEE
double operations in the kernel's own order, so the comparison with the GPU is integer equality.

Which pixels count as tapped (visible, confidence and moments calls) is decided from geomgrad_oracle.sample_cells' fp32 positions,
visibility_oracle.seen_views / moments_oracle.participating and the confidence sampling of confidence_oracle.  A voxel-view within EDGE px of
a pixel boundary (where the seeing test and the tap cell flip), with |z| tiny, or whose confidence sample is within rounding of 0 is an EDGE
voxel-view: `tap_sets` returns the pixels the others surely tap, and those plus the edge voxel-views' taps widened by one pixel.  A rig is
sound when both sets give the same K for every (b, c): `k_table` computes both, the CPU test asserts equality, the GPU test compares."""
import functools
import math

import numpy as np
import torch

from confidence_oracle import conf_unprojection
from geomgrad_oracle import sample_cells
from moments_oracle import participating

POISON = 0x7FFFFFFF
FLT_MAX = 3.4028234663852886e38
EDGE = 0.05                       # px
METHODS = ("softmax", "sum", "mean", "max")


def log2_ceil(n):
    return (int(n) - 1).bit_length() if n > 1 else 0


def exponent(bound, log2n):
    """the tail every selection shares: bound float64 (NaN allowed) -> K"""
    if bound == 0.0:
        return 0
    if not bound < FLT_MAX:
        return POISON
    return 62 - log2n - math.frexp(bound)[1]


def _amax(x, axis):
    """max |x| in float64 with Inf / NaN sorting above every finite value (as the integer maxima on the bits do); an empty range gives 0"""
    a = np.abs(np.asarray(x, np.float64))
    return np.where(np.isfinite(a), a, np.inf).max(axis=axis, initial=0.0)


# ------------------------------------------------------------------------------------------ tapped pixels
def _cells(proj, coords, H, W):
    """fp32 z, ix, iy (B, V, N) in the kernels' rounding, as float64 numpy"""
    P32, X32 = torch.as_tensor(np.asarray(proj, np.float32)), torch.as_tensor(np.asarray(coords, np.float32))
    B, V = P32.shape[:2]
    out = np.zeros((3, B, V, int(np.prod(X32.shape[1:4]))))
    for b in range(B):
        for v in range(V):
            with np.errstate(all="ignore"):
                _, _, z, ix, iy = sample_cells(P32[b, v], X32[b].reshape(-1, 3), H, W)
            out[:, b, v] = z.double().numpy(), ix.double().numpy(), iy.double().numpy()
    return out


def _conf_samples(proj, coords, conf):
    """(c, cabs), each (B, V, N) float64: the confidence sample of every voxel-view and the same with |pixel| for pixel (its rounding scale),
    from confidence_oracle's sampling: samples <= 0 are selected away there, so the signed sample is the difference of two calls"""
    conf = np.asarray(conf, np.float64)
    B, V, H, W = conf.shape
    vol = tuple(np.asarray(coords).shape[1:4])
    zf, zg = np.zeros((B, V, 1, H, W)), np.zeros((B, 1) + vol)

    def sample(maps):
        return conf_unprojection(zf, proj, coords, maps, zg, "sum", geometry=False)["csample"]

    return sample(conf) - sample(-conf), sample(np.abs(conf))


def footprint(proj, coords, H, W):
    """(B, V, H, W) bool: the pixels any voxel-view with taps touches, whatever the selection says about it"""
    z, ix, iy = _cells(proj, coords, H, W)
    fp = np.zeros(z.shape[:2] + (H, W), bool)
    any_ = (z > 0) & (ix > -1) & (ix < W) & (iy > -1) & (iy < H)
    for b, v, n in zip(*np.nonzero(any_)):
        x0, y0 = int(math.floor(ix[b, v, n])), int(math.floor(iy[b, v, n]))
        fp[b, v, np.clip([y0, y0, y0 + 1, y0 + 1], 0, H - 1), np.clip([x0, x0 + 1, x0, x0 + 1], 0, W - 1)] = True
    return fp


def tap_sets(proj, coords, H, W, mask=None, visible=False, conf=None):
    """(sure, possible), each (B, V, H, W) bool -- the marks of k_det_mark: a voxel-view marks its four clamped taps iff its view is present,
    sees the voxel (visible), has taps at all, and (conf) its confidence sample is > 0"""
    z, ix, iy = _cells(proj, coords, H, W)
    B, V, N = z.shape
    take = participating(proj, coords, H, W, mask, visible) & (z > 0) & (ix > -1) & (ix < W) & (iy > -1) & (iy < H)
    with np.errstate(all="ignore"):
        edge = (np.abs(ix - np.rint(ix)) < EDGE) | (np.abs(iy - np.rint(iy)) < EDGE) | (np.abs(z) < 1e-3 * np.abs(z).max())
    edge |= ~np.isfinite(ix) | ~np.isfinite(iy)
    if conf is not None:
        c, cabs = _conf_samples(proj, coords, conf)
        take &= c > 0
        edge |= np.abs(c) < 1e-4 * cabs                     # an fp32 bilinear sample errs by a few 2^-24 of sum w |pixel|
    if mask is not None:
        edge &= (np.asarray(mask) != 0)[:, :, None]          # an absent view taps nothing, wherever it projects
    sure, poss = np.zeros((B, V, H, W), bool), np.zeros((B, V, H, W), bool)
    for b, v, n in zip(*np.nonzero((take & ~edge) | (edge & np.isfinite(ix) & np.isfinite(iy)))):
        x0, y0 = int(math.floor(ix[b, v, n])), int(math.floor(iy[b, v, n]))
        if edge[b, v, n]:
            win = (b, v, slice(max(y0 - 1, 0), max(y0 + 3, 0)), slice(max(x0 - 1, 0), max(x0 + 3, 0)))
            with np.errstate(invalid="ignore"):
                if conf is None or (np.asarray(conf)[win] > 0).any():          # (weights >= 0: no positive pixel in reach, no sample > 0)
                    poss[win] = True
        else:
            sure[b, v, np.clip([y0, y0, y0 + 1, y0 + 1], 0, H - 1), np.clip([x0, x0 + 1, x0, x0 + 1], 0, W - 1)] = True
    return sure, sure | poss


# ------------------------------------------------------------------------------------------ K
def uses_marks(rig):
    return bool(rig.get("moments")) or (rig["method"] == "softmax" and (rig.get("visible") or rig.get("conf") is not None))


def _present(rig):
    """(B, V) bool: the views packed into slots -- mask, and with weights those of weight > 0"""
    f = rig["features"]
    p = np.ones(f.shape[:2], bool) if rig.get("mask") is None else np.asarray(rig["mask"]) != 0
    if rig.get("weights") is not None:
        with np.errstate(invalid="ignore"):
            p = p & (np.asarray(rig["weights"]) > 0)
    return p


def _k(rig, tapped):
    """K (B, C) int64 for F over `tapped` ((B, V, H, W) bool; None: every pixel of the present views)"""
    feats = np.asarray(rig["features"], np.float32)
    B, V, C, H, W = feats.shape
    go = np.asarray(rig["grad_out"], np.float32)
    N = int(np.prod(go.shape[2:]))
    log2n = log2_ceil(N)
    method, halves = rig["method"], rig.get("moments", 0)
    present = _present(rig)
    sel = np.broadcast_to(present[:, :, None, None], (B, V, H, W)) if tapped is None else tapped
    F = _amax(np.where(sel[:, :, None], feats, 0.0), axis=(1, 3, 4))                                 # (B, C)
    G = _amax(go.reshape(go.shape[0], go.shape[1], N), axis=2)                                       # (rows, C or 2C)
    K = np.zeros((B, C), np.int64)
    for b in range(B):
        nb = int(present[b].sum())
        wmax = cmax = log2c = 0
        if rig.get("weights") is not None:
            wmax = float(np.where(present[b], np.asarray(rig["weights"], np.float32)[b], 0.0).max(initial=0.0))
        if rig.get("conf") is not None:
            maps = np.asarray(rig["conf"], np.float32)[b][present[b]]
            with np.errstate(invalid="ignore"):
                cmax = float(np.where(maps > 0, maps, 0.0).max(initial=0.0))                          # NaN and negative pixels never raise it
        rows = [b]
        if rig.get("index") is not None:
            rows = [m for m, i in enumerate(rig["index"]) if i == b]
            if not rows:
                continue                                                                          # named by nobody: K = 0 before any poison test
            log2c = log2_ceil(len(rows))
        for c in range(C):
            f = float(F[b, c])
            if halves:
                gm = float(G[b, c]) if halves == 2 else 0.0
                gv = float(G[b, (halves - 1) * C + c])
                if not (math.isfinite(gm) and math.isfinite(gv) and math.isfinite(f)):
                    K[b, c] = POISON
                    continue
                K[b, c] = exponent(gm + 4.0 * gv * f, log2n)
                continue
            g = max(float(G[m, c]) for m in rows)
            reads_c = rig.get("conf") is not None and method == "sum"
            if not math.isfinite(g) or (method == "softmax" and not math.isfinite(f)) or (reads_c and not math.isfinite(cmax)):
                K[b, c] = POISON
                continue
            with np.errstate(all="ignore"):
                if method == "softmax":
                    bound = g * (1.0 + 2.0 * f)
                elif rig.get("conf") is not None:
                    bound = g * cmax if method == "sum" else g
                elif rig.get("visible"):
                    bound = g
                elif rig.get("weights") is not None:
                    bound = float(np.float64(g) * np.float64(wmax)) if method == "sum" else g      # (0 * Inf = NaN: poison)
                elif rig.get("mask") is not None:
                    bound = g / max(nb, 1) if method == "mean" else g
                else:
                    bound = g / V if method == "mean" else g
            k = exponent(bound, log2n)
            K[b, c] = k if k in (0, POISON) else k - log2c
    return K


def k_table(rig):
    """(K over the surely tapped pixels, K over the possibly tapped ones); the same table twice for a selection without marks"""
    if not uses_marks(rig):
        k = _k(rig, None)
        return k, k
    H, W = rig["features"].shape[3:]
    sure, poss = tap_sets(rig["proj"], rig["coords"], H, W, rig.get("mask"), bool(rig.get("visible")), rig.get("conf"))
    return _k(rig, sure), _k(rig, poss)


# ------------------------------------------------------------------------------------------ rigs
def cameras(B, V, H, W):
    """(B, V, 3, 4) fp32 pin-hole ring around the origin, 5 m away.  The 1 m cube at the origin projects into the middle half of either
    extent (quirk Q1: u is normalised by Hf, v by Wf), so the maps are larger than the volume's footprint; the LAST view's principal point
    is shifted so that part of the volume falls off the map's corner (voxel-views without taps, and with taps but unseen)."""
    P = np.zeros((B, V, 3, 4))
    for b in range(B):
        for v in range(V):
            az = 2 * np.pi * v / V + 0.3 + 0.1 * b
            eye = np.array([5000 * np.cos(az), 5000 * np.sin(az), 1500.0])
            fwd = -eye / np.linalg.norm(eye)
            right = np.cross(fwd, [0, 0, 1.0])
            right /= np.linalg.norm(right)
            up = np.cross(fwd, right)
            cu, cv = (0.05, 0.15) if v == V - 1 and V > 1 else (0.5, 0.5)
            R = np.stack([2.5 * H * right + cu * H * fwd, 2.5 * W * up + cv * W * fwd, fwd])
            P[b, v, :, :3] = R
            P[b, v, :, 3] = -R @ eye
    return P.astype(np.float32)


def volume(B, vol, side=1000.0, theta=0.3):
    X, Y, Z = vol
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).astype(np.float64)
    pts = -side / 2 + g * (side / np.maximum(np.array([X, Y, Z]) - 1, 1))
    ct, st = np.cos(theta), np.sin(theta)
    pts = pts @ np.array([[ct, -st, 0], [st, ct, 0], [0, 0, 1.0]]).T
    return np.broadcast_to(pts.astype(np.float32), (B,) + pts.shape).copy()


def _store(x, dtype):
    """fp32 values as the storage type keeps them"""
    return torch.from_numpy(np.asarray(x, np.float32)).to(dtype).float().numpy()


def make_rig(method="softmax", B=2, V=3, C=5, H=10, W=12, vol=(4, 3, 5), seed=0, family="plain", mask=None, weights=None, conf=False, visible=False,
             index=None, moments=0, lens=False, out_dtype=torch.float32, feat_dtype=torch.float32, outside=None, variant="auto", var_scale=1.0,
             cams=None):
    """One rig: a dict of numpy inputs (features and grad_out hold the values their storage type keeps) and what selects the call.
    `outside`: None, or the factor (64, inf) of the value planted more than one pixel outside every view's footprint."""
    rng = np.random.default_rng(seed)
    M = B if index is None else len(index)
    rig = dict(method=method, family=family, variant=variant, out_dtype=out_dtype, feat_dtype=feat_dtype, moments=moments, visible=visible,
               lens=lens, index=None if index is None else list(index),
               proj=cameras(B, V, H, W) if cams is None else cams, coords=volume(M, vol),
               mask=None if mask is None else np.asarray(mask, np.uint8), weights=None if weights is None else np.asarray(weights, np.float32), conf=None)
    feats = rng.uniform(-1.0, 1.0, (B, V, C, H, W))
    go = rng.standard_normal((M, C * max(moments, 1)) + tuple(vol)) * (1.0 + np.arange(M))[:, None, None, None, None]
    if moments:
        go[:, -C:] *= var_scale                              # the variance half
    if conf:
        cm = rng.uniform(0.2, 1.0, (B, V, H, W))
        cm[0, 0, :, W // 2:] *= -1.0                          # half of one map is negative: the views it covers are absent there
        cm[0, 1, 0, 0], cm[0, 1, 1, 1] = -50.0, np.nan        # neither raises cmax
        cm[0, 1, 2, 2] = 3.5                                  # the largest pixel of sample 0
        cm[B - 1] = -rng.uniform(0.1, 0.5, (V, H, W))         # a sample whose maps are all <= 0: no view takes part
        rig["conf"] = cm.astype(np.float32)
    rig["features"] = feats.astype(np.float32)
    rig["grad_out"] = go.astype(np.float32)
    if uses_marks(rig) or outside is not None:
        sure, poss = tap_sets(rig["proj"], rig["coords"], H, W, rig["mask"], visible, rig["conf"])
        fp = footprint(rig["proj"], rig["coords"], H, W)
        wide = np.zeros_like(fp)                             # the footprints widened by two pixels
        for b, v, y, x in zip(*np.nonzero(fp)):
            wide[b, v, max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = True
        present = _present(rig)
        for b in range(B):
            pix = np.argwhere(sure[b])
            for c in range(C):
                if len(pix):                                 # one dominant value per (b, c), at a pixel a sure voxel-view taps
                    v, y, x = pix[(7 * c + 3 * b) % len(pix)]
                    feats[b, v, c, y, x] = 8.0 * (1.0 + 0.37 * (b * C + c)) * (-1.0) ** c
            hidden = np.argwhere(fp[b] & ~poss[b] & present[b][:, None, None])
            if len(hidden):                                  # tapped only by voxel-views the selection leaves out: must not count
                v, y, x = hidden[0]
                feats[b, v, :, y, x] = 4096.0
            if outside is not None:
                v, y, x = np.argwhere(~wide[b] & present[b][:, None, None])[0]
                feats[b, v, :, y, x] = outside * 8.0 * (1.0 + 0.37 * (b * C + np.arange(C)))
        rig["hidden"] = bool(len(np.argwhere(fp & ~poss & present[:, :, None, None])))
    rig["features"] = _store(feats, feat_dtype)
    rig["grad_out"] = _store(go, out_dtype)
    return rig


def _with(rig, **edits):
    """a copy of the rig with elements overwritten: name -> (index, value)"""
    rig = dict(rig)
    for name, (idx, value) in edits.items():
        rig[name] = np.array(rig[name], copy=True)
        rig[name][idx] = value
    return rig


@functools.lru_cache(maxsize=None)
def rigs():
    """name -> rig: every case of test_detscale_gpu.py, each the smallest at which the pass can go wrong"""
    inf, nan = float("inf"), float("nan")
    r = {}
    for m in METHODS:
        r["plain %s" % m] = make_rig(m)
        r["lens %s" % m] = make_rig(m, family="lens", lens=True)                                     # K does not depend on where the taps land
        r["visible %s" % m] = make_rig(m, family="visible", visible=True, outside=64.0)
        r["masked %s" % m] = make_rig(m, B=3, family="masked", mask=[[1, 1, 1], [0, 1, 0], [0, 0, 0]])    # n_b = 3, 1, 0
    r["plain sum N=64"] = make_rig("sum", vol=(4, 4, 4))                                            # ceil log2 N: 6 ...
    r["plain sum N=65"] = make_rig("sum", vol=(5, 13, 1))                                           # ... against 7
    # storage: grad_out as fp32 (above), fp16 and bf16, features as fp32 and fp16 -- on the gather route, whose maxima read them as stored
    # (the plain AUTO rigs above take the bricks, whose quad-planar copy is fp32: k_det_fmax_quad, with pad channels)
    r["gather softmax f16 f16"] = make_rig("softmax", feat_dtype=torch.float16, out_dtype=torch.float16, variant="gather")
    r["gather softmax f32 bf16"] = make_rig("softmax", out_dtype=torch.bfloat16, variant="gather")
    r["gather sum f32 bf16"] = make_rig("sum", out_dtype=torch.bfloat16, variant="gather")
    r["visible softmax f16 f16"] = make_rig("softmax", family="visible", visible=True, outside=64.0, feat_dtype=torch.float16, out_dtype=torch.float16)
    for m in ("softmax", "sum", "mean"):
        r["weighted %s" % m] = make_rig(m, family="weighted", weights=[[0.5, 2.5, 1.0], [0.25, 0.75, 0.5]])    # wmax > 1 and < 1
        r["weighted inf %s" % m] = make_rig(m, family="weighted", weights=[[0.5, inf, 1.0], [0.25, 0.75, 0.5]])   # poisons sum only
        for vis in (False, True):
            r["confidence %s%s" % (m, " visible" if vis else "")] = make_rig(m, family="confidence", conf=True, visible=vis, outside=64.0)
    for m in METHODS:
        r["shared M=3 %s" % m] = make_rig(m, family="shared", index=[1, -1, 1])                      # one outside [0, B), sample 1 twice
    nobody = make_rig("softmax", family="shared", index=[0, 5])
    r["shared M=2 nobody"] = _with(nobody, features=((1, 0, 2, 3, 4), inf))                           # sample 1: K = 0 even so
    for halves in (1, 2):
        for vis in (False, True):
            r["moments %d%s" % (halves, " visible" if vis else "")] = make_rig("mean", family="moments", moments=halves, visible=vis, outside=64.0,
                                                                              var_scale=2.0 ** 20)
    r["visible softmax inf outside"] = make_rig("softmax", family="visible", visible=True, outside=inf)
    r["moments 2 visible inf outside"] = make_rig("mean", family="moments", moments=2, visible=True, outside=inf)
    # the brick route (k_det_fmax_quad): the smallest shapes the deterministic plan hands to the bricks
    r["brick softmax C=32"] = make_rig("softmax", B=2, V=4, C=32, H=120, W=120, vol=(8, 16, 32), variant="brick", cams=None)
    r["brick softmax C=6"] = make_rig("softmax", B=2, V=4, C=6, H=120, W=120, vol=(8, 16, 32), variant="brick")
    # non-finite inputs: Inf in one grad_out row; NaN in one tapped feature pixel (poisons softmax, not sum)
    for m in ("softmax", "sum"):
        base = r["plain %s" % m]
        r["plain %s inf grad" % m] = _with(base, grad_out=((1, 2, 1, 1, 1), inf))
        r["plain %s nan feature" % m] = _with(base, features=((0, 1, 3, 5, 6), nan))
    vis = r["visible softmax"]
    v, y, x = np.argwhere(tap_sets(vis["proj"], vis["coords"], 10, 12, None, True)[0][0])[0]
    r["visible softmax nan tapped"] = _with(vis, features=((0, v, 3, y, x), nan))
    return r


# ------------------------------------------------------------------------------------------ the call of a rig
def call_of(rig, pointers, placing=0):
    """(Desc, Call) of the rig's deterministic feature backward.  pointers: name -> address for features, proj, grad_out, grad_features,
    coords and whichever of mask, weights, conf, index, lens the rig has (the plan depends on which are non-null, never on what they hold)"""
    from multiviewhmr_amd import _capi
    B, V, C, H, W = rig["features"].shape
    X, Y, Z = rig["grad_out"].shape[2:]
    code = {torch.float32: _capi.F32, torch.float16: _capi.F16, torch.bfloat16: _capi.BF16}
    d = _capi.Desc(abi_version=_capi.ABI_VERSION, batch=B, views=V, channels=C, feat_h=H, feat_w=W, vol_x=X, vol_y=Y, vol_z=Z,
                   method=_capi.AGG[rig["method"]], feat_dtype=code[rig["feat_dtype"]], out_dtype=code[rig["out_dtype"]],
                   feat_layout=_capi.LAYOUT_BVCHW, variant=_capi.VARIANT[rig["variant"]])
    fam = rig["family"]
    fields = dict(deterministic=1, features=pointers["features"], proj=pointers["proj"], grad_out=pointers["grad_out"],
                  grad_features=pointers["grad_features"])
    if placing == _capi.PLACING_CUBOID:
        fields.update(rot=pointers["rot"], center=pointers["center"], position=pointers["position"], sides=pointers["sides"])
    else:
        fields["coords"] = pointers["coords"]
    for key, field in (("mask", "view_mask"), ("weights", "view_weights"), ("conf", "view_confidence"), ("index", "feature_index")):
        if rig.get(key) is not None:
            fields[field] = pointers[key]
    if rig.get("lens"):
        fields["lens"] = pointers["lens"]
    if fam in ("confidence", "moments"):
        fields["visible"] = int(bool(rig["visible"]))
    if fam == "moments":
        fields["moments"] = rig["moments"]
    if fam == "shared":
        fields["volumes"] = len(rig["index"])
    return d, _capi.record(fam, placing, **fields)
