"""The four fp32 MFMA GEMMs of the fused 1x1-conv route (csrc/conv1x1_quad.hip: to_quad, planar, wgrad with float atomics, deterministic
wgrad), through the C ABI, at the shapes where their tiling, double buffering and split-K change behaviour.

1. Exact arithmetic.  v_mfma_f32_32x32x2_f32 is a k-ordered fp32 fma chain, so on operands whose every partial sum (in any order, any
   split, any atomic arrival order) is an integer multiple of one power of two and below 2^24 of it, a correct kernel is BIT-EQUAL to a
   float64 matmul.  Each test asserts that condition on its own inputs first, then torch.equal on the whole output: no tolerance.
2. Rounding on random floats: per element |y - ref| <= (K + 2) * 2^-24 * sum|a||b| -- the textbook bound of a length-K fma chain plus
   one add (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), nothing measured.  The worst err / sum|a||b| is recorded
   only (against a bound no number exceeds).
3. One NaN / Inf poisons exactly the outputs W @ x poisons, everything else keeps its bits.
4. Element offsets past 2^31.  5. VolumeGenerator's fused route with C_in != C_out, with the kernel / fallback choice pinned.
Every comparison goes through conftest.record_err; the equalities record their mismatch count against a bound of 0."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import record_err
from multiviewhmr_amd import _capi, aggregation, multiview

pytestmark = pytest.mark.gpu
VP = ctypes.c_void_p
U = 2.0 ** -24                                     # fp32 unit roundoff
EXACT = 2.0 ** 24                                  # integers below it are fp32 numbers, and so are their sums in any order
NEVER = 1.7976931348623157e308                     # the bound of a value that is recorded, not asserted (finite: the table stays strict JSON)

# (BV, Cin, Cout, H, W): one K chunk (no prefetch) + one tile + one map; an even chunk count + one tile row; an odd chunk count, three
# channel tiles; many tile rows of one tile; tiles_x = 3; the backbone-without-deconv channel count
QUAD_SHAPES = ((1, 16, 128, 4, 32), (2, 32, 128, 4, 64), (3, 48, 384, 8, 32), (1, 64, 128, 64, 32), (2, 256, 256, 96, 96), (1, 2048, 256, 16, 32))
# (BV, Cin, Cout, HW)
PLANAR_SHAPES = ((1, 16, 128, 128), (3, 256, 128, 640), (2, 256, 256, 9216), (1, 256, 2048, 256))
WGRAD_SHAPES = ((1, 128, 128, 32), (2, 256, 128, 64), (1, 128, 256, 9216), (40, 256, 256, 1024), (600, 128, 128, 64), (3000, 128, 128, 64),
                (2, 2048, 256, 1024))


def _p(t):
    return VP(t.data_ptr()) if t is not None else VP(0)


def _s():
    return VP(torch.cuda.current_stream().cuda_stream)


def _gen(gpu, seed):
    return torch.Generator(device=gpu).manual_seed(seed)


def _ints(shape, lo, hi, g):
    """integers lo .. hi as fp32"""
    return torch.randint(lo, hi + 1, shape, device=g.device, generator=g).float()


def _exps(shape, lo, hi, g, on):
    """exponents of the power-of-two scales (all zero when off)"""
    return torch.randint(lo, hi + 1, shape, device=g.device, generator=g).double() if on else torch.zeros(shape, dtype=torch.float64, device=g.device)


def _same(name, got, ref):
    """bit equality of two tensors; the first mismatch is named"""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape)
    bad = got != ref
    n = int(bad.sum())
    if n:
        i = tuple(int(v) for v in bad.nonzero()[0])
        print("%s: %d of %d elements differ, first at %s: got %r, want %r" % (name, n, got.numel(), i, float(got[i]), float(ref[i])))
    record_err(name, n, 0)
    assert torch.equal(got, ref), name


def _quad_view(y, H, W):
    """planar (BV, Cout, H*W) -> MVHMR_LAYOUT_QUAD (BV, Cout/4, W, H, 4)"""
    BV, Cout = y.shape[:2]
    return y.view(BV, Cout // 4, 4, H, W).permute(0, 1, 4, 3, 2).contiguous()


def _planar_view(q):
    """MVHMR_LAYOUT_QUAD (BV, Cout/4, W, H, 4) -> planar (BV, Cout, H*W)"""
    BV, Q, W, H, _ = q.shape
    return q.permute(0, 1, 4, 3, 2).reshape(BV, Q * 4, H * W)


def _to_quad(x, w, b, H, W, out=None):
    BV, Cin, Cout = x.shape[0], x.shape[1], w.shape[0]
    assert x.is_contiguous() and w.is_contiguous() and x.numel() == BV * Cin * H * W and w.shape == (Cout, Cin)
    assert _capi.lib().mvhmr_conv1x1_to_quad_supported(Cin, Cout, H, W) == 1
    q = torch.full((BV, Cout // 4, W, H, 4), float("nan"), device=x.device) if out is None else out      # NaN: "every element is written"
    _capi.check(_capi.lib().mvhmr_conv1x1_to_quad(_p(x), _p(w), _p(b), _p(q), BV, Cin, Cout, H, W, _s()))
    return q


def _planar(x, w, b, out=None):
    BV, Cin, HW = x.shape
    Cout = w.shape[0]
    assert x.is_contiguous() and w.is_contiguous() and w.shape == (Cout, Cin)
    assert _capi.lib().mvhmr_conv1x1_planar_supported(Cin, Cout, HW) == 1
    y = torch.full((BV, Cout, HW), float("nan"), device=x.device) if out is None else out
    _capi.check(_capi.lib().mvhmr_conv1x1_planar(_p(x), _p(w), _p(b), _p(y), BV, Cin, Cout, HW, _s()))
    return y


def _wgrad(gy, x, gw, gb):
    """adds into gw (Cout, Cin) and gb (Cout) or None"""
    (BV, Cout, HW), Cin = gy.shape, x.shape[1]
    assert gy.is_contiguous() and x.is_contiguous() and x.shape == (BV, Cin, HW) and gw.shape == (Cout, Cin)
    assert _capi.lib().mvhmr_conv1x1_wgrad_supported(Cin, Cout, HW) == 1
    _capi.check(_capi.lib().mvhmr_conv1x1_wgrad(_p(gy), _p(x), _p(gw), _p(gb), BV, Cin, Cout, HW, _s()))


def _wgrad_det(gy, x, bias=True):
    """-> gw, gb: both prefilled with NaN ("written, not added into"); gb stays NaN without a bias pointer"""
    L = _capi.lib()
    (BV, Cout, HW), Cin = gy.shape, x.shape[1]
    assert gy.is_contiguous() and x.is_contiguous() and x.shape == (BV, Cin, HW)
    n = L.mvhmr_conv1x1_wgrad_deterministic_workspace_bytes(BV, Cin, Cout, HW)
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device=gy.device)
    gw = torch.full((Cout, Cin), float("nan"), device=gy.device)
    gb = torch.full((Cout,), float("nan"), device=gy.device)
    _capi.check(L.mvhmr_conv1x1_wgrad_deterministic(_p(gy), _p(x), _p(gw), _p(gb) if bias else VP(0), BV, Cin, Cout, HW, _p(ws), n, _s()))
    return gw, gb


def _matmul64(w, x, b=None):
    y = torch.matmul(w.double(), x.double())
    return y if b is None else y + b.double().view(1, -1, 1)


def _wgrad64(gy, x):
    """float64 (Cout, Cin) = sum over maps and pixels of gy[n, co, p] * x[n, ci, p], and the (Cout) sums of gy"""
    Cout, Cin = gy.shape[1], x.shape[1]
    a, b = gy.double().permute(1, 0, 2).reshape(Cout, -1), x.double().permute(1, 0, 2).reshape(Cin, -1)
    return a @ b.t(), a.sum(dim=1)


# ------------------------------------------------------------------------------------ 1. exact arithmetic: bit equality
def _exact_forward_problem(BV, Cin, Cout, HW, scaled, bias, gpu, seed):
    """w in [-4, 4], x in [-8, 8], bias in [-16, 16], integers; scaled: weight row co (and bias[co]) times 2^r[co], pixel column (bv, p) of
    x times 2^c[bv, p].  Output (bv, co, p) is then an integer in units of 2^(r[co] + min c): the condition asserted here is that the sum
    of the magnitudes of all its addends in those units stays below 2^24, so every partial sum in every order is an fp32 number."""
    g = _gen(gpu, seed)
    wi, xi, bi = _ints((Cout, Cin), -4, 4, g), _ints((BV, Cin, HW), -8, 8, g), _ints((Cout,), -16, 16, g)
    r, c = _exps((Cout,), -6, 6, g, scaled), _exps((BV, 1, HW), -3, 3, g, scaled)
    cmin = float(c.min())
    mag = torch.matmul(wi.abs().double(), xi.abs().double() * torch.exp2(c - cmin))
    if bias:
        mag = mag + (bi.abs().double() * 2.0 ** -cmin).view(1, -1, 1)
    assert float(mag.max()) < EXACT, (float(mag.max()), "the inputs of this case do not make the arithmetic exact")
    w, x = (wi.double() * torch.exp2(r).view(-1, 1)).float(), (xi.double() * torch.exp2(c)).float()
    b = (bi.double() * torch.exp2(r)).float() if bias else None
    ref = _matmul64(w, x, b)
    assert torch.equal(ref.float().double(), ref)
    return w, x, b, ref.float()


def _stamp_forward_problem(BV, Cin, Cout, HW, gpu):
    """one-hot weights w[co, co % Cin] = 1 and x[bv, ci, p] = a distinct integer code: y[bv, co, p] = x[bv, co % Cin, p] + bias[co]"""
    assert BV * Cin * HW + 16 < EXACT
    x = torch.arange(BV * Cin * HW, device=gpu, dtype=torch.float32).view(BV, Cin, HW)
    src = torch.arange(Cout, device=gpu) % Cin
    w = torch.zeros(Cout, Cin, device=gpu)
    w[torch.arange(Cout, device=gpu), src] = 1.0
    b = _ints((Cout,), -16, 16, _gen(gpu, 1))
    return w, x, b, x[:, src, :] + b.view(1, -1, 1)


@pytest.mark.parametrize("scaled", (False, True))
@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=str)
def test_to_quad_is_bit_equal_to_an_integer_matmul(shape, scaled, gpu):
    BV, Cin, Cout, H, W = shape
    w, x, b, ref = _exact_forward_problem(BV, Cin, Cout, H * W, scaled, True, gpu, seed=11)
    _same("exact to_quad %s scaled=%s" % (shape, scaled), _to_quad(x, w, b, H, W), _quad_view(ref, H, W))
    w, x, _, ref = _exact_forward_problem(BV, Cin, Cout, H * W, scaled, False, gpu, seed=12)
    _same("exact to_quad %s scaled=%s no bias" % (shape, scaled), _to_quad(x, w, None, H, W), _quad_view(ref, H, W))


@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=str)
def test_to_quad_address_stamp(shape, gpu):
    BV, Cin, Cout, H, W = shape
    w, x, b, ref = _stamp_forward_problem(BV, Cin, Cout, H * W, gpu)
    _same("stamp to_quad %s" % (shape,), _to_quad(x, w, b, H, W), _quad_view(ref, H, W))


@pytest.mark.parametrize("bias", (True, False))
@pytest.mark.parametrize("scaled", (False, True))
@pytest.mark.parametrize("shape", PLANAR_SHAPES, ids=str)
def test_planar_is_bit_equal_to_an_integer_matmul(shape, scaled, bias, gpu):
    BV, Cin, Cout, HW = shape
    w, x, b, ref = _exact_forward_problem(BV, Cin, Cout, HW, scaled, bias, gpu, seed=13)
    _same("exact planar %s scaled=%s bias=%s" % (shape, scaled, bias), _planar(x, w, b), ref)


@pytest.mark.parametrize("shape", PLANAR_SHAPES, ids=str)
def test_planar_address_stamp(shape, gpu):
    BV, Cin, Cout, HW = shape
    w, x, b, ref = _stamp_forward_problem(BV, Cin, Cout, HW, gpu)
    _same("stamp planar %s" % (shape,), _planar(x, w, b), ref)
    _same("stamp planar %s no bias" % (shape,), _planar(x, w, None), ref - b.view(1, -1, 1))


def _slices(shape):
    """(slices per map, 32-pixel chunks per map, 128 x 128 tiles) of a weight-gradient shape, from the library's own workspace size"""
    BV, Cin, Cout, HW = shape
    n = _capi.lib().mvhmr_conv1x1_wgrad_deterministic_workspace_bytes(BV, Cin, Cout, HW)
    assert n > 0 and n % (4 * (Cout * Cin + Cout) * BV) == 0
    return n // 4 // (Cout * Cin + Cout) // BV, HW // 32, (Cin // 128) * (Cout // 128)


def test_wgrad_shapes_cover_every_slice_split():
    split = {s: _slices(s) for s in WGRAD_SHAPES}
    for s, (spm, chunks, _) in split.items():
        assert 1 <= spm <= chunks and chunks % spm == 0, (s, spm, chunks)
    assert any(spm == 1 and chunks > 1 and s[0] * 2 * tiles > 2048 for s, (spm, chunks, tiles) in split.items())     # the grid cap forces one slice
    assert any(1 < spm < chunks for spm, chunks, _ in split.values())
    assert any(spm == chunks for spm, chunks, _ in split.values())                                                   # one chunk per block
    assert any(spm == chunks == 1 for spm, chunks, _ in split.values())                                              # ... of a one-chunk map
    assert any(chunks // spm > 1 for spm, chunks, _ in split.values())                                               # several chunks per block
    assert any(s[1] > 128 and s[2] > 128 for s in split)                                                             # both tile indices > 0


def _exact_wgrad_problem(BV, Cin, Cout, HW, scaled, gpu, seed):
    """gy in {-1, 0, 1}, x in [-2, 2]; scaled: channel co of gy times 2^a[co], channel ci of x times 2^b[ci], so dW[co, ci] is an integer
    in units of 2^(a[co] + b[ci]) and db[co] one in units of 2^a[co].  The outputs start from integers in [-8, 8] of the same units."""
    g = _gen(gpu, seed)
    gyi, xi = _ints((BV, Cout, HW), -1, 1, g), _ints((BV, Cin, HW), -2, 2, g)
    a, b = _exps((Cout,), -4, 4, g, scaled), _exps((Cin,), -4, 4, g, scaled)
    jw, jb = _ints((Cout, Cin), -8, 8, g), _ints((Cout,), -8, 8, g)
    mag_w, mag_b = _wgrad64(gyi.abs(), xi.abs())
    assert float((mag_w + jw.abs().double()).max()) < EXACT and float((mag_b + jb.abs().double()).max()) < EXACT
    gy, x = (gyi.double() * torch.exp2(a).view(1, -1, 1)).float(), (xi.double() * torch.exp2(b).view(1, -1, 1)).float()
    fill_w, fill_b = jw.double() * torch.exp2(a).view(-1, 1) * torch.exp2(b).view(1, -1), jb.double() * torch.exp2(a)
    ref_w, ref_b = _wgrad64(gy, x)
    for t in (ref_w, ref_b, fill_w, fill_b, ref_w + fill_w, ref_b + fill_b):
        assert torch.equal(t.float().double(), t)
    return gy, x, fill_w, fill_b, ref_w, ref_b


def _check_both_wgrads(name, gy, x, fill_w, fill_b, ref_w, ref_b):
    """the atomic form adds into non-zero outputs (once without a bias pointer); the deterministic form writes NaN-filled ones, three
    times with the same bits, which are the atomic form's minus what it started from"""
    gw, gb = fill_w.float(), fill_b.float()
    _wgrad(gy, x, gw, gb)
    _same(name + " atomic dW", gw, (ref_w + fill_w).float())
    _same(name + " atomic db", gb, (ref_b + fill_b).float())
    gw2, gb2 = fill_w.float(), fill_b.float()
    _wgrad(gy, x, gw2, None)
    _same(name + " atomic dW, db = NULL", gw2, (ref_w + fill_w).float())
    assert torch.equal(gb2, fill_b.float())
    runs = [_wgrad_det(gy, x) for _ in range(3)]
    _same(name + " deterministic dW", runs[0][0], ref_w.float())
    _same(name + " deterministic db", runs[0][1], ref_b.float())
    for dw, db in runs[1:]:
        assert torch.equal(dw, runs[0][0]) and torch.equal(db, runs[0][1]), name
    assert torch.equal(runs[0][0], (gw.double() - fill_w).float()) and torch.equal(runs[0][1], (gb.double() - fill_b).float()), name
    dw, db = _wgrad_det(gy, x, bias=False)
    _same(name + " deterministic dW, db = NULL", dw, ref_w.float())
    assert bool(torch.isnan(db).all())


@pytest.mark.parametrize("scaled", (False, True))
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=str)
def test_both_wgrads_are_bit_equal_to_an_integer_matmul(shape, scaled, gpu):
    _check_both_wgrads("exact wgrad %s scaled=%s" % (shape, scaled), *_exact_wgrad_problem(*shape, scaled, gpu, seed=17))


@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=str)
def test_both_wgrads_address_stamp(shape, gpu):
    """gy[., co, .] is 1 at one (map, pixel) slot of its own and 0 elsewhere, x holds integer codes of (bv, ci, p):
    dW[co, ci] = x[slot(co), ci] names the element that was read, db[co] = 1"""
    BV, Cin, Cout, HW = shape
    code = 16777213                                                               # < 2^24 - 2: codes repeat only where x has more elements
    x = (torch.arange(BV * Cin * HW, device=gpu) % code).float().view(BV, Cin, HW)
    slot = (torch.arange(Cout, device=gpu) * 2654435761) % (BV * HW)
    gy = torch.zeros(BV, Cout, HW, device=gpu)
    gy[slot // HW, torch.arange(Cout, device=gpu), slot % HW] = 1.0
    ref_w = x[slot // HW, :, slot % HW].double()                                  # (Cout, Cin)
    ref_b = torch.ones(Cout, dtype=torch.float64, device=gpu)
    zero_w, zero_b = torch.zeros_like(ref_w), torch.zeros_like(ref_b)
    _check_both_wgrads("stamp wgrad %s" % (shape,), gy, x, zero_w, zero_b, ref_w, ref_b)


# ------------------------------------------------------------------------------------ 2. rounding on random floats: a derived bound
def _rounding(name, got, ref, mag, K):
    """worst |got - ref| / ((K + 2) u mag) over all elements must be <= 1; worst |got - ref| / mag is recorded only"""
    err = (got.double() - ref).abs()
    assert float(mag.min()) > 0
    record_err(name + ": err / ((K + 2) u sum|a||b|)", float((err / ((K + 2) * U * mag)).max()), 1.0)
    record_err(name + ": err / sum|a||b| (recorded only)", float((err / mag).max()), NEVER)


def _random_forward(BV, Cin, Cout, HW, gpu, seed):
    g = _gen(gpu, seed)
    x = torch.randn(BV, Cin, HW, device=gpu, generator=g)
    w = torch.randn(Cout, Cin, device=gpu, generator=g)
    b = torch.randn(Cout, device=gpu, generator=g)
    return w, x, b


@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=str)
def test_to_quad_rounding_is_within_the_fma_chain_bound(shape, gpu):
    BV, Cin, Cout, H, W = shape
    w, x, b = _random_forward(BV, Cin, Cout, H * W, gpu, seed=21)
    mag = _matmul64(w.abs(), x.abs(), b.abs())
    _rounding("random to_quad %s" % (shape,), _planar_view(_to_quad(x, w, b, H, W)), _matmul64(w, x, b), mag, Cin)


@pytest.mark.parametrize("bias", (True, False))
@pytest.mark.parametrize("shape", PLANAR_SHAPES, ids=str)
def test_planar_rounding_is_within_the_fma_chain_bound(shape, bias, gpu):
    BV, Cin, Cout, HW = shape
    w, x, b = _random_forward(BV, Cin, Cout, HW, gpu, seed=22)
    b = b if bias else None
    mag = _matmul64(w.abs(), x.abs(), b.abs() if bias else None)
    _rounding("random planar %s bias=%s" % (shape, bias), _planar(x, w, b), _matmul64(w, x, b), mag, Cin)


@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=str)
def test_both_wgrads_rounding_is_within_the_summation_bound(shape, gpu):
    BV, Cin, Cout, HW = shape
    g = _gen(gpu, 23)
    gy = torch.randn(BV, Cout, HW, device=gpu, generator=g)
    x = torch.randn(BV, Cin, HW, device=gpu, generator=g)
    ref_w, ref_b = _wgrad64(gy, x)
    mag_w, mag_b = _wgrad64(gy.abs(), x.abs())
    gw, gb = torch.zeros(Cout, Cin, device=gpu), torch.zeros(Cout, device=gpu)
    _wgrad(gy, x, gw, gb)
    dw, db = _wgrad_det(gy, x)
    n = BV * HW
    _rounding("random wgrad atomic dW %s" % (shape,), gw, ref_w, mag_w, n)
    _rounding("random wgrad atomic db %s" % (shape,), gb, ref_b, mag_b, n)
    _rounding("random wgrad deterministic dW %s" % (shape,), dw, ref_w, mag_w, n)
    _rounding("random wgrad deterministic db %s" % (shape,), db, ref_b, mag_b, n)


# ------------------------------------------------------------------------------------ 3. non-finite locality
def _poisoned_exactly(name, got, clean, bv0, p0):
    """planar (BV, Cout, HW) results: non-finite exactly at [bv0, :, p0], every other element with the bits of the clean run"""
    want = torch.zeros_like(got, dtype=torch.bool)
    want[bv0, :, p0] = True
    assert bool(torch.isfinite(clean).all())
    assert torch.equal(~torch.isfinite(got), want), (name, int((~torch.isfinite(got)).sum()), int(want.sum()))
    _same(name, torch.where(want, clean, got), clean)


@pytest.mark.parametrize("poison", (float("nan"), float("inf")), ids=("nan", "inf"))
@pytest.mark.parametrize("shape", ((3, 48, 384, 8, 32), (2, 256, 256, 96, 96)), ids=str)
def test_to_quad_non_finite_input_stays_in_its_pixel(shape, poison, gpu):
    BV, Cin, Cout, H, W = shape
    w, x, b = _random_forward(BV, Cin, Cout, H * W, gpu, seed=31)
    w = torch.where(w == 0, torch.ones_like(w), w)
    clean = _planar_view(_to_quad(x, w, b, H, W))
    bv0, ci0, p0 = BV - 1, Cin // 2 + 1, (H - 2) * W + W // 2 + 3
    x[bv0, ci0, p0] = poison
    _poisoned_exactly("to_quad %s with one %s" % (shape, poison), _planar_view(_to_quad(x, w, b, H, W)), clean, bv0, p0)


@pytest.mark.parametrize("poison", (float("nan"), float("inf")), ids=("nan", "inf"))
@pytest.mark.parametrize("shape", ((3, 256, 128, 640), (1, 256, 2048, 256)), ids=str)
def test_planar_non_finite_input_stays_in_its_pixel(shape, poison, gpu):
    BV, Cin, Cout, HW = shape
    w, x, b = _random_forward(BV, Cin, Cout, HW, gpu, seed=32)
    w = torch.where(w == 0, torch.ones_like(w), w)
    clean = _planar(x, w, b)
    bv0, ci0, p0 = BV - 1, Cin - 3, HW // 2 + 37
    x[bv0, ci0, p0] = poison
    _poisoned_exactly("planar %s with one %s" % (shape, poison), _planar(x, w, b), clean, bv0, p0)


@pytest.mark.parametrize("poison", (float("nan"), float("inf")), ids=("nan", "inf"))
@pytest.mark.parametrize("shape", ((2, 256, 128, 64), (40, 256, 256, 1024)), ids=str)
def test_both_wgrads_non_finite_gradient_stays_in_its_row(shape, poison, gpu):
    """exact-integer operands, so that the clean rows are the same bits in any atomic order"""
    BV, Cin, Cout, HW = shape
    gy, x, _, _, ref_w, ref_b = _exact_wgrad_problem(BV, Cin, Cout, HW, False, gpu, seed=33)
    bv0, co0, p0 = BV - 1, Cout - 5, HW // 2 + 9
    gy[bv0, co0, p0] = poison
    gw, gb = torch.zeros(Cout, Cin, device=gpu), torch.zeros(Cout, device=gpu)
    _wgrad(gy, x, gw, gb)
    dw, db = _wgrad_det(gy, x)
    rows = torch.arange(Cout, device=gpu) == co0
    for form, w_, b_ in (("atomic", gw, gb), ("deterministic", dw, db)):
        name = "wgrad %s %s with one %s" % (form, shape, poison)
        assert torch.equal(~torch.isfinite(w_), rows.view(-1, 1).expand(Cout, Cin)), name
        assert torch.equal(~torch.isfinite(b_), rows), name
        _same(name + " dW", torch.where(rows.view(-1, 1), ref_w.float(), w_), ref_w.float())
        _same(name + " db", torch.where(rows, ref_b.float(), b_), ref_b.float())


# ------------------------------------------------------------------------------------ 4. element offsets beyond 2^31, n_maps at the grid limit
def test_element_offsets_beyond_2_to_the_31(gpu):
    """257 maps of 512 channels x 128 x 128: the last map of x and of every output starts 2^31 elements in.  Exact-integer operands
    (x in [-2, 2] serves all four kernels: with gy in {-1, 0, 1} the 4.2 M-term sums of the weight gradient stay below 2^24)."""
    BV, C, H, W = 257, 512, 128, 128
    HW = H * W
    assert (BV - 1) * C * HW >= 2 ** 31
    footprint = 2 * BV * C * HW * 4
    free = torch.cuda.mem_get_info()[0]
    if free < 3 * footprint:
        pytest.skip("needs %.1f GB free device memory (three times the %.1f GB of its buffers), %.1f GB are free" % (3 * footprint / 1e9, footprint / 1e9, free / 1e9))
    g = _gen(gpu, 41)
    x = torch.empty(BV, C, HW, device=gpu).random_(-2, 3, generator=g)
    out = torch.empty(BV * C * HW, device=gpu)
    w, b = _ints((C, C), -4, 4, g), _ints((C,), -16, 16, g)
    assert C * 4 * 2 + 16 < EXACT
    ends = (0, BV - 1)
    refs = {m: _matmul64(w, x[m:m + 1], b).float() for m in ends}
    # to_quad, then planar, into the same buffer
    q = _to_quad(x, w, b, H, W, out=out.fill_(float("nan")).view(BV, C // 4, W, H, 4))
    assert bool(torch.isfinite(out).all())
    for m in ends:
        _same("2^31 to_quad map %d" % m, q[m:m + 1], _quad_view(refs[m], H, W))
    y = _planar(x, w, b, out=out.fill_(float("nan")).view(BV, C, HW))
    assert bool(torch.isfinite(out).all())
    for m in ends:
        _same("2^31 planar map %d" % m, y[m:m + 1], refs[m])
    del refs
    # both weight gradients: the output buffer becomes grad_y
    gy = out.random_(-1, 2, generator=g).view(BV, C, HW)
    ref_w = torch.zeros(C, C, dtype=torch.float64, device=gpu)
    ref_b = torch.zeros(C, dtype=torch.float64, device=gpu)
    mag_w = torch.zeros_like(ref_w)
    for m in range(BV):
        a, xm = gy[m].double(), x[m].double()
        ref_w += a @ xm.t()
        ref_b += a.sum(dim=1)
        mag_w += a.abs() @ xm.abs().t()
    assert float(mag_w.max()) + 8 < EXACT and BV * HW + 8 < EXACT
    fill_w, fill_b = _ints((C, C), -8, 8, g).double(), _ints((C,), -8, 8, g).double()
    _check_both_wgrads("2^31 wgrad", gy, x, fill_w, fill_b, ref_w, ref_b)


def test_n_maps_at_the_grid_limit(gpu):
    """65535 maps, the most to_quad and planar take (one more is MVHMR_ERR_UNSUPPORTED: tests/test_conv1x1_gemm_cpu.py)"""
    BV, Cin, Cout, H, W = 65535, 16, 128, 4, 32
    g = _gen(gpu, 43)
    x, w, b = _ints((BV, Cin, H * W), -8, 8, g), _ints((Cout, Cin), -4, 4, g), _ints((Cout,), -16, 16, g)
    assert Cin * 32 + 16 < EXACT
    q, y = _planar_view(_to_quad(x, w, b, H, W)), _planar(x, w, b)
    bad_q = bad_y = 0
    for m0 in range(0, BV, 4096):
        ref = _matmul64(w, x[m0:m0 + 4096], b).float()
        bad_q += int((q[m0:m0 + 4096] != ref).sum())
        bad_y += int((y[m0:m0 + 4096] != ref).sum())
    record_err("65535 maps to_quad", bad_q, 0)
    record_err("65535 maps planar", bad_y, 0)


# ------------------------------------------------------------------------------------ 5. the fused route at module level, C_in != C_out
def _scene(B, V, IMG, gpu):
    rng = np.random.default_rng(61)
    cams = [[None] * B for _ in range(V)]
    for v in range(V):
        az = 2 * np.pi * v / V + 0.3
        eye = np.array([5000 * np.cos(az), 5000 * np.sin(az), 1500.0])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0, 0, 1.0])
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        for b in range(B):
            cam = multiview.Camera(R, -R @ eye, [[1145.0, 0, 512], [0, 1145.0, 512], [0, 0, 1]])
            cam.update_after_crop((150, 150, 850, 850))
            cam.update_after_resize((700, 700), (IMG, IMG))
            cams[v][b] = cam
    batch = dict(images=np.zeros((B, V, IMG, IMG, 3), np.uint8), cameras=cams,
                 keypoints_3d=[rng.normal(0, 100, (17, 3)).astype(np.float32) for _ in range(B)])
    proj_org = torch.from_numpy(np.stack([[cams[v][b].projection for v in range(V)] for b in range(B)]).astype(np.float32)).to(gpu)
    return batch, proj_org


def _count_fused(monkeypatch):
    calls = []
    real_apply = aggregation._FusedAggregate.apply
    monkeypatch.setattr(aggregation._FusedAggregate, "apply", lambda *a: (calls.append(1), real_apply(*a))[1])
    return calls


def _count_entry_points(monkeypatch, names):
    """{name: [argument tuples]} of every call of L.mvhmr_conv1x1_<name> from here on"""
    L = _capi.lib()
    calls = {k: [] for k in names}
    for k in names:
        real = getattr(L, "mvhmr_conv1x1_" + k)
        monkeypatch.setattr(L, "mvhmr_conv1x1_" + k, lambda *a, _real=real, _k=k: (calls[_k].append(a), _real(*a))[1])
    return calls


# (Cin, Cout, Hf, Wf, the backward's GEMMs run as kernels): the third falls back to torch everywhere, C_in % 128 != 0
FUSED_CASES = ((256, 128, 24, 64, True), (128, 256, 32, 32, True), (64, 128, 32, 64, False), (2048, 256, 16, 32, True))


@pytest.mark.parametrize("wants", ("features", "conv", "both"))
@pytest.mark.parametrize("bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("det", (False, True), ids=("default", "deterministic"))
@pytest.mark.parametrize("case", FUSED_CASES, ids=str)
def test_fused_route_with_unequal_channels_equals_the_unfused_one(case, det, bias, wants, gpu, monkeypatch):
    """VolumeGenerator's fused route against the same module with fused_conv off, C_in != C_out and non-square maps: the volume, the
    gradients that were asked for, and which of the backward's GEMMs ran as kernels with which (n_maps, c_in, c_out, pixels)"""
    Cin, Cout, Hf, Wf, kernels = case
    B, V, S, IMG = 2, 4, 32, 128
    HW = Hf * Wf
    L = _capi.lib()
    assert L.mvhmr_conv1x1_planar_supported(Cout, Cin, HW) == int(kernels) and L.mvhmr_conv1x1_wgrad_supported(Cin, Cout, HW) == int(kernels)
    batch, proj_org = _scene(B, V, IMG, gpu)
    torch.manual_seed(9)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=Cin, output_channels=Cout, device=gpu).train(True)
    conv = gen.process_feature[0]
    if not bias:
        conv.bias = None
    for p in conv.parameters():
        p.requires_grad_(wants != "features")
    x = torch.randn(B, V, Cin, Hf, Wf, device=gpu)
    fused_calls = _count_fused(monkeypatch)
    calls = _count_entry_points(monkeypatch, ("planar", "wgrad", "wgrad_deterministic"))

    def step(fused, deterministic):
        gen.fused_conv = fused
        gen.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(wants != "conv")
        np.random.seed(77)
        vol = gen(xi, proj_org, batch)
        go = torch.randn(vol.shape, device=gpu, generator=_gen(gpu, 5))
        was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(deterministic)
        try:
            vol.backward(go)
        finally:
            torch.use_deterministic_algorithms(was)
        grads = {}
        if wants != "conv":
            grads["input"] = xi.grad.clone()
        if wants != "features":
            grads["weight"] = conv.weight.grad.clone()
            if bias:
                grads["bias"] = conv.bias.grad.clone()
        return vol.detach(), grads

    vol, grads = step(True, det)
    assert len(fused_calls) == 1
    want_calls = {"planar": int(kernels and wants != "conv"), "wgrad": int(kernels and wants != "features" and not det),
                  "wgrad_deterministic": int(kernels and wants != "features" and det)}
    assert {k: len(v) for k, v in calls.items()} == want_calls
    for k, dims in (("planar", (B * V, Cout, Cin, HW)), ("wgrad", (B * V, Cin, Cout, HW)), ("wgrad_deterministic", (B * V, Cin, Cout, HW))):
        for a in calls[k]:
            assert tuple(a[4:8]) == dims, (k, a[4:8])
    for a in calls["wgrad"] + calls["wgrad_deterministic"]:
        assert bool(a[3].value) == bias                                             # a bias gradient exactly when the conv has a bias
    if det:
        vol2, grads2 = step(True, True)
        assert len(fused_calls) == 2 and torch.equal(vol, vol2) and sorted(grads) == sorted(grads2)
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), k
    before = {k: len(v) for k, v in calls.items()}
    ref_vol, ref_grads = step(False, False)
    assert len(fused_calls) == (2 if det else 1) and {k: len(v) for k, v in calls.items()} == before   # the unfused module ran none of it
    assert sorted(grads) == sorted(ref_grads) == sorted({"features": ["input"], "conv": ["weight"] + ["bias"] * bias,
                                                          "both": ["input", "weight"] + ["bias"] * bias}[wants])
    tag = "fused %s %s %s wants=%s" % (case[:4], "deterministic" if det else "default", "bias" if bias else "no bias", wants)
    scale = float(ref_vol.abs().max())
    assert scale > 0
    record_err(tag + " volume", float((vol - ref_vol).abs().max()), 2e-5 * scale + 1e-6)
    for k in grads:
        assert float(ref_grads[k].abs().max()) > 0
        record_err(tag + " grad " + k, float((grads[k] - ref_grads[k]).abs().max()), 32 * 2.0 ** -23 * float(ref_grads[k].abs().max()) + 1e-6)


def test_features_off_a_16_byte_boundary_take_the_unfused_route(gpu, monkeypatch):
    """a contiguous view one float into a larger buffer: the 16-byte loads of the fused GEMMs must never see it"""
    B, V, C, H, S, IMG = 2, 4, 128, 32, 32, 128
    batch, proj_org = _scene(B, V, IMG, gpu)
    torch.manual_seed(9)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=C, output_channels=C, device=gpu).eval()
    n = B * V * C * H * H
    big = torch.randn(n + 4, device=gpu)
    feats = big[1:1 + n].view(B, V, C, H, H)
    assert feats.is_contiguous() and feats.data_ptr() % 16 == 4
    fused_calls = _count_fused(monkeypatch)
    calls = _count_entry_points(monkeypatch, ("to_quad", "planar", "wgrad", "wgrad_deterministic"))
    with torch.no_grad():
        vol = gen(feats, proj_org, batch)
        assert not fused_calls and not any(calls.values())
        gen.fused_conv = False
        assert torch.equal(vol, gen(feats, proj_org, batch))
        gen.fused_conv = True
        aligned = gen(feats.clone(), proj_org, batch)                               # the same numbers on a boundary: the fused route
    assert len(fused_calls) == 1 and len(calls["to_quad"]) == 1
    record_err("unfused volume of misaligned features vs fused volume of their aligned copy", float((vol - aligned).abs().max()),
               2e-5 * float(vol.abs().max()) + 1e-6)
