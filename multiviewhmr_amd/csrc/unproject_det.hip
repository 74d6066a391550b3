// Deterministic mode of the feature-gradient backward (mvhmr_unproject_backward_deterministic): the scale pass that fixes
// K[b][c] (det_scale.h) before any tap is added -- ONE pass for every family: its kernels, the layout of its scratch and its launcher are
// all here -- and the passes that turn the int64 accumulator of the deterministic backward kernels into the caller's gradient.  Every pass
// here is order-independent: maxima are taken with integer atomicMax on the bits of |x| (det_scale.h), counts with integer atomicAdd,
// marks are bytes every writer sets to the same 1, conversions are element-wise.
#include "device_common.h"
#include "det_scale.h"
#include "kernels.h"

namespace mvhmr {

// ------------------------------------------------------------------------------------------ inputs of the bound
// (max |grad_out| per row: k_det_gmax, det_scale.h)

// cnt[b] = the number of volumes that name feature sample b (shared feature maps; entries outside [0, B) name none)
__global__ void __launch_bounds__(256) k_det_count(const int *__restrict__ fidx, int *__restrict__ cnt, int M, int B)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int fb = fidx[m];
    if ((unsigned)fb < (unsigned)B) atomicAdd(cnt + fb, 1);
}

// the largest positive pixel of a sample's confidence maps (bits of the float; NaN and negative pixels never raise it, +Inf does): a
// bilinear sample is a convex combination of its taps and zeros, so this bounds every c_v of the sample
__global__ void __launch_bounds__(256) k_det_cmax(const float *__restrict__ conf, unsigned *__restrict__ cmax, long long per_sample)
{
    const int b = blockIdx.y;
    const float *c = conf + (long long)b * per_sample;
    unsigned m = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per_sample; i += (long long)gridDim.x * 256) {
        const float x = c[i];
        const unsigned a = x > 0.f ? __builtin_bit_cast(unsigned, x) : 0u;
        m = a > m ? a : m;
    }
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(cmax + b, m);
}

// One byte per pixel of every (b, slot) map that a voxel-view TAKING PART taps (visible, confidence and moments calls: a view that takes no
// part for a voxel is not read for it, so a non-finite value under its taps must neither poison the (b, c) nor widen its scale).  Thread
// per (voxel, slot); the test and the taps are the very ones the backward kernels use (view_sees, make_taps, sample_conf).  A voxel-view
// marks iff its slot is present, it passes view_sees (visible), it has taps at all (Taps::any) and -- with confidence maps -- its
// confidence sample is > 0.  Either of the last two tests alone implies `any`: view_sees demands z > 0 and 0 <= ix <= W - 1, 0 <= iy <= H - 1,
// inside make_taps' own window -1 < ix < W, -1 < iy < H, on the same fp32 values; sample_conf returns 0 without `any`.  Only a moments call
// without the seeing test rests on `any` itself.  All four clamped taps are marked, those of weight 0 too: the kernels multiply every tap
// they load, so a non-finite value under a zero-weight tap reaches s_v.
__global__ void __launch_bounds__(256) k_det_mark(const float *__restrict__ proj, const Coords coords, const float *__restrict__ conf,
                                                  unsigned char *__restrict__ marks, int V, int H, int W, long long N, const int *__restrict__ nvs,
                                                  int visible)
{
    const long long bv = blockIdx.y;
    const int b = (int)(bv / V), v = (int)(bv % V);
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N || (nvs && v >= nvs[b])) return;                                   // slots behind the present views are absent
    float X0, X1, X2;
    voxel_xyz(coords, b, N, n, X0, X1, X2);
    const float *P = proj + bv * 12;
    if (visible && !view_sees(P, X0, X1, X2, H, W)) return;
    const Taps t = make_taps(P, X0, X1, X2, H, W);                                // clamped to the map whatever the position
    if (!t.any) return;
    if (conf && !(sample_conf(conf + bv * H * W, t, H, W) > 0.f)) return;         // (zero, negative, NaN: absent)
    unsigned char *m = marks + bv * (long long)H * W;
    m[t.y0 * W + t.x0] = 1;
    m[t.y0 * W + t.x1] = 1;
    m[t.y1 * W + t.x0] = 1;
    m[t.y1 * W + t.x1] = 1;
}

// max |feature| of each (b, c) over all views and pixels -- MARKED: over the marked pixels -- from the channels-last copy (BV, HW, C4):
// block (pixel chunk, bv), thread per channel
constexpr int kDetPix = 64;
template <typename TF, bool MARKED>
__global__ void __launch_bounds__(256) k_det_fmax(const TF *__restrict__ featT, unsigned *__restrict__ fmax, int V, int C, int C4, int HW,
                                                  const unsigned char *__restrict__ marks)
{
    const long long bv = blockIdx.y;
    const int b = (int)(bv / V), p0 = blockIdx.x * kDetPix, p1 = p0 + kDetPix < HW ? p0 + kDetPix : HW;
    const TF *f = featT + bv * (long long)HW * C4;
    for (int c = threadIdx.x; c < C; c += 256) {
        unsigned m = 0;
        for (int p = p0; p < p1; ++p) {
            if constexpr (MARKED) {
                if (!marks[bv * HW + p]) continue;                                // block-uniform
            }
            const unsigned a = abs_bits(to_f32<TF>(f[(long long)p * C4 + c]));
            m = a > m ? a : m;
        }
        if (m) atomicMax(fmax + (long long)b * C + c, m);
    }
}

// the same from the column-major quad-planar fp32 copy (BV, C4/4, W, H, 4) the brick kernels stage: block (pixel chunk, bv * nqv + q), lanes
// 4 apart hold the same channel
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) k_det_fmax_quad(const float4 *__restrict__ featK, unsigned *__restrict__ fmax, int V, int C, int nqv, int HW)
{
    const long long bq = blockIdx.y;
    const int q = (int)(bq % nqv), b = (int)(bq / nqv / V);
    const float4 *f = featK + bq * HW;
    const int i = threadIdx.x & 3;
    unsigned m = 0;
    for (int p = blockIdx.x * kDetPix * 4 + (threadIdx.x >> 2); p < HW && p < (blockIdx.x + 1) * kDetPix * 4; p += 64) {
        const float4 v = f[p];
        const unsigned a = abs_bits(i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w);
        m = a > m ? a : m;
    }
#pragma unroll
    for (int o = 32; o >= 4; o >>= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m, o);
        m = t > m ? t : m;
    }
    const int c = q * 4 + i;
    if ((threadIdx.x & 63) < 4 && m && c < C) atomicMax(fmax + (long long)b * C + c, m);
}

// ------------------------------------------------------------------------------------------ the exponent
// what the bound of one call reads besides gmax and fmax (det_scale.h has the table).  A null pointer = the call does not select it.
struct DetBound {
    int method, moments;           // AGG_*; moments != 0: the cross-view variance (gmax2 is the variance half's table)
    int V, C, log2n;
    int mean_div;                  // the mean's divisor: V (plain), 1 (visible, weights, confidence); read where nvs is null
    int reads_f;                   // fmax enters the bound (softmax, moments)
    const int *nvs;                // view mask alone: the mean divides by max(n_b, 1)
    const float *wts;              // view weights (B, V) in slot order: the sum carries the sample's largest
    const unsigned *cmax;          // confidence maps: the sum carries the sample's largest positive pixel
    const int *cnt;                // shared feature maps: cnt_b volumes add into sample b
    const unsigned *gmax2;
};

// K[b][c]: N * bound * 2^K < 2^62
__global__ void __launch_bounds__(256) k_det_exponent(const unsigned *__restrict__ gmax, const unsigned *__restrict__ fmax, int *__restrict__ kexp,
                                                      long long BC, const DetBound d)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    const long long b = i / d.C;
    const int n = d.cnt ? d.cnt[b] : 1;
    if (n == 0) { kexp[i] = 0; return; }                                          // a sample no volume names adds nothing
    const bool sum_c = d.cmax && d.method == AGG_SUM;
    const unsigned gb = gmax[i], g2b = d.gmax2 ? d.gmax2[i] : 0u, fb = d.reads_f ? fmax[i] : 0u, cb = sum_c ? d.cmax[b] : 0u;
    if (gb >= 0x7f800000u || g2b >= 0x7f800000u || fb >= 0x7f800000u || cb >= 0x7f800000u) { kexp[i] = kDetPoison; return; }
    const double g = (double)__builtin_bit_cast(float, gb), g2 = (double)__builtin_bit_cast(float, g2b), f = (double)__builtin_bit_cast(float, fb);
    double bound = g;
    if (d.moments) {
        bound = g + 4.0 * g2 * f;
    } else if (d.method == AGG_SOFTMAX) {
        bound = g * (1.0 + 2.0 * f);
    } else if (d.method == AGG_SUM && sum_c) {
        bound = g * (double)__builtin_bit_cast(float, cb);
    } else if (d.method == AGG_SUM && d.wts) {
        float wmax = 0.f;
        for (int v = 0; v < d.V; ++v) wmax = fmaxf(wmax, d.wts[b * d.V + v]);
        bound = g * (double)wmax;
    } else if (d.method == AGG_MEAN) {
        const int nv = d.nvs ? d.nvs[b] : d.mean_div;
        bound = g / (nv > 1 ? nv : 1);
    }
    if (bound == 0.0) { kexp[i] = 0; return; }
    // ds itself may overflow fp32.  Written so that NaN is caught too: 0 * Inf under an infinite view weight.  (Every other input has
    // passed the finite tests above, and a sum or product of finite non-negative doubles of fp32 range is never NaN.)
    if (!(bound < 3.4028234663852886e38)) { kexp[i] = kDetPoison; return; }
    int e;
    frexp(bound, &e);                                                             // bound < 2^e
    const int log2c = n > 1 ? 32 - __builtin_clz((unsigned)(n - 1)) : 0;          // cnt <= 2^log2c
    kexp[i] = 62 - d.log2n - log2c - e;
}

// ------------------------------------------------------------------------------------------ conversions
// (det_value: det_scale.h)
// int64 channels-last accumulator (BV, HW, C4) -> planar (BV, C, HW) in the feature dtype, 64 x 64 tiles turned through LDS
template <typename T>
__global__ void __launch_bounds__(256)
k_det_to_planar(const unsigned long long *__restrict__ srcI, const int *__restrict__ kexp, T *__restrict__ dst, int V, int C, int C4, int HW)
{
    __shared__ float t[64][65];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long bv = blockIdx.z;
    const int b = (int)(bv / V);
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int c = c0 + lane;
    const int k = c < C ? kexp[(long long)b * C + c] : 0;
    for (int r = w; r < 64; r += 4) {
        const int p = p0 + r;
        t[r][lane] = (p < HW && c < C) ? det_value(srcI[(bv * HW + p) * C4 + c], k) : 0.f;
    }
    __syncthreads();
    for (int r = w; r < 64; r += 4) {
        const int cc = c0 + r, p = p0 + lane;
        if (cc < C && p < HW) dst[(bv * C + cc) * HW + p] = from_f32<T>(t[lane][r]);
    }
}

// int64 channels-last accumulator -> channels-last gradient (C4 == C) in the feature dtype
template <typename T>
__global__ void __launch_bounds__(256)
k_det_cast(const unsigned long long *__restrict__ srcI, const int *__restrict__ kexp, T *__restrict__ dst, long long n, int V, int C, long long mapsz)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long b = i / mapsz / V;
        const int c = (int)(i % C);
        dst[i] = from_f32<T>(det_value(srcI[i], kexp[b * C + c]));
    }
}

// int64 COLUMN-major quad-planar accumulator (BV, C4/4, W, H, 4) -> planar (BV, C, H, W), as k_quad_planar_to_planar: a band of BW image
// columns of one channel quad, read linearly, turned through LDS, written as runs along x
template <typename TF, int BW>
__global__ void __launch_bounds__(512)
k_det_quad_to_planar(const unsigned long long *__restrict__ src, const int *__restrict__ kexp, TF *__restrict__ dst, int V, int C, int H, int W)
{
    extern __shared__ float tile[];                                              // [4][H][BW + 1]
    constexpr int TS = BW + 1;
    const long long bv = blockIdx.z;
    const int q = blockIdx.y, x0 = blockIdx.x * BW, b = (int)(bv / V);
    const int cols = W - x0 < BW ? W - x0 : BW;
    const int nc = C - q * 4 < 4 ? C - q * 4 : 4;
    int k[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) k[i] = i < nc ? kexp[(long long)b * C + q * 4 + i] : 0;
    const unsigned long long *s = src + ((bv * ((C + 3) >> 2) + q) * W + x0) * (long long)H * 4;
    for (int e = threadIdx.x; e < cols * H * 4; e += 512) {
        const int i = e & 3, pix = e >> 2;
        const int xl = pix / H, y = pix - xl * H;
        tile[(i * H + y) * TS + xl] = det_value(s[e], k[i]);
    }
    __syncthreads();
    TF *d = dst + (bv * C + q * 4) * (long long)H * W + x0;
    const int xl = threadIdx.x & (BW - 1);
    if (xl < cols)
        for (int r = threadIdx.x / BW; r < nc * H; r += 512 / BW) d[(long long)r * W + xl] = from_f32<TF>(tile[r * TS + xl]);
}

// ------------------------------------------------------------------------------------------ the scale pass's scratch and launcher
// The regions of `scale`, as byte offsets (kNone: the call has none): gmax, the moments' second gmax, fmax and K are B * C words each,
// then cmax (confidence: B words padded to 16 B) or cnt (shared: B words), then the tap marks (one byte per pixel of every (b, slot) map).
// Decided by the route flags alone (volumes, moments, conf, visible), which the workspace plans set before any pointer exists.
namespace {
constexpr size_t kNone = ~(size_t)0;
struct DetScaleLayout {
    size_t gmax = 0, gmax2 = kNone, fmax = 0, kexp = 0, cmax = kNone, cnt = kNone, marks = kNone, total = 0;
};
DetScaleLayout det_scale_layout(const Problem &p)
{
    DetScaleLayout l;
    const size_t table = (size_t)p.B * p.C * sizeof(int), maps = (size_t)p.B * p.V * p.H * p.W;
    size_t top = table;
    const auto take = [&top](size_t bytes) { const size_t at = top; top += bytes; return at; };
    if (!p.volumes && p.moments) l.gmax2 = take(table);
    l.fmax = take(table);
    l.kexp = take(table);
    if (p.volumes) l.cnt = take((size_t)p.B * sizeof(int));
    else if (p.moments) l.marks = take(maps);
    else if (p.conf) l.cmax = take(((size_t)p.B * sizeof(unsigned) + 15) / 16 * 16), l.marks = take(maps);
    else if (p.visible) l.marks = take(maps);
    l.total = top;
    return l;
}
template <typename T> T *region(void *scale, size_t offset) { return offset == kNone ? nullptr : reinterpret_cast<T *>(static_cast<unsigned char *>(scale) + offset); }

template <typename ROWS, typename... FIELDS>
void launch_det_gmax(const void *grad_out, unsigned *gmax, long long rows_n, const Problem &p, hipStream_t s, FIELDS... fields)
{
    const dim3 grid((unsigned)rows_n, chunks_of(p.N));
    if (p.out_bf16) hipLaunchKernelGGL((k_det_gmax<bf16_t, ROWS, FIELDS...>), grid, dim3(256), 0, s, (const bf16_t *)grad_out, gmax, p.N, fields...);
    else if (p.out_f16) hipLaunchKernelGGL((k_det_gmax<__half, ROWS, FIELDS...>), grid, dim3(256), 0, s, (const __half *)grad_out, gmax, p.N, fields...);
    else hipLaunchKernelGGL((k_det_gmax<float, ROWS, FIELDS...>), grid, dim3(256), 0, s, (const float *)grad_out, gmax, p.N, fields...);
}
}  // namespace

size_t det_scale_bytes(const Problem &p) { return det_scale_layout(p).total; }

const int *det_exponents(const void *scale, const Problem &p)
{
    return reinterpret_cast<const int *>(static_cast<const unsigned char *>(scale) + det_scale_layout(p).kexp);
}

hipError_t launch_det_scale(const void *grad_out, const void *feat, void *scale, const Problem &p, hipStream_t s, bool quad, const float *proj,
                            const Coords *coords)
{
    const DetScaleLayout l = det_scale_layout(p);
    const long long BC = (long long)p.B * p.C;
    const long long rows = p.volumes ? (long long)p.volumes * p.C : p.moments ? BC * p.moments : BC;
    const bool reads_f = p.moments || p.method == AGG_SOFTMAX, marked = reads_f && l.marks != kNone;
    if (p.volumes ? !p.feature_index : p.feature_index != nullptr) return hipErrorNotSupported;
    if (!p.volumes && p.moments && p.moments != 1 && p.moments != 2) return hipErrorInvalidValue;
    if ((p.conf != 0) != (p.confidence != nullptr) || (p.conf && (!proj || !coords))) return hipErrorInvalidValue;
    if (marked && (!proj || !coords)) return hipErrorInvalidValue;
    if (quad && (p.volumes || p.moments || p.conf || p.visible)) return hipErrorInvalidValue;        // quad-planar features: the plain route only
    if (BC > 0x7fffffffll || rows > 0x7fffffffll) return hipErrorNotSupported;
    if ((!p.volumes || reads_f) && (long long)p.B * p.V > 65535) return hipErrorNotSupported;          // (the maps are the grid's y extent)
    hipError_t e = hipMemsetAsync(scale, 0, l.total, s);
    if (e != hipSuccess) return e;
    unsigned *gmax = region<unsigned>(scale, l.gmax), *fmax = region<unsigned>(scale, l.fmax), *cmax = region<unsigned>(scale, l.cmax);
    int *cnt = region<int>(scale, l.cnt);
    unsigned char *marks = region<unsigned char>(scale, l.marks);
    const int HW = p.H * p.W;
    if (p.volumes) {
        hipLaunchKernelGGL(k_det_count, dim3((unsigned)((p.volumes + 255) / 256)), dim3(256), 0, s, p.feature_index, cnt, p.volumes, p.B);
        launch_det_gmax<DetRowsShared>(grad_out, gmax, rows, p, s, p.feature_index, p.B, p.C);
    } else if (p.moments) {
        launch_det_gmax<DetRowsMoments>(grad_out, gmax, rows, p, s, p.C, p.moments, BC);
    } else {
        launch_det_gmax<DetRowsIdentity>(grad_out, gmax, rows, p, s);
    }
    if (cmax && p.method == AGG_SUM) {
        const long long per = (long long)p.V * HW;
        hipLaunchKernelGGL(k_det_cmax, dim3(chunks_of(per), (unsigned)p.B), dim3(256), 0, s, p.confidence, cmax, per);
    }
    if (marked)
        hipLaunchKernelGGL(k_det_mark, dim3((unsigned)((p.N + 255) / 256), (unsigned)(p.B * p.V)), dim3(256), 0, s, proj, *coords, p.confidence, marks, p.V,
                           p.H, p.W, p.N, p.view_count, p.visible);
    if (reads_f && quad) {
        const int nqv = p.C4 / 4;
        const dim3 g2((unsigned)((HW + 4 * kDetPix - 1) / (4 * kDetPix)), (unsigned)((long long)p.B * p.V * nqv));
        hipLaunchKernelGGL(k_det_fmax_quad<>, g2, dim3(256), 0, s, (const float4 *)feat, fmax, p.V, p.C, nqv, HW);
    } else if (reads_f) {
        const dim3 g2((unsigned)((HW + kDetPix - 1) / kDetPix), (unsigned)(p.B * p.V));
        if (marked && p.feat_f16) hipLaunchKernelGGL((k_det_fmax<__half, true>), g2, dim3(256), 0, s, (const __half *)feat, fmax, p.V, p.C, p.C4, HW, marks);
        else if (marked) hipLaunchKernelGGL((k_det_fmax<float, true>), g2, dim3(256), 0, s, (const float *)feat, fmax, p.V, p.C, p.C4, HW, marks);
        else if (p.feat_f16) hipLaunchKernelGGL((k_det_fmax<__half, false>), g2, dim3(256), 0, s, (const __half *)feat, fmax, p.V, p.C, p.C4, HW, marks);
        else hipLaunchKernelGGL((k_det_fmax<float, false>), g2, dim3(256), 0, s, (const float *)feat, fmax, p.V, p.C, p.C4, HW, marks);
    }
    // the selection, in the precedence of DESIGN.md 5.7's table: confidence, visible, view weights, view mask, plain.  Visible, weighted
    // and confidence means are bounded by |g| alone (a voxel may be seen by ONE view; w_v / W <= 1): a divisor of 1
    DetBound d{};
    d.method = p.method, d.moments = p.volumes ? 0 : p.moments, d.V = p.V, d.C = p.C, d.log2n = log2_ceil(p.N), d.reads_f = reads_f;
    d.cnt = cnt, d.cmax = cmax, d.gmax2 = region<const unsigned>(scale, l.gmax2);
    const bool alone = !p.volumes && !p.moments && !p.conf && !p.visible;         // what the mask and the weights select by themselves
    d.wts = alone ? p.view_weights : nullptr;
    d.nvs = alone && !p.view_weights ? p.view_count : nullptr;
    d.mean_div = p.conf || p.visible || d.wts ? 1 : p.V;
    hipLaunchKernelGGL(k_det_exponent, dim3((unsigned)((BC + 255) / 256)), dim3(256), 0, s, gmax, fmax, region<int>(scale, l.kexp), BC, d);
    return hipGetLastError();
}

hipError_t launch_det_grad_to_planar(const unsigned long long *gradI, const int *kexp, void *dst, const Problem &p, hipStream_t s)
{
    const int HW = p.H * p.W;
    const dim3 grid((HW + 63) / 64, (p.C4 + 63) / 64, (unsigned)(p.B * p.V));
    if (p.feat_f16) hipLaunchKernelGGL(k_det_to_planar<__half>, grid, dim3(256), 0, s, gradI, kexp, (__half *)dst, p.V, p.C, p.C4, HW);
    else hipLaunchKernelGGL(k_det_to_planar<float>, grid, dim3(256), 0, s, gradI, kexp, (float *)dst, p.V, p.C, p.C4, HW);
    return hipGetLastError();
}

hipError_t launch_det_quad_to_planar(const unsigned long long *acc, const int *kexp, void *dst, const Problem &p, hipStream_t s)
{
    const int bw = (size_t)4 * p.H * 33 * sizeof(float) <= 64 * 1024 ? 32 : 8;   // as the default's layout pass (grad_band)
    const dim3 grid((p.W + bw - 1) / bw, p.C4 / 4, p.B * p.V);
    const size_t lds = (size_t)4 * p.H * (bw + 1) * sizeof(float);
    if (bw == 32) {
        if (p.feat_f16) hipLaunchKernelGGL((k_det_quad_to_planar<__half, 32>), grid, dim3(512), lds, s, acc, kexp, (__half *)dst, p.V, p.C, p.H, p.W);
        else hipLaunchKernelGGL((k_det_quad_to_planar<float, 32>), grid, dim3(512), lds, s, acc, kexp, (float *)dst, p.V, p.C, p.H, p.W);
    } else {
        if (p.feat_f16) hipLaunchKernelGGL((k_det_quad_to_planar<__half, 8>), grid, dim3(512), lds, s, acc, kexp, (__half *)dst, p.V, p.C, p.H, p.W);
        else hipLaunchKernelGGL((k_det_quad_to_planar<float, 8>), grid, dim3(512), lds, s, acc, kexp, (float *)dst, p.V, p.C, p.H, p.W);
    }
    return hipGetLastError();
}

hipError_t launch_det_grad_cast(const unsigned long long *gradI, const int *kexp, void *dst, const Problem &p, hipStream_t s)
{
    const long long mapsz = (long long)p.H * p.W * p.C4, n = (long long)p.B * p.V * mapsz;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    if (p.feat_f16) hipLaunchKernelGGL(k_det_cast<__half>, dim3(blocks), dim3(256), 0, s, gradI, kexp, (__half *)dst, n, p.V, p.C4, mapsz);
    else hipLaunchKernelGGL(k_det_cast<float>, dim3(blocks), dim3(256), 0, s, gradI, kexp, (float *)dst, n, p.V, p.C4, mapsz);
    return hipGetLastError();
}

}  // namespace mvhmr
