// Deterministic mode of the feature-gradient backward (mvhmr_unproject_backward_deterministic): the scale pass that fixes
// K[b][c] (det_scale.h) before any tap is added, and the passes that turn the int64 channels-last accumulator of k_bwd_gather_det into the
// caller's gradient.  Every pass here is order-independent: maxima are taken with integer atomicMax on the bits of |x| (non-negative floats
// order as integers, and Inf / NaN sort above every finite value), conversions are element-wise.
#include "device_common.h"
#include "det_scale.h"
#include "kernels.h"

namespace mvhmr {

namespace {
__device__ __forceinline__ unsigned abs_bits(float x) { return __builtin_bit_cast(unsigned, x) & 0x7fffffffu; }

__device__ __forceinline__ unsigned wave_max_u32(unsigned m)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m, o);
        m = t > m ? t : m;
    }
    return m;
}
}  // namespace

// max |grad_out| of each (b, c) row of the (B, C, N) volume gradient: block (row, chunk)
template <typename TO>
__global__ void __launch_bounds__(256) k_det_gmax(const TO *__restrict__ grad_out, unsigned *__restrict__ gmax, long long N)
{
    const long long row = blockIdx.x;
    const TO *g = grad_out + row * N;
    unsigned m = 0;
    for (long long n = (long long)blockIdx.y * 256 + threadIdx.x; n < N; n += (long long)gridDim.y * 256) {
        const unsigned a = abs_bits(to_f32<TO>(g[n]));
        m = a > m ? a : m;
    }
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(gmax + row, m);
}

// max |feature| of each (b, c) over all views and pixels, from the channels-last copy (BV, HW, C4): block (pixel chunk, bv), thread per channel
constexpr int kDetPix = 64;
template <typename TF>
__global__ void __launch_bounds__(256) k_det_fmax(const TF *__restrict__ featT, unsigned *__restrict__ fmax, int V, int C, int C4, int HW)
{
    const long long bv = blockIdx.y;
    const int b = (int)(bv / V), p0 = blockIdx.x * kDetPix, p1 = p0 + kDetPix < HW ? p0 + kDetPix : HW;
    const TF *f = featT + bv * (long long)HW * C4;
    for (int c = threadIdx.x; c < C; c += 256) {
        unsigned m = 0;
        for (int p = p0; p < p1; ++p) {
            const unsigned a = abs_bits(to_f32<TF>(f[(long long)p * C4 + c]));
            m = a > m ? a : m;
        }
        if (m) atomicMax(fmax + (long long)b * C + c, m);
    }
}

// Visibility-aware softmax: a view that does not see a voxel is not read for it, so the bound may range only over the pixels
// a seeing voxel-view taps -- a non-finite value elsewhere must neither poison the (b, c) nor widen its scale.  k_det_mark_seen sets one byte
// per tapped pixel of every (b, slot) map (thread per (voxel, slot): view_sees and make_taps, the very test and taps k_bwd_gather_seen uses;
// every writer stores the same 1, so the order plays no part), k_det_fmax_seen is k_det_fmax over the marked pixels.
__global__ void __launch_bounds__(256) k_det_mark_seen(const float *__restrict__ proj, const Coords coords, unsigned char *__restrict__ marks, int V,
                                                       int H, int W, long long N, const int *__restrict__ nvs)
{
    const long long bv = blockIdx.y;
    const int b = (int)(bv / V), v = (int)(bv % V);
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N || (nvs && v >= nvs[b])) return;                                   // slots behind the present views are absent
    float X0, X1, X2;
    voxel_xyz(coords, b, N, n, X0, X1, X2);
    const float *P = proj + bv * 12;
    if (!view_sees(P, X0, X1, X2, H, W)) return;
    const Taps t = make_taps(P, X0, X1, X2, H, W);                                // clamped to the map whatever the position
    unsigned char *m = marks + bv * (long long)H * W;
    m[t.y0 * W + t.x0] = 1;
    m[t.y0 * W + t.x1] = 1;
    m[t.y1 * W + t.x0] = 1;
    m[t.y1 * W + t.x1] = 1;
}

template <typename TF>
__global__ void __launch_bounds__(256) k_det_fmax_seen(const TF *__restrict__ featT, const unsigned char *__restrict__ marks, unsigned *__restrict__ fmax,
                                                       int V, int C, int C4, int HW)
{
    const long long bv = blockIdx.y;
    const int b = (int)(bv / V), p0 = blockIdx.x * kDetPix, p1 = p0 + kDetPix < HW ? p0 + kDetPix : HW;
    const TF *f = featT + bv * (long long)HW * C4;
    const unsigned char *mk = marks + bv * (long long)HW;
    for (int c = threadIdx.x; c < C; c += 256) {
        unsigned m = 0;
        for (int p = p0; p < p1; ++p) {
            if (!mk[p]) continue;                                                 // block-uniform
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

// K[b][c] from the two maxima: N * bound * 2^K < 2^62 (det_scale.h)
__global__ void __launch_bounds__(256) k_det_exponent(const unsigned *__restrict__ gmax, const unsigned *__restrict__ fmax, int *__restrict__ kexp,
                                                      long long BC, int method, int V, int log2n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    const unsigned gb = gmax[i], fb = method == AGG_SOFTMAX ? fmax[i] : 0u;
    if (gb >= 0x7f800000u || fb >= 0x7f800000u) { kexp[i] = kDetPoison; return; }
    const double g = (double)__builtin_bit_cast(float, gb), f = (double)__builtin_bit_cast(float, fb);
    const double bound = method == AGG_SOFTMAX ? g * (1.0 + 2.0 * f) : method == AGG_MEAN ? g / V : g;
    if (bound == 0.0) { kexp[i] = 0; return; }
    if (bound >= 3.4028234663852886e38) { kexp[i] = kDetPoison; return; }  // ds itself may overflow fp32
    int e;
    frexp(bound, &e);                                                    // bound < 2^e
    kexp[i] = 62 - log2n - e;
}

// the same for a view-masked call: the mean's ds is g / n_b with n_b = nvs[b] present views, so the bound divides by n_b
// (>= 1; a sample without views adds nothing) -- with every view present exactly k_det_exponent's
__global__ void __launch_bounds__(256) k_masked_det_exponent(const unsigned *__restrict__ gmax, const unsigned *__restrict__ fmax, int *__restrict__ kexp,
                                                             long long BC, int method, int C, int log2n, const int *__restrict__ nvs)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    const unsigned gb = gmax[i], fb = method == AGG_SOFTMAX ? fmax[i] : 0u;
    if (gb >= 0x7f800000u || fb >= 0x7f800000u) { kexp[i] = kDetPoison; return; }
    const int nv = nvs[i / C];
    const double g = (double)__builtin_bit_cast(float, gb), f = (double)__builtin_bit_cast(float, fb);
    const double bound = method == AGG_SOFTMAX ? g * (1.0 + 2.0 * f) : method == AGG_MEAN ? g / (nv > 1 ? nv : 1) : g;
    if (bound == 0.0) { kexp[i] = 0; return; }
    if (bound >= 3.4028234663852886e38) { kexp[i] = kDetPoison; return; }
    int e;
    frexp(bound, &e);
    kexp[i] = 62 - log2n - e;
}

// the same under per-view weights, wts (B, V) packed in slot order: the sum's ds is g w_v, so its bound carries the sample's
// largest weight (without it the int64 sums can wrap); the mean's is g w_v / W <= g, the softmax's g p_v (1 + s_v - out) as unweighted
__global__ void __launch_bounds__(256) k_weighted_det_exponent(const unsigned *__restrict__ gmax, const unsigned *__restrict__ fmax, int *__restrict__ kexp,
                                                               long long BC, int method, int C, int V, int log2n, const float *__restrict__ wts)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    const unsigned gb = gmax[i], fb = method == AGG_SOFTMAX ? fmax[i] : 0u;
    if (gb >= 0x7f800000u || fb >= 0x7f800000u) { kexp[i] = kDetPoison; return; }
    const float *w = wts + (i / C) * V;
    float wmax = 0.f;
    for (int v = 0; v < V; ++v) wmax = fmaxf(wmax, w[v]);
    const double g = (double)__builtin_bit_cast(float, gb), f = (double)__builtin_bit_cast(float, fb);
    const double bound = method == AGG_SOFTMAX ? g * (1.0 + 2.0 * f) : method == AGG_SUM ? g * (double)wmax : g;
    if (bound == 0.0) { kexp[i] = 0; return; }
    if (!(bound < 3.4028234663852886e38)) { kexp[i] = kDetPoison; return; }   // ds itself may overflow fp32 (an infinite weight too)
    int e;
    frexp(bound, &e);
    kexp[i] = 62 - log2n - e;
}

__device__ __forceinline__ float det_value(unsigned long long acc, int k)
{
    if (k == kDetPoison) return __builtin_nanf("");
    return (float)ldexp((double)(long long)acc, -k);
}

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

// gmax, fmax, K: three words per (b, c); a visible problem's tap marks (one byte per pixel of every (b, slot) map) lie behind them
size_t det_scale_bytes(const Problem &p)
{
    if (p.conf) return (size_t)p.B * p.C * 3 * sizeof(int) + conf_det_scale_extra_bytes(p);     // (per-pixel view confidence: unproject_confidence.hip)
    return (size_t)p.B * p.C * 3 * sizeof(int) + (p.visible ? (size_t)p.B * p.V * p.H * p.W : 0);
}

hipError_t launch_det_scale(const void *grad_out, const void *feat, void *scale, const Problem &p, hipStream_t s, bool quad, const float *proj,
                            const Coords *coords)
{
    if (p.confidence) return quad ? hipErrorInvalidValue : launch_det_scale_conf(grad_out, feat, scale, p, s, proj, coords);
    const void *featT = feat;
    const long long BC = (long long)p.B * p.C;
    unsigned *gmax = static_cast<unsigned *>(scale), *fmax = gmax + BC;
    int *kexp = reinterpret_cast<int *>(fmax + BC);
    if (BC > 0x7fffffffll || (long long)p.B * p.V > 65535) return hipErrorNotSupported;
    hipError_t e = hipMemsetAsync(gmax, 0, (size_t)BC * 2 * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    long long chunks = (p.N + 2047) / 2048;
    chunks = chunks < 1 ? 1 : chunks > 64 ? 64 : chunks;
    const dim3 g1((unsigned)BC, (unsigned)chunks);
    if (p.out_bf16) hipLaunchKernelGGL(k_det_gmax<bf16_t>, g1, dim3(256), 0, s, (const bf16_t *)grad_out, gmax, p.N);
    else if (p.out_f16) hipLaunchKernelGGL(k_det_gmax<__half>, g1, dim3(256), 0, s, (const __half *)grad_out, gmax, p.N);
    else hipLaunchKernelGGL(k_det_gmax<float>, g1, dim3(256), 0, s, (const float *)grad_out, gmax, p.N);
    if (p.method == AGG_SOFTMAX && p.visible) {
        if (quad || !proj || !coords) return hipErrorInvalidValue;               // the gather family only
        const int HW = p.H * p.W;
        unsigned char *marks = reinterpret_cast<unsigned char *>(kexp + BC);
        e = hipMemsetAsync(marks, 0, (size_t)p.B * p.V * HW, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_det_mark_seen, dim3((unsigned)((p.N + 255) / 256), (unsigned)(p.B * p.V)), dim3(256), 0, s, proj, *coords, marks, p.V, p.H,
                           p.W, p.N, p.view_count);
        const dim3 g2((unsigned)((HW + kDetPix - 1) / kDetPix), (unsigned)(p.B * p.V));
        if (p.feat_f16) hipLaunchKernelGGL(k_det_fmax_seen<__half>, g2, dim3(256), 0, s, (const __half *)featT, marks, fmax, p.V, p.C, p.C4, HW);
        else hipLaunchKernelGGL(k_det_fmax_seen<float>, g2, dim3(256), 0, s, (const float *)featT, marks, fmax, p.V, p.C, p.C4, HW);
    } else if (p.method == AGG_SOFTMAX && quad) {
        const int HW = p.H * p.W, nqv = p.C4 / 4;
        const dim3 g2((unsigned)((HW + 4 * kDetPix - 1) / (4 * kDetPix)), (unsigned)((long long)p.B * p.V * nqv));
        hipLaunchKernelGGL(k_det_fmax_quad<>, g2, dim3(256), 0, s, (const float4 *)feat, fmax, p.V, p.C, nqv, HW);
    } else if (p.method == AGG_SOFTMAX) {
        const int HW = p.H * p.W;
        const dim3 g2((unsigned)((HW + kDetPix - 1) / kDetPix), (unsigned)(p.B * p.V));
        if (p.feat_f16) hipLaunchKernelGGL(k_det_fmax<__half>, g2, dim3(256), 0, s, (const __half *)featT, fmax, p.V, p.C, p.C4, HW);
        else hipLaunchKernelGGL(k_det_fmax<float>, g2, dim3(256), 0, s, (const float *)featT, fmax, p.V, p.C, p.C4, HW);
    }
    const int log2n = p.N > 1 ? 64 - __builtin_clzll((unsigned long long)(p.N - 1)) : 0;
    if (p.visible)
        // visibility-aware aggregation: a voxel may be seen by ONE view, so the mean's |ds| = |g| / |S| is bounded by |g| alone
        // -- not g / V, not g / n_b: k_det_exponent with a divisor of 1
        hipLaunchKernelGGL(k_det_exponent, dim3((unsigned)((BC + 255) / 256)), dim3(256), 0, s, gmax, fmax, kexp, BC, p.method, 1, log2n);
    else if (p.view_weights)
        hipLaunchKernelGGL(k_weighted_det_exponent, dim3((unsigned)((BC + 255) / 256)), dim3(256), 0, s, gmax, fmax, kexp, BC, p.method, p.C, p.V, log2n,
                           p.view_weights);
    else if (p.view_count)
        hipLaunchKernelGGL(k_masked_det_exponent, dim3((unsigned)((BC + 255) / 256)), dim3(256), 0, s, gmax, fmax, kexp, BC, p.method, p.C, log2n,
                           p.view_count);
    else
        hipLaunchKernelGGL(k_det_exponent, dim3((unsigned)((BC + 255) / 256)), dim3(256), 0, s, gmax, fmax, kexp, BC, p.method, p.V, log2n);
    return hipGetLastError();
}

const int *det_exponents(const void *scale, const Problem &p) { return static_cast<const int *>(scale) + 2 * (long long)p.B * p.C; }

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
