// Ray-marching volumes into camera-view maps (include/mvhmr_unproject.h: mvhmr_project_volume_*): renders (B,C,X,Y,Z)
// volumes that live on the cuboid recipe into (B,V,C,Hm,Wm) maps, the direction opposite to un-projection.  No sample is ever stored.
//
// Arithmetic contract (tests/volproject_oracle.py restates it in numpy, operation for operation; every line one rounded fp32 operation).
// rays[b][v] is a 3 x 4 row-major matrix [D | o]; pixel (u, v) = (column, row) of the map, as floats:
//   t_o   = vs_index(o)                                                      volume_sample.hip's index of the point o, bit for bit
//   d_i   = fma(D[i][1], v, fma(D[i][0], u, D[i][2]))
//   r_a   = fma(R[2][a], d_2, fma(R[1][a], d_1, fmul(R[0][a], d_0)))         R^T d
//   e_a   = fdiv(r_a, step_a)                                                index units per unit of lambda
//   clip, with hi_a = float(S_a - 1), lin = min_depth, lout = max_depth, axes in order a = 0, 1, 2:
//     e_a == 0 (+-0):  the ray misses unless 0 <= t_o,a <= hi_a (a NaN fails)
//     else  l0 = fdiv(fsub(0, t_o,a), e_a),  l1 = fdiv(fsub(hi_a, t_o,a), e_a);  a NaN l0 or l1 is a miss
//           near = l0 < l1 ? l0 : l1,  far = l0 < l1 ? l1 : l0;  lin = near > lin ? near : lin;  lout = far < lout ? far : lout
//   hit iff  lin < lout  and  lin > -inf  and  lout < +inf                   ranges = (lin, lout), (0, 0) for a miss
//   h     = fdiv(fsub(lout, lin), float(K))
//   lam_k = fma(float(k) + 0.5, h, lin),   t_k,a = fma(lam_k, e_a, t_o,a)      k = 0 .. K-1
//   s_k   = the sample at index t_k by volume_sample.hip's rule (vs_live, vs_taps, the fma chain of vs_sample: zero padding, a tap of
//           weight 0 is not read, taps in the order dx*4 + dy*2 + dz)
// Methods, over k ascending:
//   mean     acc = fadd(acc, s_k) from 0;  out = fdiv(acc, float(K))
//   max      m = s_0, arg = 0;  s_k > m replaces m and arg (so ties keep the lowest k);  out = m
//   softmax  z = fmul(beta, s_k);  from m = -inf, S = W = 0:
//              if z > m:  r = expf(fsub(m, z)), S = fmul(S, r), W = fmul(W, r), m = z
//              p = expf(fsub(z, m)),  S = fadd(S, p),  W = fma(p, s_k, W)
//            out = fdiv(W, S),  lse = fadd(m, logf(S))
//   a miss gives 0 in every channel (lse 0, arg 0) and adds to no gradient
// Volume gradient: the rays are marched again.  ds_k = fdiv(g, float(K)) (mean); g at k = arg (max);
//   fmul(fmul(g, p), fma(beta, fsub(s_k, out), 1)) with p = expf(fsub(z, lse)) (softmax).  Every live tap adds det_fixed(fmul(w, ds_k), E)
// to an int64 accumulator with a 64-bit integer atomic (det_scale.h: integer adds are associative, so the sums carry the same bits in any
// order); a term that rounds to 0 is not added.  E[b][c] is fixed before any add (k_pv3d_exponent): N * bound * 2^E < 2^62 with
// N = V * Hm * Wm * K, the most taps a voxel can receive, and bound = gmax / K (mean), gmax (max), gmax (1 + 2 |beta| F) (softmax;
// F = max |volume| of the (b, c), |s_k - out| <= 2 F and p <= 1).  A non-finite bound poisons the (b, c): NaN, nothing added.
// k_pv3d_cast does the one rounding to the volume's dtype.  No float atomic anywhere.
#include "device_common.h"
#include "det_scale.h"
#include "kernels.h"
#include "mvhmr_unproject.h"
#include "volume_taps.h"

#include <type_traits>

namespace mvhmr {

namespace {

constexpr int kPvTile = 8;                      // a wave covers 8 x 8 pixels: neighbouring rays touch neighbouring voxels
constexpr int kPvGroup = 8;                     // channels per block: their accumulators stay in registers over the march
constexpr int kPvUnroll = 4;                    // channels per trip of a sample's channel loop: 4 x 8 taps = 32 loads in flight per lane
constexpr int kPvMaxSamples = 1024;
constexpr size_t kPvAccBudget = (size_t)1 << 30;

struct PvDims {
    int V, C, X, Hm, Wm, K, tiles_x, tiles, groups;
    float dmin, dmax, beta;
};

struct PvRay {
    float to[3], e[3], lin, lout, h;
    bool hit;
};

__device__ __forceinline__ void pv_ray(const Coords &cs, const float *__restrict__ ray, int b, float u, float v, const PvDims &d, PvRay &r)
{
    float y[3];
    vs_index(cs, b, ray[3], ray[7], ray[11], r.to, y);
    float dir[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) dir[i] = __fmaf_rn(ray[4 * i + 1], v, __fmaf_rn(ray[4 * i], u, ray[4 * i + 2]));
    const float *R = cs.rot + b * 9;
    const float st[3] = {cs.sx, cs.sy, cs.sz};
    const int S[3] = {d.X, cs.Y, cs.Z};
    bool ok = true;
    float lin = d.dmin, lout = d.dmax;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float ra = __fmaf_rn(R[6 + a], dir[2], __fmaf_rn(R[3 + a], dir[1], __fmul_rn(R[a], dir[0])));
        const float e = __fdiv_rn(ra, st[a]), hi = (float)(S[a] - 1), to = r.to[a];
        r.e[a] = e;
        if (e == 0.f) {
            ok = ok && to >= 0.f && to <= hi;
        } else {
            const float l0 = __fdiv_rn(__fsub_rn(0.f, to), e), l1 = __fdiv_rn(__fsub_rn(hi, to), e);
            ok = ok && l0 == l0 && l1 == l1;
            const float near = l0 < l1 ? l0 : l1, far = l0 < l1 ? l1 : l0;
            lin = near > lin ? near : lin;
            lout = far < lout ? far : lout;
        }
    }
    const float inf = __builtin_inff();
    r.hit = ok && lin < lout && lin > -inf && lout < inf;
    r.lin = r.hit ? lin : 0.f;
    r.lout = r.hit ? lout : 0.f;
    r.h = __fdiv_rn(__fsub_rn(r.lout, r.lin), (float)d.K);
}

__device__ __forceinline__ void pv_taps(const PvRay &r, int k, int X, int Y, int Z, VsTaps &tp)
{
    const float lam = __fmaf_rn((float)k + 0.5f, r.h, r.lin);
    const float t[3] = {__fmaf_rn(lam, r.e[0], r.to[0]), __fmaf_rn(lam, r.e[1], r.to[1]), __fmaf_rn(lam, r.e[2], r.to[2])};
    vs_taps(t, vs_live(t, X, Y, Z), X, Y, Z, tp);
}

// which (sample, channel group, view, pixel) this lane works on: blocks of one sample are adjacent, the tiles of a view innermost
struct PvWhere {
    int b, g, v, px, py;
    bool in;
};
__device__ __forceinline__ PvWhere pv_where(const PvDims &d, int groups)
{
    PvWhere w;
    long long bid = blockIdx.x;
    const int tile = (int)(bid % d.tiles);
    bid /= d.tiles;
    w.v = (int)(bid % d.V);
    bid /= d.V;
    w.g = (int)(bid % groups);
    w.b = (int)(bid / groups);
    w.px = (tile % d.tiles_x) * kPvTile + (threadIdx.x & 7);
    w.py = (tile / d.tiles_x) * kPvTile + (threadIdx.x >> 3);
    w.in = w.px < d.Wm && w.py < d.Hm;
    return w;
}

// ---- forward: one lane per pixel; per sample the taps once, then the block's channels kPvUnroll at a time
template <typename T, int METHOD>
__global__ void __launch_bounds__(64)
k_pv3d_fwd(const T *__restrict__ vol, const Coords cs, const float *__restrict__ rays, const PvDims d, float *__restrict__ maps,
           float *__restrict__ ranges, void *__restrict__ aux)
{
    const PvWhere w = pv_where(d, d.groups);
    if (!w.in) return;
    const int Y = cs.Y, Z = cs.Z, HW = d.Hm * d.Wm, pix = w.py * d.Wm + w.px;
    const long long bv = (long long)w.b * d.V + w.v;
    PvRay r;
    pv_ray(cs, rays + bv * 12, w.b, (float)w.px, (float)w.py, d, r);
    if (w.g == 0) {
        float *o = ranges + (bv * HW + pix) * 2;
        o[0] = r.lin; o[1] = r.lout;
    }
    const size_t Vox = (size_t)d.X * Y * Z;
    const int c0 = w.g * kPvGroup;
    float a0[kPvGroup], a1[kPvGroup], a2[kPvGroup];
    int ak[kPvGroup];
#pragma unroll
    for (int u = 0; u < kPvGroup; ++u) {
        a0[u] = METHOD == MVHMR_PROJECT_SOFTMAX ? -__builtin_inff() : 0.f;
        a1[u] = 0.f; a2[u] = 0.f; ak[u] = 0;
    }
    const int K = r.hit ? d.K : 0;
    for (int k = 0; k < K; ++k) {
        VsTaps tp;
        pv_taps(r, k, d.X, Y, Z, tp);
#pragma unroll
        for (int u0 = 0; u0 < kPvGroup; u0 += kPvUnroll) {
            if (c0 + u0 >= d.C) break;
            float val[kPvUnroll][8];
#pragma unroll
            for (int u = 0; u < kPvUnroll; ++u) {
                const bool have = c0 + u0 + u < d.C;
                const T *plane = vol + ((size_t)w.b * d.C + (have ? c0 + u0 + u : c0)) * Vox;
#pragma unroll
                for (int j = 0; j < 8; ++j) val[u][j] = have && ((tp.live >> j) & 1u) ? to_f32<T>(plane[tp.off[j]]) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kPvUnroll; ++u) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) s = (tp.live >> j) & 1u ? __fmaf_rn(tp.w[j], val[u][j], s) : s;
                const int i = u0 + u;
                if constexpr (METHOD == MVHMR_PROJECT_MEAN) {
                    a0[i] = __fadd_rn(a0[i], s);
                } else if constexpr (METHOD == MVHMR_PROJECT_MAX) {
                    const bool take = k == 0 || s > a0[i];
                    a0[i] = take ? s : a0[i];
                    ak[i] = take ? k : ak[i];
                } else {
                    const float z = __fmul_rn(d.beta, s);
                    if (z > a0[i]) {
                        const float rs = expf(__fsub_rn(a0[i], z));
                        a1[i] = __fmul_rn(a1[i], rs);
                        a2[i] = __fmul_rn(a2[i], rs);
                        a0[i] = z;
                    }
                    const float p = expf(__fsub_rn(z, a0[i]));
                    a1[i] = __fadd_rn(a1[i], p);
                    a2[i] = __fmaf_rn(p, s, a2[i]);
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kPvGroup; ++u) {
        const int c = c0 + u;
        if (c >= d.C) break;
        const size_t at = ((size_t)bv * d.C + c) * HW + pix;
        if constexpr (METHOD == MVHMR_PROJECT_MEAN) {
            maps[at] = r.hit ? __fdiv_rn(a0[u], (float)d.K) : 0.f;
        } else if constexpr (METHOD == MVHMR_PROJECT_MAX) {
            maps[at] = a0[u];
            static_cast<int *>(aux)[at] = ak[u];
        } else {
            maps[at] = r.hit ? __fdiv_rn(a2[u], a1[u]) : 0.f;
            static_cast<float *>(aux)[at] = r.hit ? __fadd_rn(a0[u], logf(a1[u])) : 0.f;
        }
    }
}

// ---- the exponent E[b][c] of the fixed-point accumulator: N * bound * 2^E < 2^62 (det_scale.h's scheme, this op's bounds)
__global__ void __launch_bounds__(256)
k_pv3d_exponent(const unsigned *__restrict__ gmax, const unsigned *__restrict__ fmax, int *__restrict__ kexp, long long BC, int method, int K,
                int log2n, float abs_beta)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    const unsigned gb = gmax[i], fb = method == MVHMR_PROJECT_SOFTMAX ? fmax[i] : 0u;
    if (gb >= 0x7f800000u || fb >= 0x7f800000u) { kexp[i] = kDetPoison; return; }
    const double g = (double)__builtin_bit_cast(float, gb), f = (double)__builtin_bit_cast(float, fb);
    const double bound = method == MVHMR_PROJECT_MEAN ? g / K : method == MVHMR_PROJECT_MAX ? g : g * (1.0 + 2.0 * (double)abs_beta * f);
    if (bound == 0.0) { kexp[i] = 0; return; }
    if (!(bound < 3.4028234663852886e38)) { kexp[i] = kDetPoison; return; }
    int e;
    frexp(bound, &e);                                                             // bound < 2^e
    kexp[i] = 62 - log2n - e;
}

__device__ __forceinline__ void pv_add(unsigned long long *__restrict__ plane, const VsTaps &tp, float ds, int k)
{
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (!((tp.live >> j) & 1u)) continue;
        const unsigned long long q = det_fixed(__fmul_rn(tp.w[j], ds), k);
        if (q) atomicAdd(plane + tp.off[j], q);
    }
}

// ---- volume gradient of one pass of `cg` channels from `c_first`: the rays marched again, the taps added to acc (B, cg, X*Y*Z)
template <typename T, int METHOD>
__global__ void __launch_bounds__(64)
k_pv3d_bwd(const T *__restrict__ vol, const Coords cs, const float *__restrict__ rays, const PvDims d, const float *__restrict__ grad_maps,
           const float *__restrict__ maps, const void *__restrict__ aux, const int *__restrict__ kexp, unsigned long long *__restrict__ acc,
           int c_first, int cg, int groups)
{
    const PvWhere w = pv_where(d, groups);
    if (!w.in) return;
    const int Y = cs.Y, Z = cs.Z, HW = d.Hm * d.Wm, pix = w.py * d.Wm + w.px;
    const long long bv = (long long)w.b * d.V + w.v;
    PvRay r;
    pv_ray(cs, rays + bv * 12, w.b, (float)w.px, (float)w.py, d, r);
    if (!r.hit) return;
    const size_t Vox = (size_t)d.X * Y * Z;
    const int l0 = w.g * kPvGroup;                                                // the block's first channel inside the pass
    float g[kPvGroup], out[kPvGroup], lse[kPvGroup];
    int ke[kPvGroup], ak[kPvGroup];
    unsigned active = 0;
#pragma unroll
    for (int u = 0; u < kPvGroup; ++u) {
        g[u] = 0.f; out[u] = 0.f; lse[u] = 0.f; ke[u] = 0; ak[u] = 0;
        if (l0 + u >= cg) continue;
        const int c = c_first + l0 + u;
        const size_t at = ((size_t)bv * d.C + c) * HW + pix;
        ke[u] = kexp[(size_t)w.b * d.C + c];
        const float gu = grad_maps[at];
        if (ke[u] == kDetPoison || gu == 0.f) continue;
        active |= 1u << u;
        if constexpr (METHOD == MVHMR_PROJECT_MEAN) g[u] = __fdiv_rn(gu, (float)d.K);
        else g[u] = gu;
        if constexpr (METHOD == MVHMR_PROJECT_MAX) ak[u] = static_cast<const int *>(aux)[at];
        if constexpr (METHOD == MVHMR_PROJECT_SOFTMAX) { out[u] = maps[at]; lse[u] = static_cast<const float *>(aux)[at]; }
    }
    if (!active) return;
    unsigned long long *acc_b = acc + ((size_t)w.b * cg + l0) * Vox;
    if constexpr (METHOD == MVHMR_PROJECT_MAX) {
#pragma unroll
        for (int u = 0; u < kPvGroup; ++u) {
            if (!((active >> u) & 1u)) continue;
            VsTaps tp;
            pv_taps(r, ak[u], d.X, Y, Z, tp);
            pv_add(acc_b + (size_t)u * Vox, tp, g[u], ke[u]);
        }
    } else {
        for (int k = 0; k < d.K; ++k) {
            VsTaps tp;
            pv_taps(r, k, d.X, Y, Z, tp);
#pragma unroll
            for (int u = 0; u < kPvGroup; ++u) {
                if (!((active >> u) & 1u)) continue;
                float ds = g[u];
                if constexpr (METHOD == MVHMR_PROJECT_SOFTMAX) {
                    const float s = vs_sample<T>(vol + ((size_t)w.b * d.C + c_first + l0 + u) * Vox, tp);
                    const float p = expf(__fsub_rn(__fmul_rn(d.beta, s), lse[u]));
                    ds = __fmul_rn(__fmul_rn(g[u], p), __fmaf_rn(d.beta, __fsub_rn(s, out[u]), 1.f));
                }
                pv_add(acc_b + (size_t)u * Vox, tp, ds, ke[u]);
            }
        }
    }
}

// ---- the accumulator of one pass -> grad_volumes in the volume's dtype: the one rounding
template <typename T>
__global__ void __launch_bounds__(256)
k_pv3d_cast(const unsigned long long *__restrict__ acc, const int *__restrict__ kexp, T *__restrict__ grad_vol, long long n, int C, int c_first, int cg,
            long long Vox)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long row = i / Vox, b = row / cg;
        const int c = c_first + (int)(row % cg);
        grad_vol[(b * C + c) * Vox + (i - row * Vox)] = from_f32<T>(det_value(acc[i], kexp[b * C + c]));
    }
}

template <typename F> hipError_t with_storage(int dtype, F f)
{
    switch (dtype) {
    case MVHMR_F32: return f((float *)nullptr);
    case MVHMR_F16: return f((__half *)nullptr);
    case MVHMR_BF16: return f((bf16_t *)nullptr);
    }
    return hipErrorNotSupported;
}

template <typename F> hipError_t with_method(int method, F f)
{
    switch (method) {
    case MVHMR_PROJECT_MEAN: return f(std::integral_constant<int, MVHMR_PROJECT_MEAN>());
    case MVHMR_PROJECT_MAX: return f(std::integral_constant<int, MVHMR_PROJECT_MAX>());
    case MVHMR_PROJECT_SOFTMAX: return f(std::integral_constant<int, MVHMR_PROJECT_SOFTMAX>());
    }
    return hipErrorInvalidValue;
}

PvDims pv_dims(int V, int C, int X, int Hm, int Wm, int K, float beta, float dmin, float dmax)
{
    PvDims d;
    d.V = V; d.C = C; d.X = X; d.Hm = Hm; d.Wm = Wm; d.K = K;
    d.tiles_x = (Wm + kPvTile - 1) / kPvTile;
    d.tiles = d.tiles_x * ((Hm + kPvTile - 1) / kPvTile);
    d.groups = (C + kPvGroup - 1) / kPvGroup;
    d.dmin = dmin; d.dmax = dmax; d.beta = beta;
    return d;
}

size_t pv_tables_bytes(long long B, long long C) { return ((size_t)B * C * 3 * sizeof(int) + 255) / 256 * 256; }

}  // namespace

int pv3d_max_samples() { return kPvMaxSamples; }
void pv3d_channel_group(int group_unroll[2]) { group_unroll[0] = kPvGroup; group_unroll[1] = kPvUnroll; }

// channels per pass of the volume gradient: as many as keep the accumulator within 2^30 bytes, one at the least
int pv3d_pass_channels(long long B, long long C, long long vox)
{
    const size_t per = (size_t)B * vox * sizeof(unsigned long long);
    const size_t fit = kPvAccBudget > pv_tables_bytes(B, C) ? (kPvAccBudget - pv_tables_bytes(B, C)) / per : 0;
    return (int)(fit < 1 ? 1 : fit > (size_t)C ? (size_t)C : fit);
}

// the three tables (gmax, fmax, E: B * C words each), then the accumulator of one pass
size_t pv3d_workspace_bytes(long long B, long long C, long long vox)
{
    return pv_tables_bytes(B, C) + (size_t)B * pv3d_pass_channels(B, C, vox) * vox * sizeof(unsigned long long);
}

hipError_t launch_pv3d_forward(const void *vol, int dtype, const Coords &cs, const float *rays, int B, int V, int C, int X, int Hm, int Wm, int K,
                               int method, float beta, float dmin, float dmax, float *maps, float *ranges, void *aux, hipStream_t s)
{
    const PvDims d = pv_dims(V, C, X, Hm, Wm, K, beta, dmin, dmax);
    const long long blocks = (long long)B * d.groups * V * d.tiles;
    if (blocks > 0x7fffffffLL) return hipErrorNotSupported;
    return with_storage(dtype, [&](auto *tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        return with_method(method, [&](auto m) {
            hipLaunchKernelGGL((k_pv3d_fwd<T, decltype(m)::value>), dim3((unsigned)blocks), dim3(64), 0, s, static_cast<const T *>(vol), cs, rays, d, maps,
                               ranges, aux);
            return hipGetLastError();
        });
    });
}

hipError_t launch_pv3d_backward_volumes(const void *vol, int dtype, const Coords &cs, const float *rays, int B, int V, int C, int X, int Hm, int Wm,
                                        int K, int method, float beta, float dmin, float dmax, const float *grad_maps, const float *maps,
                                        const void *aux, void *grad_vol, void *ws, hipStream_t s)
{
    const PvDims d = pv_dims(V, C, X, Hm, Wm, K, beta, dmin, dmax);
    const long long BC = (long long)B * C, Vox = (long long)X * cs.Y * cs.Z, HW = (long long)Hm * Wm, rows = BC * V;
    const int cg_max = pv3d_pass_channels(B, C, Vox);
    if (rows > 0x7fffffffLL || (long long)B * ((cg_max + kPvGroup - 1) / kPvGroup) * V * d.tiles > 0x7fffffffLL) return hipErrorNotSupported;
    const size_t tables = pv_tables_bytes(B, C);
    unsigned *gmax = static_cast<unsigned *>(ws), *fmax = gmax + BC;
    int *kexp = reinterpret_cast<int *>(fmax + BC);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(ws) + tables);
    hipError_t e = hipMemsetAsync(ws, 0, tables, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_det_gmax<float, DetRowsViews, int, int>), dim3((unsigned)rows, chunks_of(HW)), dim3(256), 0, s, grad_maps, gmax, HW, V, C);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return with_storage(dtype, [&](auto *tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        if (method == MVHMR_PROJECT_SOFTMAX) {
            hipLaunchKernelGGL((k_det_gmax<T, DetRowsIdentity>), dim3((unsigned)BC, chunks_of(Vox)), dim3(256), 0, s, static_cast<const T *>(vol), fmax, Vox);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_pv3d_exponent, dim3((unsigned)((BC + 255) / 256)), dim3(256), 0, s, gmax, fmax, kexp, BC, method, K,
                           log2_ceil((long long)V * HW * K), fabsf(beta));
        if ((e = hipGetLastError()) != hipSuccess) return e;
        for (int c_first = 0; c_first < C; c_first += cg_max) {
            const int cg = C - c_first < cg_max ? C - c_first : cg_max, groups = (cg + kPvGroup - 1) / kPvGroup;
            const long long n = (long long)B * cg * Vox;
            if ((e = hipMemsetAsync(acc, 0, (size_t)n * sizeof(unsigned long long), s)) != hipSuccess) return e;
            e = with_method(method, [&](auto m) {
                hipLaunchKernelGGL((k_pv3d_bwd<T, decltype(m)::value>), dim3((unsigned)((long long)B * groups * V * d.tiles)), dim3(64), 0, s,
                                   static_cast<const T *>(vol), cs, rays, d, grad_maps, maps, aux, kexp, acc, c_first, cg, groups);
                return hipGetLastError();
            });
            if (e != hipSuccess) return e;
            const unsigned blocks = (unsigned)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
            hipLaunchKernelGGL(k_pv3d_cast<T>, dim3(blocks), dim3(256), 0, s, acc, kexp, static_cast<T *>(grad_vol), n, C, c_first, cg, Vox);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        return hipSuccess;
    });
}

}  // namespace mvhmr
