// What the geometry backward's two translation units share (unproject_geom_bwd.hip describes the kernel; unproject_geom_bwd_weighted.hip
// holds its instances under per-view weights): the tap record, the row loads, the fixed-order wave sum.
#pragma once
#include "device_common.h"
#include "kernels.h"

namespace mvhmr {

namespace {

constexpr int kGeoTile = 32;                 // voxels per block
constexpr int kGeoGroup = 256;               // channels of the grad_out tile per pass
constexpr int kGeoLd = kGeoGroup + 4;        // tile row stride (floats): rows stay 16-B aligned, consecutive voxels 4 banks apart

// One voxel seen by one camera, with the taps of grid_sampler_2d_backward
struct alignas(16) GeoRec {
    int o00, o01, o10, o11;      // element offsets of the taps (y0,x0) (y0,x1) (y1,x0) (y1,x1) in a channels-last map, clamped into it
    float w00, w01, w10, w11;    // the forward's bilinear weights, 0 for a tap outside the map
    float tx, ty;                // ix - floor(ix), iy - floor(iy)
    int mask;                    // bit k: tap k lies inside the map (its value is read); bit 4: the view takes part
    int pad;
};

__device__ __forceinline__ GeoRec make_geo_rec(const float *__restrict__ P, float X0, float X1, float X2, int H, int W, int C4)
{
    GeoRec r;
    r.o00 = r.o01 = r.o10 = r.o11 = 0;
    r.w00 = r.w01 = r.w10 = r.w11 = 0.f;
    r.tx = r.ty = 0.f;
    r.mask = 0;
    r.pad = 0;
    // projection, divides and Q1 exactly as make_taps (the forward's rounding order)
    const float a = __fmaf_rn(P[3], 1.f, __fmaf_rn(P[2], X2, __fmaf_rn(P[1], X1, __fmul_rn(P[0], X0))));
    const float b = __fmaf_rn(P[7], 1.f, __fmaf_rn(P[6], X2, __fmaf_rn(P[5], X1, __fmul_rn(P[4], X0))));
    const float z = __fmaf_rn(P[11], 1.f, __fmaf_rn(P[10], X2, __fmaf_rn(P[9], X1, __fmul_rn(P[8], X0))));
    if (!(z > 0.f)) return r;
    const float u = __fdiv_rn(a, z), v = __fdiv_rn(b, z);
    const float gx = __fmul_rn(2.f, __fsub_rn(__fdiv_rn(u, (float)H), 0.5f));
    const float gy = __fmul_rn(2.f, __fsub_rn(__fdiv_rn(v, (float)W), 0.5f));
    const float ix = __fmul_rn(__fmul_rn(__fadd_rn(gx, 1.f), 0.5f), (float)(W - 1));
    const float iy = __fmul_rn(__fmul_rn(__fadd_rn(gy, 1.f), 0.5f), (float)(H - 1));
    // every tap outside (or NaN): value and gradient 0.  ix == -1 is KEPT: the tap at x = 0 has weight 0 but a gradient
    if (!(ix >= -1.f && ix < (float)W && iy >= -1.f && iy < (float)H)) return r;
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
    const float wx1 = __fsub_rn(ix, fx0), wx0 = __fsub_rn(__fadd_rn(fx0, 1.f), ix);
    const float wy1 = __fsub_rn(iy, fy0), wy0 = __fsub_rn(__fadd_rn(fy0, 1.f), iy);
    const bool xin0 = x0 >= 0, xin1 = x1 <= W - 1, yin0 = y0 >= 0, yin1 = y1 <= H - 1;
    r.w00 = (xin0 && yin0) ? __fmul_rn(wx0, wy0) : 0.f;
    r.w01 = (xin1 && yin0) ? __fmul_rn(wx1, wy0) : 0.f;
    r.w10 = (xin0 && yin1) ? __fmul_rn(wx0, wy1) : 0.f;
    r.w11 = (xin1 && yin1) ? __fmul_rn(wx1, wy1) : 0.f;
    const int xc0 = xin0 ? x0 : 0, xc1 = xin1 ? x1 : W - 1, yc0 = yin0 ? y0 : 0, yc1 = yin1 ? y1 : H - 1;
    r.o00 = (yc0 * W + xc0) * C4;
    r.o01 = (yc0 * W + xc1) * C4;
    r.o10 = (yc1 * W + xc0) * C4;
    r.o11 = (yc1 * W + xc1) * C4;
    r.tx = wx1;
    r.ty = wy1;
    r.mask = (xin0 && yin0 ? 1 : 0) | (xin1 && yin0 ? 2 : 0) | (xin0 && yin1 ? 4 : 0) | (xin1 && yin1 ? 8 : 0) | 16;
    return r;
}

__device__ __forceinline__ GeoRec uniform_geo(const GeoRec &r)
{
    GeoRec u;
    u.o00 = uniform(r.o00); u.o01 = uniform(r.o01); u.o10 = uniform(r.o10); u.o11 = uniform(r.o11);
    u.w00 = uniform(r.w00); u.w01 = uniform(r.w01); u.w10 = uniform(r.w10); u.w11 = uniform(r.w11);
    u.tx = uniform(r.tx); u.ty = uniform(r.ty);
    u.mask = uniform(r.mask);
    u.pad = 0;
    return u;
}

// CPL consecutive channels of one channels-last row (CPL * sizeof(T)-byte aligned)
template <typename T, int CPL> struct Row;
template <typename T> struct Row<T, 4> {
    static __device__ __forceinline__ void load(const T *p, float (&o)[4])
    {
        const f32x4 a = Vec4<T>::load(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = a.v[i];
    }
};
template <> struct Row<float, 2> {
    static __device__ __forceinline__ void load(const float *p, float (&o)[2])
    {
        const float2 a = *reinterpret_cast<const float2 *>(p);
        o[0] = a.x; o[1] = a.y;
    }
};
template <> struct Row<__half, 2> {
    static __device__ __forceinline__ void load(const __half *p, float (&o)[2])
    {
        const float2 a = __half22float2(*reinterpret_cast<const __half2 *>(p));
        o[0] = a.x; o[1] = a.y;
    }
};
template <typename T> struct Row<T, 1> {
    static __device__ __forceinline__ void load(const T *p, float (&o)[1]) { o[0] = to_f32<T>(*p); }
};

// sum over the wave, in a fixed order (DPP inside each row of 16 lanes, then the four row sums): the same bits every run
__device__ __forceinline__ float wave_sum(float x)
{
    auto dpp = [](float y, auto ctrl) __attribute__((always_inline)) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, y), decltype(ctrl)::value, 0xF, 0xF, false));
    };
    x += dpp(x, std::integral_constant<int, 0xB1>());     // quad_perm [1,0,3,2]
    x += dpp(x, std::integral_constant<int, 0x4E>());     // quad_perm [2,3,0,1]
    x += dpp(x, std::integral_constant<int, 0x124>());    // row_ror:4
    x += dpp(x, std::integral_constant<int, 0x128>());    // row_ror:8
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 48));
    return (r0 + r1) + (r2 + r3);
}

constexpr int geo_cpl(int V) { return V <= 4 ? 4 : V <= 8 ? 2 : 1; }

size_t geo_lds_bytes(int V)
{
    return sizeof(GeoRec) * kGeoTile * V + sizeof(float2) * kGeoTile * V + sizeof(float) * kGeoTile * 4 + sizeof(float) * kGeoTile * kGeoLd;
}
// the weighted instances keep the per-(voxel, view) sums of the weight gradient behind the tile
size_t geo_lds_bytes_weighted(int V) { return geo_lds_bytes(V) + sizeof(float) * kGeoTile * V; }
unsigned geom_tiles(const Problem &p) { return (unsigned)((p.N + kGeoTile - 1) / kGeoTile); }

}  // namespace

}  // namespace mvhmr
