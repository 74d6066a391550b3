// The continuous voxel index of a world point on the cuboid recipe and the eight trilinear taps of an index: the arithmetic that
// volume_sample.hip (sampling at points) and volume_project.hip (ray-marching) share bit for bit.  The contract of every line is in
// volume_sample.hip's header.
#pragma once
#include "device_common.h"

namespace mvhmr {

struct VsTaps {
    int off[8];                                 // flat voxel of tap dx*4 + dy*2 + dz (0 when outside the grid)
    float w[8];
    unsigned in;                                // bit per tap: inside the grid (all clear for a dead point)
    unsigned live;                              // ... and of nonzero weight
    float wa[3][2];                             // per axis: w0, w1
};

// t of point x of sample b
__device__ __forceinline__ void vs_index(const Coords &cs, int b, float x0, float x1, float x2, float (&t)[3], float (&y)[3])
{
    const float *R = cs.rot + b * 9, *ce = cs.center + b * 3;
    const float c[3] = {ce[0], ce[1], ce[2]}, p[3] = {cs.px, cs.py, cs.pz}, st[3] = {cs.sx, cs.sy, cs.sz};
    y[0] = __fsub_rn(x0, c[0]); y[1] = __fsub_rn(x1, c[1]); y[2] = __fsub_rn(x2, c[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float d = __fmaf_rn(R[6 + a], y[2], __fmaf_rn(R[3 + a], y[1], __fmul_rn(R[a], y[0])));
        t[a] = __fdiv_rn(__fadd_rn(d, __fsub_rn(c[a], p[a])), st[a]);
    }
}

__device__ __forceinline__ bool vs_live(const float (&t)[3], int X, int Y, int Z)
{
    return t[0] > -1.f && t[0] < (float)X && t[1] > -1.f && t[1] < (float)Y && t[2] > -1.f && t[2] < (float)Z;
}

// the eight taps of index t; `ok` false (a dead point, or a lane past N) clears both masks
__device__ __forceinline__ void vs_taps(const float (&t)[3], bool ok, int X, int Y, int Z, VsTaps &tp)
{
    const int S[3] = {X, Y, Z};
    int i0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float ta = ok ? t[a] : 0.f, f = floorf(ta);
        i0[a] = (int)f;
        tp.wa[a][1] = __fsub_rn(ta, f);
        tp.wa[a][0] = __fsub_rn(__fadd_rn(f, 1.f), ta);
    }
    tp.in = 0; tp.live = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dx = k >> 2, dy = (k >> 1) & 1, dz = k & 1;
        const int ix = i0[0] + dx, iy = i0[1] + dy, iz = i0[2] + dz;
        const bool in = ok && ix >= 0 && ix < S[0] && iy >= 0 && iy < S[1] && iz >= 0 && iz < S[2];
        tp.w[k] = __fmul_rn(__fmul_rn(tp.wa[0][dx], tp.wa[1][dy]), tp.wa[2][dz]);
        tp.off[k] = in ? (ix * Y + iy) * Z + iz : 0;
        if (in) tp.in |= 1u << k;
        if (in && tp.w[k] != 0.f) tp.live |= 1u << k;
    }
}

// one channel's sample: the fma chain over the live taps
template <typename T> __device__ __forceinline__ float vs_sample(const T *__restrict__ plane, const VsTaps &tp)
{
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (tp.live >> k) & 1u ? to_f32<T>(plane[tp.off[k]]) : 0.f;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = (tp.live >> k) & 1u ? __fmaf_rn(tp.w[k], v[k], acc) : acc;
    return acc;
}

}  // namespace mvhmr
