// Lens distortion: the Brown-Conrady model of OpenCV's projectPoints between the perspective divide and the Q1 grid
// normalisation of make_taps.  One record per (sample, view), ten floats:
//     fx, fy, cx, cy      the intrinsics that went into the projection matrix (feature level, zero skew)
//     k1, k2, p1, p2, k3  the coefficients, in OpenCV's order
//     r2max               the fold-back guard: a ray with !(r2 <= r2max) gives an exactly zero sample (as z <= 0 does)
// Every operation of lens_apply is one separately rounded fp32 operation in the order written here (no FMA), so that a float32
// restatement on the host reproduces the positions bit for bit and oracle and kernel pick the same bilinear cell.
#pragma once
#include "device_common.h"

namespace mvhmr {

constexpr int kLensWords = 10;

struct Lens {
    float fx, fy, cx, cy, k1, k2, p1, p2, k3, r2max;
};

__device__ __forceinline__ Lens load_lens(const float *__restrict__ L)
{
    return Lens{L[0], L[1], L[2], L[3], L[4], L[5], L[6], L[7], L[8], L[9]};
}

// all five coefficients are +0.0 or -0.0: the view takes the plain path (make_taps), whatever its intrinsics say
__device__ __forceinline__ bool lens_is_plain(const float *__restrict__ L)
{
    return L[4] == 0.f && L[5] == 0.f && L[6] == 0.f && L[7] == 0.f && L[8] == 0.f;
}

// normalised coordinates of the pin-hole pixel position and r2; false when the ray lies past the guard (or anything is NaN)
__device__ __forceinline__ bool lens_normalise(const Lens &l, float u, float v, float &xn, float &yn, float &xx, float &yy, float &xy, float &r2)
{
    xn = __fdiv_rn(__fsub_rn(u, l.cx), l.fx);
    yn = __fdiv_rn(__fsub_rn(v, l.cy), l.fy);
    xx = __fmul_rn(xn, xn);
    yy = __fmul_rn(yn, yn);
    xy = __fmul_rn(xn, yn);
    r2 = __fadd_rn(xx, yy);
    return r2 <= l.r2max;
}

// (u, v) -> (u', v'): the distorted pixel position.  false: the view gives this voxel an exactly zero sample
__device__ __forceinline__ bool lens_apply(const Lens &l, float u, float v, float &ud, float &vd)
{
    float xn, yn, xx, yy, xy, r2;
    if (!lens_normalise(l, u, v, xn, yn, xx, yy, xy, r2)) return false;
    const float rad = __fadd_rn(1.f, __fmul_rn(r2, __fadd_rn(l.k1, __fmul_rn(r2, __fadd_rn(l.k2, __fmul_rn(r2, l.k3))))));   // Horner, innermost first
    const float xd = __fadd_rn(__fadd_rn(__fmul_rn(xn, rad), __fmul_rn(__fmul_rn(2.f, l.p1), xy)), __fmul_rn(l.p2, __fadd_rn(r2, __fmul_rn(2.f, xx))));
    const float yd = __fadd_rn(__fadd_rn(__fmul_rn(yn, rad), __fmul_rn(l.p1, __fadd_rn(r2, __fmul_rn(2.f, yy)))), __fmul_rn(__fmul_rn(2.f, l.p2), xy));
    ud = __fadd_rn(__fmul_rn(l.fx, xd), l.cx);
    vd = __fadd_rn(__fmul_rn(l.fy, yd), l.cy);
    return true;
}

// (d/du', d/dv') -> (d/du, d/dv): the transposed 2x2 Jacobian of lens_apply at (u, v).  In normalised coordinates it is symmetric,
//     Jxx = rad + 2 xn^2 rad' + 2 p1 yn + 6 p2 xn      Jxy = 2 xn yn rad' + 2 p1 xn + 2 p2 yn      Jyy = rad + 2 yn^2 rad' + 6 p1 yn + 2 p2 xn
// with rad' = d rad / d r2 = k1 + 2 k2 r2 + 3 k3 r2^2; in pixels the off-diagonal terms carry fx / fy and fy / fx.  Plain fp32: the
// gradient has no pinned rounding.
__device__ __forceinline__ void lens_pull_back(const Lens &l, float u, float v, float &du, float &dv)
{
    float xn, yn, xx, yy, xy, r2;
    lens_normalise(l, u, v, xn, yn, xx, yy, xy, r2);
    const float rad = 1.f + r2 * (l.k1 + r2 * (l.k2 + r2 * l.k3));
    const float drad = l.k1 + r2 * (2.f * l.k2 + 3.f * l.k3 * r2);
    const float jxx = rad + 2.f * xx * drad + 2.f * l.p1 * yn + 6.f * l.p2 * xn;
    const float jxy = 2.f * xy * drad + 2.f * l.p1 * xn + 2.f * l.p2 * yn;
    const float jyy = rad + 2.f * yy * drad + 6.f * l.p1 * yn + 2.f * l.p2 * xn;
    const float gu = du * jxx + dv * (jxy * __fdiv_rn(l.fy, l.fx));       // du'/du = Jxx, dv'/du = (fy / fx) Jxy
    const float gv = du * (jxy * __fdiv_rn(l.fx, l.fy)) + dv * jyy;       // du'/dv = (fx / fy) Jxy, dv'/dv = Jyy
    du = gu;
    dv = gv;
}

// make_taps (device_common.h) with the lens step between the divides and the Q1 grid normalisation: a copy, so that every kernel that
// calls make_taps keeps the code it had
__device__ __forceinline__ Taps make_taps_lens(const float *__restrict__ P, const Lens &l, float X0, float X1, float X2, int H, int W)
{
    const float a = __fmaf_rn(P[3], 1.f, __fmaf_rn(P[2], X2, __fmaf_rn(P[1], X1, __fmul_rn(P[0], X0))));
    const float b = __fmaf_rn(P[7], 1.f, __fmaf_rn(P[6], X2, __fmaf_rn(P[5], X1, __fmul_rn(P[4], X0))));
    const float z = __fmaf_rn(P[11], 1.f, __fmaf_rn(P[10], X2, __fmaf_rn(P[9], X1, __fmul_rn(P[8], X0))));
    Taps t;
    t.x0 = t.y0 = t.x1 = t.y1 = 0;
    t.w00 = t.w01 = t.w10 = t.w11 = 0.f;
    t.rx0 = t.ry0 = 0;
    t.any = 0;
    if (!(z > 0.f)) return t;                        // z <= 0 (or NaN): sample is exactly 0
    float u, v;
    if (!lens_apply(l, __fdiv_rn(a, z), __fdiv_rn(b, z), u, v)) return t;             // past the fold-back guard: exactly 0 as well
    // quirk Q1: x is normalised by feature_shape[0] = Hf, y by feature_shape[1] = Wf
    const float gx = __fmul_rn(2.f, __fsub_rn(__fdiv_rn(u, (float)H), 0.5f));
    const float gy = __fmul_rn(2.f, __fsub_rn(__fdiv_rn(v, (float)W), 0.5f));
    const float ix = __fmul_rn(__fmul_rn(__fadd_rn(gx, 1.f), 0.5f), (float)(W - 1));
    const float iy = __fmul_rn(__fmul_rn(__fadd_rn(gy, 1.f), 0.5f), (float)(H - 1));
    if (!(ix > -1.f && ix < (float)W && iy > -1.f && iy < (float)H)) return t;        // all four taps outside
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
    const float wx1 = __fsub_rn(ix, fx0), wx0 = __fsub_rn(__fadd_rn(fx0, 1.f), ix);
    const float wy1 = __fsub_rn(iy, fy0), wy0 = __fsub_rn(__fadd_rn(fy0, 1.f), iy);
    const bool xin0 = x0 >= 0, xin1 = x1 <= W - 1, yin0 = y0 >= 0, yin1 = y1 <= H - 1;
    t.w00 = (xin0 && yin0) ? __fmul_rn(wx0, wy0) : 0.f;
    t.w01 = (xin1 && yin0) ? __fmul_rn(wx1, wy0) : 0.f;
    t.w10 = (xin0 && yin1) ? __fmul_rn(wx0, wy1) : 0.f;
    t.w11 = (xin1 && yin1) ? __fmul_rn(wx1, wy1) : 0.f;
    t.x0 = xin0 ? x0 : 0;
    t.y0 = yin0 ? y0 : 0;
    t.x1 = xin1 ? x1 : W - 1;
    t.y1 = yin1 ? y1 : H - 1;
    t.rx0 = x0;
    t.ry0 = y0;
    t.any = 1;
    return t;
}

// the taps of one (voxel, view) of a lens call: the plain path for a view without distortion (a per-view branch), else through the lens.
// L points at the view's record (LDS or global)
__device__ __forceinline__ Taps lens_taps(const float *__restrict__ P, const float *__restrict__ L, float X0, float X1, float X2, int H, int W)
{
    if (lens_is_plain(L)) return make_taps(P, X0, X1, X2, H, W);
    return make_taps_lens(P, load_lens(L), X0, X1, X2, H, W);
}

}  // namespace mvhmr
