// Geometry backward of the lens-distortion-aware un-projection (unproject_geom_bwd.hip describes the kernel and its mapping).
// k_bwd_geom_lens is k_bwd_geom -- a copy, not a template flag: that kernel's instances keep the code they had.  What differs:
//   the V lens records of the block's sample are read once per block into LDS (behind the grad_out tile, in the dynamic region);
//   phase 1 builds the tap record of a view without distortion with make_geo_rec -- the plain call's positions bit for bit -- and of every
//   other view at the DISTORTED position; a ray past the fold-back guard takes no part (mask bit 4 clear, as z <= 0);
//   phase 3 has (d/du', d/dv') where the plain kernel has (d/du, d/dv): it is pulled back through the transposed 2x2 Jacobian of the lens
//   step (lens.h::lens_pull_back) before the unchanged chain through the perspective divide, which uses the PIN-HOLE u and w.
// Phase 2 never sees a position.  The partials are summed by the plain fixed-order reductions (k_geom_reduce, k_pose_reduce):
// launch_bwd_geom[_cuboid] call launch_bwd_geom_lens_kernel for a lens problem.
#include "geom_bwd_common.h"
#include "lens.h"

namespace mvhmr {

namespace {

// make_geo_rec (geom_bwd_common.h) at the distorted position
__device__ __forceinline__ GeoRec make_geo_rec_lens(const float *__restrict__ P, const Lens &l, float X0, float X1, float X2, int H, int W, int C4)
{
    GeoRec r;
    r.o00 = r.o01 = r.o10 = r.o11 = 0;
    r.w00 = r.w01 = r.w10 = r.w11 = 0.f;
    r.tx = r.ty = 0.f;
    r.mask = 0;
    r.pad = 0;
    const float a = __fmaf_rn(P[3], 1.f, __fmaf_rn(P[2], X2, __fmaf_rn(P[1], X1, __fmul_rn(P[0], X0))));
    const float b = __fmaf_rn(P[7], 1.f, __fmaf_rn(P[6], X2, __fmaf_rn(P[5], X1, __fmul_rn(P[4], X0))));
    const float z = __fmaf_rn(P[11], 1.f, __fmaf_rn(P[10], X2, __fmaf_rn(P[9], X1, __fmul_rn(P[8], X0))));
    if (!(z > 0.f)) return r;
    float u, v;
    if (!lens_apply(l, __fdiv_rn(a, z), __fdiv_rn(b, z), u, v)) return r;            // past the fold-back guard: value and gradient 0
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

}  // namespace

template <typename TF, typename TO, int METHOD, int VT, bool POSE>
__global__ void __launch_bounds__(256)
k_bwd_geom_lens(const TO *__restrict__ grad_out, const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords,
                float *__restrict__ part, float *__restrict__ grad_coords, const float *__restrict__ lens, int C, int C4, int H, int W, long long N,
                float *__restrict__ pose_part)
{
    constexpr int CPL = geo_cpl(VT);
    constexpr int kPass = kGeoGroup / (64 * CPL);
    extern __shared__ __align__(16) unsigned char smem[];
    GeoRec *recs = reinterpret_cast<GeoRec *>(smem);                                      // [kGeoTile * VT], (voxel, view)
    float2 *acc = reinterpret_cast<float2 *>(smem + sizeof(GeoRec) * kGeoTile * VT);      // (Gx, Gy) per (voxel, view)
    float *xyz = reinterpret_cast<float *>(acc + kGeoTile * VT);                          // [kGeoTile][3] (+ padding to 16 B)
    float *gtile = xyz + kGeoTile * 4;                                                    // [kGeoTile][kGeoLd]; phase 3: dh [kGeoTile * VT][3]
    float *lens_s = gtile + kGeoTile * kGeoLd;                                            // [VT][kLensWords], behind the tile: the dynamic region keeps its 16-byte base
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const long long n0 = (long long)blockIdx.x * kGeoTile;
    const long long mapsz = (long long)H * W * C4;

    for (int i = tid; i < VT * kLensWords; i += blockDim.x) lens_s[i] = lens[(long long)b * VT * kLensWords + i];   // once per block and view
    __syncthreads();

    for (int idx = tid; idx < kGeoTile * VT; idx += blockDim.x) {
        const int j = idx / VT, v = idx - j * VT;
        long long n = n0 + j;
        n = n < N ? n : N - 1;                          // tail voxels are computed and dropped
        float X0, X1, X2;
        voxel_xyz(coords, b, N, n, X0, X1, X2);
        const float *P = proj + ((long long)b * VT + v) * 12, *L = lens_s + v * kLensWords;
        recs[idx] = lens_is_plain(L) ? make_geo_rec(P, X0, X1, X2, H, W, C4) : make_geo_rec_lens(P, load_lens(L), X0, X1, X2, H, W, C4);
        acc[idx] = make_float2(0.f, 0.f);
        if (v == 0) { xyz[j * 3 + 0] = X0; xyz[j * 3 + 1] = X1; xyz[j * 3 + 2] = X2; }
    }

    const TF *fb = featT + (long long)b * VT * mapsz;
    for (int c0 = 0; c0 < C4; c0 += kGeoGroup) {
        __syncthreads();                                // records ready / the previous group's tile consumed
        {   // grad_out tile, coalesced along voxels: the two half-waves load alternate channels
            const int vl = lane & (kGeoTile - 1), half = lane / kGeoTile;
            const long long n = n0 + vl;
            for (int r = wave * 64 + half; r < wave * 64 + 64; r += 64 / kGeoTile) {
                const int c = c0 + r;
                float g = 0.f;
                if (c < C && n < N) g = to_f32<TO>(grad_out[((long long)b * C + c) * N + n]);
                gtile[vl * kGeoLd + r] = g;
            }
        }
        __syncthreads();

        for (int jj = 0; jj < kGeoTile / 4; ++jj) {
            const int j = wave * (kGeoTile / 4) + jj;
            if (n0 + j >= N) break;                     // wave-uniform
            float gx[VT], gy[VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) gx[v] = gy[v] = 0.f;
            for (int ps = 0; ps < kPass; ++ps) {
                const int lc0 = ps * 64 * CPL;
                if (c0 + lc0 >= C4) break;              // wave-uniform: the group's last channels lie past the row
                const int lc = lc0 + lane * CPL, c = c0 + lc;
                const bool act = c < C4;                // C4 % CPL == 0: a lane's channels are all in or all out
                const int cc = act ? c : 0;             // idle lanes read a valid row and contribute nothing
                float g[CPL];
#pragma unroll
                for (int i = 0; i < CPL; ++i) g[i] = gtile[j * kGeoLd + lc + i];
                float s[CPL][VT], dx[CPL][VT], dy[CPL][VT];
#pragma unroll
                for (int v = 0; v < VT; ++v) {
                    const GeoRec u = uniform_geo(recs[j * VT + v]);
                    if (!(u.mask & 16)) {               // the view takes no part: s = 0 and no gradient (wave-uniform)
#pragma unroll
                        for (int i = 0; i < CPL; ++i) s[i][v] = dx[i][v] = dy[i][v] = 0.f;
                        continue;
                    }
                    const TF *fv = fb + v * mapsz + cc;
                    float f00[CPL], f01[CPL], f10[CPL], f11[CPL];
                    Row<TF, CPL>::load(fv + u.o00, f00);
                    Row<TF, CPL>::load(fv + u.o01, f01);
                    Row<TF, CPL>::load(fv + u.o10, f10);
                    Row<TF, CPL>::load(fv + u.o11, f11);
                    const float wx0 = 1.f - u.tx, wy0 = 1.f - u.ty;   // exact: the fractions lie in [0, 1)
#pragma unroll
                    for (int i = 0; i < CPL; ++i) {
                        // a tap outside the map has the value 0 (zero padding), not just the weight 0
                        const float a00 = (u.mask & 1) ? f00[i] : 0.f, a01 = (u.mask & 2) ? f01[i] : 0.f;
                        const float a10 = (u.mask & 4) ? f10[i] : 0.f, a11 = (u.mask & 8) ? f11[i] : 0.f;
                        s[i][v] = bilerp(a00, a01, a10, a11, u.w00, u.w01, u.w10, u.w11);
                        dx[i][v] = fmaf(wy0, a01 - a00, u.ty * (a11 - a10));
                        dy[i][v] = fmaf(wx0, a10 - a00, u.tx * (a11 - a01));
                    }
                }
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    float ds[VT];
                    aggregate_grad<METHOD, VT>(s[i], g[i], ds);
#pragma unroll
                    for (int v = 0; v < VT; ++v) {
                        gx[v] = act ? fmaf(ds[v], dx[i][v], gx[v]) : gx[v];
                        gy[v] = act ? fmaf(ds[v], dy[i][v], gy[v]) : gy[v];
                    }
                }
            }
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                const float sx = wave_sum(gx[v]), sy = wave_sum(gy[v]);
                if (lane == 0) {
                    float2 a = acc[j * VT + v];
                    a.x += sx;
                    a.y += sy;
                    acc[j * VT + v] = a;
                }
            }
        }
    }
    __syncthreads();

    // phase 3: dh per (voxel, view); the grad_out tile is dead, its space holds dh
    float *dh = gtile;
    const float kx = __fdiv_rn((float)(W - 1), (float)H), ky = __fdiv_rn((float)(H - 1), (float)W);   // dix/du', diy/dw' (Q1)
    for (int idx = tid; idx < kGeoTile * VT; idx += blockDim.x) {
        const int j = idx / VT, v = idx - j * VT;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (n0 + j < N && (recs[idx].mask & 16)) {
            const float *P = proj + ((long long)b * VT + v) * 12, *L = lens_s + v * kLensWords;
            const float X0 = xyz[j * 3 + 0], X1 = xyz[j * 3 + 1], X2 = xyz[j * 3 + 2];
            const float a = __fmaf_rn(P[3], 1.f, __fmaf_rn(P[2], X2, __fmaf_rn(P[1], X1, __fmul_rn(P[0], X0))));
            const float bb = __fmaf_rn(P[7], 1.f, __fmaf_rn(P[6], X2, __fmaf_rn(P[5], X1, __fmul_rn(P[4], X0))));
            const float z = __fmaf_rn(P[11], 1.f, __fmaf_rn(P[10], X2, __fmaf_rn(P[9], X1, __fmul_rn(P[8], X0))));
            const float u = __fdiv_rn(a, z), w = __fdiv_rn(bb, z);
            const float2 G = acc[idx];
            float du = G.x * kx, dw = G.y * ky;
            if (!lens_is_plain(L)) lens_pull_back(load_lens(L), u, w, du, dw);      // (d/du', d/dw') -> (d/du, d/dw)
            d0 = __fdiv_rn(du, z);
            d1 = __fdiv_rn(dw, z);
            d2 = -__fdiv_rn(fmaf(du, u, dw * w), z);
        }
        dh[idx * 3 + 0] = d0;
        dh[idx * 3 + 1] = d1;
        dh[idx * 3 + 2] = d2;
    }
    __syncthreads();
    if (!POSE && grad_coords && tid < kGeoTile && n0 + tid < N) {
        // grad_coords[b, n] = sum_v P_v[:, :3]^T dh_v, views in order; one plain store per coordinate
        const int j = tid;
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            const float *P = proj + ((long long)b * VT + v) * 12;
            const float e0 = dh[(j * VT + v) * 3 + 0], e1 = dh[(j * VT + v) * 3 + 1], e2 = dh[(j * VT + v) * 3 + 2];
            g0 = fmaf(P[8], e2, fmaf(P[4], e1, fmaf(P[0], e0, g0)));
            g1 = fmaf(P[9], e2, fmaf(P[5], e1, fmaf(P[1], e0, g1)));
            g2 = fmaf(P[10], e2, fmaf(P[6], e1, fmaf(P[2], e0, g2)));
        }
        float *o = grad_coords + ((long long)b * N + n0 + j) * 3;
        o[0] = g0; o[1] = g1; o[2] = g2;
    }
    if (part && tid < VT * 12) {
        // this block's share of grad_proj[b, v][r][k] = sum_n dh_v[r] (X, 1)[k], voxels in order (tail voxels have dh = 0)
        const int v = tid / 12, r = (tid % 12) / 4, k = tid % 4;
        float sum = 0.f;
        for (int j = 0; j < kGeoTile; ++j) {
            const float d = dh[(j * VT + v) * 3 + r];
            sum = d != 0.f ? fmaf(d, k < 3 ? xyz[j * 3 + k] : 1.f, sum) : sum;
        }
        part[(((long long)b * gridDim.x + blockIdx.x) * VT + v) * 12 + tid % 12] = sum;
    }
    if constexpr (POSE) {
        // epilogue of the cuboid route: gX and d per voxel (0 for tail voxels) behind dh, then this block's 12 pose partials
        float *gxd = dh + kGeoTile * VT * 3;            // [kGeoTile][6]: gX, d
        if (tid < kGeoTile) {
            const int j = tid;
            float g0 = 0.f, g1 = 0.f, g2 = 0.f, e0 = 0.f, e1 = 0.f, e2 = 0.f;
            if (n0 + j < N) {
#pragma unroll 1
                for (int v = 0; v < VT; ++v) {                  // (not unrolled: keeps the 16-view instances at the tensor route's registers)
                    const float *P = proj + ((long long)b * VT + v) * 12;
                    const float h0 = dh[(j * VT + v) * 3 + 0], h1 = dh[(j * VT + v) * 3 + 1], h2 = dh[(j * VT + v) * 3 + 2];
                    g0 = fmaf(P[8], h2, fmaf(P[4], h1, fmaf(P[0], h0, g0)));
                    g1 = fmaf(P[9], h2, fmaf(P[5], h1, fmaf(P[1], h0, g1)));
                    g2 = fmaf(P[10], h2, fmaf(P[6], h1, fmaf(P[2], h0, g2)));
                }
                cuboid_offset(coords, b, n0 + j, e0, e1, e2);
            }
            gxd[j * 6 + 0] = g0; gxd[j * 6 + 1] = g1; gxd[j * 6 + 2] = g2;
            gxd[j * 6 + 3] = e0; gxd[j * 6 + 4] = e1; gxd[j * 6 + 5] = e2;
        }
        __syncthreads();
        if (tid >= 256 - 12) {                          // threads the grad_proj partials leave idle (VT * 12 <= 192)
            const int t = tid - (256 - 12), r = t < 9 ? t / 3 : t - 9, k = t % 3;
            float sum = 0.f;
            for (int j = 0; j < kGeoTile; ++j) sum = t < 9 ? fmaf(gxd[j * 6 + r], gxd[j * 6 + 3 + k], sum) : sum + gxd[j * 6 + r];
            pose_part[((long long)b * gridDim.x + blockIdx.x) * 12 + t] = sum;
        }
    }
}

// ------------------------------------------------------------------------------------------ launchers
template <typename TF, typename TO, int METHOD, bool POSE>
static hipError_t geom_lens_dispatch_v(const TO *go_, const TF *featT, const float *proj, const Coords &coords, float *part, float *grad_coords,
                                       float *pose_part, const Problem &p, hipStream_t s)
{
    const size_t lds = geo_lds_bytes(p.V) + sizeof(float) * kLensWords * (size_t)p.V;
    const dim3 grid(geom_tiles(p), (unsigned)p.B);
    auto go = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, go_, featT, proj, coords, part, grad_coords, p.lens, p.C, p.C4, p.H, p.W, p.N, pose_part);
        return hipGetLastError();
    };
    switch (p.V) {
    case 1: return go(k_bwd_geom_lens<TF, TO, METHOD, 1, POSE>);
    case 2: return go(k_bwd_geom_lens<TF, TO, METHOD, 2, POSE>);
    case 3: return go(k_bwd_geom_lens<TF, TO, METHOD, 3, POSE>);
    case 4: return go(k_bwd_geom_lens<TF, TO, METHOD, 4, POSE>);
    case 5: return go(k_bwd_geom_lens<TF, TO, METHOD, 5, POSE>);
    case 6: return go(k_bwd_geom_lens<TF, TO, METHOD, 6, POSE>);
    case 7: return go(k_bwd_geom_lens<TF, TO, METHOD, 7, POSE>);
    case 8: return go(k_bwd_geom_lens<TF, TO, METHOD, 8, POSE>);
    case 9: return go(k_bwd_geom_lens<TF, TO, METHOD, 9, POSE>);
    case 10: return go(k_bwd_geom_lens<TF, TO, METHOD, 10, POSE>);
    case 11: return go(k_bwd_geom_lens<TF, TO, METHOD, 11, POSE>);
    case 12: return go(k_bwd_geom_lens<TF, TO, METHOD, 12, POSE>);
    case 13: return go(k_bwd_geom_lens<TF, TO, METHOD, 13, POSE>);
    case 14: return go(k_bwd_geom_lens<TF, TO, METHOD, 14, POSE>);
    case 15: return go(k_bwd_geom_lens<TF, TO, METHOD, 15, POSE>);
    case 16: return go(k_bwd_geom_lens<TF, TO, METHOD, 16, POSE>);
    }
    return hipErrorNotSupported;
}

template <typename TF, typename TO, bool POSE>
static hipError_t geom_lens_dispatch_m(const TO *go_, const TF *featT, const float *proj, const Coords &coords, float *part, float *grad_coords,
                                       float *pose_part, const Problem &p, hipStream_t s)
{
    switch (p.method) {
    case AGG_SOFTMAX: return geom_lens_dispatch_v<TF, TO, AGG_SOFTMAX, POSE>(go_, featT, proj, coords, part, grad_coords, pose_part, p, s);
    case AGG_SUM: return geom_lens_dispatch_v<TF, TO, AGG_SUM, POSE>(go_, featT, proj, coords, part, grad_coords, pose_part, p, s);
    case AGG_MEAN: return geom_lens_dispatch_v<TF, TO, AGG_MEAN, POSE>(go_, featT, proj, coords, part, grad_coords, pose_part, p, s);
    case AGG_MAX: return geom_lens_dispatch_v<TF, TO, AGG_MAX, POSE>(go_, featT, proj, coords, part, grad_coords, pose_part, p, s);
    }
    return hipErrorInvalidValue;
}

template <bool POSE>
static hipError_t geom_lens_dispatch(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part, float *grad_coords,
                                     float *pose_part, const Problem &p, hipStream_t s)
{
    if (p.out_bf16)
        return p.feat_f16 ? hipErrorNotSupported
                          : geom_lens_dispatch_m<float, bf16_t, POSE>((const bf16_t *)grad_out, (const float *)featT, proj, coords, part, grad_coords, pose_part, p, s);
    if (!p.feat_f16 && !p.out_f16)
        return geom_lens_dispatch_m<float, float, POSE>((const float *)grad_out, (const float *)featT, proj, coords, part, grad_coords, pose_part, p, s);
    if (p.feat_f16 && p.out_f16)
        return geom_lens_dispatch_m<__half, __half, POSE>((const __half *)grad_out, (const __half *)featT, proj, coords, part, grad_coords, pose_part, p, s);
    if (p.feat_f16 && !p.out_f16)
        return geom_lens_dispatch_m<__half, float, POSE>((const float *)grad_out, (const __half *)featT, proj, coords, part, grad_coords, pose_part, p, s);
    return hipErrorNotSupported;
}

hipError_t launch_bwd_geom_lens_kernel(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part,
                                       float *grad_coords, float *pose_part, bool pose, const Problem &p, hipStream_t s)
{
    if (!p.lens || p.view_count || p.view_weights || p.visible || p.confidence || p.feature_index) return hipErrorInvalidValue;
    return pose ? geom_lens_dispatch<true>(grad_out, featT, proj, coords, part, grad_coords, pose_part, p, s)
                : geom_lens_dispatch<false>(grad_out, featT, proj, coords, part, grad_coords, pose_part, p, s);
}

}  // namespace mvhmr
