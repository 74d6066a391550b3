// The geometry backward of the cross-view variance aggregates: k_bwd_geom_moments and its instantiations, a translation unit
// of their own beside unproject_geom_bwd.hip (parallel builds), whose launchers hand moments problems (Problem::moments) to
// launch_bwd_geom_moments_kernel and sum the partials with k_geom_reduce / k_pose_reduce as for every other call
#include "geom_bwd_common.h"

namespace mvhmr {

// k_bwd_geom_seen (unproject_visible_geom.hip) with the ds_v of the variance -- a copy, not a template flag: that kernel's instances keep the
// code they had.  With S the participating views of a voxel (every present slot, or -- `visible` -- the present slots that see it), n = |S|,
// mu the rounded mean of the samples over S, g_m / g_v the two halves of grad_out (g_m = 0 when the volume holds the variance alone):
//     ds_v = fmaf(fdiv(2 g_v, n), fsub(s_v, mu), fdiv(g_m, n))   for v in S, 0 outside S
// S is piecewise constant in the geometry, so the gradients are the existing chain rule driven by these ds_v.  Phase 1 marks the slots that
// take part in the record's spare word; a participating view behind the camera or outside the map keeps make_geo_rec's empty taps: its
// sample of zero enters mu, it loads nothing and has dh = 0.  No float atomics: per-block partials, summed in a fixed order by the callers.
template <typename TF, typename TO, int VT, bool POSE>
__global__ void __launch_bounds__(256)
k_bwd_geom_moments(const TO *__restrict__ grad_out, const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords,
                   float *__restrict__ part, float *__restrict__ grad_coords, int C, int C4, int H, int W, long long N, float *__restrict__ pose_part,
                   const int *__restrict__ nvs, int visible, int halves)
{
    constexpr int CPL = geo_cpl(VT);
    constexpr int kPass = kGeoGroup / (64 * CPL);
    extern __shared__ __align__(16) unsigned char smem[];
    GeoRec *recs = reinterpret_cast<GeoRec *>(smem);                                      // [kGeoTile * VT], (voxel, view)
    float2 *acc = reinterpret_cast<float2 *>(smem + sizeof(GeoRec) * kGeoTile * VT);      // (Gx, Gy) per (voxel, view)
    float *xyz = reinterpret_cast<float *>(acc + kGeoTile * VT);                          // [kGeoTile][3] (+ padding to 16 B)
    float *gtile = xyz + kGeoTile * 4;                                                    // g_v [kGeoTile][kGeoLd]; phase 3: dh [kGeoTile * VT][3]
    float *gtile_mu = gtile + kGeoTile * kGeoLd;                                          // g_m, when halves == 2 (not allocated otherwise)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int nvb = nvs ? nvs[b] : VT;
    const long long n0 = (long long)blockIdx.x * kGeoTile;
    const long long mapsz = (long long)H * W * C4;
    const int CO = halves * C, cvar = halves == 2 ? C : 0;

    for (int idx = tid; idx < kGeoTile * VT; idx += blockDim.x) {
        const int j = idx / VT, v = idx - j * VT;
        long long n = n0 + j;
        n = n < N ? n : N - 1;                          // tail voxels are computed and dropped
        float X0, X1, X2;
        voxel_xyz(coords, b, N, n, X0, X1, X2);
        const float *P = proj + ((long long)b * VT + v) * 12;
        GeoRec rec = make_geo_rec(P, X0, X1, X2, H, W, C4);
        const bool takes_part = v < nvb && (!visible || view_sees(P, X0, X1, X2, H, W));
        if (!takes_part) {                              // outside S: the empty record
            rec.o00 = rec.o01 = rec.o10 = rec.o11 = 0;
            rec.w00 = rec.w01 = rec.w10 = rec.w11 = 0.f;
            rec.tx = rec.ty = 0.f;
            rec.mask = 0;
        }
        rec.pad = takes_part ? 1 : 0;
        recs[idx] = rec;
        acc[idx] = make_float2(0.f, 0.f);
        if (v == 0) { xyz[j * 3 + 0] = X0; xyz[j * 3 + 1] = X1; xyz[j * 3 + 2] = X2; }
    }

    const TF *fb = featT + (long long)b * VT * mapsz;
    for (int c0 = 0; c0 < C4; c0 += kGeoGroup) {
        __syncthreads();                                // records ready / the previous group's tiles consumed
        {   // grad_out tiles, coalesced along voxels: the two half-waves load alternate channels
            const int vl = lane & (kGeoTile - 1), half = lane / kGeoTile;
            const long long n = n0 + vl;
            for (int r = wave * 64 + half; r < wave * 64 + 64; r += 64 / kGeoTile) {
                const int c = c0 + r;
                float gv = 0.f, gm = 0.f;
                if (c < C && n < N) {
                    gv = to_f32<TO>(grad_out[((long long)b * CO + cvar + c) * N + n]);
                    if (halves == 2) gm = to_f32<TO>(grad_out[((long long)b * CO + c) * N + n]);
                }
                gtile[vl * kGeoLd + r] = gv;
                if (halves == 2) gtile_mu[vl * kGeoLd + r] = gm;
            }
        }
        __syncthreads();

        for (int jj = 0; jj < kGeoTile / 4; ++jj) {
            const int j = wave * (kGeoTile / 4) + jj;
            if (n0 + j >= N) break;                     // wave-uniform
            float gx[VT], gy[VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) gx[v] = gy[v] = 0.f;
            unsigned bits = 0u;                         // the views that take part for this voxel (wave-uniform)
#pragma unroll
            for (int v = 0; v < VT; ++v) bits |= (unsigned)(uniform(recs[j * VT + v].pad) & 1) << v;
            if (bits == 0u) continue;                   // no view takes part: every gradient of the voxel is zero
            const float cnt = (float)__builtin_popcount(bits);
            for (int ps = 0; ps < kPass; ++ps) {
                const int lc0 = ps * 64 * CPL;
                if (c0 + lc0 >= C4) break;              // wave-uniform: the group's last channels lie past the row
                const int lc = lc0 + lane * CPL, c = c0 + lc;
                const bool act = c < C4;                // C4 % CPL == 0: a lane's channels are all in or all out
                const int cc = act ? c : 0;             // idle lanes read a valid row and contribute nothing
                float gvn[CPL], gmn[CPL];               // 2 g_v / n and g_m / n
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    gvn[i] = __fdiv_rn(__fmul_rn(2.f, gtile[j * kGeoLd + lc + i]), cnt);
                    gmn[i] = halves == 2 ? __fdiv_rn(gtile_mu[j * kGeoLd + lc + i], cnt) : 0.f;
                }
                float s[CPL][VT], dx[CPL][VT], dy[CPL][VT];
#pragma unroll
                for (int v = 0; v < VT; ++v) {
                    const int m = uniform(recs[j * VT + v].mask);
                    if (!(bits >> v & 1u) || !(m & 15)) {   // outside S, or no tap inside the map: no loads, a sample of zero (scalar branch)
#pragma unroll
                        for (int i = 0; i < CPL; ++i) s[i][v] = dx[i][v] = dy[i][v] = 0.f;
                        continue;
                    }
                    const GeoRec u = uniform_geo(recs[j * VT + v]);
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
                    float sum = 0.f;
#pragma unroll
                    for (int v = 0; v < VT; ++v) sum = (bits >> v & 1u) ? __fadd_rn(sum, s[i][v]) : sum;
                    const float mu = __fdiv_rn(sum, cnt);
#pragma unroll
                    for (int v = 0; v < VT; ++v) {
                        const float ds = (bits >> v & 1u) ? __fmaf_rn(gvn[i], __fsub_rn(s[i][v], mu), gmn[i]) : 0.f;
                        gx[v] = act ? fmaf(ds, dx[i][v], gx[v]) : gx[v];
                        gy[v] = act ? fmaf(ds, dy[i][v], gy[v]) : gy[v];
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
    const float kx = __fdiv_rn((float)(W - 1), (float)H), ky = __fdiv_rn((float)(H - 1), (float)W);   // dix/du, diy/dw (Q1)
    for (int idx = tid; idx < kGeoTile * VT; idx += blockDim.x) {
        const int j = idx / VT, v = idx - j * VT;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (n0 + j < N && (recs[idx].mask & 16)) {
            const float *P = proj + ((long long)b * VT + v) * 12;
            const float X0 = xyz[j * 3 + 0], X1 = xyz[j * 3 + 1], X2 = xyz[j * 3 + 2];
            const float a = __fmaf_rn(P[3], 1.f, __fmaf_rn(P[2], X2, __fmaf_rn(P[1], X1, __fmul_rn(P[0], X0))));
            const float bb = __fmaf_rn(P[7], 1.f, __fmaf_rn(P[6], X2, __fmaf_rn(P[5], X1, __fmul_rn(P[4], X0))));
            const float z = __fmaf_rn(P[11], 1.f, __fmaf_rn(P[10], X2, __fmaf_rn(P[9], X1, __fmul_rn(P[8], X0))));
            const float u = __fdiv_rn(a, z), w = __fdiv_rn(bb, z);
            const float2 G = acc[idx];
            const float du = G.x * kx, dw = G.y * ky;
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

template <typename TF, typename TO, bool POSE>
static hipError_t geom_moments_dispatch_v(const TO *go_, const TF *featT, const float *proj, const Coords &coords, float *part, float *grad_coords,
                                          float *pose_part, const Problem &p, hipStream_t s)
{
    // the mean's grad_out tile lies behind the variance's
    const size_t lds = geo_lds_bytes(p.V) + (p.moments == 2 ? sizeof(float) * kGeoTile * kGeoLd : 0);
    const dim3 grid(geom_tiles(p), (unsigned)p.B);
    auto go_mom = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, go_, featT, proj, coords, part, grad_coords, p.C, p.C4, p.H, p.W, p.N, pose_part,
                           p.view_count, p.visible, p.moments);
        return hipGetLastError();
    };
    switch (p.V) {
    case 1: return go_mom(k_bwd_geom_moments<TF, TO, 1, POSE>);
    case 2: return go_mom(k_bwd_geom_moments<TF, TO, 2, POSE>);
    case 3: return go_mom(k_bwd_geom_moments<TF, TO, 3, POSE>);
    case 4: return go_mom(k_bwd_geom_moments<TF, TO, 4, POSE>);
    case 5: return go_mom(k_bwd_geom_moments<TF, TO, 5, POSE>);
    case 6: return go_mom(k_bwd_geom_moments<TF, TO, 6, POSE>);
    case 7: return go_mom(k_bwd_geom_moments<TF, TO, 7, POSE>);
    case 8: return go_mom(k_bwd_geom_moments<TF, TO, 8, POSE>);
    case 9: return go_mom(k_bwd_geom_moments<TF, TO, 9, POSE>);
    case 10: return go_mom(k_bwd_geom_moments<TF, TO, 10, POSE>);
    case 11: return go_mom(k_bwd_geom_moments<TF, TO, 11, POSE>);
    case 12: return go_mom(k_bwd_geom_moments<TF, TO, 12, POSE>);
    case 13: return go_mom(k_bwd_geom_moments<TF, TO, 13, POSE>);
    case 14: return go_mom(k_bwd_geom_moments<TF, TO, 14, POSE>);
    case 15: return go_mom(k_bwd_geom_moments<TF, TO, 15, POSE>);
    case 16: return go_mom(k_bwd_geom_moments<TF, TO, 16, POSE>);
    }
    return hipErrorNotSupported;
}

template <bool POSE>
static hipError_t geom_moments_dispatch(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part, float *grad_coords,
                                        float *pose_part, const Problem &p, hipStream_t s)
{
    if (p.out_bf16)
        return p.feat_f16 ? hipErrorNotSupported
                          : geom_moments_dispatch_v<float, bf16_t, POSE>((const bf16_t *)grad_out, (const float *)featT, proj, coords, part, grad_coords, pose_part, p, s);
    if (!p.feat_f16 && !p.out_f16)
        return geom_moments_dispatch_v<float, float, POSE>((const float *)grad_out, (const float *)featT, proj, coords, part, grad_coords, pose_part, p, s);
    if (p.feat_f16 && p.out_f16)
        return geom_moments_dispatch_v<__half, __half, POSE>((const __half *)grad_out, (const __half *)featT, proj, coords, part, grad_coords, pose_part, p, s);
    if (p.feat_f16 && !p.out_f16)
        return geom_moments_dispatch_v<__half, float, POSE>((const float *)grad_out, (const __half *)featT, proj, coords, part, grad_coords, pose_part, p, s);
    return hipErrorNotSupported;
}

hipError_t launch_bwd_geom_moments_kernel(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part,
                                          float *grad_coords, float *pose_part, bool pose, const Problem &p, hipStream_t s)
{
    if ((p.moments != 1 && p.moments != 2) || p.view_weights || p.confidence || p.lens || p.feature_index) return hipErrorInvalidValue;
    return pose ? geom_moments_dispatch<true>(grad_out, featT, proj, coords, part, grad_coords, pose_part, p, s)
                : geom_moments_dispatch<false>(grad_out, featT, proj, coords, part, grad_coords, pose_part, p, s);
}

}  // namespace mvhmr
