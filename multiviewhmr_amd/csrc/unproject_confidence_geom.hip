// The geometry backward of per-pixel view confidence: k_bwd_geom_conf and its instantiations, a translation unit of their
// own beside unproject_geom_bwd.hip (parallel builds), whose launchers hand confidence problems (Problem::confidence) to
// launch_bwd_geom_conf_kernel and sum the partials with k_geom_reduce / k_pose_reduce as for every other call
#include "geom_bwd_common.h"

namespace mvhmr {

// k_bwd_geom (unproject_geom_bwd.hip) under per-pixel confidence -- a copy of k_bwd_geom_seen / k_bwd_geom_weighted, not a template flag:
// those kernels' instances keep the code they had.  Phase 1 samples the confidence map of (b, v) with the record's own taps and weights (a
// tap outside the map has the value 0): c_v, and the sample's position derivative (dc/dix, dc/diy) from the same four taps.  A view takes
// part for a voxel iff its slot is present (v < nvs[b]; null: all), c_v > 0 and -- `visible` -- it sees the voxel; every other view gets
// the empty record: no loads, dh = 0.  Per channel conf_aggregate_grad gives ds (which carries c_v) and dc; the channel sum of dc leaves as
// the fp32 stream cstream[b, v, n] (null: not asked for; 0 where the view takes no part; channels across the lanes of the voxel's wave and
// over the channel groups in order, the DPP wave sum: the same bits every run), and enters the position gradient as one more term per view,
// (sum_channels dc_v) * grad c_v(ix, iy).  S is piecewise constant, so that is the whole chain rule.
template <typename TF, typename TO, int METHOD, int VT, bool POSE>
__global__ void __launch_bounds__(256)
k_bwd_geom_conf(const TO *__restrict__ grad_out, const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords,
                float *__restrict__ part, float *__restrict__ grad_coords, int C, int C4, int H, int W, long long N, float *__restrict__ pose_part,
                const int *__restrict__ nvs, const float *__restrict__ conf, float *__restrict__ cstream, int visible)
{
    constexpr int CPL = geo_cpl(VT);
    constexpr int kPass = kGeoGroup / (64 * CPL);
    extern __shared__ __align__(16) unsigned char smem[];
    GeoRec *recs = reinterpret_cast<GeoRec *>(smem);                                      // [kGeoTile * VT], (voxel, view)
    float2 *acc = reinterpret_cast<float2 *>(smem + sizeof(GeoRec) * kGeoTile * VT);      // (Gx, Gy) per (voxel, view)
    float *xyz = reinterpret_cast<float *>(acc + kGeoTile * VT);                          // [kGeoTile][3] (+ padding to 16 B)
    float *gtile = xyz + kGeoTile * 4;                                                    // [kGeoTile][kGeoLd]; phase 3: dh [kGeoTile * VT][3]
    float *accw = gtile + kGeoTile * kGeoLd;                                              // sum_channels dc per (voxel, view)
    float *cw = accw + kGeoTile * VT;                                                     // c per (voxel, view)
    float2 *cgrad = reinterpret_cast<float2 *>(cw + kGeoTile * VT);                       // (dc/dix, dc/diy) per (voxel, view)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int nvb = nvs ? nvs[b] : VT;
    const long long n0 = (long long)blockIdx.x * kGeoTile;
    const long long mapsz = (long long)H * W * C4;

    for (int idx = tid; idx < kGeoTile * VT; idx += blockDim.x) {
        const int j = idx / VT, v = idx - j * VT;
        long long n = n0 + j;
        n = n < N ? n : N - 1;                          // tail voxels are computed and dropped
        float X0, X1, X2;
        voxel_xyz(coords, b, N, n, X0, X1, X2);
        const float *P = proj + ((long long)b * VT + v) * 12;
        GeoRec rec = make_geo_rec(P, X0, X1, X2, H, W, C4);
        float c = 0.f, cx = 0.f, cy = 0.f;
        if (v < nvb && (rec.mask & 16) && (!visible || view_sees(P, X0, X1, X2, H, W))) {
            const float *cm = conf + ((long long)b * VT + v) * H * W;
            const float c00 = (rec.mask & 1) ? cm[rec.o00 / C4] : 0.f, c01 = (rec.mask & 2) ? cm[rec.o01 / C4] : 0.f;
            const float c10 = (rec.mask & 4) ? cm[rec.o10 / C4] : 0.f, c11 = (rec.mask & 8) ? cm[rec.o11 / C4] : 0.f;
            c = bilerp(c00, c01, c10, c11, rec.w00, rec.w01, rec.w10, rec.w11);
            const float wx0 = 1.f - rec.tx, wy0 = 1.f - rec.ty;
            cx = fmaf(wy0, c01 - c00, rec.ty * (c11 - c10));
            cy = fmaf(wx0, c10 - c00, rec.tx * (c11 - c01));
        }
        if (!(c > 0.f)) {                               // takes no part (zero, negative, NaN confidence included): the empty record
            rec.o00 = rec.o01 = rec.o10 = rec.o11 = 0;
            rec.w00 = rec.w01 = rec.w10 = rec.w11 = 0.f;
            rec.tx = rec.ty = 0.f;
            rec.mask = 0;
            c = cx = cy = 0.f;
        }
        recs[idx] = rec;
        acc[idx] = make_float2(0.f, 0.f);
        accw[idx] = 0.f;
        cw[idx] = c;
        cgrad[idx] = make_float2(cx, cy);
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
            float gx[VT], gy[VT], gw[VT], cv[VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) gx[v] = gy[v] = gw[v] = 0.f;
            unsigned bits = 0u;                         // the views that take part for this voxel (wave-uniform)
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                bits |= (unsigned)((uniform(recs[j * VT + v].mask) >> 4) & 1) << v;
                cv[v] = uniform(cw[j * VT + v]);
            }
            if (bits == 0u) continue;                   // no view takes part: every gradient of the voxel is zero
            // a lone present view: out == s_v whatever its confidence is, so dc is exactly 0 for mean and softmax (not the rounding of s - out)
            const bool lone = METHOD != AGG_SUM && (bits & (bits - 1u)) == 0u;
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
                    if (!(bits >> v & 1u)) {            // the view takes no part: no loads, no gradient (scalar branch)
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
                    float ds[VT], dc[VT];
                    conf_aggregate_grad<METHOD, VT>(s[i], cv, g[i], ds, dc, bits);
#pragma unroll
                    for (int v = 0; v < VT; ++v) {
                        gw[v] = act && !lone ? gw[v] + dc[v] : gw[v];
                        gx[v] = act ? fmaf(ds[v], dx[i][v], gx[v]) : gx[v];
                        gy[v] = act ? fmaf(ds[v], dy[i][v], gy[v]) : gy[v];
                    }
                }
            }
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                const float sx = wave_sum(gx[v]), sy = wave_sum(gy[v]), sw = wave_sum(gw[v]);
                if (lane == 0) {
                    float2 a = acc[j * VT + v];
                    a.x += sx;
                    a.y += sy;
                    acc[j * VT + v] = a;
                    accw[j * VT + v] += sw;
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
            const float2 G = acc[idx], cg = cgrad[idx];
            const float Gw = accw[idx];
            const float du = fmaf(Gw, cg.x, G.x) * kx, dw = fmaf(Gw, cg.y, G.y) * ky;   // features' term + the confidence sample's own
            d0 = __fdiv_rn(du, z);
            d1 = __fdiv_rn(dw, z);
            d2 = -__fdiv_rn(fmaf(du, u, dw * w), z);
        }
        dh[idx * 3 + 0] = d0;
        dh[idx * 3 + 1] = d1;
        dh[idx * 3 + 2] = d2;
        if (cstream && n0 + j < N) cstream[((long long)b * VT + v) * N + n0 + j] = accw[idx];   // every element written, 0 where absent
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

// the records, (Gx, Gy), xyz and the tile of geo_lds_bytes, then per (voxel, view): sum dc, c and (dc/dix, dc/diy)
static size_t geo_lds_bytes_conf(int V) { return geo_lds_bytes(V) + sizeof(float) * 4 * kGeoTile * V; }

template <typename TF, typename TO, int METHOD, bool POSE>
static hipError_t geom_conf_dispatch_v(const TO *go_, const TF *featT, const float *proj, const Coords &coords, float *part, float *grad_coords,
                                       float *pose_part, float *cstream, const Problem &p, hipStream_t s)
{
    const size_t lds = geo_lds_bytes_conf(p.V);
    const dim3 grid(geom_tiles(p), (unsigned)p.B);
    auto go_conf = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, go_, featT, proj, coords, part, grad_coords, p.C, p.C4, p.H, p.W, p.N, pose_part,
                           p.view_count, p.confidence, cstream, p.visible);
        return hipGetLastError();
    };
    switch (p.V) {
    case 1: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 1, POSE>);
    case 2: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 2, POSE>);
    case 3: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 3, POSE>);
    case 4: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 4, POSE>);
    case 5: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 5, POSE>);
    case 6: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 6, POSE>);
    case 7: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 7, POSE>);
    case 8: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 8, POSE>);
    case 9: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 9, POSE>);
    case 10: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 10, POSE>);
    case 11: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 11, POSE>);
    case 12: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 12, POSE>);
    case 13: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 13, POSE>);
    case 14: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 14, POSE>);
    case 15: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 15, POSE>);
    case 16: return go_conf(k_bwd_geom_conf<TF, TO, METHOD, 16, POSE>);
    }
    return hipErrorNotSupported;
}

template <typename TF, typename TO, bool POSE>
static hipError_t geom_conf_dispatch_m(const TO *go_, const TF *featT, const float *proj, const Coords &coords, float *part, float *grad_coords,
                                       float *pose_part, float *cstream, const Problem &p, hipStream_t s)
{
    switch (p.method) {
    case AGG_SOFTMAX: return geom_conf_dispatch_v<TF, TO, AGG_SOFTMAX, POSE>(go_, featT, proj, coords, part, grad_coords, pose_part, cstream, p, s);
    case AGG_SUM: return geom_conf_dispatch_v<TF, TO, AGG_SUM, POSE>(go_, featT, proj, coords, part, grad_coords, pose_part, cstream, p, s);
    case AGG_MEAN: return geom_conf_dispatch_v<TF, TO, AGG_MEAN, POSE>(go_, featT, proj, coords, part, grad_coords, pose_part, cstream, p, s);
    }
    return hipErrorNotSupported;                // no weighted max (refused before any launch)
}

template <bool POSE>
static hipError_t geom_conf_dispatch(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part, float *grad_coords,
                                     float *pose_part, float *cstream, const Problem &p, hipStream_t s)
{
    if (p.out_bf16)
        return p.feat_f16 ? hipErrorNotSupported
                          : geom_conf_dispatch_m<float, bf16_t, POSE>((const bf16_t *)grad_out, (const float *)featT, proj, coords, part, grad_coords, pose_part, cstream, p, s);
    if (!p.feat_f16 && !p.out_f16)
        return geom_conf_dispatch_m<float, float, POSE>((const float *)grad_out, (const float *)featT, proj, coords, part, grad_coords, pose_part, cstream, p, s);
    if (p.feat_f16 && p.out_f16)
        return geom_conf_dispatch_m<__half, __half, POSE>((const __half *)grad_out, (const __half *)featT, proj, coords, part, grad_coords, pose_part, cstream, p, s);
    if (p.feat_f16 && !p.out_f16)
        return geom_conf_dispatch_m<__half, float, POSE>((const float *)grad_out, (const __half *)featT, proj, coords, part, grad_coords, pose_part, cstream, p, s);
    return hipErrorNotSupported;
}

hipError_t launch_bwd_geom_conf_kernel(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part,
                                       float *grad_coords, float *pose_part, bool pose, const Problem &p, hipStream_t s)
{
    if (!p.confidence || p.view_weights) return hipErrorInvalidValue;
    return pose ? geom_conf_dispatch<true>(grad_out, featT, proj, coords, part, grad_coords, pose_part, p.conf_stream, p, s)
                : geom_conf_dispatch<false>(grad_out, featT, proj, coords, part, grad_coords, pose_part, p.conf_stream, p, s);
}

}  // namespace mvhmr
