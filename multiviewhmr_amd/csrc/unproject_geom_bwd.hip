// Gradient of the un-projection w.r.t. the GEOMETRY: proj_matricies and coord_volumes (models/aggregation.py:20-87 differentiates
// with respect to all three of its tensors; mvhmr_unproject_backward covers the features).
//
// Per sample b, voxel n at X, view v:  h = P_v [X, 1] = (a, b, z), u = a / z, w = b / z, and with quirk Q1 and align_corners=True
//     ix = u (Wf - 1) / Hf,   iy = w (Hf - 1) / Wf          (computed in the forward's fp32 rounding order, device_common.h)
// The bilinear sample s = sum of the four taps at floor(ix), floor(iy); a tap outside the map has the VALUE 0 (zero padding), so
//     ds/dix = (1 - ty)(f01 - f00) + ty (f11 - f10),   ds/diy = (1 - tx)(f10 - f00) + tx (f11 - f01)
// with tx, ty the fractions -- the taps grid_sampler_2d_backward uses, also on the boundary ix == -1 / iy == -1, where the forward
// (make_taps) has no taps at all but the grid gradient is not zero: this file builds its own tap record.  With
// ds_vc = aggregate_grad (device_common.h) and G_v = sum_c ds_vc ds_vc/dix (Gx) resp. /diy (Gy):
//     dL/du = Gx (Wf - 1) / Hf,   dL/dw = Gy (Hf - 1) / Wf,   dh_v = (dL/du / z, dL/dw / z, -(dL/du u + dL/dw w) / z)
//     grad_coords[b, n] = sum_v P_v[:, :3]^T dh_v            grad_proj[b, v] = sum_n dh_v (X0, X1, X2, 1)^T
// A view with z <= 0 (or NaN) takes no part (the reference masks the sample): all its geometric gradients are 0.
//
// Mapping (the gather family's, unproject_gather.hip):
//   block   = 32 consecutive voxels of one sample x EVERY channel (256 threads, 4 waves): the sum over C ends on chip
//   phase 1 = one thread per (voxel, view): project, tap record -> LDS
//   phase 2 = per 256-channel group: the grad_out tile turned through LDS (loads along voxels); one wave per voxel, channels across
//             lanes, channels-last feature rows read as wave-uniform coalesced rows; all V views' s, ds/dix, ds/diy are held in
//             registers until aggregate_grad gives ds -- 3 V values per channel, so a lane takes 4 / 2 / 1 channels for V <= 4 / <= 8
//             / <= 16; then one DPP reduction of Gx and Gy per (voxel, view) into LDS (each voxel belongs to one wave: no atomics)
//   phase 3 = one thread per (voxel, view): dh_v; grad_coords written once per voxel by plain stores; 12 fp32 partials of grad_proj
//             per (block, view) into the workspace, summed per (b, v) by k_geom_reduce in float64 in a fixed order.
// No float atomics anywhere: both outputs are bitwise reproducible from run to run.
//
// Cuboid route (POSE instances): the voxel centre is X = R d + c with d = fl(g - c), g = position + step (i,j,k) (voxel_xyz).  With
// gX_n = sum_v P_v[:, :3]^T dh_v (what grad_coords would hold)
//     grad_rot[b][r][k] = sum_n gX_n[r] d_n[k]          grad_center[b] = sum_n gX_n - R^T sum_n gX_n     (dX/dc = I - R)
// phase 3 gains an epilogue: gX and d (recomputed from (i,j,k) in voxel_xyz's rounding) per voxel into LDS, then 12 fp32 partials per
// block (9 of sum gX (x) d, 3 of sum gX), voxels in order; k_pose_reduce sums them per sample in float64 in a fixed order and applies
// R^T in float64 (R = I gives grad_center == 0 exactly).  grad_coords is not written on this route.
#include "geom_bwd_common.h"

namespace mvhmr {

// MASK: nvs[b] present views packed into the first slots (k_fwd_gather); the absent ones take no part and have dh = 0
template <typename TF, typename TO, int METHOD, int VT, bool POSE, bool MASK = false>
__global__ void __launch_bounds__(256)
k_bwd_geom(const TO *__restrict__ grad_out, const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords,
           float *__restrict__ part, float *__restrict__ grad_coords, int C, int C4, int H, int W, long long N, float *__restrict__ pose_part,
           const int *__restrict__ nvs = nullptr)
{
    constexpr int CPL = geo_cpl(VT);
    constexpr int kPass = kGeoGroup / (64 * CPL);
    extern __shared__ __align__(16) unsigned char smem[];
    GeoRec *recs = reinterpret_cast<GeoRec *>(smem);                                      // [kGeoTile * VT], (voxel, view)
    float2 *acc = reinterpret_cast<float2 *>(smem + sizeof(GeoRec) * kGeoTile * VT);      // (Gx, Gy) per (voxel, view)
    float *xyz = reinterpret_cast<float *>(acc + kGeoTile * VT);                          // [kGeoTile][3] (+ padding to 16 B)
    float *gtile = xyz + kGeoTile * 4;                                                    // [kGeoTile][kGeoLd]; phase 3: dh [kGeoTile * VT][3]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int nvb = MASK ? nvs[b] : VT;
    const long long n0 = (long long)blockIdx.x * kGeoTile;
    const long long mapsz = (long long)H * W * C4;

    for (int idx = tid; idx < kGeoTile * VT; idx += blockDim.x) {
        const int j = idx / VT, v = idx - j * VT;
        long long n = n0 + j;
        n = n < N ? n : N - 1;                          // tail voxels are computed and dropped
        float X0, X1, X2;
        voxel_xyz(coords, b, N, n, X0, X1, X2);
        recs[idx] = make_geo_rec(proj + ((long long)b * VT + v) * 12, X0, X1, X2, H, W, C4);
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
                    if ((MASK && v >= nvb) || !(u.mask & 16)) {   // the view takes no part: s = 0 and no gradient (wave-uniform)
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
                    if constexpr (MASK) masked_aggregate_grad<METHOD, VT>(s[i], g[i], ds, nvb > 0 ? nvb : 1);   // (none present: dx = dy = 0)
                    else aggregate_grad<METHOD, VT>(s[i], g[i], ds);
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
    const float kx = __fdiv_rn((float)(W - 1), (float)H), ky = __fdiv_rn((float)(H - 1), (float)W);   // dix/du, diy/dw (Q1)
    for (int idx = tid; idx < kGeoTile * VT; idx += blockDim.x) {
        const int j = idx / VT, v = idx - j * VT;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (n0 + j < N && (recs[idx].mask & 16) && (!MASK || v < nvb)) {
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

// grad_weights[b, slot] = sum over the blocks of sample b of their partial: float64, a fixed stride of blocks per thread, then a fixed tree
__global__ void __launch_bounds__(256) k_weight_reduce(const float *__restrict__ wpart, float *__restrict__ grad_w, int V, int tiles)
{
    __shared__ double red[256];
    const int tid = threadIdx.x, bv = blockIdx.x, b = bv / V, v = bv - b * V;
    double s = 0.0;
    for (int t = tid; t < tiles; t += 256) s += (double)wpart[((long long)b * tiles + t) * V + v];
    red[tid] = s;
    for (int w = 128; w > 0; w >>= 1) {
        __syncthreads();
        if (tid < w) red[tid] += red[tid + w];
    }
    if (tid == 0) grad_w[bv] = (float)red[0];
}

// grad_proj[b, v] = sum over the blocks of sample b of their 12 partials: float64, each thread a fixed stride of blocks, then a fixed
// tree over the threads -- the same bits every run
__global__ void __launch_bounds__(256) k_geom_reduce(const float *__restrict__ part, float *__restrict__ grad_proj, int V, int tiles)
{
    __shared__ double red[12][256];
    const int tid = threadIdx.x, bv = blockIdx.x, b = bv / V, v = bv - b * V;
    double s[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = 0.0;
    for (int t = tid; t < tiles; t += 256) {
        const float *p = part + (((long long)b * tiles + t) * V + v) * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) s[k] += (double)p[k];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) red[k][tid] = s[k];
    for (int w = 128; w > 0; w >>= 1) {
        __syncthreads();
        if (tid < w) {
#pragma unroll
            for (int k = 0; k < 12; ++k) red[k][tid] += red[k][tid + w];
        }
    }
    __syncthreads();
    if (tid < 12) grad_proj[(long long)bv * 12 + tid] = (float)red[tid][0];
}

// grad_rot[b] = S_gd, grad_center[b] = S_g - R^T S_g from the pose partials of sample b (sum over blocks as k_geom_reduce: float64,
// fixed order); either output may be null
__global__ void __launch_bounds__(256) k_pose_reduce(const float *__restrict__ pose_part, const float *__restrict__ rot, float *__restrict__ grad_rot,
                                                     float *__restrict__ grad_center, int tiles)
{
    __shared__ double red[12][256];
    const int tid = threadIdx.x, b = blockIdx.x;
    double s[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = 0.0;
    for (int t = tid; t < tiles; t += 256) {
        const float *p = pose_part + ((long long)b * tiles + t) * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) s[k] += (double)p[k];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) red[k][tid] = s[k];
    for (int w = 128; w > 0; w >>= 1) {
        __syncthreads();
        if (tid < w) {
#pragma unroll
            for (int k = 0; k < 12; ++k) red[k][tid] += red[k][tid + w];
        }
    }
    __syncthreads();
    if (grad_rot && tid < 9) grad_rot[(long long)b * 9 + tid] = (float)red[tid][0];
    if (grad_center && tid < 3) {
        const float *R = rot + (long long)b * 9;
        const double rt = (double)R[tid] * red[9][0] + (double)R[3 + tid] * red[10][0] + (double)R[6 + tid] * red[11][0];   // (R^T S_g)[tid]
        grad_center[(long long)b * 3 + tid] = (float)(red[9 + tid][0] - rt);
    }
}

// ------------------------------------------------------------------------------------------ launchers
size_t geom_partial_bytes(const Problem &p) { return (size_t)p.B * geom_tiles(p) * p.V * 12 * sizeof(float); }
size_t pose_partial_bytes(const Problem &p) { return (size_t)p.B * geom_tiles(p) * 12 * sizeof(float); }
size_t geom_weight_partial_bytes(const Problem &p) { return (size_t)p.B * geom_tiles(p) * p.V * sizeof(float); }

template <typename TF, typename TO, int METHOD, bool POSE>
static hipError_t geom_dispatch_v(const TO *go_, const TF *featT, const float *proj, const Coords &coords, float *part, float *grad_coords,
                                  float *pose_part, const Problem &p, hipStream_t s)
{
    const size_t lds = geo_lds_bytes(p.V);
    const dim3 grid(geom_tiles(p), (unsigned)p.B);
    auto go = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, go_, featT, proj, coords, part, grad_coords, p.C, p.C4, p.H, p.W, p.N, pose_part,
                           p.view_count);
        return hipGetLastError();
    };
    if (p.view_count) {
        switch (p.V) {
        case 1: return go(k_bwd_geom<TF, TO, METHOD, 1, POSE, true>);
        case 2: return go(k_bwd_geom<TF, TO, METHOD, 2, POSE, true>);
        case 3: return go(k_bwd_geom<TF, TO, METHOD, 3, POSE, true>);
        case 4: return go(k_bwd_geom<TF, TO, METHOD, 4, POSE, true>);
        case 5: return go(k_bwd_geom<TF, TO, METHOD, 5, POSE, true>);
        case 6: return go(k_bwd_geom<TF, TO, METHOD, 6, POSE, true>);
        case 7: return go(k_bwd_geom<TF, TO, METHOD, 7, POSE, true>);
        case 8: return go(k_bwd_geom<TF, TO, METHOD, 8, POSE, true>);
        case 9: return go(k_bwd_geom<TF, TO, METHOD, 9, POSE, true>);
        case 10: return go(k_bwd_geom<TF, TO, METHOD, 10, POSE, true>);
        case 11: return go(k_bwd_geom<TF, TO, METHOD, 11, POSE, true>);
        case 12: return go(k_bwd_geom<TF, TO, METHOD, 12, POSE, true>);
        case 13: return go(k_bwd_geom<TF, TO, METHOD, 13, POSE, true>);
        case 14: return go(k_bwd_geom<TF, TO, METHOD, 14, POSE, true>);
        case 15: return go(k_bwd_geom<TF, TO, METHOD, 15, POSE, true>);
        case 16: return go(k_bwd_geom<TF, TO, METHOD, 16, POSE, true>);
        }
        return hipErrorNotSupported;
    }
    switch (p.V) {
    case 1: return go(k_bwd_geom<TF, TO, METHOD, 1, POSE>);
    case 2: return go(k_bwd_geom<TF, TO, METHOD, 2, POSE>);
    case 3: return go(k_bwd_geom<TF, TO, METHOD, 3, POSE>);
    case 4: return go(k_bwd_geom<TF, TO, METHOD, 4, POSE>);
    case 5: return go(k_bwd_geom<TF, TO, METHOD, 5, POSE>);
    case 6: return go(k_bwd_geom<TF, TO, METHOD, 6, POSE>);
    case 7: return go(k_bwd_geom<TF, TO, METHOD, 7, POSE>);
    case 8: return go(k_bwd_geom<TF, TO, METHOD, 8, POSE>);
    case 9: return go(k_bwd_geom<TF, TO, METHOD, 9, POSE>);
    case 10: return go(k_bwd_geom<TF, TO, METHOD, 10, POSE>);
    case 11: return go(k_bwd_geom<TF, TO, METHOD, 11, POSE>);
    case 12: return go(k_bwd_geom<TF, TO, METHOD, 12, POSE>);
    case 13: return go(k_bwd_geom<TF, TO, METHOD, 13, POSE>);
    case 14: return go(k_bwd_geom<TF, TO, METHOD, 14, POSE>);
    case 15: return go(k_bwd_geom<TF, TO, METHOD, 15, POSE>);
    case 16: return go(k_bwd_geom<TF, TO, METHOD, 16, POSE>);
    }
    return hipErrorNotSupported;
}

template <typename TF, typename TO, bool POSE>
static hipError_t geom_dispatch_m(const TO *go_, const TF *featT, const float *proj, const Coords &coords, float *part, float *grad_coords,
                                  float *pose_part, const Problem &p, hipStream_t s)
{
    switch (p.method) {
    case AGG_SOFTMAX: return geom_dispatch_v<TF, TO, AGG_SOFTMAX, POSE>(go_, featT, proj, coords, part, grad_coords, pose_part, p, s);
    case AGG_SUM: return geom_dispatch_v<TF, TO, AGG_SUM, POSE>(go_, featT, proj, coords, part, grad_coords, pose_part, p, s);
    case AGG_MEAN: return geom_dispatch_v<TF, TO, AGG_MEAN, POSE>(go_, featT, proj, coords, part, grad_coords, pose_part, p, s);
    case AGG_MAX: return geom_dispatch_v<TF, TO, AGG_MAX, POSE>(go_, featT, proj, coords, part, grad_coords, pose_part, p, s);
    }
    return hipErrorInvalidValue;
}

template <bool POSE>
static hipError_t geom_dispatch(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part, float *grad_coords,
                                float *pose_part, float *wpart, const Problem &p, hipStream_t s)
{
    if (p.moments) return launch_bwd_geom_moments_kernel(grad_out, featT, proj, coords, part, grad_coords, pose_part, POSE, p, s);   // cross-view variance: unproject_moments_geom.hip
    if (p.view_weights) return launch_bwd_geom_weighted_kernel(grad_out, featT, proj, coords, part, grad_coords, pose_part, wpart, POSE, p, s);
    if (p.confidence) return launch_bwd_geom_conf_kernel(grad_out, featT, proj, coords, part, grad_coords, pose_part, POSE, p, s);
    if (p.visible) return launch_bwd_geom_seen_kernel(grad_out, featT, proj, coords, part, grad_coords, pose_part, POSE, p, s);
    if (p.lens) return launch_bwd_geom_lens_kernel(grad_out, featT, proj, coords, part, grad_coords, pose_part, POSE, p, s);     // lens distortion: unproject_lens_geom.hip
    if (p.out_bf16)
        return p.feat_f16 ? hipErrorNotSupported
                          : geom_dispatch_m<float, bf16_t, POSE>((const bf16_t *)grad_out, (const float *)featT, proj, coords, part, grad_coords, pose_part, p, s);
    if (!p.feat_f16 && !p.out_f16)
        return geom_dispatch_m<float, float, POSE>((const float *)grad_out, (const float *)featT, proj, coords, part, grad_coords, pose_part, p, s);
    if (p.feat_f16 && p.out_f16)
        return geom_dispatch_m<__half, __half, POSE>((const __half *)grad_out, (const __half *)featT, proj, coords, part, grad_coords, pose_part, p, s);
    if (p.feat_f16 && !p.out_f16)
        return geom_dispatch_m<__half, float, POSE>((const float *)grad_out, (const __half *)featT, proj, coords, part, grad_coords, pose_part, p, s);
    return hipErrorNotSupported;
}

// grad_weights (packed, slot order) from wpart, when asked for
static hipError_t reduce_weights(float *wpart, float *grad_weights, const Problem &p, hipStream_t s)
{
    if (!grad_weights) return hipSuccess;
    hipLaunchKernelGGL(k_weight_reduce, dim3((unsigned)(p.B * p.V)), dim3(256), 0, s, (const float *)wpart, grad_weights, p.V, (int)geom_tiles(p));
    return hipGetLastError();
}

hipError_t launch_bwd_geom(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part, float *grad_proj,
                           float *grad_coords, const Problem &p, hipStream_t s, float *wpart, float *grad_weights)
{
    if (p.V < 1 || p.V > kMaxViews || (grad_proj && !part) || (grad_weights && (!wpart || !p.view_weights))) return hipErrorInvalidValue;
    hipError_t e = geom_dispatch<false>(grad_out, featT, proj, coords, grad_proj ? part : nullptr, grad_coords, nullptr, grad_weights ? wpart : nullptr, p, s);
    if (e != hipSuccess) return e;
    if (grad_proj) {
        hipLaunchKernelGGL(k_geom_reduce, dim3((unsigned)(p.B * p.V)), dim3(256), 0, s, (const float *)part, grad_proj, p.V, (int)geom_tiles(p));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return reduce_weights(wpart, grad_weights, p, s);
}

hipError_t launch_bwd_geom_cuboid(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *part, float *grad_proj,
                                  float *pose_part, float *grad_rot, float *grad_center, const Problem &p, hipStream_t s, float *wpart,
                                  float *grad_weights)
{
    const bool pose = grad_rot || grad_center;
    if (p.V < 1 || p.V > kMaxViews || coords.ptr || (grad_proj && !part) || (pose && !pose_part) || (!grad_proj && !pose && !grad_weights && !p.conf_stream) ||
        (grad_weights && (!wpart || !p.view_weights)))
        return hipErrorInvalidValue;
    float *wp = grad_weights ? wpart : nullptr;
    hipError_t e = pose ? geom_dispatch<true>(grad_out, featT, proj, coords, grad_proj ? part : nullptr, nullptr, pose_part, wp, p, s)
                        : geom_dispatch<false>(grad_out, featT, proj, coords, grad_proj ? part : nullptr, nullptr, nullptr, wp, p, s);
    if (e != hipSuccess) return e;
    if (grad_proj) {
        hipLaunchKernelGGL(k_geom_reduce, dim3((unsigned)(p.B * p.V)), dim3(256), 0, s, (const float *)part, grad_proj, p.V, (int)geom_tiles(p));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (pose) {
        hipLaunchKernelGGL(k_pose_reduce, dim3((unsigned)p.B), dim3(256), 0, s, (const float *)pose_part, coords.rot, grad_rot, grad_center,
                           (int)geom_tiles(p));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return reduce_weights(wpart, grad_weights, p, s);
}

}  // namespace mvhmr
