// Lens-distortion-aware un-projection (include/mvhmr_unproject.h: the *_lens entry points): every (sample, view) carries a
// Brown-Conrady record (lens.h) and the voxels are projected THROUGH it, so the features may come from raw, un-rectified images.
//
// k_fwd_gather_lens and k_bwd_gather_lens are the gather kernels (unproject_gather.hip: same block, same three phases) -- copies, not
// template flags of k_fwd_gather / k_bwd_gather: those kernels' instances keep the code they had.  What differs:
//   the V lens records of the block's sample are read ONCE per block into LDS (one more barrier in front of phase 1), behind the tile in the
//   dynamic region: a static array in front of it would move its base off the 16-byte boundary the 128-bit LDS accesses want;
//   phase 1 takes a view without distortion (five coefficients +-0) through make_taps -- the plain call's positions bit for bit -- and
//   every other view through make_taps_lens; a ray past the fold-back guard gets the all-zero record of z <= 0: nothing read, no gradient.
// Phases 2 and 3 never see a position: they are the plain kernels'.  k_bwd_gather_lens serves both modes of the feature backward (float
// atomics / int64 fixed point), as k_bwd_gather_shared does; the deterministic scale pass is the plain one -- its bound does not depend on
// where the taps land.  k_plane_taps_lens is k_plane_taps (unproject_plane_bwd.hip) with the same phase 1: the plane backward's other two
// kernels read positions only through its table and run as they are.
#include "brick_common.h"
#include "det_scale.h"
#include "kernels.h"
#include "lens.h"

namespace mvhmr {

namespace {

constexpr int kLnTile = 32;          // voxels per block (k_fwd_gather's tile)
constexpr int kLnQuads = 64;         // 64 lanes x 4 channels
constexpr int kLnCh = 256;

struct alignas(16) LnRec {
    int o00, o01, o10, o11;          // element offsets (pixel * C4) inside one (b,v) channels-last map
    float w00, w01, w10, w11;
};
struct ULn { int o00, o01, o10, o11; float w00, w01, w10, w11; };
__device__ __forceinline__ ULn uniform_ln(const LnRec &r)
{
    ULn u;
    u.o00 = uniform(r.o00); u.o01 = uniform(r.o01); u.o10 = uniform(r.o10); u.o11 = uniform(r.o11);
    u.w00 = uniform(r.w00); u.w01 = uniform(r.w01); u.w10 = uniform(r.w10); u.w11 = uniform(r.w11);
    return u;
}

// the sample's lens records into LDS: one read per block and view
__device__ __forceinline__ void stage_lens(float *lens_s, const float *__restrict__ lens, int b, int V)
{
    for (int i = threadIdx.x; i < V * kLensWords; i += blockDim.x) lens_s[i] = lens[(long long)b * V * kLensWords + i];
    __syncthreads();
}

// phase 1 (build_records of unproject_gather.hip) through the lens records in LDS
__device__ __forceinline__ void build_lens_records(LnRec *recs, const float *__restrict__ proj, const float *lens_s, const Coords &coords, int b, int V,
                                                   long long n0, long long N, int H, int W, int C4)
{
    for (int idx = threadIdx.x; idx < kLnTile * V; idx += blockDim.x) {
        const int v = idx / kLnTile, j = idx % kLnTile;
        long long n = n0 + j;
        n = n < N ? n : N - 1;       // tail voxels are computed and dropped
        float X0, X1, X2;
        voxel_xyz(coords, b, N, n, X0, X1, X2);
        const Taps t = lens_taps(proj + ((long long)b * V + v) * 12, lens_s + v * kLensWords, X0, X1, X2, H, W);
        LnRec r;
        r.o00 = (t.y0 * W + t.x0) * C4;
        r.o01 = (t.y0 * W + t.x1) * C4;
        r.o10 = (t.y1 * W + t.x0) * C4;
        r.o11 = (t.y1 * W + t.x1) * C4;
        r.w00 = t.w00; r.w01 = t.w01; r.w10 = t.w10; r.w11 = t.w11;
        recs[j * V + v] = r;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------ forward
template <typename TF, typename TO, int METHOD, int VT>
__global__ void __launch_bounds__(256)
k_fwd_gather_lens(const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords, TO *__restrict__ out,
                  const float *__restrict__ lens, int Vrt, int C, int C4, int H, int W, long long N, int tstride)
{
    const int V = VT > 0 ? VT : Vrt;
    const int b = blockIdx.y, cg = blockIdx.z;
    extern __shared__ __align__(16) unsigned char smem[];
    LnRec *recs = reinterpret_cast<LnRec *>(smem);
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem + sizeof(LnRec) * kLnTile * V);
    float *lens_s = reinterpret_cast<float *>(tile + kLnTile * tstride);      // [V][kLensWords]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n0 = (long long)blockIdx.x * kLnTile;
    const long long mapsz = (long long)H * W * C4;
    const int Q = C4 >> 2;
    const int vl = lane & (kLnTile - 1), half = lane / kLnTile;

    stage_lens(lens_s, lens, b, V);
    build_lens_records(recs, proj, lens_s, coords, b, V, n0, N, H, W, C4);
    __syncthreads();

    int q = cg * kLnQuads + lane;
    const bool q_active = q < Q;
    q = q_active ? q : Q - 1;                                // idle lanes shadow the last quad and write nothing
    const TF *fp = featT + (long long)b * V * mapsz + q * 4;

    for (int jj = 0; jj < kLnTile / 4; ++jj) {
        const int j = wave * (kLnTile / 4) + jj;
        f32x4 o;
        if constexpr (VT > 0) {
            float s[4][VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                const ULn u = uniform_ln(recs[j * VT + v]);
                const TF *fv = fp + v * mapsz;
                // a sample that is identically zero (z <= 0, past the guard, or all four taps outside the map) reads nothing (k_fwd_gather)
                if (u.w00 == 0.f && u.w01 == 0.f && u.w10 == 0.f && u.w11 == 0.f) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) s[i][v] = 0.f;
                    continue;
                }
                const f32x4 a = Vec4<TF>::load(fv + u.o00), bb = Vec4<TF>::load(fv + u.o01);
                const f32x4 c = Vec4<TF>::load(fv + u.o10), d = Vec4<TF>::load(fv + u.o11);
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i][v] = bilerp(a.v[i], bb.v[i], c.v[i], d.v[i], u.w00, u.w01, u.w10, u.w11);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) o.v[i] = aggregate<METHOD, VT>(s[i]);
        } else {
            RunningAgg<METHOD> ra[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) ra[i].init();
            for (int v = 0; v < V; ++v) {
                const ULn u = uniform_ln(recs[j * V + v]);
                const TF *fv = fp + v * mapsz;
                if (u.w00 == 0.f && u.w01 == 0.f && u.w10 == 0.f && u.w11 == 0.f) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) ra[i].push(0.f);
                    continue;
                }
                const f32x4 a = Vec4<TF>::load(fv + u.o00), bb = Vec4<TF>::load(fv + u.o01);
                const f32x4 c = Vec4<TF>::load(fv + u.o10), d = Vec4<TF>::load(fv + u.o11);
#pragma unroll
                for (int i = 0; i < 4; ++i) ra[i].push(bilerp(a.v[i], bb.v[i], c.v[i], d.v[i], u.w00, u.w01, u.w10, u.w11));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) o.v[i] = ra[i].result(V);
        }
        if (q_active) tile[j * tstride + lane] = o;
    }
    __syncthreads();

    const long long n = n0 + vl;                              // the store phase of k_fwd_gather
    if (n < N) {
        for (int qq = wave * 16 + half; qq < wave * 16 + 16; qq += 64 / kLnTile) {
            const int cq = cg * kLnQuads + qq;
            if (cq >= Q) break;
            const f32x4 t = tile[vl * tstride + qq];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = cq * 4 + i;
                if (c < C) store_streaming(&out[((long long)b * C + c) * N + n], t.v[i]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ feature backward, both modes
// ACC = float adds ds * tap weight with float atomics into the channels-last fp32 gradient (k_bwd_gather), ACC = unsigned long long adds
// det_fixed(.., K[b][c]) into the int64 one (k_bwd_gather_det; kexp null otherwise).  Both accumulators are (B, V, HW, C4).
template <typename TF, typename TO, int METHOD, int VT, typename ACC>
__global__ void __launch_bounds__(256)
k_bwd_gather_lens(const TO *__restrict__ grad_out, const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords,
                  ACC *__restrict__ gradT, const int *__restrict__ kexp, const float *__restrict__ lens, int Vrt, int C, int C4, int H, int W, long long N)
{
    constexpr bool DET = sizeof(ACC) == 8;
    const int V = VT > 0 ? VT : Vrt;
    const int b = blockIdx.y, cg = blockIdx.z;
    extern __shared__ __align__(16) unsigned char smem[];
    LnRec *recs = reinterpret_cast<LnRec *>(smem);
    float *gtile = reinterpret_cast<float *>(smem + sizeof(LnRec) * kLnTile * V);   // [256 ch][kLnTile + 1]
    float *lens_s = gtile + kLnCh * (kLnTile + 1);                                  // [V][kLensWords]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n0 = (long long)blockIdx.x * kLnTile;
    const long long mapsz = (long long)H * W * C4;

    stage_lens(lens_s, lens, b, V);
    build_lens_records(recs, proj, lens_s, coords, b, V, n0, N, H, W, C4);
    {   // grad_out tile, coalesced along voxels: the two half-waves load alternate channels
        const int vl = lane & (kLnTile - 1), half = lane / kLnTile;
        const long long n = n0 + vl;
        for (int r = wave * 64 + half; r < wave * 64 + 64; r += 64 / kLnTile) {
            const int c = cg * kLnCh + r;
            float g = 0.f;
            if (c < C && n < N) g = to_f32<TO>(grad_out[((long long)b * C + c) * N + n]);
            gtile[r * (kLnTile + 1) + vl] = g;
        }
    }
    __syncthreads();

    int ch[4], kx[4];
    bool act[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = cg * kLnCh + i * 64 + lane;
        act[i] = c < C;
        ch[i] = act[i] ? c : 0;
        kx[i] = 0;
        if constexpr (DET) {
            kx[i] = act[i] ? kexp[(long long)b * C + ch[i]] : kDetPoison;
            act[i] = act[i] && kx[i] != kDetPoison;                             // a poisoned channel adds nothing
        }
    }
    const TF *fp = featT + (long long)b * V * mapsz;
    ACC *gb = gradT + (long long)b * V * mapsz;

    auto sample4 = [&](const ULn &u, int v, float (&sv)[4]) {
        const TF *fv = fp + v * mapsz;
        if (u.w00 == 0.f && u.w01 == 0.f && u.w10 == 0.f && u.w11 == 0.f) {        // identically zero: reads nothing (see k_fwd_gather)
#pragma unroll
            for (int i = 0; i < 4; ++i) sv[i] = 0.f;
            return;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            sv[i] = bilerp(to_f32<TF>(fv[u.o00 + ch[i]]), to_f32<TF>(fv[u.o01 + ch[i]]), to_f32<TF>(fv[u.o10 + ch[i]]),
                           to_f32<TF>(fv[u.o11 + ch[i]]), u.w00, u.w01, u.w10, u.w11);
    };
    auto add = [&](ACC *at, float x, int k) {
        if constexpr (DET) atomicAdd(at, det_fixed(x, k));
        else atomicAdd(at, x);
    };
    auto scatter4 = [&](const ULn &u, int v, const float (&dsv)[4]) {
        ACC *gv = gb + v * mapsz;
        // zero-weight taps (outside the map, z <= 0, past the guard) receive nothing -- wave-uniform branches
        if (u.w00 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o00 + ch[i], dsv[i] * u.w00, kx[i]); }
        if (u.w01 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o01 + ch[i], dsv[i] * u.w01, kx[i]); }
        if (u.w10 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o10 + ch[i], dsv[i] * u.w10, kx[i]); }
        if (u.w11 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o11 + ch[i], dsv[i] * u.w11, kx[i]); }
    };

    for (int jj = 0; jj < kLnTile / 4; ++jj) {
        const int j = wave * (kLnTile / 4) + jj;
        if (n0 + j >= N) break;
        float g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = gtile[(i * 64 + lane) * (kLnTile + 1) + j];

        if constexpr (VT > 0) {
            float s[4][VT], ds[4][VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                float sv[4] = {0.f, 0.f, 0.f, 0.f};
                sample4(uniform_ln(recs[j * VT + v]), v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i][v] = sv[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) aggregate_grad<METHOD, VT>(s[i], g[i], ds[i]);
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                const float dsv[4] = {ds[0][v], ds[1][v], ds[2][v], ds[3][v]};
                scatter4(uniform_ln(recs[j * VT + v]), v, dsv);
            }
        } else {
            // run-time view count: pass 1 accumulates the aggregate, pass 2 re-samples and scatters
            RunningAgg<METHOD> ra[4];
            int am[4] = {0, 0, 0, 0};
            float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int i = 0; i < 4; ++i) ra[i].init();
            for (int v = 0; v < V; ++v) {
                float sv[4];
                sample4(uniform_ln(recs[j * V + v]), v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ra[i].push(sv[i]);
                    if (sv[i] > best[i]) { best[i] = sv[i]; am[i] = v; }
                }
            }
            for (int v = 0; v < V; ++v) {
                const ULn u = uniform_ln(recs[j * V + v]);
                float sv[4], dsv[4];
                sample4(u, v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if constexpr (METHOD == AGG_SUM) dsv[i] = g[i];
                    else if constexpr (METHOD == AGG_MEAN) dsv[i] = __fdiv_rn(g[i], (float)V);
                    else if constexpr (METHOD == AGG_MAX) dsv[i] = am[i] == v ? g[i] : 0.f;
                    else {
                        const float rden = __builtin_amdgcn_rcpf(ra[i].den);
                        const float o = ra[i].num * rden;
                        dsv[i] = g[i] * __expf(sv[i] - ra[i].m) * rden * (1.f + sv[i] - o);
                    }
                }
                scatter4(u, v, dsv);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ the plane backward's tap table
// k_plane_taps (unproject_plane_bwd.hip: one block per (sample, view), the table's layout and the per-pixel tap count) through the view's
// lens record, read once per block
__global__ void __launch_bounds__(1024)
k_plane_taps_lens(const float *__restrict__ proj, const float *__restrict__ lens, const Coords coords, float4 *__restrict__ tabW, int *__restrict__ tabX,
                  int *__restrict__ cmax, int V, int H, int W, long long N, Gate gate)
{
    if (gated_off(gate)) return;
    extern __shared__ int cnt[];                                                  // [H * W] + 1
    const int b = blockIdx.x / V, v = blockIdx.x % V, HW = H * W;
    for (int i = threadIdx.x; i <= HW; i += 1024) cnt[i] = 0;
    __shared__ float P[12];
    __shared__ float L[kLensWords];                                                // (every LDS access of this kernel is 32 bits wide: the statics in front of cnt cost nothing)
    if (threadIdx.x < 12) P[threadIdx.x] = proj[((long long)b * V + v) * 12 + threadIdx.x];
    if (threadIdx.x >= 64 && threadIdx.x < 64 + kLensWords) L[threadIdx.x - 64] = lens[((long long)b * V + v) * kLensWords + threadIdx.x - 64];
    __syncthreads();
    const long long base = ((long long)b * V + v) * N;
    for (long long n = threadIdx.x; n < N; n += 1024) {
        float c0, c1, c2;
        voxel_xyz(coords, b, N, n, c0, c1, c2);
        const Taps t = lens_taps(P, L, c0, c1, c2, H, W);
        tabW[base + n] = make_float4(t.w00, t.w01, t.w10, t.w11);
        tabX[base + n] = t.x0 | ((t.x1 - t.x0) << 15) | (t.y0 << 16) | ((t.y1 - t.y0) << 31);   // x0, y0 < 2^15; x1 - x0, y1 - y0 in {0, 1}
        if (t.w00 != 0.f) lds_add(cnt + t.y0 * W + t.x0, 1);
        if (t.w01 != 0.f) lds_add(cnt + t.y0 * W + t.x1, 1);
        if (t.w10 != 0.f) lds_add(cnt + t.y1 * W + t.x0, 1);
        if (t.w11 != 0.f) lds_add(cnt + t.y1 * W + t.x1, 1);
    }
    __syncthreads();
    int m = 1;
    for (int i = threadIdx.x; i < HW; i += 1024) { const int c = cnt[i]; m = c > m ? c : m; }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) atomicMax(&cnt[HW], m);
    __syncthreads();
    if (threadIdx.x == 0) cmax[blockIdx.x] = cnt[HW];
}

// ------------------------------------------------------------------------------------------ launchers
namespace {

template <typename TF, typename TO, int METHOD>
hipError_t fwd_lens_v(const TF *featT, const float *proj, const Coords &coords, TO *out, const Problem &p, hipStream_t s)
{
    const int Q = p.C4 / 4;
    int tstride = (Q < kLnQuads ? Q : kLnQuads) + 1;
    tstride |= 1;
    const size_t lds = sizeof(LnRec) * kLnTile * (size_t)p.V + sizeof(f32x4) * kLnTile * (size_t)tstride + sizeof(float) * kLensWords * (size_t)p.V;
    const dim3 grid((unsigned)((p.N + kLnTile - 1) / kLnTile), (unsigned)p.B, (unsigned)((Q + kLnQuads - 1) / kLnQuads));
    auto go = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, featT, proj, coords, out, p.lens, p.V, p.C, p.C4, p.H, p.W, p.N, tstride);
        return hipGetLastError();
    };
    switch (p.V) {
    case 2: return go(k_fwd_gather_lens<TF, TO, METHOD, 2>);
    case 4: return go(k_fwd_gather_lens<TF, TO, METHOD, 4>);
    case 8: return go(k_fwd_gather_lens<TF, TO, METHOD, 8>);
    default: return go(k_fwd_gather_lens<TF, TO, METHOD, 0>);
    }
}

template <typename TF, typename TO>
hipError_t fwd_lens_m(const TF *featT, const float *proj, const Coords &coords, TO *out, const Problem &p, hipStream_t s)
{
    switch (p.method) {
    case AGG_SOFTMAX: return fwd_lens_v<TF, TO, AGG_SOFTMAX>(featT, proj, coords, out, p, s);
    case AGG_SUM: return fwd_lens_v<TF, TO, AGG_SUM>(featT, proj, coords, out, p, s);
    case AGG_MEAN: return fwd_lens_v<TF, TO, AGG_MEAN>(featT, proj, coords, out, p, s);
    case AGG_MAX: return fwd_lens_v<TF, TO, AGG_MAX>(featT, proj, coords, out, p, s);
    }
    return hipErrorInvalidValue;
}

template <typename ACC, typename TF, typename TO, int METHOD>
hipError_t bwd_lens_v(const TO *go_, const TF *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                      hipStream_t s)
{
    const size_t lds = sizeof(LnRec) * kLnTile * (size_t)p.V + sizeof(float) * kLnCh * (kLnTile + 1) + sizeof(float) * kLensWords * (size_t)p.V;
    const dim3 grid((unsigned)((p.N + kLnTile - 1) / kLnTile), (unsigned)p.B, (unsigned)((p.C + kLnCh - 1) / kLnCh));
    auto go = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, go_, featT, proj, coords, gradT, kexp, p.lens, p.V, p.C, p.C4, p.H, p.W, p.N);
        return hipGetLastError();
    };
    switch (p.V) {
    case 2: return go(k_bwd_gather_lens<TF, TO, METHOD, 2, ACC>);
    case 4: return go(k_bwd_gather_lens<TF, TO, METHOD, 4, ACC>);
    case 8: return go(k_bwd_gather_lens<TF, TO, METHOD, 8, ACC>);
    default: return go(k_bwd_gather_lens<TF, TO, METHOD, 0, ACC>);
    }
}

template <typename ACC, typename TF, typename TO>
hipError_t bwd_lens_m(const TO *go_, const TF *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                      hipStream_t s)
{
    switch (p.method) {
    case AGG_SOFTMAX: return bwd_lens_v<ACC, TF, TO, AGG_SOFTMAX>(go_, featT, proj, coords, gradT, kexp, p, s);
    case AGG_SUM: return bwd_lens_v<ACC, TF, TO, AGG_SUM>(go_, featT, proj, coords, gradT, kexp, p, s);
    case AGG_MEAN: return bwd_lens_v<ACC, TF, TO, AGG_MEAN>(go_, featT, proj, coords, gradT, kexp, p, s);
    case AGG_MAX: return bwd_lens_v<ACC, TF, TO, AGG_MAX>(go_, featT, proj, coords, gradT, kexp, p, s);
    }
    return hipErrorInvalidValue;
}

// grid.y is the sample, as in the plain kernels; the records in LDS hold at most kMaxViews views
bool lens_launchable(const Problem &p) { return p.lens && p.V >= 1 && p.V <= kMaxViews && p.B <= 65535; }

template <typename ACC>
hipError_t bwd_lens(const void *grad_out, const void *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                    hipStream_t s)
{
    if (!lens_launchable(p)) return hipErrorInvalidValue;
    if (p.out_bf16) return p.feat_f16 ? hipErrorNotSupported : bwd_lens_m((const bf16_t *)grad_out, (const float *)featT, proj, coords, gradT, kexp, p, s);
    if (!p.feat_f16 && !p.out_f16) return bwd_lens_m((const float *)grad_out, (const float *)featT, proj, coords, gradT, kexp, p, s);
    if (p.feat_f16 && p.out_f16) return bwd_lens_m((const __half *)grad_out, (const __half *)featT, proj, coords, gradT, kexp, p, s);
    if (p.feat_f16 && !p.out_f16) return bwd_lens_m((const float *)grad_out, (const __half *)featT, proj, coords, gradT, kexp, p, s);
    return hipErrorNotSupported;
}

}  // namespace

hipError_t launch_fwd_gather_lens(const void *featT, const float *proj, const Coords &coords, void *out, const Problem &p, hipStream_t s)
{
    if (!lens_launchable(p)) return hipErrorInvalidValue;
    if (p.out_bf16) return p.feat_f16 ? hipErrorNotSupported : fwd_lens_m((const float *)featT, proj, coords, (bf16_t *)out, p, s);
    if (!p.feat_f16 && !p.out_f16) return fwd_lens_m((const float *)featT, proj, coords, (float *)out, p, s);
    if (p.feat_f16 && p.out_f16) return fwd_lens_m((const __half *)featT, proj, coords, (__half *)out, p, s);
    if (p.feat_f16 && !p.out_f16) return fwd_lens_m((const __half *)featT, proj, coords, (float *)out, p, s);
    return hipErrorNotSupported;
}

hipError_t launch_bwd_gather_lens(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *gradT, const Problem &p,
                                  hipStream_t s)
{
    return bwd_lens<float>(grad_out, featT, proj, coords, gradT, nullptr, p, s);
}

hipError_t launch_bwd_gather_lens_det(const void *grad_out, const void *featT, const float *proj, const Coords &coords, unsigned long long *gradI,
                                      const int *kexp, const Problem &p, hipStream_t s)
{
    return bwd_lens<unsigned long long>(grad_out, featT, proj, coords, gradI, kexp, p, s);
}

hipError_t launch_plane_taps_lens(const float *proj, const Coords &coords, void *tabW, int *tabX, int *cmax, const Problem &p, hipStream_t s)
{
    if (!p.lens) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_plane_taps_lens, dim3((unsigned)(p.B * p.V)), dim3(1024), (size_t)(p.H * p.W + 1) * sizeof(int), s, proj, p.lens, coords,
                       static_cast<float4 *>(tabW), tabX, cmax, p.V, p.H, p.W, p.N, make_gate(p, false));
    return hipGetLastError();
}

}  // namespace mvhmr
