// Shared feature maps (include/mvhmr_unproject.h: the *_shared entry points): M volumes read the B feature samples through an
// index -- volume m is the plain un-projection of features[idx[m]] under proj[idx[m]] onto coords[m] (or the cuboid of pose m).
//
// k_fwd_gather_shared and k_bwd_gather_shared are the gather kernels (unproject_gather.hip: same block, same three phases) -- copies, not
// template flags of k_fwd_gather / k_bwd_gather: those kernels' instances keep the code they had.  What differs:
//   m = blockIdx.y is the VOLUME; fb = idx[m], read once per block into an SGPR, is the feature sample.  The feature rows, the projections
//   (and in deterministic mode the exponents) come from fb; the coordinates or the cuboid pose, the output and grad_out from m.
//   fb outside [0, B) is "no sample": a block-uniform branch taken before the first barrier and before anything is read through fb -- the
//   forward writes its tile's zeros and returns, the backward returns.
// k_bwd_gather_shared serves both modes of the feature backward (float atomics / int64 fixed point), as k_bwd_gather_weighted does; volumes
// that share a sample add into the same rows of the (B, V, HW, C4) accumulator, which the atomics sum.
// The deterministic scale pass (unproject_det.hip: k_det_count, the shared row map of k_det_gmax) fixes ONE exponent K[b][c] per FEATURE sample and channel: max|g| over every volume that names b
// (integer atomicMax over (idx[m], c): exact in any order), and the bound carries the number of those volumes, cnt[b] (a B-word histogram built
// with integer atomics): cnt[b] * N * bound * 2^K < 2^62.  A pixel receives at most one tap per voxel, view and VOLUME; without cnt[b] the int64
// sums of a sample named many times can wrap.
#include "device_common.h"
#include "det_scale.h"
#include "kernels.h"

namespace mvhmr {

namespace {

constexpr int kShTile = 32;          // voxels per block (k_fwd_gather's tile)
constexpr int kShQuads = 64;         // 64 lanes x 4 channels
constexpr int kShCh = 256;

struct alignas(16) ShRec {
    int o00, o01, o10, o11;          // element offsets (pixel * C4) inside one (b,v) channels-last map
    float w00, w01, w10, w11;
};
struct USh { int o00, o01, o10, o11; float w00, w01, w10, w11; };
__device__ __forceinline__ USh uniform_sh(const ShRec &r)
{
    USh u;
    u.o00 = uniform(r.o00); u.o01 = uniform(r.o01); u.o10 = uniform(r.o10); u.o11 = uniform(r.o11);
    u.w00 = uniform(r.w00); u.w01 = uniform(r.w01); u.w10 = uniform(r.w10); u.w11 = uniform(r.w11);
    return u;
}

// phase 1 (build_records of unproject_gather.hip): the voxel centre comes from volume m, the projection from feature sample fb
__device__ __forceinline__ void build_shared_records(ShRec *recs, const float *__restrict__ proj, const Coords &coords, int m, int fb, int V,
                                                     long long n0, long long N, int H, int W, int C4)
{
    for (int idx = threadIdx.x; idx < kShTile * V; idx += blockDim.x) {
        const int v = idx / kShTile, j = idx % kShTile;
        long long n = n0 + j;
        n = n < N ? n : N - 1;       // tail voxels are computed and dropped
        float X0, X1, X2;
        voxel_xyz(coords, m, N, n, X0, X1, X2);
        const Taps t = make_taps(proj + ((long long)fb * V + v) * 12, X0, X1, X2, H, W);
        ShRec r;
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
k_fwd_gather_shared(const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords, TO *__restrict__ out,
                    const int *__restrict__ fidx, int B, int Vrt, int C, int C4, int H, int W, long long N, int tstride)
{
    const int V = VT > 0 ? VT : Vrt;
    const int m = blockIdx.y, cg = blockIdx.z;
    const int fb = uniform(fidx[m]);                          // the feature sample of this volume: one scalar load per block
    extern __shared__ __align__(16) unsigned char smem[];
    ShRec *recs = reinterpret_cast<ShRec *>(smem);
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem + sizeof(ShRec) * kShTile * V);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n0 = (long long)blockIdx.x * kShTile;
    const long long mapsz = (long long)H * W * C4;
    const int Q = C4 >> 2;
    const int vl = lane & (kShTile - 1), half = lane / kShTile;

    if ((unsigned)fb >= (unsigned)B) {
        // no sample: the tile's zeros in the store phase's shape, nothing read through fb (block-uniform, before the first barrier)
        const long long n = n0 + vl;
        if (n < N) {
            for (int qq = wave * 16 + half; qq < wave * 16 + 16; qq += 64 / kShTile) {
                const int cq = cg * kShQuads + qq;
                if (cq >= Q) break;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = cq * 4 + i;
                    if (c < C) store_streaming(&out[((long long)m * C + c) * N + n], 0.f);
                }
            }
        }
        return;
    }

    build_shared_records(recs, proj, coords, m, fb, V, n0, N, H, W, C4);
    __syncthreads();

    int q = cg * kShQuads + lane;
    const bool q_active = q < Q;
    q = q_active ? q : Q - 1;                                // idle lanes shadow the last quad and write nothing
    const TF *fp = featT + (long long)fb * V * mapsz + q * 4;

    for (int jj = 0; jj < kShTile / 4; ++jj) {
        const int j = wave * (kShTile / 4) + jj;
        f32x4 o;
        if constexpr (VT > 0) {
            float s[4][VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                const USh u = uniform_sh(recs[j * VT + v]);
                const TF *fv = fp + v * mapsz;
                // a sample that is identically zero (z <= 0, or all four taps outside the map) reads nothing (k_fwd_gather)
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
                const USh u = uniform_sh(recs[j * V + v]);
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
        for (int qq = wave * 16 + half; qq < wave * 16 + 16; qq += 64 / kShTile) {
            const int cq = cg * kShQuads + qq;
            if (cq >= Q) break;
            const f32x4 t = tile[vl * tstride + qq];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = cq * 4 + i;
                if (c < C) store_streaming(&out[((long long)m * C + c) * N + n], t.v[i]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ feature backward, both modes
// ACC = float adds ds * tap weight with float atomics into the channels-last fp32 gradient (k_bwd_gather), ACC = unsigned long long adds
// det_fixed(.., K[fb][c]) into the int64 one (k_bwd_gather_det; kexp null otherwise).  Both accumulators are (B, V, HW, C4).
template <typename TF, typename TO, int METHOD, int VT, typename ACC>
__global__ void __launch_bounds__(256)
k_bwd_gather_shared(const TO *__restrict__ grad_out, const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords,
                    ACC *__restrict__ gradT, const int *__restrict__ kexp, const int *__restrict__ fidx, int B, int Vrt, int C, int C4, int H, int W,
                    long long N)
{
    constexpr bool DET = sizeof(ACC) == 8;
    const int V = VT > 0 ? VT : Vrt;
    const int m = blockIdx.y, cg = blockIdx.z;
    const int fb = uniform(fidx[m]);
    if ((unsigned)fb >= (unsigned)B) return;                  // no sample: contributes to no gradient (block-uniform, before any barrier)
    extern __shared__ __align__(16) unsigned char smem[];
    ShRec *recs = reinterpret_cast<ShRec *>(smem);
    float *gtile = reinterpret_cast<float *>(smem + sizeof(ShRec) * kShTile * V);   // [256 ch][kShTile + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n0 = (long long)blockIdx.x * kShTile;
    const long long mapsz = (long long)H * W * C4;

    build_shared_records(recs, proj, coords, m, fb, V, n0, N, H, W, C4);
    {   // grad_out tile of volume m, coalesced along voxels: the two half-waves load alternate channels
        const int vl = lane & (kShTile - 1), half = lane / kShTile;
        const long long n = n0 + vl;
        for (int r = wave * 64 + half; r < wave * 64 + 64; r += 64 / kShTile) {
            const int c = cg * kShCh + r;
            float g = 0.f;
            if (c < C && n < N) g = to_f32<TO>(grad_out[((long long)m * C + c) * N + n]);
            gtile[r * (kShTile + 1) + vl] = g;
        }
    }
    __syncthreads();

    int ch[4], kx[4];
    bool act[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = cg * kShCh + i * 64 + lane;
        act[i] = c < C;
        ch[i] = act[i] ? c : 0;
        kx[i] = 0;
        if constexpr (DET) {
            kx[i] = act[i] ? kexp[(long long)fb * C + ch[i]] : kDetPoison;
            act[i] = act[i] && kx[i] != kDetPoison;                             // a poisoned channel adds nothing
        }
    }
    const TF *fp = featT + (long long)fb * V * mapsz;
    ACC *gb = gradT + (long long)fb * V * mapsz;

    auto sample4 = [&](const USh &u, int v, float (&sv)[4]) {
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
    auto scatter4 = [&](const USh &u, int v, const float (&dsv)[4]) {
        ACC *gv = gb + v * mapsz;
        // zero-weight taps (outside the map, or z <= 0) receive nothing -- wave-uniform branches
        if (u.w00 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o00 + ch[i], dsv[i] * u.w00, kx[i]); }
        if (u.w01 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o01 + ch[i], dsv[i] * u.w01, kx[i]); }
        if (u.w10 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o10 + ch[i], dsv[i] * u.w10, kx[i]); }
        if (u.w11 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o11 + ch[i], dsv[i] * u.w11, kx[i]); }
    };

    for (int jj = 0; jj < kShTile / 4; ++jj) {
        const int j = wave * (kShTile / 4) + jj;
        if (n0 + j >= N) break;
        float g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = gtile[(i * 64 + lane) * (kShTile + 1) + j];

        if constexpr (VT > 0) {
            float s[4][VT], ds[4][VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                float sv[4] = {0.f, 0.f, 0.f, 0.f};
                sample4(uniform_sh(recs[j * VT + v]), v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i][v] = sv[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) aggregate_grad<METHOD, VT>(s[i], g[i], ds[i]);
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                const float dsv[4] = {ds[0][v], ds[1][v], ds[2][v], ds[3][v]};
                scatter4(uniform_sh(recs[j * VT + v]), v, dsv);
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
                sample4(uniform_sh(recs[j * V + v]), v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ra[i].push(sv[i]);
                    if (sv[i] > best[i]) { best[i] = sv[i]; am[i] = v; }
                }
            }
            for (int v = 0; v < V; ++v) {
                const USh u = uniform_sh(recs[j * V + v]);
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

// ------------------------------------------------------------------------------------------ launchers
namespace {

template <typename TF, typename TO, int METHOD>
hipError_t fwd_shared_v(const TF *featT, const float *proj, const Coords &coords, TO *out, const Problem &p, hipStream_t s)
{
    const int Q = p.C4 / 4;
    int tstride = (Q < kShQuads ? Q : kShQuads) + 1;
    tstride |= 1;
    const size_t lds = sizeof(ShRec) * kShTile * (size_t)p.V + sizeof(f32x4) * kShTile * (size_t)tstride;
    const dim3 grid((unsigned)((p.N + kShTile - 1) / kShTile), (unsigned)p.volumes, (unsigned)((Q + kShQuads - 1) / kShQuads));
    auto go = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, featT, proj, coords, out, p.feature_index, p.B, p.V, p.C, p.C4, p.H, p.W, p.N, tstride);
        return hipGetLastError();
    };
    switch (p.V) {
    case 2: return go(k_fwd_gather_shared<TF, TO, METHOD, 2>);
    case 4: return go(k_fwd_gather_shared<TF, TO, METHOD, 4>);
    case 8: return go(k_fwd_gather_shared<TF, TO, METHOD, 8>);
    default: return go(k_fwd_gather_shared<TF, TO, METHOD, 0>);
    }
}

template <typename TF, typename TO>
hipError_t fwd_shared_m(const TF *featT, const float *proj, const Coords &coords, TO *out, const Problem &p, hipStream_t s)
{
    switch (p.method) {
    case AGG_SOFTMAX: return fwd_shared_v<TF, TO, AGG_SOFTMAX>(featT, proj, coords, out, p, s);
    case AGG_SUM: return fwd_shared_v<TF, TO, AGG_SUM>(featT, proj, coords, out, p, s);
    case AGG_MEAN: return fwd_shared_v<TF, TO, AGG_MEAN>(featT, proj, coords, out, p, s);
    case AGG_MAX: return fwd_shared_v<TF, TO, AGG_MAX>(featT, proj, coords, out, p, s);
    }
    return hipErrorInvalidValue;
}

template <typename ACC, typename TF, typename TO, int METHOD>
hipError_t bwd_shared_v(const TO *go_, const TF *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                        hipStream_t s)
{
    const size_t lds = sizeof(ShRec) * kShTile * (size_t)p.V + sizeof(float) * kShCh * (kShTile + 1);
    const dim3 grid((unsigned)((p.N + kShTile - 1) / kShTile), (unsigned)p.volumes, (unsigned)((p.C + kShCh - 1) / kShCh));
    auto go = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, go_, featT, proj, coords, gradT, kexp, p.feature_index, p.B, p.V, p.C, p.C4, p.H, p.W, p.N);
        return hipGetLastError();
    };
    switch (p.V) {
    case 2: return go(k_bwd_gather_shared<TF, TO, METHOD, 2, ACC>);
    case 4: return go(k_bwd_gather_shared<TF, TO, METHOD, 4, ACC>);
    case 8: return go(k_bwd_gather_shared<TF, TO, METHOD, 8, ACC>);
    default: return go(k_bwd_gather_shared<TF, TO, METHOD, 0, ACC>);
    }
}

template <typename ACC, typename TF, typename TO>
hipError_t bwd_shared_m(const TO *go_, const TF *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                        hipStream_t s)
{
    switch (p.method) {
    case AGG_SOFTMAX: return bwd_shared_v<ACC, TF, TO, AGG_SOFTMAX>(go_, featT, proj, coords, gradT, kexp, p, s);
    case AGG_SUM: return bwd_shared_v<ACC, TF, TO, AGG_SUM>(go_, featT, proj, coords, gradT, kexp, p, s);
    case AGG_MEAN: return bwd_shared_v<ACC, TF, TO, AGG_MEAN>(go_, featT, proj, coords, gradT, kexp, p, s);
    case AGG_MAX: return bwd_shared_v<ACC, TF, TO, AGG_MAX>(go_, featT, proj, coords, gradT, kexp, p, s);
    }
    return hipErrorInvalidValue;
}

template <typename ACC>
hipError_t bwd_shared(const void *grad_out, const void *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                      hipStream_t s)
{
    if (!p.feature_index || p.volumes < 1 || p.volumes > kSharedMaxVolumes) return hipErrorInvalidValue;
    if (p.out_bf16) return p.feat_f16 ? hipErrorNotSupported : bwd_shared_m((const bf16_t *)grad_out, (const float *)featT, proj, coords, gradT, kexp, p, s);
    if (!p.feat_f16 && !p.out_f16) return bwd_shared_m((const float *)grad_out, (const float *)featT, proj, coords, gradT, kexp, p, s);
    if (p.feat_f16 && p.out_f16) return bwd_shared_m((const __half *)grad_out, (const __half *)featT, proj, coords, gradT, kexp, p, s);
    if (p.feat_f16 && !p.out_f16) return bwd_shared_m((const float *)grad_out, (const __half *)featT, proj, coords, gradT, kexp, p, s);
    return hipErrorNotSupported;
}

}  // namespace

hipError_t launch_fwd_gather_shared(const void *featT, const float *proj, const Coords &coords, void *out, const Problem &p, hipStream_t s)
{
    if (!p.feature_index || p.volumes < 1 || p.volumes > kSharedMaxVolumes) return hipErrorInvalidValue;
    if (p.out_bf16) return p.feat_f16 ? hipErrorNotSupported : fwd_shared_m((const float *)featT, proj, coords, (bf16_t *)out, p, s);
    if (!p.feat_f16 && !p.out_f16) return fwd_shared_m((const float *)featT, proj, coords, (float *)out, p, s);
    if (p.feat_f16 && p.out_f16) return fwd_shared_m((const __half *)featT, proj, coords, (__half *)out, p, s);
    if (p.feat_f16 && !p.out_f16) return fwd_shared_m((const __half *)featT, proj, coords, (float *)out, p, s);
    return hipErrorNotSupported;
}

hipError_t launch_bwd_gather_shared(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *gradT, const Problem &p,
                                    hipStream_t s)
{
    return bwd_shared<float>(grad_out, featT, proj, coords, gradT, nullptr, p, s);
}

hipError_t launch_bwd_gather_shared_det(const void *grad_out, const void *featT, const float *proj, const Coords &coords, unsigned long long *gradI,
                                        const int *kexp, const Problem &p, hipStream_t s)
{
    return bwd_shared<unsigned long long>(grad_out, featT, proj, coords, gradI, kexp, p, s);
}

}  // namespace mvhmr
