// Visibility-aware aggregation (include/mvhmr_unproject.h: the *_visible entry points): every voxel aggregates only the
// views that SEE it -- z > 0 and the projection inside the feature map, both ends inclusive (view_sees, device_common.h) -- instead of
// letting the other views contribute a sample of zero.
//
// k_fwd_gather_seen and k_bwd_gather_seen are the gather kernels (unproject_gather.hip: same block, same three phases) -- copies, not template
// flags of k_fwd_gather / k_bwd_gather: those kernels' instances keep the code they had.  What differs:
//   phase 1  the thread of (voxel, view) also evaluates view_sees from the same ix, iy, z and ORs its bit into the voxel's bitmask in LDS
//            (one word per voxel beside the tap records; an integer OR: no order dependence)
//   phase 2  the wave that owns a voxel reads the bitmask into an SGPR; an unseen view is a scalar branch that issues no feature loads;
//            the aggregate ranges over the set bits (seen_aggregate / seen_aggregate_grad; the run-time instances loop over set bits)
// With a view mask the packed route of DESIGN.md 5.8 is reused whole: nvs[b] bounds the slots (null: every view present).
// k_bwd_gather_seen serves both modes of the feature backward (float atomics / int64 fixed point), as k_bwd_gather_weighted does.
// k_view_visibility writes the bitmask itself, bit v = view v is present and sees the voxel: one thread per voxel, plain stores.
#include "device_common.h"
#include "det_scale.h"
#include "kernels.h"

namespace mvhmr {

namespace {

constexpr int kSeenTile = 32;          // voxels per block (k_fwd_gather's tile)
constexpr int kSeenQuads = 64;         // 64 lanes x 4 channels
constexpr int kSeenCh = 256;

struct alignas(16) SeenRec {
    int o00, o01, o10, o11;            // element offsets (pixel * C4) inside one (b,v) channels-last map
    float w00, w01, w10, w11;
};
struct USeen { int o00, o01, o10, o11; float w00, w01, w10, w11; };
__device__ __forceinline__ USeen uniform_seen(const SeenRec &r)
{
    USeen u;
    u.o00 = uniform(r.o00); u.o01 = uniform(r.o01); u.o10 = uniform(r.o10); u.o11 = uniform(r.o11);
    u.w00 = uniform(r.w00); u.w01 = uniform(r.w01); u.w10 = uniform(r.w10); u.w11 = uniform(r.w11);
    return u;
}

// LDS: [ tap records (voxel, view) | bitmask, one word per voxel (padded to 16 B) | the kernel's tile ]
__device__ __forceinline__ size_t seen_head_bytes(int V) { return sizeof(SeenRec) * kSeenTile * V + sizeof(unsigned) * kSeenTile; }

// phase 1: records and bitmask of the tile at n0; nvb slots are present.  Ends with the barrier that publishes both.
__device__ __forceinline__ void build_seen_records(SeenRec *recs, unsigned *vbits, const float *__restrict__ proj, const Coords &coords, int b, int V,
                                                   int nvb, long long n0, long long N, int H, int W, int C4)
{
    if (threadIdx.x < kSeenTile) vbits[threadIdx.x] = 0u;
    __syncthreads();
    for (int idx = threadIdx.x; idx < kSeenTile * V; idx += blockDim.x) {
        const int v = idx / kSeenTile, j = idx % kSeenTile;
        long long n = n0 + j;
        n = n < N ? n : N - 1;       // tail voxels are computed and dropped
        float X0, X1, X2;
        voxel_xyz(coords, b, N, n, X0, X1, X2);
        const float *P = proj + ((long long)b * V + v) * 12;
        const bool seen = v < nvb && view_sees(P, X0, X1, X2, H, W);
        SeenRec r;
        r.o00 = r.o01 = r.o10 = r.o11 = 0;
        r.w00 = r.w01 = r.w10 = r.w11 = 0.f;
        if (seen) {
            const Taps t = make_taps(P, X0, X1, X2, H, W);
            r.o00 = (t.y0 * W + t.x0) * C4;
            r.o01 = (t.y0 * W + t.x1) * C4;
            r.o10 = (t.y1 * W + t.x0) * C4;
            r.o11 = (t.y1 * W + t.x1) * C4;
            r.w00 = t.w00; r.w01 = t.w01; r.w10 = t.w10; r.w11 = t.w11;
            atomicOr(&vbits[j], 1u << v);
        }
        recs[j * V + v] = r;
    }
    __syncthreads();
}

}  // namespace

// ------------------------------------------------------------------------------------------ forward
template <typename TF, typename TO, int METHOD, int VT>
__global__ void __launch_bounds__(256)
k_fwd_gather_seen(const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords, TO *__restrict__ out, int Vrt, int C, int C4,
                  int H, int W, long long N, int tstride, const int *__restrict__ nvs)
{
    const int V = VT > 0 ? VT : Vrt;
    const int b = blockIdx.y, cg = blockIdx.z;
    const int nvb = nvs ? nvs[b] : V;                         // present views of this sample (block-uniform)
    extern __shared__ __align__(16) unsigned char smem[];
    SeenRec *recs = reinterpret_cast<SeenRec *>(smem);
    unsigned *vbits = reinterpret_cast<unsigned *>(smem + sizeof(SeenRec) * kSeenTile * V);
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem + seen_head_bytes(V));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n0 = (long long)blockIdx.x * kSeenTile;
    const long long mapsz = (long long)H * W * C4;
    const int Q = C4 >> 2;

    build_seen_records(recs, vbits, proj, coords, b, V, nvb, n0, N, H, W, C4);

    int q = cg * kSeenQuads + lane;
    const bool q_active = q < Q;
    q = q_active ? q : Q - 1;                                // idle lanes shadow the last quad and write nothing
    const TF *fb = featT + (long long)b * V * mapsz + q * 4;

    for (int jj = 0; jj < kSeenTile / 4; ++jj) {
        const int j = wave * (kSeenTile / 4) + jj;
        const unsigned bits = (unsigned)uniform((int)vbits[j]);      // the views that see this voxel: wave-uniform
        f32x4 o;
        if constexpr (VT > 0) {
            float s[4][VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                if (!(bits >> v & 1u)) {                             // scalar branch: an unseen view loads nothing, not even its record
#pragma unroll
                    for (int i = 0; i < 4; ++i) s[i][v] = 0.f;
                    continue;
                }
                const USeen u = uniform_seen(recs[j * VT + v]);
                const TF *fv = fb + v * mapsz;
                const f32x4 a = Vec4<TF>::load(fv + u.o00), bb = Vec4<TF>::load(fv + u.o01);
                const f32x4 c = Vec4<TF>::load(fv + u.o10), d = Vec4<TF>::load(fv + u.o11);
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i][v] = bilerp(a.v[i], bb.v[i], c.v[i], d.v[i], u.w00, u.w01, u.w10, u.w11);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) o.v[i] = seen_aggregate<METHOD, VT>(s[i], bits);
        } else {
            RunningAgg<METHOD> ra[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) ra[i].init();
            for (unsigned m = bits; m; m &= m - 1u) {                // set bits in view order
                const int v = __builtin_ctz(m);
                const USeen u = uniform_seen(recs[j * V + v]);
                const TF *fv = fb + v * mapsz;
                const f32x4 a = Vec4<TF>::load(fv + u.o00), bb = Vec4<TF>::load(fv + u.o01);
                const f32x4 c = Vec4<TF>::load(fv + u.o10), d = Vec4<TF>::load(fv + u.o11);
#pragma unroll
                for (int i = 0; i < 4; ++i) ra[i].push(bilerp(a.v[i], bb.v[i], c.v[i], d.v[i], u.w00, u.w01, u.w10, u.w11));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) o.v[i] = ra[i].result(__builtin_popcount(bits));
            if (bits == 0u) o = f32x4{{0.f, 0.f, 0.f, 0.f}};         // seen by no view: zero
        }
        if (q_active) tile[j * tstride + lane] = o;
    }
    __syncthreads();

    const int vl = lane & (kSeenTile - 1), half = lane / kSeenTile;   // the store phase of k_fwd_gather
    const long long n = n0 + vl;
    if (n < N) {
        for (int qq = wave * 16 + half; qq < wave * 16 + 16; qq += 64 / kSeenTile) {
            const int cq = cg * kSeenQuads + qq;
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
// det_fixed(.., K[b][c]) into the int64 one (k_bwd_gather_det; kexp null otherwise).  A view that does not see the voxel receives nothing.
template <typename TF, typename TO, int METHOD, int VT, typename ACC>
__global__ void __launch_bounds__(256)
k_bwd_gather_seen(const TO *__restrict__ grad_out, const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords,
                  ACC *__restrict__ gradT, const int *__restrict__ kexp, int Vrt, int C, int C4, int H, int W, long long N,
                  const int *__restrict__ nvs)
{
    constexpr bool DET = sizeof(ACC) == 8;
    const int V = VT > 0 ? VT : Vrt;
    const int b = blockIdx.y, cg = blockIdx.z;
    const int nvb = nvs ? nvs[b] : V;                         // present views; none: nothing to scatter
    if (nvb == 0) return;
    extern __shared__ __align__(16) unsigned char smem[];
    SeenRec *recs = reinterpret_cast<SeenRec *>(smem);
    unsigned *vbits = reinterpret_cast<unsigned *>(smem + sizeof(SeenRec) * kSeenTile * V);
    float *gtile = reinterpret_cast<float *>(smem + seen_head_bytes(V));                 // [256 ch][kSeenTile + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n0 = (long long)blockIdx.x * kSeenTile;
    const long long mapsz = (long long)H * W * C4;

    {   // grad_out tile, coalesced along voxels: the two half-waves load alternate channels (published by build_seen_records' barriers)
        const int vl = lane & (kSeenTile - 1), half = lane / kSeenTile;
        const long long n = n0 + vl;
        for (int r = wave * 64 + half; r < wave * 64 + 64; r += 64 / kSeenTile) {
            const int c = cg * kSeenCh + r;
            float g = 0.f;
            if (c < C && n < N) g = to_f32<TO>(grad_out[((long long)b * C + c) * N + n]);
            gtile[r * (kSeenTile + 1) + vl] = g;
        }
    }
    build_seen_records(recs, vbits, proj, coords, b, V, nvb, n0, N, H, W, C4);

    int ch[4], kx[4];
    bool act[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = cg * kSeenCh + i * 64 + lane;
        act[i] = c < C;
        ch[i] = act[i] ? c : 0;
        kx[i] = 0;
        if constexpr (DET) {
            kx[i] = act[i] ? kexp[(long long)b * C + ch[i]] : kDetPoison;
            act[i] = act[i] && kx[i] != kDetPoison;                             // a poisoned channel adds nothing
        }
    }
    const TF *fb = featT + (long long)b * V * mapsz;
    ACC *gb = gradT + (long long)b * V * mapsz;

    // (a seen view's taps all lie inside the map; a tap of weight 0 -- ix or iy a whole number -- still reads a valid pixel)
    auto sample4 = [&](const USeen &u, int v, float (&sv)[4]) {
        const TF *fv = fb + v * mapsz;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            sv[i] = bilerp(to_f32<TF>(fv[u.o00 + ch[i]]), to_f32<TF>(fv[u.o01 + ch[i]]), to_f32<TF>(fv[u.o10 + ch[i]]),
                           to_f32<TF>(fv[u.o11 + ch[i]]), u.w00, u.w01, u.w10, u.w11);
    };
    auto add = [&](ACC *at, float x, int k) {
        if constexpr (DET) atomicAdd(at, det_fixed(x, k));
        else atomicAdd(at, x);
    };
    auto scatter4 = [&](const USeen &u, int v, const float (&dsv)[4]) {
        ACC *gv = gb + v * mapsz;
        // zero-weight taps receive nothing -- wave-uniform branches
        if (u.w00 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o00 + ch[i], dsv[i] * u.w00, kx[i]); }
        if (u.w01 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o01 + ch[i], dsv[i] * u.w01, kx[i]); }
        if (u.w10 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o10 + ch[i], dsv[i] * u.w10, kx[i]); }
        if (u.w11 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o11 + ch[i], dsv[i] * u.w11, kx[i]); }
    };

    for (int jj = 0; jj < kSeenTile / 4; ++jj) {
        const int j = wave * (kSeenTile / 4) + jj;
        if (n0 + j >= N) break;
        const unsigned bits = (unsigned)uniform((int)vbits[j]);
        if (bits == 0u) continue;                                               // seen by no view: every gradient of the voxel is zero
        float g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = gtile[(i * 64 + lane) * (kSeenTile + 1) + j];

        if constexpr (VT > 0) {
            float s[4][VT], ds[4][VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                float sv[4] = {0.f, 0.f, 0.f, 0.f};
                if (bits >> v & 1u) sample4(uniform_seen(recs[j * VT + v]), v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i][v] = sv[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) seen_aggregate_grad<METHOD, VT>(s[i], g[i], ds[i], bits);
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                if (!(bits >> v & 1u)) continue;                                // an unseen view receives nothing
                const float dsv[4] = {ds[0][v], ds[1][v], ds[2][v], ds[3][v]};
                scatter4(uniform_seen(recs[j * VT + v]), v, dsv);
            }
        } else {
            // run-time view count: pass 1 accumulates the aggregate over the set bits, pass 2 re-samples and scatters
            RunningAgg<METHOD> ra[4];
            int am[4] = {0, 0, 0, 0};
            float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            const float cnt = (float)__builtin_popcount(bits);
#pragma unroll
            for (int i = 0; i < 4; ++i) ra[i].init();
            for (unsigned m = bits; m; m &= m - 1u) {
                const int v = __builtin_ctz(m);
                float sv[4];
                sample4(uniform_seen(recs[j * V + v]), v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ra[i].push(sv[i]);
                    if (sv[i] > best[i]) { best[i] = sv[i]; am[i] = v; }
                }
            }
            for (unsigned m = bits; m; m &= m - 1u) {
                const int v = __builtin_ctz(m);
                const USeen u = uniform_seen(recs[j * V + v]);
                float sv[4], dsv[4];
                sample4(u, v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if constexpr (METHOD == AGG_SUM) dsv[i] = g[i];
                    else if constexpr (METHOD == AGG_MEAN) dsv[i] = __fdiv_rn(g[i], cnt);
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

// ------------------------------------------------------------------------------------------ the bits themselves
// bits[b, n] bit v = view v is present (mask null: every view) and sees voxel n: one thread per voxel, views in order, one plain store
__global__ void __launch_bounds__(256)
k_view_visibility(const float *__restrict__ proj, const Coords coords, const uint8_t *__restrict__ mask, int *__restrict__ bits, int V, int H, int W,
                  long long N)
{
    const int b = blockIdx.y;
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float X0, X1, X2;
    voxel_xyz(coords, b, N, n, X0, X1, X2);
    int r = 0;
    for (int v = 0; v < V; ++v) {
        const bool present = !mask || mask[(long long)b * V + v] != 0;
        if (present && view_sees(proj + ((long long)b * V + v) * 12, X0, X1, X2, H, W)) r |= 1 << v;
    }
    bits[(long long)b * N + n] = r;
}

// ------------------------------------------------------------------------------------------ launchers
namespace {

size_t seen_head_host(int V) { return sizeof(SeenRec) * kSeenTile * (size_t)V + sizeof(unsigned) * kSeenTile; }

template <typename TF, typename TO, int METHOD>
hipError_t fwd_seen_v(const TF *featT, const float *proj, const Coords &coords, TO *out, const Problem &p, hipStream_t s)
{
    const int Q = p.C4 / 4;
    int tstride = (Q < kSeenQuads ? Q : kSeenQuads) + 1;
    tstride |= 1;
    const size_t lds = seen_head_host(p.V) + sizeof(f32x4) * kSeenTile * (size_t)tstride;
    const dim3 grid((unsigned)((p.N + kSeenTile - 1) / kSeenTile), (unsigned)p.B, (unsigned)((Q + kSeenQuads - 1) / kSeenQuads));
    auto go = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, featT, proj, coords, out, p.V, p.C, p.C4, p.H, p.W, p.N, tstride, p.view_count);
        return hipGetLastError();
    };
    switch (p.V) {
    case 2: return go(k_fwd_gather_seen<TF, TO, METHOD, 2>);
    case 4: return go(k_fwd_gather_seen<TF, TO, METHOD, 4>);
    case 8: return go(k_fwd_gather_seen<TF, TO, METHOD, 8>);
    default: return go(k_fwd_gather_seen<TF, TO, METHOD, 0>);
    }
}

template <typename TF, typename TO>
hipError_t fwd_seen_m(const TF *featT, const float *proj, const Coords &coords, TO *out, const Problem &p, hipStream_t s)
{
    switch (p.method) {
    case AGG_SOFTMAX: return fwd_seen_v<TF, TO, AGG_SOFTMAX>(featT, proj, coords, out, p, s);
    case AGG_SUM: return fwd_seen_v<TF, TO, AGG_SUM>(featT, proj, coords, out, p, s);
    case AGG_MEAN: return fwd_seen_v<TF, TO, AGG_MEAN>(featT, proj, coords, out, p, s);
    case AGG_MAX: return fwd_seen_v<TF, TO, AGG_MAX>(featT, proj, coords, out, p, s);
    }
    return hipErrorInvalidValue;
}

template <typename ACC, typename TF, typename TO, int METHOD>
hipError_t bwd_seen_v(const TO *go_, const TF *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                      hipStream_t s)
{
    const size_t lds = seen_head_host(p.V) + sizeof(float) * kSeenCh * (kSeenTile + 1);
    const dim3 grid((unsigned)((p.N + kSeenTile - 1) / kSeenTile), (unsigned)p.B, (unsigned)((p.C + kSeenCh - 1) / kSeenCh));
    auto go = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, go_, featT, proj, coords, gradT, kexp, p.V, p.C, p.C4, p.H, p.W, p.N, p.view_count);
        return hipGetLastError();
    };
    switch (p.V) {
    case 2: return go(k_bwd_gather_seen<TF, TO, METHOD, 2, ACC>);
    case 4: return go(k_bwd_gather_seen<TF, TO, METHOD, 4, ACC>);
    case 8: return go(k_bwd_gather_seen<TF, TO, METHOD, 8, ACC>);
    default: return go(k_bwd_gather_seen<TF, TO, METHOD, 0, ACC>);
    }
}

template <typename ACC, typename TF, typename TO>
hipError_t bwd_seen_m(const TO *go_, const TF *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                      hipStream_t s)
{
    switch (p.method) {
    case AGG_SOFTMAX: return bwd_seen_v<ACC, TF, TO, AGG_SOFTMAX>(go_, featT, proj, coords, gradT, kexp, p, s);
    case AGG_SUM: return bwd_seen_v<ACC, TF, TO, AGG_SUM>(go_, featT, proj, coords, gradT, kexp, p, s);
    case AGG_MEAN: return bwd_seen_v<ACC, TF, TO, AGG_MEAN>(go_, featT, proj, coords, gradT, kexp, p, s);
    case AGG_MAX: return bwd_seen_v<ACC, TF, TO, AGG_MAX>(go_, featT, proj, coords, gradT, kexp, p, s);
    }
    return hipErrorInvalidValue;
}

template <typename ACC>
hipError_t bwd_seen(const void *grad_out, const void *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                    hipStream_t s)
{
    if (p.out_bf16) return p.feat_f16 ? hipErrorNotSupported : bwd_seen_m((const bf16_t *)grad_out, (const float *)featT, proj, coords, gradT, kexp, p, s);
    if (!p.feat_f16 && !p.out_f16) return bwd_seen_m((const float *)grad_out, (const float *)featT, proj, coords, gradT, kexp, p, s);
    if (p.feat_f16 && p.out_f16) return bwd_seen_m((const __half *)grad_out, (const __half *)featT, proj, coords, gradT, kexp, p, s);
    if (p.feat_f16 && !p.out_f16) return bwd_seen_m((const float *)grad_out, (const __half *)featT, proj, coords, gradT, kexp, p, s);
    return hipErrorNotSupported;
}

}  // namespace

hipError_t launch_fwd_gather_seen(const void *featT, const float *proj, const Coords &coords, void *out, const Problem &p, hipStream_t s)
{
    if (p.out_bf16) return p.feat_f16 ? hipErrorNotSupported : fwd_seen_m((const float *)featT, proj, coords, (bf16_t *)out, p, s);
    if (!p.feat_f16 && !p.out_f16) return fwd_seen_m((const float *)featT, proj, coords, (float *)out, p, s);
    if (p.feat_f16 && p.out_f16) return fwd_seen_m((const __half *)featT, proj, coords, (__half *)out, p, s);
    if (p.feat_f16 && !p.out_f16) return fwd_seen_m((const __half *)featT, proj, coords, (float *)out, p, s);
    return hipErrorNotSupported;
}

hipError_t launch_bwd_gather_seen(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *gradT, const Problem &p,
                                  hipStream_t s)
{
    return bwd_seen<float>(grad_out, featT, proj, coords, gradT, nullptr, p, s);
}

hipError_t launch_bwd_gather_seen_det(const void *grad_out, const void *featT, const float *proj, const Coords &coords, unsigned long long *gradI,
                                      const int *kexp, const Problem &p, hipStream_t s)
{
    return bwd_seen<unsigned long long>(grad_out, featT, proj, coords, gradI, kexp, p, s);
}

hipError_t launch_view_visibility(const float *proj, const Coords &coords, const uint8_t *mask, int *bits, const Problem &p, hipStream_t s)
{
    hipLaunchKernelGGL(k_view_visibility, dim3((unsigned)((p.N + 255) / 256), (unsigned)p.B), dim3(256), 0, s, proj, coords, mask, bits, p.V, p.H, p.W,
                       p.N);
    return hipGetLastError();
}

}  // namespace mvhmr
