// Cross-view variance (include/mvhmr_unproject.h: the *_moments entry points): the volume holds the population variance of the
// participating views' samples, alone ('var', HALVES = 1) or behind their mean ('meanvar', HALVES = 2: channels [0, C) the mean, [C, 2C) the
// variance).  With S the participating views of one (voxel, channel), n = |S| and s_v the per-view bilinear samples:
//     mu  = (sum_S s_v) / n              acc = 0; acc = fadd(acc, s_v) in view order; fdiv(acc, n)
//     var = (sum_S (s_v - mu)^2) / n     d_v = fsub(s_v, mu); acc = 0; acc = fmaf(d_v, d_v, acc) in view order; fdiv(acc, n)
// the two-pass form around the ROUNDED mu: non-negative by construction, exactly 0 for n = 1; n = 0 gives 0 for both halves.  The gradient is
//     ds_v = fmaf(fdiv(2 g_v, n), d_v, fdiv(g_m, n))  for v in S, exactly 0 outside S
// (the term through mu vanishes: sum_S (s_u - mu) = 0).  S is every present view (VISIBLE = false: a view behind the camera or outside the map
// takes part with its sample of zero, as in the reference's mean) or the present views that see the voxel (VISIBLE = true: view_sees).
//
// k_fwd_gather_moments and k_bwd_gather_moments are k_fwd_gather_seen / k_bwd_gather_seen (unproject_visible.hip: same block, same three
// phases) -- copies, not template flags: those kernels' instances keep the code they had.  What differs:
//   phase 1  VISIBLE = false sets the bit of every present slot and builds the taps with make_taps whether or not the view sees the voxel
//   phase 2  every feature tap is read once per (voxel, view, channel quad) and serves both statistics; the run-time instances (V not 2, 4 or
//            8) sample again in a second pass instead of holding 16 samples per channel: the same operations in the same order, the same bits
//   phase 3  meanvar stores two tiles (a doubled LDS tile: DESIGN.md 5.14 has the occupancy), each in the 128-B-run shape of k_fwd_gather
// k_bwd_gather_moments serves both modes of the feature backward (float atomics / int64 fixed point) and loads one or two grad_out tiles.
#include "device_common.h"
#include "det_scale.h"
#include "kernels.h"

namespace mvhmr {

namespace {

constexpr int kMomTile = 32;           // voxels per block (k_fwd_gather's tile)
constexpr int kMomQuads = 64;          // 64 lanes x 4 channels
constexpr int kMomCh = 256;

struct alignas(16) MomRec {
    int o00, o01, o10, o11;            // element offsets (pixel * C4) inside one (b,v) channels-last map
    float w00, w01, w10, w11;
};
struct UMom { int o00, o01, o10, o11; float w00, w01, w10, w11; };
__device__ __forceinline__ UMom uniform_mom(const MomRec &r)
{
    UMom u;
    u.o00 = uniform(r.o00); u.o01 = uniform(r.o01); u.o10 = uniform(r.o10); u.o11 = uniform(r.o11);
    u.w00 = uniform(r.w00); u.w01 = uniform(r.w01); u.w10 = uniform(r.w10); u.w11 = uniform(r.w11);
    return u;
}
__device__ __forceinline__ bool no_taps(const UMom &u) { return u.w00 == 0.f && u.w01 == 0.f && u.w10 == 0.f && u.w11 == 0.f; }

// LDS: [ tap records (voxel, view) | bitmask, one word per voxel | the kernel's tiles ]
__device__ __forceinline__ size_t mom_head_bytes(int V) { return sizeof(MomRec) * kMomTile * V + sizeof(unsigned) * kMomTile; }

// phase 1: records and bitmask of the tile at n0; nvb slots are present.  Bit v = slot v takes part for the voxel: present and (VISIBLE) seeing
// it.  A participating view whose sample is identically zero keeps the empty record (make_taps).  Ends with the barrier that publishes both.
template <bool VISIBLE>
__device__ __forceinline__ void build_mom_records(MomRec *recs, unsigned *vbits, const float *__restrict__ proj, const Coords &coords, int b, int V,
                                                  int nvb, long long n0, long long N, int H, int W, int C4)
{
    if (threadIdx.x < kMomTile) vbits[threadIdx.x] = 0u;
    __syncthreads();
    for (int idx = threadIdx.x; idx < kMomTile * V; idx += blockDim.x) {
        const int v = idx / kMomTile, j = idx % kMomTile;
        long long n = n0 + j;
        n = n < N ? n : N - 1;       // tail voxels are computed and dropped
        float X0, X1, X2;
        voxel_xyz(coords, b, N, n, X0, X1, X2);
        const float *P = proj + ((long long)b * V + v) * 12;
        const bool part = v < nvb && (!VISIBLE || view_sees(P, X0, X1, X2, H, W));
        MomRec r;
        r.o00 = r.o01 = r.o10 = r.o11 = 0;
        r.w00 = r.w01 = r.w10 = r.w11 = 0.f;
        if (part) {
            const Taps t = make_taps(P, X0, X1, X2, H, W);       // clamped into the map whatever the position
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

// the pinned arithmetic over the set bits of a fixed-V instance; bits != 0
template <int V>
__device__ __forceinline__ float mom_mean(const float (&s)[V], unsigned bits, float cnt)
{
    float acc = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) acc = (bits >> v & 1u) ? __fadd_rn(acc, s[v]) : acc;
    return __fdiv_rn(acc, cnt);
}
template <int V>
__device__ __forceinline__ float mom_var(const float (&s)[V], unsigned bits, float cnt, float mu)
{
    float acc = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const float d = __fsub_rn(s[v], mu);
        acc = (bits >> v & 1u) ? __fmaf_rn(d, d, acc) : acc;
    }
    return __fdiv_rn(acc, cnt);
}


}  // namespace

// ------------------------------------------------------------------------------------------ forward
template <typename TF, typename TO, int VT, bool VISIBLE, int HALVES>
__global__ void __launch_bounds__(256)
k_fwd_gather_moments(const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords, TO *__restrict__ out, int Vrt, int C, int C4,
                     int H, int W, long long N, int tstride, const int *__restrict__ nvs)
{
    const int V = VT > 0 ? VT : Vrt;
    const int b = blockIdx.y, cg = blockIdx.z;
    const int nvb = nvs ? nvs[b] : V;                         // present views of this sample (block-uniform)
    extern __shared__ __align__(16) unsigned char smem[];
    MomRec *recs = reinterpret_cast<MomRec *>(smem);
    unsigned *vbits = reinterpret_cast<unsigned *>(smem + sizeof(MomRec) * kMomTile * V);
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem + mom_head_bytes(V));      // the variance; meanvar: the mean behind it
    f32x4 *tile_mu = tile + kMomTile * tstride;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n0 = (long long)blockIdx.x * kMomTile;
    const long long mapsz = (long long)H * W * C4;
    const int Q = C4 >> 2;

    build_mom_records<VISIBLE>(recs, vbits, proj, coords, b, V, nvb, n0, N, H, W, C4);

    int q = cg * kMomQuads + lane;
    const bool q_active = q < Q;
    q = q_active ? q : Q - 1;                                // idle lanes shadow the last quad and write nothing
    const TF *fb = featT + (long long)b * V * mapsz + q * 4;

    // one view's samples of the lane's four channels; a sample that is identically zero reads nothing (its dummy taps must not turn a
    // non-finite pixel (0, 0) into 0 * Inf), as in k_fwd_gather: a wave-uniform branch
    auto sample4 = [&](const UMom &u, int v, float (&sv)[4]) {
        if (!VISIBLE && no_taps(u)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sv[i] = 0.f;
            return;
        }
        const TF *fv = fb + v * mapsz;
        const f32x4 a = Vec4<TF>::load(fv + u.o00), bb = Vec4<TF>::load(fv + u.o01);
        const f32x4 c = Vec4<TF>::load(fv + u.o10), d = Vec4<TF>::load(fv + u.o11);
#pragma unroll
        for (int i = 0; i < 4; ++i) sv[i] = bilerp(a.v[i], bb.v[i], c.v[i], d.v[i], u.w00, u.w01, u.w10, u.w11);
    };

    for (int jj = 0; jj < kMomTile / 4; ++jj) {
        const int j = wave * (kMomTile / 4) + jj;
        const unsigned bits = (unsigned)uniform((int)vbits[j]);      // the views that take part for this voxel: wave-uniform
        const float cnt = (float)__builtin_popcount(bits);
        f32x4 mu = f32x4{{0.f, 0.f, 0.f, 0.f}}, var = f32x4{{0.f, 0.f, 0.f, 0.f}};     // no view takes part: zero
        if (bits != 0u) {
            if constexpr (VT > 0) {
                float s[4][VT];
#pragma unroll
                for (int v = 0; v < VT; ++v) {
                    float sv[4] = {0.f, 0.f, 0.f, 0.f};
                    if (bits >> v & 1u) sample4(uniform_mom(recs[j * VT + v]), v, sv);      // scalar branch: an absent view loads nothing
#pragma unroll
                    for (int i = 0; i < 4; ++i) s[i][v] = sv[i];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    mu.v[i] = mom_mean<VT>(s[i], bits, cnt);
                    var.v[i] = mom_var<VT>(s[i], bits, cnt, mu.v[i]);
                }
            } else {
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
                for (unsigned m = bits; m; m &= m - 1u) {            // set bits in view order
                    const int v = __builtin_ctz(m);
                    float sv[4];
                    sample4(uniform_mom(recs[j * V + v]), v, sv);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = __fadd_rn(acc[i], sv[i]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) { mu.v[i] = __fdiv_rn(acc[i], cnt); acc[i] = 0.f; }
                for (unsigned m = bits; m; m &= m - 1u) {            // second pass: the same samples again
                    const int v = __builtin_ctz(m);
                    float sv[4];
                    sample4(uniform_mom(recs[j * V + v]), v, sv);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float d = __fsub_rn(sv[i], mu.v[i]);
                        acc[i] = __fmaf_rn(d, d, acc[i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) var.v[i] = __fdiv_rn(acc[i], cnt);
            }
        }
        if (q_active) {
            tile[j * tstride + lane] = var;
            if constexpr (HALVES == 2) tile_mu[j * tstride + lane] = mu;
        }
    }
    __syncthreads();

    const int vl = lane & (kMomTile - 1), half = lane / kMomTile;    // the store phase of k_fwd_gather, once per half
    const long long n = n0 + vl;
    const int CO = HALVES * C;
    if (n < N) {
#pragma unroll
        for (int h = 0; h < HALVES; ++h) {
            const f32x4 *src = (HALVES == 2 && h == 0) ? tile_mu : tile;
            const int coff = (HALVES == 2 && h == 1) ? C : 0;
            for (int qq = wave * 16 + half; qq < wave * 16 + 16; qq += 64 / kMomTile) {
                const int cq = cg * kMomQuads + qq;
                if (cq >= Q) break;
                const f32x4 t = src[vl * tstride + qq];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = cq * 4 + i;
                    if (c < C) store_streaming(&out[((long long)b * CO + coff + c) * N + n], t.v[i]);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ feature backward, both modes
// ACC = float adds ds * tap weight with float atomics into the channels-last fp32 gradient, ACC = unsigned long long adds det_fixed(.., K[b][c])
// into the int64 one (kexp null otherwise).  A view that takes no part for the voxel receives nothing.
template <typename TF, typename TO, int VT, bool VISIBLE, int HALVES, typename ACC>
__global__ void __launch_bounds__(256)
k_bwd_gather_moments(const TO *__restrict__ grad_out, const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords,
                     ACC *__restrict__ gradT, const int *__restrict__ kexp, int Vrt, int C, int C4, int H, int W, long long N,
                     const int *__restrict__ nvs)
{
    constexpr bool DET = sizeof(ACC) == 8;
    constexpr int kLd = kMomTile + 1;
    const int V = VT > 0 ? VT : Vrt;
    const int b = blockIdx.y, cg = blockIdx.z;
    const int nvb = nvs ? nvs[b] : V;                         // present views; none: nothing to scatter
    if (nvb == 0) return;
    extern __shared__ __align__(16) unsigned char smem[];
    MomRec *recs = reinterpret_cast<MomRec *>(smem);
    unsigned *vbits = reinterpret_cast<unsigned *>(smem + sizeof(MomRec) * kMomTile * V);
    float *gtile = reinterpret_cast<float *>(smem + mom_head_bytes(V));                  // g_v [256 ch][kMomTile + 1]; meanvar: g_m behind it
    float *gtile_mu = gtile + kMomCh * kLd;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n0 = (long long)blockIdx.x * kMomTile;
    const long long mapsz = (long long)H * W * C4;
    const int CO = HALVES * C;

    {   // grad_out tiles, coalesced along voxels: the two half-waves load alternate channels (published by build_mom_records' barriers)
        const int vl = lane & (kMomTile - 1), half = lane / kMomTile;
        const long long n = n0 + vl;
        for (int r = wave * 64 + half; r < wave * 64 + 64; r += 64 / kMomTile) {
            const int c = cg * kMomCh + r;
            float gv = 0.f, gm = 0.f;
            if (c < C && n < N) {
                gv = to_f32<TO>(grad_out[((long long)b * CO + (HALVES == 2 ? C : 0) + c) * N + n]);
                if constexpr (HALVES == 2) gm = to_f32<TO>(grad_out[((long long)b * CO + c) * N + n]);
            }
            gtile[r * kLd + vl] = gv;
            if constexpr (HALVES == 2) gtile_mu[r * kLd + vl] = gm;
        }
    }
    build_mom_records<VISIBLE>(recs, vbits, proj, coords, b, V, nvb, n0, N, H, W, C4);

    int ch[4], kx[4];
    bool act[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = cg * kMomCh + i * 64 + lane;
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

    // (every record's taps lie inside the map: make_taps clamps them; a sample that is identically zero reads nothing)
    auto sample4 = [&](const UMom &u, int v, float (&sv)[4]) {
        if (!VISIBLE && no_taps(u)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sv[i] = 0.f;
            return;
        }
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
    auto scatter4 = [&](const UMom &u, int v, const float (&dsv)[4]) {
        ACC *gv = gb + v * mapsz;
        // zero-weight taps receive nothing -- wave-uniform branches
        if (u.w00 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o00 + ch[i], dsv[i] * u.w00, kx[i]); }
        if (u.w01 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o01 + ch[i], dsv[i] * u.w01, kx[i]); }
        if (u.w10 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o10 + ch[i], dsv[i] * u.w10, kx[i]); }
        if (u.w11 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o11 + ch[i], dsv[i] * u.w11, kx[i]); }
    };

    for (int jj = 0; jj < kMomTile / 4; ++jj) {
        const int j = wave * (kMomTile / 4) + jj;
        if (n0 + j >= N) break;
        const unsigned bits = (unsigned)uniform((int)vbits[j]);
        if (bits == 0u) continue;                                               // no view takes part: every gradient of the voxel is zero
        const float cnt = (float)__builtin_popcount(bits);
        float gvn[4], gmn[4];                                                   // 2 g_v / n and g_m / n
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            gvn[i] = __fdiv_rn(__fmul_rn(2.f, gtile[(i * 64 + lane) * kLd + j]), cnt);
            gmn[i] = HALVES == 2 ? __fdiv_rn(gtile_mu[(i * 64 + lane) * kLd + j], cnt) : 0.f;
        }

        if constexpr (VT > 0) {
            float s[4][VT], mu[4];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                float sv[4] = {0.f, 0.f, 0.f, 0.f};
                if (bits >> v & 1u) sample4(uniform_mom(recs[j * VT + v]), v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i][v] = sv[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) mu[i] = mom_mean<VT>(s[i], bits, cnt);
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                if (!(bits >> v & 1u)) continue;                                // a view outside S receives nothing
                float dsv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) dsv[i] = __fmaf_rn(gvn[i], __fsub_rn(s[i][v], mu[i]), gmn[i]);
                scatter4(uniform_mom(recs[j * VT + v]), v, dsv);
            }
        } else {
            // run-time view count: pass 1 accumulates the mean over the set bits, pass 2 samples again and scatters
            float acc[4] = {0.f, 0.f, 0.f, 0.f}, mu[4];
            for (unsigned m = bits; m; m &= m - 1u) {
                const int v = __builtin_ctz(m);
                float sv[4];
                sample4(uniform_mom(recs[j * V + v]), v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __fadd_rn(acc[i], sv[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) mu[i] = __fdiv_rn(acc[i], cnt);
            for (unsigned m = bits; m; m &= m - 1u) {
                const int v = __builtin_ctz(m);
                const UMom u = uniform_mom(recs[j * V + v]);
                float sv[4], dsv[4];
                sample4(u, v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) dsv[i] = __fmaf_rn(gvn[i], __fsub_rn(sv[i], mu[i]), gmn[i]);
                scatter4(u, v, dsv);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ launchers
namespace {

size_t mom_head_host(int V) { return sizeof(MomRec) * kMomTile * (size_t)V + sizeof(unsigned) * kMomTile; }

template <typename TF, typename TO, bool VISIBLE, int HALVES>
hipError_t fwd_mom_v(const TF *featT, const float *proj, const Coords &coords, TO *out, const Problem &p, hipStream_t s)
{
    const int Q = p.C4 / 4;
    int tstride = (Q < kMomQuads ? Q : kMomQuads) + 1;
    tstride |= 1;
    const size_t lds = mom_head_host(p.V) + sizeof(f32x4) * kMomTile * (size_t)tstride * HALVES;
    const dim3 grid((unsigned)((p.N + kMomTile - 1) / kMomTile), (unsigned)p.B, (unsigned)((Q + kMomQuads - 1) / kMomQuads));
    auto go = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, featT, proj, coords, out, p.V, p.C, p.C4, p.H, p.W, p.N, tstride, p.view_count);
        return hipGetLastError();
    };
    switch (p.V) {
    case 2: return go(k_fwd_gather_moments<TF, TO, 2, VISIBLE, HALVES>);
    case 4: return go(k_fwd_gather_moments<TF, TO, 4, VISIBLE, HALVES>);
    case 8: return go(k_fwd_gather_moments<TF, TO, 8, VISIBLE, HALVES>);
    default: return go(k_fwd_gather_moments<TF, TO, 0, VISIBLE, HALVES>);
    }
}

template <typename TF, typename TO>
hipError_t fwd_mom_m(const TF *featT, const float *proj, const Coords &coords, TO *out, const Problem &p, hipStream_t s)
{
    if (p.moments == 1) return p.visible ? fwd_mom_v<TF, TO, true, 1>(featT, proj, coords, out, p, s) : fwd_mom_v<TF, TO, false, 1>(featT, proj, coords, out, p, s);
    if (p.moments == 2) return p.visible ? fwd_mom_v<TF, TO, true, 2>(featT, proj, coords, out, p, s) : fwd_mom_v<TF, TO, false, 2>(featT, proj, coords, out, p, s);
    return hipErrorInvalidValue;
}

template <typename ACC, typename TF, typename TO, bool VISIBLE, int HALVES>
hipError_t bwd_mom_v(const TO *go_, const TF *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                     hipStream_t s)
{
    const size_t lds = mom_head_host(p.V) + sizeof(float) * kMomCh * (kMomTile + 1) * HALVES;
    const dim3 grid((unsigned)((p.N + kMomTile - 1) / kMomTile), (unsigned)p.B, (unsigned)((p.C + kMomCh - 1) / kMomCh));
    auto go = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, go_, featT, proj, coords, gradT, kexp, p.V, p.C, p.C4, p.H, p.W, p.N, p.view_count);
        return hipGetLastError();
    };
    switch (p.V) {
    case 2: return go(k_bwd_gather_moments<TF, TO, 2, VISIBLE, HALVES, ACC>);
    case 4: return go(k_bwd_gather_moments<TF, TO, 4, VISIBLE, HALVES, ACC>);
    case 8: return go(k_bwd_gather_moments<TF, TO, 8, VISIBLE, HALVES, ACC>);
    default: return go(k_bwd_gather_moments<TF, TO, 0, VISIBLE, HALVES, ACC>);
    }
}

template <typename ACC, typename TF, typename TO>
hipError_t bwd_mom_m(const TO *go_, const TF *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                     hipStream_t s)
{
    if (p.moments == 1)
        return p.visible ? bwd_mom_v<ACC, TF, TO, true, 1>(go_, featT, proj, coords, gradT, kexp, p, s)
                         : bwd_mom_v<ACC, TF, TO, false, 1>(go_, featT, proj, coords, gradT, kexp, p, s);
    if (p.moments == 2)
        return p.visible ? bwd_mom_v<ACC, TF, TO, true, 2>(go_, featT, proj, coords, gradT, kexp, p, s)
                         : bwd_mom_v<ACC, TF, TO, false, 2>(go_, featT, proj, coords, gradT, kexp, p, s);
    return hipErrorInvalidValue;
}

template <typename ACC>
hipError_t bwd_mom(const void *grad_out, const void *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                   hipStream_t s)
{
    if (p.out_bf16) return p.feat_f16 ? hipErrorNotSupported : bwd_mom_m((const bf16_t *)grad_out, (const float *)featT, proj, coords, gradT, kexp, p, s);
    if (!p.feat_f16 && !p.out_f16) return bwd_mom_m((const float *)grad_out, (const float *)featT, proj, coords, gradT, kexp, p, s);
    if (p.feat_f16 && p.out_f16) return bwd_mom_m((const __half *)grad_out, (const __half *)featT, proj, coords, gradT, kexp, p, s);
    if (p.feat_f16 && !p.out_f16) return bwd_mom_m((const float *)grad_out, (const __half *)featT, proj, coords, gradT, kexp, p, s);
    return hipErrorNotSupported;
}

}  // namespace

hipError_t launch_fwd_gather_moments(const void *featT, const float *proj, const Coords &coords, void *out, const Problem &p, hipStream_t s)
{
    if (p.out_bf16) return p.feat_f16 ? hipErrorNotSupported : fwd_mom_m((const float *)featT, proj, coords, (bf16_t *)out, p, s);
    if (!p.feat_f16 && !p.out_f16) return fwd_mom_m((const float *)featT, proj, coords, (float *)out, p, s);
    if (p.feat_f16 && p.out_f16) return fwd_mom_m((const __half *)featT, proj, coords, (__half *)out, p, s);
    if (p.feat_f16 && !p.out_f16) return fwd_mom_m((const __half *)featT, proj, coords, (float *)out, p, s);
    return hipErrorNotSupported;
}

hipError_t launch_bwd_gather_moments(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *gradT, const Problem &p,
                                     hipStream_t s)
{
    return bwd_mom<float>(grad_out, featT, proj, coords, gradT, nullptr, p, s);
}

hipError_t launch_bwd_gather_moments_det(const void *grad_out, const void *featT, const float *proj, const Coords &coords, unsigned long long *gradI,
                                         const int *kexp, const Problem &p, hipStream_t s)
{
    return bwd_mom<unsigned long long>(grad_out, featT, proj, coords, gradI, kexp, p, s);
}

}  // namespace mvhmr
