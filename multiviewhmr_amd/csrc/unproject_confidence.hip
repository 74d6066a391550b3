// Per-pixel view confidence maps (include/mvhmr_unproject.h: the *_confidence entry points): every view carries an fp32 map
// (B, V, Hf, Wf) that is sampled at the voxel with the very taps and weights of the view's features -- one more channel -- and every voxel
// aggregates its views weighted by that sample c_v.  A view takes part for a voxel iff it is present (slot < nvs[b]), c_v > 0 and, with
// Problem::visible, it sees the voxel (view_sees); every other view is not read for that voxel and receives exact zeros.
//
// k_fwd_gather_conf and k_bwd_gather_conf are k_fwd_gather_seen / k_bwd_gather_seen (unproject_visible.hip: same block, same three phases)
// -- copies, not template flags: those kernels' instances keep the code they had.  What differs:
//   phase 1  the thread of (voxel, view) also samples the confidence map (four fp32 loads, bilerp; a tap outside the map has the value 0),
//            keeps c_v in a float array beside the tap records and ORs the presence bit into the voxel's bitmask in LDS
//   phase 2  the wave reads the bitmask and the c_v wave-uniformly; conf_aggregate / conf_aggregate_grad range over the set bits
// k_bwd_gather_conf serves both modes of the feature backward (float atomics / int64 fixed point).  The deterministic scale pass bounds the
// sum's |ds| = |g| c_v by max |g| times the sample's largest confidence pixel (a bilinear sample never exceeds the largest tap).
//
// grad_confidence (launch_conf_grad) is bitwise reproducible in every mode and uses no float atomics: the geometry kernel
// (unproject_confidence_geom.hip) writes the (B, V, N) fp32 stream of sum_channels dc_v in a fixed order; here one pass takes the largest
// magnitude per (b, v) with integer atomicMax, which fixes one power-of-two exponent K per (b, v) with N * max * 2^K < 2^62; the scatter adds
// det_fixed(dc * tap weight, K) into an int64 map with integer atomics (associative: the same bits in any arrival order); a last pass
// writes every element of the fp32 gradient.
#include "device_common.h"
#include "det_scale.h"
#include "kernels.h"

namespace mvhmr {

namespace {

constexpr int kConfTile = 32;          // voxels per block (k_fwd_gather's tile)
constexpr int kConfQuads = 64;         // 64 lanes x 4 channels
constexpr int kConfCh = 256;

struct alignas(16) ConfRec {
    int o00, o01, o10, o11;            // element offsets (pixel * C4) inside one (b,v) channels-last map
    float w00, w01, w10, w11;
};
struct UConf { int o00, o01, o10, o11; float w00, w01, w10, w11; };
__device__ __forceinline__ UConf uniform_conf(const ConfRec &r)
{
    UConf u;
    u.o00 = uniform(r.o00); u.o01 = uniform(r.o01); u.o10 = uniform(r.o10); u.o11 = uniform(r.o11);
    u.w00 = uniform(r.w00); u.w01 = uniform(r.w01); u.w10 = uniform(r.w10); u.w11 = uniform(r.w11);
    return u;
}

// LDS: [ tap records (voxel, view) | c (voxel, view) | bitmask, one word per voxel | the kernel's tile ]
__device__ __forceinline__ size_t conf_head_bytes(int V) { return (sizeof(ConfRec) + sizeof(float)) * kConfTile * V + sizeof(unsigned) * kConfTile; }

// phase 1: records, confidences and bitmask of the tile at n0; nvb slots are present.  Ends with the barrier that publishes them.
__device__ __forceinline__ void build_conf_records(ConfRec *recs, float *cw, unsigned *vbits, const float *__restrict__ proj, const Coords &coords,
                                                   const float *__restrict__ conf, int b, int V, int nvb, long long n0, long long N, int H, int W, int C4,
                                                   int visible)
{
    if (threadIdx.x < kConfTile) vbits[threadIdx.x] = 0u;
    __syncthreads();
    for (int idx = threadIdx.x; idx < kConfTile * V; idx += blockDim.x) {
        const int v = idx / kConfTile, j = idx % kConfTile;
        long long n = n0 + j;
        n = n < N ? n : N - 1;       // tail voxels are computed and dropped
        float X0, X1, X2;
        voxel_xyz(coords, b, N, n, X0, X1, X2);
        const float *P = proj + ((long long)b * V + v) * 12;
        ConfRec r;
        r.o00 = r.o01 = r.o10 = r.o11 = 0;
        r.w00 = r.w01 = r.w10 = r.w11 = 0.f;
        float c = 0.f;
        if (v < nvb && (!visible || view_sees(P, X0, X1, X2, H, W))) {
            const Taps t = make_taps(P, X0, X1, X2, H, W);
            c = sample_conf(conf + ((long long)b * V + v) * H * W, t, H, W);
            if (c > 0.f) {                                                        // (zero, negative, NaN: absent)
                r.o00 = (t.y0 * W + t.x0) * C4;
                r.o01 = (t.y0 * W + t.x1) * C4;
                r.o10 = (t.y1 * W + t.x0) * C4;
                r.o11 = (t.y1 * W + t.x1) * C4;
                r.w00 = t.w00; r.w01 = t.w01; r.w10 = t.w10; r.w11 = t.w11;
                atomicOr(&vbits[j], 1u << v);
            } else {
                c = 0.f;
            }
        }
        recs[j * V + v] = r;
        cw[j * V + v] = c;
    }
    __syncthreads();
}

}  // namespace

// ------------------------------------------------------------------------------------------ forward
template <typename TF, typename TO, int METHOD, int VT>
__global__ void __launch_bounds__(256)
k_fwd_gather_conf(const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords, const float *__restrict__ conf,
                  TO *__restrict__ out, int Vrt, int C, int C4, int H, int W, long long N, int tstride, const int *__restrict__ nvs, int visible)
{
    const int V = VT > 0 ? VT : Vrt;
    const int b = blockIdx.y, cg = blockIdx.z;
    const int nvb = nvs ? nvs[b] : V;                         // present views of this sample (block-uniform)
    extern __shared__ __align__(16) unsigned char smem[];
    ConfRec *recs = reinterpret_cast<ConfRec *>(smem);
    float *cw = reinterpret_cast<float *>(smem + sizeof(ConfRec) * kConfTile * V);
    unsigned *vbits = reinterpret_cast<unsigned *>(cw + kConfTile * V);
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem + conf_head_bytes(V));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n0 = (long long)blockIdx.x * kConfTile;
    const long long mapsz = (long long)H * W * C4;
    const int Q = C4 >> 2;

    build_conf_records(recs, cw, vbits, proj, coords, conf, b, V, nvb, n0, N, H, W, C4, visible);

    int q = cg * kConfQuads + lane;
    const bool q_active = q < Q;
    q = q_active ? q : Q - 1;                                // idle lanes shadow the last quad and write nothing
    const TF *fb = featT + (long long)b * V * mapsz + q * 4;

    for (int jj = 0; jj < kConfTile / 4; ++jj) {
        const int j = wave * (kConfTile / 4) + jj;
        const unsigned bits = (unsigned)uniform((int)vbits[j]);      // the views that take part for this voxel: wave-uniform
        f32x4 o;
        if constexpr (VT > 0) {
            float s[4][VT], c[VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                c[v] = 0.f;
                if (!(bits >> v & 1u)) {                             // scalar branch: an absent view loads nothing, not even its record
#pragma unroll
                    for (int i = 0; i < 4; ++i) s[i][v] = 0.f;
                    continue;
                }
                c[v] = uniform(cw[j * VT + v]);
                const UConf u = uniform_conf(recs[j * VT + v]);
                const TF *fv = fb + v * mapsz;
                const f32x4 a = Vec4<TF>::load(fv + u.o00), bb = Vec4<TF>::load(fv + u.o01);
                const f32x4 cc = Vec4<TF>::load(fv + u.o10), d = Vec4<TF>::load(fv + u.o11);
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i][v] = bilerp(a.v[i], bb.v[i], cc.v[i], d.v[i], u.w00, u.w01, u.w10, u.w11);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) o.v[i] = conf_aggregate<METHOD, VT>(s[i], c, bits);
        } else {
            WeightedRunningAgg<METHOD> ra[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) ra[i].init();
            for (unsigned m = bits; m; m &= m - 1u) {                // set bits in view order
                const int v = __builtin_ctz(m);
                const float c = uniform(cw[j * V + v]);
                const UConf u = uniform_conf(recs[j * V + v]);
                const TF *fv = fb + v * mapsz;
                const f32x4 a = Vec4<TF>::load(fv + u.o00), bb = Vec4<TF>::load(fv + u.o01);
                const f32x4 cc = Vec4<TF>::load(fv + u.o10), d = Vec4<TF>::load(fv + u.o11);
#pragma unroll
                for (int i = 0; i < 4; ++i) ra[i].push(bilerp(a.v[i], bb.v[i], cc.v[i], d.v[i], u.w00, u.w01, u.w10, u.w11), c);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) o.v[i] = ra[i].result();
            if (bits == 0u) o = f32x4{{0.f, 0.f, 0.f, 0.f}};         // no view takes part: zero
        }
        if (q_active) tile[j * tstride + lane] = o;
    }
    __syncthreads();

    const int vl = lane & (kConfTile - 1), half = lane / kConfTile;   // the store phase of k_fwd_gather
    const long long n = n0 + vl;
    if (n < N) {
        for (int qq = wave * 16 + half; qq < wave * 16 + 16; qq += 64 / kConfTile) {
            const int cq = cg * kConfQuads + qq;
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
// ACC = float adds ds * tap weight with float atomics into the channels-last fp32 gradient, ACC = unsigned long long adds
// det_fixed(.., K[b][c]) into the int64 one (kexp null otherwise).  A view that takes no part for the voxel receives nothing.
template <typename TF, typename TO, int METHOD, int VT, typename ACC>
__global__ void __launch_bounds__(256)
k_bwd_gather_conf(const TO *__restrict__ grad_out, const TF *__restrict__ featT, const float *__restrict__ proj, const Coords coords,
                  const float *__restrict__ conf, ACC *__restrict__ gradT, const int *__restrict__ kexp, int Vrt, int C, int C4, int H, int W,
                  long long N, const int *__restrict__ nvs, int visible)
{
    constexpr bool DET = sizeof(ACC) == 8;
    const int V = VT > 0 ? VT : Vrt;
    const int b = blockIdx.y, cg = blockIdx.z;
    const int nvb = nvs ? nvs[b] : V;                         // present views; none: nothing to scatter
    if (nvb == 0) return;
    extern __shared__ __align__(16) unsigned char smem[];
    ConfRec *recs = reinterpret_cast<ConfRec *>(smem);
    float *cw = reinterpret_cast<float *>(smem + sizeof(ConfRec) * kConfTile * V);
    unsigned *vbits = reinterpret_cast<unsigned *>(cw + kConfTile * V);
    float *gtile = reinterpret_cast<float *>(smem + conf_head_bytes(V));                 // [256 ch][kConfTile + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n0 = (long long)blockIdx.x * kConfTile;
    const long long mapsz = (long long)H * W * C4;

    {   // grad_out tile, coalesced along voxels: the two half-waves load alternate channels (published by build_conf_records' barriers)
        const int vl = lane & (kConfTile - 1), half = lane / kConfTile;
        const long long n = n0 + vl;
        for (int r = wave * 64 + half; r < wave * 64 + 64; r += 64 / kConfTile) {
            const int c = cg * kConfCh + r;
            float g = 0.f;
            if (c < C && n < N) g = to_f32<TO>(grad_out[((long long)b * C + c) * N + n]);
            gtile[r * (kConfTile + 1) + vl] = g;
        }
    }
    build_conf_records(recs, cw, vbits, proj, coords, conf, b, V, nvb, n0, N, H, W, C4, visible);

    int ch[4], kx[4];
    bool act[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = cg * kConfCh + i * 64 + lane;
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

    auto sample4 = [&](const UConf &u, int v, float (&sv)[4]) {
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
    auto scatter4 = [&](const UConf &u, int v, const float (&dsv)[4]) {
        ACC *gv = gb + v * mapsz;
        // zero-weight taps receive nothing -- wave-uniform branches
        if (u.w00 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o00 + ch[i], dsv[i] * u.w00, kx[i]); }
        if (u.w01 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o01 + ch[i], dsv[i] * u.w01, kx[i]); }
        if (u.w10 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o10 + ch[i], dsv[i] * u.w10, kx[i]); }
        if (u.w11 != 0.f) { for (int i = 0; i < 4; ++i) if (act[i]) add(gv + u.o11 + ch[i], dsv[i] * u.w11, kx[i]); }
    };

    for (int jj = 0; jj < kConfTile / 4; ++jj) {
        const int j = wave * (kConfTile / 4) + jj;
        if (n0 + j >= N) break;
        const unsigned bits = (unsigned)uniform((int)vbits[j]);
        if (bits == 0u) continue;                                               // no view takes part: every gradient of the voxel is zero
        float g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = gtile[(i * 64 + lane) * (kConfTile + 1) + j];

        if constexpr (VT > 0) {
            float s[4][VT], ds[4][VT], c[VT], dc[VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                float sv[4] = {0.f, 0.f, 0.f, 0.f};
                c[v] = 0.f;
                if (bits >> v & 1u) {
                    c[v] = uniform(cw[j * VT + v]);
                    sample4(uniform_conf(recs[j * VT + v]), v, sv);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i][v] = sv[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) conf_aggregate_grad<METHOD, VT>(s[i], c, g[i], ds[i], dc, bits);
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                if (!(bits >> v & 1u)) continue;                                // an absent view receives nothing
                const float dsv[4] = {ds[0][v], ds[1][v], ds[2][v], ds[3][v]};
                scatter4(uniform_conf(recs[j * VT + v]), v, dsv);
            }
        } else {
            // run-time view count: pass 1 accumulates the aggregate over the set bits, pass 2 re-samples and scatters
            WeightedRunningAgg<METHOD> ra[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) ra[i].init();
            for (unsigned m = bits; m; m &= m - 1u) {
                const int v = __builtin_ctz(m);
                const float c = uniform(cw[j * V + v]);
                float sv[4];
                sample4(uniform_conf(recs[j * V + v]), v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) ra[i].push(sv[i], c);
            }
            for (unsigned m = bits; m; m &= m - 1u) {
                const int v = __builtin_ctz(m);
                const float c = uniform(cw[j * V + v]);
                const UConf u = uniform_conf(recs[j * V + v]);
                float sv[4], dsv[4];
                sample4(u, v, sv);
#pragma unroll
                for (int i = 0; i < 4; ++i) dsv[i] = ra[i].grad(g[i], sv[i], c);
                scatter4(u, v, dsv);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ grad_confidence
// the exponent of one (b, v) from the bits of its largest |dc|: N * max * 2^K < 2^62; poison when the maximum is not finite
__device__ __forceinline__ int conf_grad_exponent(unsigned maxbits, int log2n)
{
    if (maxbits >= 0x7f800000u) return kDetPoison;
    const int e = (int)(maxbits >> 23) - 126;                                     // max < 2^e (a denormal maximum: < 2^-126)
    return 62 - log2n - e;
}

// thread per (voxel, slot): dc of the stream times the four tap weights, in fixed point, into the int64 map of (b, slot).  The taps are those
// the confidence was sampled with; a tap outside the map or of weight 0 receives nothing.  (dc != 0 only where the view took part.)
__global__ void __launch_bounds__(256) k_conf_grad_scatter(const float *__restrict__ stream, const unsigned *__restrict__ smax, const float *__restrict__ proj,
                                                           const Coords coords, unsigned long long *__restrict__ acc, int V, int H, int W, long long N,
                                                           int log2n)
{
    const long long bv = blockIdx.y;
    const int b = (int)(bv / V);
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float dc = stream[bv * N + n];
    if (dc == 0.f) return;
    const int k = conf_grad_exponent(smax[bv], log2n);
    if (k == kDetPoison) return;                                                  // the whole map of (b, v) is NaN (k_conf_grad_convert)
    float X0, X1, X2;
    voxel_xyz(coords, b, N, n, X0, X1, X2);
    const Taps t = make_taps(proj + bv * 12, X0, X1, X2, H, W);
    if (!t.any) return;
    unsigned long long *a = acc + bv * (long long)H * W;
    if (t.w00 != 0.f) atomicAdd(a + t.y0 * W + t.x0, det_fixed(dc * t.w00, k));   // (an outside tap has weight 0)
    if (t.w01 != 0.f) atomicAdd(a + t.y0 * W + t.x1, det_fixed(dc * t.w01, k));
    if (t.w10 != 0.f) atomicAdd(a + t.y1 * W + t.x0, det_fixed(dc * t.w10, k));
    if (t.w11 != 0.f) atomicAdd(a + t.y1 * W + t.x1, det_fixed(dc * t.w11, k));
}

// int64 map -> fp32 gradient, every element written (NaN for a poisoned (b, v))
__global__ void __launch_bounds__(256) k_conf_grad_convert(const unsigned long long *__restrict__ acc, const unsigned *__restrict__ smax,
                                                           float *__restrict__ grad_conf, long long HW, int log2n)
{
    const long long bv = blockIdx.y;
    const int k = conf_grad_exponent(smax[bv], log2n);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)gridDim.x * 256)
        grad_conf[bv * HW + i] = k == kDetPoison ? __builtin_nanf("") : (float)ldexp((double)(long long)acc[bv * HW + i], -k);
}

// ------------------------------------------------------------------------------------------ launchers
namespace {

size_t conf_head_host(int V) { return (sizeof(ConfRec) + sizeof(float)) * kConfTile * (size_t)V + sizeof(unsigned) * kConfTile; }
template <typename TF, typename TO, int METHOD>
hipError_t fwd_conf_v(const TF *featT, const float *proj, const Coords &coords, TO *out, const Problem &p, hipStream_t s)
{
    const int Q = p.C4 / 4;
    int tstride = (Q < kConfQuads ? Q : kConfQuads) + 1;
    tstride |= 1;
    const size_t lds = conf_head_host(p.V) + sizeof(f32x4) * kConfTile * (size_t)tstride;
    const dim3 grid((unsigned)((p.N + kConfTile - 1) / kConfTile), (unsigned)p.B, (unsigned)((Q + kConfQuads - 1) / kConfQuads));
    auto go = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, featT, proj, coords, p.confidence, out, p.V, p.C, p.C4, p.H, p.W, p.N, tstride, p.view_count,
                           p.visible);
        return hipGetLastError();
    };
    switch (p.V) {
    case 2: return go(k_fwd_gather_conf<TF, TO, METHOD, 2>);
    case 4: return go(k_fwd_gather_conf<TF, TO, METHOD, 4>);
    case 8: return go(k_fwd_gather_conf<TF, TO, METHOD, 8>);
    default: return go(k_fwd_gather_conf<TF, TO, METHOD, 0>);
    }
}

template <typename TF, typename TO>
hipError_t fwd_conf_m(const TF *featT, const float *proj, const Coords &coords, TO *out, const Problem &p, hipStream_t s)
{
    switch (p.method) {
    case AGG_SOFTMAX: return fwd_conf_v<TF, TO, AGG_SOFTMAX>(featT, proj, coords, out, p, s);
    case AGG_SUM: return fwd_conf_v<TF, TO, AGG_SUM>(featT, proj, coords, out, p, s);
    case AGG_MEAN: return fwd_conf_v<TF, TO, AGG_MEAN>(featT, proj, coords, out, p, s);
    }
    return hipErrorNotSupported;                // no weighted max (refused before any launch)
}

template <typename ACC, typename TF, typename TO, int METHOD>
hipError_t bwd_conf_v(const TO *go_, const TF *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                      hipStream_t s)
{
    const size_t lds = conf_head_host(p.V) + sizeof(float) * kConfCh * (kConfTile + 1);
    const dim3 grid((unsigned)((p.N + kConfTile - 1) / kConfTile), (unsigned)p.B, (unsigned)((p.C + kConfCh - 1) / kConfCh));
    auto go = [&](auto kern) -> hipError_t {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, go_, featT, proj, coords, p.confidence, gradT, kexp, p.V, p.C, p.C4, p.H, p.W, p.N,
                           p.view_count, p.visible);
        return hipGetLastError();
    };
    switch (p.V) {
    case 2: return go(k_bwd_gather_conf<TF, TO, METHOD, 2, ACC>);
    case 4: return go(k_bwd_gather_conf<TF, TO, METHOD, 4, ACC>);
    case 8: return go(k_bwd_gather_conf<TF, TO, METHOD, 8, ACC>);
    default: return go(k_bwd_gather_conf<TF, TO, METHOD, 0, ACC>);
    }
}

template <typename ACC, typename TF, typename TO>
hipError_t bwd_conf_m(const TO *go_, const TF *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                      hipStream_t s)
{
    switch (p.method) {
    case AGG_SOFTMAX: return bwd_conf_v<ACC, TF, TO, AGG_SOFTMAX>(go_, featT, proj, coords, gradT, kexp, p, s);
    case AGG_SUM: return bwd_conf_v<ACC, TF, TO, AGG_SUM>(go_, featT, proj, coords, gradT, kexp, p, s);
    case AGG_MEAN: return bwd_conf_v<ACC, TF, TO, AGG_MEAN>(go_, featT, proj, coords, gradT, kexp, p, s);
    }
    return hipErrorNotSupported;
}

template <typename ACC>
hipError_t bwd_conf(const void *grad_out, const void *featT, const float *proj, const Coords &coords, ACC *gradT, const int *kexp, const Problem &p,
                    hipStream_t s)
{
    if (!p.confidence) return hipErrorInvalidValue;
    if (p.out_bf16) return p.feat_f16 ? hipErrorNotSupported : bwd_conf_m((const bf16_t *)grad_out, (const float *)featT, proj, coords, gradT, kexp, p, s);
    if (!p.feat_f16 && !p.out_f16) return bwd_conf_m((const float *)grad_out, (const float *)featT, proj, coords, gradT, kexp, p, s);
    if (p.feat_f16 && p.out_f16) return bwd_conf_m((const __half *)grad_out, (const __half *)featT, proj, coords, gradT, kexp, p, s);
    if (p.feat_f16 && !p.out_f16) return bwd_conf_m((const float *)grad_out, (const __half *)featT, proj, coords, gradT, kexp, p, s);
    return hipErrorNotSupported;
}

}  // namespace

hipError_t launch_fwd_gather_conf(const void *featT, const float *proj, const Coords &coords, void *out, const Problem &p, hipStream_t s)
{
    if (!p.confidence) return hipErrorInvalidValue;
    if (p.out_bf16) return p.feat_f16 ? hipErrorNotSupported : fwd_conf_m((const float *)featT, proj, coords, (bf16_t *)out, p, s);
    if (!p.feat_f16 && !p.out_f16) return fwd_conf_m((const float *)featT, proj, coords, (float *)out, p, s);
    if (p.feat_f16 && p.out_f16) return fwd_conf_m((const __half *)featT, proj, coords, (__half *)out, p, s);
    if (p.feat_f16 && !p.out_f16) return fwd_conf_m((const __half *)featT, proj, coords, (float *)out, p, s);
    return hipErrorNotSupported;
}

hipError_t launch_bwd_gather_conf(const void *grad_out, const void *featT, const float *proj, const Coords &coords, float *gradT, const Problem &p,
                                  hipStream_t s)
{
    return bwd_conf<float>(grad_out, featT, proj, coords, gradT, nullptr, p, s);
}

hipError_t launch_bwd_gather_conf_det(const void *grad_out, const void *featT, const float *proj, const Coords &coords, unsigned long long *gradI,
                                      const int *kexp, const Problem &p, hipStream_t s)
{
    return bwd_conf<unsigned long long>(grad_out, featT, proj, coords, gradI, kexp, p, s);
}

// grad_confidence (B, V, Hf, Wf) fp32 from the stream the geometry kernel wrote: acc conf_grad_acc_bytes of int64, smax conf_grad_max_bytes
size_t conf_grad_stream_bytes(const Problem &p) { return (size_t)p.B * p.V * p.N * sizeof(float); }
size_t conf_grad_acc_bytes(const Problem &p) { return (size_t)p.B * p.V * p.H * p.W * sizeof(long long); }
size_t conf_grad_max_bytes(const Problem &p) { return (size_t)p.B * p.V * sizeof(unsigned); }

hipError_t launch_conf_grad(const float *stream, const float *proj, const Coords &coords, unsigned long long *acc, unsigned *smax, float *grad_conf,
                            const Problem &p, hipStream_t s)
{
    if (!stream || !acc || !smax || !grad_conf) return hipErrorInvalidValue;
    if ((long long)p.B * p.V > 65535) return hipErrorNotSupported;
    const long long HW = (long long)p.H * p.W;
    const int log2n = log2_ceil(p.N);
    hipError_t e = hipMemsetAsync(acc, 0, conf_grad_acc_bytes(p), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(smax, 0, conf_grad_max_bytes(p), s);
    if (e != hipSuccess) return e;
    // largest |dc| of each (b, v) row of the (B, V, N) stream: the scale pass's row maxima (det_scale.h)
    hipLaunchKernelGGL((k_det_gmax<float, DetRowsIdentity>), dim3((unsigned)(p.B * p.V), chunks_of(p.N)), dim3(256), 0, s, stream, smax, p.N);
    hipLaunchKernelGGL(k_conf_grad_scatter, dim3((unsigned)((p.N + 255) / 256), (unsigned)(p.B * p.V)), dim3(256), 0, s, stream, smax, proj, coords, acc,
                       p.V, p.H, p.W, p.N, log2n);
    hipLaunchKernelGGL(k_conf_grad_convert, dim3(chunks_of(HW), (unsigned)(p.B * p.V)), dim3(256), 0, s, acc, smax, grad_conf, HW, log2n);
    return hipGetLastError();
}

}  // namespace mvhmr
