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

// the confidence map of one (b, v), (H, W) fp32, sampled with the taps of the features: a tap outside the map has the value 0
__device__ __forceinline__ float sample_conf(const float *__restrict__ cm, const Taps &t, int H, int W)
{
    if (!t.any) return 0.f;
    const bool xin0 = t.rx0 >= 0, xin1 = t.rx0 + 1 <= W - 1, yin0 = t.ry0 >= 0, yin1 = t.ry0 + 1 <= H - 1;
    const float c00 = (xin0 && yin0) ? cm[t.y0 * W + t.x0] : 0.f, c01 = (xin1 && yin0) ? cm[t.y0 * W + t.x1] : 0.f;
    const float c10 = (xin0 && yin1) ? cm[t.y1 * W + t.x0] : 0.f, c11 = (xin1 && yin1) ? cm[t.y1 * W + t.x1] : 0.f;
    return bilerp(c00, c01, c10, c11, t.w00, t.w01, t.w10, t.w11);
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

__device__ __forceinline__ void store_conf(float *p, float v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void store_conf(__half *p, float v)
{
    __builtin_nontemporal_store(__half_as_ushort(from_f32<__half>(v)), reinterpret_cast<unsigned short *>(p));   // fp32 first, then fp16
}
__device__ __forceinline__ void store_conf(bf16_t *p, float v)
{
    __builtin_nontemporal_store(__builtin_bit_cast(unsigned short, (bf16_t)v), reinterpret_cast<unsigned short *>(p));
}

__device__ __forceinline__ unsigned abs_bits(float x) { return __builtin_bit_cast(unsigned, x) & 0x7fffffffu; }
__device__ __forceinline__ unsigned wave_max_u32(unsigned m)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m, o);
        m = t > m ? t : m;
    }
    return m;
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
                if (c < C) store_conf(&out[((long long)b * C + c) * N + n], t.v[i]);
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

// ------------------------------------------------------------------------------------------ deterministic scale pass
// max |grad_out| of each (b, c) row of the (B, C, N) volume gradient: block (row, chunk) -- k_det_gmax
template <typename TO>
__global__ void __launch_bounds__(256) k_conf_gmax(const TO *__restrict__ grad_out, unsigned *__restrict__ gmax, long long N)
{
    const long long row = blockIdx.x;
    const TO *g = grad_out + row * N;
    unsigned m = 0;
    for (long long n = (long long)blockIdx.y * 256 + threadIdx.x; n < N; n += (long long)gridDim.y * 256) {
        const unsigned a = abs_bits(to_f32<TO>(g[n]));
        m = a > m ? a : m;
    }
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(gmax + row, m);
}

// the largest positive pixel of a sample's maps (bits of the float; NaN and negative pixels never raise it, +Inf does): a bilinear sample is a
// convex combination of its taps and zeros, so this bounds every c_v of the sample
__global__ void __launch_bounds__(256) k_conf_cmax(const float *__restrict__ conf, unsigned *__restrict__ cmax, long long per_sample)
{
    const int b = blockIdx.y;
    const float *c = conf + (long long)b * per_sample;
    unsigned m = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per_sample; i += (long long)gridDim.x * 256) {
        const float x = c[i];
        const unsigned a = x > 0.f ? __builtin_bit_cast(unsigned, x) : 0u;
        m = a > m ? a : m;
    }
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(cmax + b, m);
}

// softmax: one byte per pixel of every (b, slot) map that a voxel-view taking part taps -- all four clamped taps, those of weight 0 too: the
// kernels' samples multiply every tap they load, so a non-finite value under a zero-weight tap reaches s_v and must poison the (b, c)
// (thread per (voxel, slot): the very test and taps of build_conf_records; every writer stores the same 1) -- k_det_mark_seen
__global__ void __launch_bounds__(256) k_conf_mark(const float *__restrict__ proj, const Coords coords, const float *__restrict__ conf,
                                                   unsigned char *__restrict__ marks, int V, int H, int W, long long N, const int *__restrict__ nvs,
                                                   int visible)
{
    const long long bv = blockIdx.y;
    const int b = (int)(bv / V), v = (int)(bv % V);
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N || (nvs && v >= nvs[b])) return;
    float X0, X1, X2;
    voxel_xyz(coords, b, N, n, X0, X1, X2);
    const float *P = proj + bv * 12;
    if (visible && !view_sees(P, X0, X1, X2, H, W)) return;
    const Taps t = make_taps(P, X0, X1, X2, H, W);
    if (!(sample_conf(conf + bv * H * W, t, H, W) > 0.f)) return;
    unsigned char *m = marks + bv * (long long)H * W;
    m[t.y0 * W + t.x0] = 1;                                                       // (clamped into the map whatever the position)
    m[t.y0 * W + t.x1] = 1;
    m[t.y1 * W + t.x0] = 1;
    m[t.y1 * W + t.x1] = 1;
}

constexpr int kConfPix = 64;
template <typename TF>
__global__ void __launch_bounds__(256) k_conf_fmax(const TF *__restrict__ featT, const unsigned char *__restrict__ marks, unsigned *__restrict__ fmax,
                                                   int V, int C, int C4, int HW)
{
    const long long bv = blockIdx.y;
    const int b = (int)(bv / V), p0 = blockIdx.x * kConfPix, p1 = p0 + kConfPix < HW ? p0 + kConfPix : HW;
    const TF *f = featT + bv * (long long)HW * C4;
    const unsigned char *mk = marks + bv * (long long)HW;
    for (int c = threadIdx.x; c < C; c += 256) {
        unsigned m = 0;
        for (int p = p0; p < p1; ++p) {
            if (!mk[p]) continue;                                                 // block-uniform
            const unsigned a = abs_bits(to_f32<TF>(f[(long long)p * C4 + c]));
            m = a > m ? a : m;
        }
        if (m) atomicMax(fmax + (long long)b * C + c, m);
    }
}

// K[b][c]: N * bound * 2^K < 2^62 with bound = max|g| (1 + 2 Fmax) for softmax, max|g| * cmax[b] for sum (|ds| = |g| c_v: without the
// confidence the int64 sums can wrap), max|g| for mean (|ds| = |g| c_v / W <= |g|)
__global__ void __launch_bounds__(256) k_conf_det_exponent(const unsigned *__restrict__ gmax, const unsigned *__restrict__ fmax,
                                                           const unsigned *__restrict__ cmax, int *__restrict__ kexp, long long BC, int method, int C,
                                                           int log2n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    const unsigned gb = gmax[i], fb = method == AGG_SOFTMAX ? fmax[i] : 0u, cb = method == AGG_SUM ? cmax[i / C] : 0u;
    if (gb >= 0x7f800000u || fb >= 0x7f800000u || cb >= 0x7f800000u) { kexp[i] = kDetPoison; return; }
    const double g = (double)__builtin_bit_cast(float, gb), f = (double)__builtin_bit_cast(float, fb), c = (double)__builtin_bit_cast(float, cb);
    const double bound = method == AGG_SOFTMAX ? g * (1.0 + 2.0 * f) : method == AGG_SUM ? g * c : g;
    if (bound == 0.0) { kexp[i] = 0; return; }
    if (!(bound < 3.4028234663852886e38)) { kexp[i] = kDetPoison; return; }     // ds itself may overflow fp32
    int e;
    frexp(bound, &e);                                                           // bound < 2^e
    kexp[i] = 62 - log2n - e;
}

// ------------------------------------------------------------------------------------------ grad_confidence
// the exponent of one (b, v) from the bits of its largest |dc|: N * max * 2^K < 2^62; poison when the maximum is not finite
__device__ __forceinline__ int conf_grad_exponent(unsigned maxbits, int log2n)
{
    if (maxbits >= 0x7f800000u) return kDetPoison;
    const int e = (int)(maxbits >> 23) - 126;                                     // max < 2^e (a denormal maximum: < 2^-126)
    return 62 - log2n - e;
}

// largest |dc| of each (b, v) row of the (B, V, N) stream: block (row, chunk), integer atomicMax on the bits
__global__ void __launch_bounds__(256) k_conf_grad_max(const float *__restrict__ stream, unsigned *__restrict__ smax, long long N)
{
    const long long row = blockIdx.x;
    const float *g = stream + row * N;
    unsigned m = 0;
    for (long long n = (long long)blockIdx.y * 256 + threadIdx.x; n < N; n += (long long)gridDim.y * 256) {
        const unsigned a = abs_bits(g[n]);
        m = a > m ? a : m;
    }
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(smax + row, m);
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
int log2_ceil(long long N) { return N > 1 ? 64 - __builtin_clzll((unsigned long long)(N - 1)) : 0; }
unsigned chunks_of(long long N)
{
    const long long c = (N + 2047) / 2048;
    return (unsigned)(c < 1 ? 1 : c > 64 ? 64 : c);
}

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

// behind the three words per (b, c) of det_scale_bytes: cmax (B words, padded to 16 B), then the tap marks of every (b, slot) map
size_t conf_det_scale_extra_bytes(const Problem &p) { return ((size_t)p.B * sizeof(unsigned) + 15) / 16 * 16 + (size_t)p.B * p.V * p.H * p.W; }

hipError_t launch_det_scale_conf(const void *grad_out, const void *featT, void *scale, const Problem &p, hipStream_t s, const float *proj,
                                 const Coords *coords)
{
    if (!p.confidence || !proj || !coords) return hipErrorInvalidValue;
    const long long BC = (long long)p.B * p.C;
    if (BC > 0x7fffffffll || (long long)p.B * p.V > 65535) return hipErrorNotSupported;
    unsigned *gmax = static_cast<unsigned *>(scale), *fmax = gmax + BC;
    int *kexp = reinterpret_cast<int *>(fmax + BC);
    unsigned *cmax = reinterpret_cast<unsigned *>(kexp + BC);
    unsigned char *marks = reinterpret_cast<unsigned char *>(cmax) + ((size_t)p.B * sizeof(unsigned) + 15) / 16 * 16;
    const int HW = p.H * p.W;
    hipError_t e = hipMemsetAsync(gmax, 0, (size_t)BC * 2 * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(cmax, 0, (size_t)p.B * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const dim3 g1((unsigned)BC, chunks_of(p.N));
    if (p.out_bf16) hipLaunchKernelGGL(k_conf_gmax<bf16_t>, g1, dim3(256), 0, s, (const bf16_t *)grad_out, gmax, p.N);
    else if (p.out_f16) hipLaunchKernelGGL(k_conf_gmax<__half>, g1, dim3(256), 0, s, (const __half *)grad_out, gmax, p.N);
    else hipLaunchKernelGGL(k_conf_gmax<float>, g1, dim3(256), 0, s, (const float *)grad_out, gmax, p.N);
    if (p.method == AGG_SUM) {
        const long long per = (long long)p.V * HW;
        hipLaunchKernelGGL(k_conf_cmax, dim3(chunks_of(per), (unsigned)p.B), dim3(256), 0, s, p.confidence, cmax, per);
    }
    if (p.method == AGG_SOFTMAX) {
        e = hipMemsetAsync(marks, 0, (size_t)p.B * p.V * HW, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_conf_mark, dim3((unsigned)((p.N + 255) / 256), (unsigned)(p.B * p.V)), dim3(256), 0, s, proj, *coords, p.confidence, marks,
                           p.V, p.H, p.W, p.N, p.view_count, p.visible);
        const dim3 g2((unsigned)((HW + kConfPix - 1) / kConfPix), (unsigned)(p.B * p.V));
        if (p.feat_f16) hipLaunchKernelGGL(k_conf_fmax<__half>, g2, dim3(256), 0, s, (const __half *)featT, marks, fmax, p.V, p.C, p.C4, HW);
        else hipLaunchKernelGGL(k_conf_fmax<float>, g2, dim3(256), 0, s, (const float *)featT, marks, fmax, p.V, p.C, p.C4, HW);
    }
    hipLaunchKernelGGL(k_conf_det_exponent, dim3((unsigned)((BC + 255) / 256)), dim3(256), 0, s, gmax, fmax, cmax, kexp, BC, p.method, p.C, log2_ceil(p.N));
    return hipGetLastError();
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
    hipLaunchKernelGGL(k_conf_grad_max, dim3((unsigned)(p.B * p.V), chunks_of(p.N)), dim3(256), 0, s, stream, smax, p.N);
    hipLaunchKernelGGL(k_conf_grad_scatter, dim3((unsigned)((p.N + 255) / 256), (unsigned)(p.B * p.V)), dim3(256), 0, s, stream, smax, proj, coords, acc,
                       p.V, p.H, p.W, p.N, log2n);
    hipLaunchKernelGGL(k_conf_grad_convert, dim3(chunks_of(HW), (unsigned)(p.B * p.V)), dim3(256), 0, s, acc, smax, grad_conf, HW, log2n);
    return hipGetLastError();
}

}  // namespace mvhmr
