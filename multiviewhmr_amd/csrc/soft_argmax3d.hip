// Volumetric 3-D soft-argmax (include/mvhmr_unproject.h: mvhmr_soft_argmax3d_*): keypoints from (B,J,X,Y,Z) heat
// volumes in one pass over the volume, without a softmaxed copy and -- on the cuboid route -- without coordinate volumes.
//
// Arithmetic contract (tests/softargmax_oracle.py::emulate_fp32 restates it in numpy, operation for operation):
//   t_n   = fmul(c2, v_n),  c2 = fl32(beta * log2 e)                          the softmax runs in the log2 domain
//   chunk = VEC consecutive voxels (one 16-byte vector of the volume: 4 fp32 / 8 halves; VEC = 1 when N % VEC != 0 or a pointer is
//           not 16-byte aligned: with such an N every second slice starts off a vector boundary, and the joints of a tile share
//           their voxel index, so no vector start suits them all)
//   split s of S owns chunks [s*Cs, min((s+1)*Cs, C)), Cs = ceil(C / S); lane t of the 256 walks chunks first + t + 256 i
//   record (m, D, a[3]), initially (-inf, 0, 0); per chunk and joint:
//       tm = max_e t_e (in element order, from -inf);  m' = fmaxf(m, tm);  ms = m' == -inf ? 0 : m';  sc = exp2(m - ms)
//       D = fmul(D, sc), a = fmul(a, sc);  then per element in order:  p = exp2(t_e - ms);  D = fadd(D, p);  a_c = fma(p, u_c, a_c)
//   merge(A, B): m = fmaxf(mA, mB), ms as above, sA = exp2(mA - ms), sB = exp2(mB - ms), x = fadd(fmul(xA, sA), fmul(xB, sB)) for D, a
//   lanes merge by xor butterflies 1, 2, 4, 8, 16, 32 (a balanced tree: merge is bitwise symmetric), the 4 waves in order
//   ((w0 + w1) + w2) + w3, the S records of a slice lane-strided (lane l: l, l + 64, ... in order) and then by the same butterfly
//   mu = fdiv(a, D),  L = fmul(fadd(m, log2(D)), ln 2),  both NaN when D == 0 (nothing but -inf)
// fmaxf drops a NaN, but exp2(NaN - ms) does not: a NaN reaches D.  +inf makes ms = +inf and inf - inf = NaN.  The ms guard keeps
// -inf entries at exp2(-inf) = 0 while no finite entry has been seen.  No atomics: the order above is the only order.
#include "device_common.h"
#include "kernels.h"
#include "mvhmr_unproject.h"

#include <type_traits>

namespace mvhmr {

namespace {

constexpr int kSaThreads = 256;
constexpr int kSaRec = 5;                       // floats per record: m, D, ax, ay, az
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

struct SaRec { float m, D, x, y, z; };

__device__ __forceinline__ float sa_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float sa_safe(float m) { return m == -__builtin_inff() ? 0.f : m; }

__device__ __forceinline__ SaRec sa_merge(const SaRec &A, const SaRec &B)
{
    const float ms = sa_safe(fmaxf(A.m, B.m));
    const float sA = sa_exp2(__fsub_rn(A.m, ms)), sB = sa_exp2(__fsub_rn(B.m, ms));
    SaRec r;
    r.m = fmaxf(A.m, B.m);
    r.D = __fadd_rn(__fmul_rn(A.D, sA), __fmul_rn(B.D, sB));
    r.x = __fadd_rn(__fmul_rn(A.x, sA), __fmul_rn(B.x, sB));
    r.y = __fadd_rn(__fmul_rn(A.y, sA), __fmul_rn(B.y, sB));
    r.z = __fadd_rn(__fmul_rn(A.z, sA), __fmul_rn(B.z, sB));
    return r;
}

__device__ __forceinline__ SaRec sa_wave_merge(SaRec r)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        SaRec o;
        o.m = __shfl_xor(r.m, off); o.D = __shfl_xor(r.D, off);
        o.x = __shfl_xor(r.x, off); o.y = __shfl_xor(r.y, off); o.z = __shfl_xor(r.z, off);
        r = sa_merge(r, o);
    }
    return r;
}

// VEC values of one slice from element n0 on, as fp32.  VEC > 1 is one 16-byte load (the launcher checked the alignment).
template <typename T, int VEC> __device__ __forceinline__ void sa_load(const T *p, float (&v)[VEC])
{
    if constexpr (VEC == 1) {
        v[0] = to_f32<T>(p[0]);
    } else if constexpr (sizeof(T) == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = to_f32<T>(__builtin_bit_cast(T, (unsigned short)(w[i] & 0xffffu)));
            v[2 * i + 1] = to_f32<T>(__builtin_bit_cast(T, (unsigned short)(w[i] >> 16)));
        }
    }
}

template <typename T, int VEC> __device__ __forceinline__ void sa_store(T *p, const float (&v)[VEC])
{
    if constexpr (VEC == 1) {
        p[0] = from_f32<T>(v[0]);
    } else if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *reinterpret_cast<uint4 *>(p) = make_uint4(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7]));
    }
}

// u of the VEC voxels from flat index n0 on: the caller's tensor, or cuboid_offset's roundings with the index split once, in 32 bits
template <bool TENSOR, int VEC> __device__ __forceinline__ void sa_coords(const Coords &cs, int b, unsigned N, unsigned n0, float (&u)[VEC][3])
{
    if constexpr (TENSOR) {
        const float *p = cs.ptr + ((size_t)b * N + n0) * 3;
        if constexpr (VEC == 1) {
            u[0][0] = p[0]; u[0][1] = p[1]; u[0][2] = p[2];
        } else {
            float flat[VEC * 3];
#pragma unroll
            for (int i = 0; i < VEC * 3 / 4; ++i) {
                const float4 q = reinterpret_cast<const float4 *>(p)[i];
                flat[4 * i] = q.x; flat[4 * i + 1] = q.y; flat[4 * i + 2] = q.z; flat[4 * i + 3] = q.w;
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) { u[e][0] = flat[3 * e]; u[e][1] = flat[3 * e + 1]; u[e][2] = flat[3 * e + 2]; }
        }
    } else {
        const unsigned Z = (unsigned)cs.Z, Y = (unsigned)cs.Y;
        unsigned k = n0 % Z, r = n0 / Z;
        unsigned j = r % Y, i = r / Y;
        const float *ce = cs.center + b * 3;
        const float c0 = ce[0], c1 = ce[1], c2 = ce[2];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            u[e][0] = __fsub_rn(__fadd_rn(cs.px, __fmul_rn(cs.sx, (float)i)), c0);
            u[e][1] = __fsub_rn(__fadd_rn(cs.py, __fmul_rn(cs.sy, (float)j)), c1);
            u[e][2] = __fsub_rn(__fadd_rn(cs.pz, __fmul_rn(cs.sz, (float)k)), c2);
            if (++k == Z) { k = 0; if (++j == Y) { j = 0; ++i; } }
        }
    }
}

// ---- forward, first launch: one block per (tile of JT joints of one sample, split s of S); JT records to ws[slice][s]
template <typename T, int JT, bool TENSOR, int VEC>
__global__ void __launch_bounds__(kSaThreads)
k_sa3d_partial(const T *__restrict__ vol, const Coords cs, int J, int j0, int tiles, unsigned N, int S, float c2, float *__restrict__ ws)
{
    const int tile = blockIdx.x / S, s = blockIdx.x % S;
    const int b = tile / tiles, slice0 = b * J + j0 + (tile % tiles) * JT;
    const unsigned C = N / VEC, Cs = (C + S - 1) / S;
    const unsigned first = (unsigned)s * Cs, last = min(first + Cs, C);
    const float ninf = -__builtin_inff();

    SaRec rec[JT];
#pragma unroll
    for (int q = 0; q < JT; ++q) rec[q] = SaRec{ninf, 0.f, 0.f, 0.f, 0.f};

    for (unsigned c = first + threadIdx.x; c < last; c += kSaThreads) {
        const unsigned n0 = c * VEC;
        float u[VEC][3];
        sa_coords<TENSOR, VEC>(cs, b, N, n0, u);
#pragma unroll
        for (int q = 0; q < JT; ++q) {
            float t[VEC];
            sa_load<T, VEC>(vol + (size_t)(slice0 + q) * N + n0, t);
            float tm = ninf;
#pragma unroll
            for (int e = 0; e < VEC; ++e) { t[e] = __fmul_rn(c2, t[e]); tm = fmaxf(tm, t[e]); }
            SaRec &r = rec[q];
            const float mn = fmaxf(r.m, tm), ms = sa_safe(mn);
            const float sc = sa_exp2(__fsub_rn(r.m, ms));
            r.m = mn;
            r.D = __fmul_rn(r.D, sc); r.x = __fmul_rn(r.x, sc); r.y = __fmul_rn(r.y, sc); r.z = __fmul_rn(r.z, sc);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float p = sa_exp2(__fsub_rn(t[e], ms));
                r.D = __fadd_rn(r.D, p);
                r.x = __fmaf_rn(p, u[e][0], r.x); r.y = __fmaf_rn(p, u[e][1], r.y); r.z = __fmaf_rn(p, u[e][2], r.z);
            }
        }
    }

    __shared__ float lds[kSaThreads / 64][JT][kSaRec];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < JT; ++q) {
        const SaRec r = sa_wave_merge(rec[q]);
        if (lane == 0) { float *o = lds[wave][q]; o[0] = r.m; o[1] = r.D; o[2] = r.x; o[3] = r.y; o[4] = r.z; }
    }
    __syncthreads();
    if (threadIdx.x < JT) {
        const int q = threadIdx.x;
        SaRec r{lds[0][q][0], lds[0][q][1], lds[0][q][2], lds[0][q][3], lds[0][q][4]};
#pragma unroll
        for (int w = 1; w < kSaThreads / 64; ++w)
            r = sa_merge(r, SaRec{lds[w][q][0], lds[w][q][1], lds[w][q][2], lds[w][q][3], lds[w][q][4]});
        float *o = ws + ((size_t)(slice0 + q) * S + s) * kSaRec;
        o[0] = r.m; o[1] = r.D; o[2] = r.x; o[3] = r.y; o[4] = r.z;
    }
}

// ---- forward, second launch: one wave per slice merges its S records and writes L, mu and the keypoint
__global__ void __launch_bounds__(64)
k_sa3d_combine(const float *__restrict__ ws, const Coords cs, int J, int S, float *__restrict__ keypoints, float *__restrict__ lse,
               float *__restrict__ moment)
{
    const int slice = blockIdx.x, lane = threadIdx.x;
    SaRec r{-__builtin_inff(), 0.f, 0.f, 0.f, 0.f};
    for (int s = lane; s < S; s += 64) {
        const float *o = ws + ((size_t)slice * S + s) * kSaRec;
        r = sa_merge(r, SaRec{o[0], o[1], o[2], o[3], o[4]});
    }
    r = sa_wave_merge(r);
    if (lane != 0) return;
    const float nan = __builtin_nanf("");
    const bool empty = r.D == 0.f;
    const float mx = empty ? nan : __fdiv_rn(r.x, r.D), my = empty ? nan : __fdiv_rn(r.y, r.D), mz = empty ? nan : __fdiv_rn(r.z, r.D);
    lse[slice] = empty ? nan : __fmul_rn(__fadd_rn(r.m, log2f(r.D)), kLn2);
    float *mo = moment + (size_t)slice * 3, *kp = keypoints + (size_t)slice * 3;
    mo[0] = mx; mo[1] = my; mo[2] = mz;
    if (cs.ptr) {
        kp[0] = mx; kp[1] = my; kp[2] = mz;
    } else {
        const int b = slice / J;
        const float *R = cs.rot + b * 9, *ce = cs.center + b * 3;                      // voxel_xyz's order
        kp[0] = __fadd_rn(__fmaf_rn(R[2], mz, __fmaf_rn(R[1], my, __fmul_rn(R[0], mx))), ce[0]);
        kp[1] = __fadd_rn(__fmaf_rn(R[5], mz, __fmaf_rn(R[4], my, __fmul_rn(R[3], mx))), ce[1]);
        kp[2] = __fadd_rn(__fmaf_rn(R[8], mz, __fmaf_rn(R[7], my, __fmul_rn(R[6], mx))), ce[2]);
    }
}

// ---- backward w.r.t. the volume: one thread per chunk and tile; grad_v = fmul(fmul(beta, p), fadd(h . (u - mu), g_L)) with
// p = exp2(t - fmul(L, log2 e)) and the dot product fma(hz, dz, fma(hy, dy, fmul(hx, dx))), d = fsub(u, mu)
template <typename T, int JT, bool TENSOR, int VEC>
__global__ void __launch_bounds__(kSaThreads)
k_sa3d_bwd(const T *__restrict__ vol, const Coords cs, int J, int j0, int tiles, unsigned N, unsigned nblk, float c2, float beta,
           const float *__restrict__ lse, const float *__restrict__ moment, const float *__restrict__ gk, const float *__restrict__ gl,
           T *__restrict__ grad_vol)
{
    const int tile = blockIdx.x / nblk;
    const unsigned c = (blockIdx.x % nblk) * kSaThreads + threadIdx.x, C = N / VEC;
    if (c >= C) return;
    const int b = tile / tiles, slice0 = b * J + j0 + (tile % tiles) * JT;
    const unsigned n0 = c * VEC;
    float u[VEC][3];
    sa_coords<TENSOR, VEC>(cs, b, N, n0, u);
#pragma unroll
    for (int q = 0; q < JT; ++q) {
        const int slice = slice0 + q;
        const float L2 = __fmul_rn(lse[slice], kLog2e);
        const float *mo = moment + (size_t)slice * 3;
        const float m0 = mo[0], m1 = mo[1], m2 = mo[2];
        float h0 = 0.f, h1 = 0.f, h2 = 0.f;
        if (gk) {
            const float *g = gk + (size_t)slice * 3;
            const float g0 = g[0], g1 = g[1], g2 = g[2];
            if constexpr (TENSOR) {
                h0 = g0; h1 = g1; h2 = g2;
            } else {
                const float *R = cs.rot + b * 9;                                        // h = R^T g
                h0 = __fmaf_rn(R[6], g2, __fmaf_rn(R[3], g1, __fmul_rn(R[0], g0)));
                h1 = __fmaf_rn(R[7], g2, __fmaf_rn(R[4], g1, __fmul_rn(R[1], g0)));
                h2 = __fmaf_rn(R[8], g2, __fmaf_rn(R[5], g1, __fmul_rn(R[2], g0)));
            }
        }
        const float gL = gl ? gl[slice] : 0.f;
        float v[VEC];
        sa_load<T, VEC>(vol + (size_t)slice * N + n0, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float p = sa_exp2(__fsub_rn(__fmul_rn(c2, v[e]), L2));
            const float dot = __fmaf_rn(h2, __fsub_rn(u[e][2], m2), __fmaf_rn(h1, __fsub_rn(u[e][1], m1), __fmul_rn(h0, __fsub_rn(u[e][0], m0))));
            v[e] = __fmul_rn(__fmul_rn(beta, p), __fadd_rn(dot, gL));
        }
        sa_store<T, VEC>(grad_vol + (size_t)slice * N + n0, v);
    }
}

// ---- tensor route, gradient w.r.t. the coordinates: one thread per chunk of one sample, joints in index order, acc = fma(p, g, acc)
template <typename T, int VEC>
__global__ void __launch_bounds__(kSaThreads)
k_sa3d_bwd_coords(const T *__restrict__ vol, int J, unsigned N, unsigned nblk, float c2, const float *__restrict__ lse,
                  const float *__restrict__ gk, float *__restrict__ grad_coords)
{
    const int b = blockIdx.x / nblk;
    const unsigned c = (blockIdx.x % nblk) * kSaThreads + threadIdx.x, C = N / VEC;
    if (c >= C) return;
    const unsigned n0 = c * VEC;
    float acc[VEC * 3];
#pragma unroll
    for (int i = 0; i < VEC * 3; ++i) acc[i] = 0.f;
    for (int j = 0; j < J; ++j) {
        const int slice = b * J + j;
        const float L2 = __fmul_rn(lse[slice], kLog2e);
        const float *g = gk + (size_t)slice * 3;
        const float g0 = g[0], g1 = g[1], g2 = g[2];
        float v[VEC];
        sa_load<T, VEC>(vol + (size_t)slice * N + n0, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float p = sa_exp2(__fsub_rn(__fmul_rn(c2, v[e]), L2));
            acc[3 * e] = __fmaf_rn(p, g0, acc[3 * e]); acc[3 * e + 1] = __fmaf_rn(p, g1, acc[3 * e + 1]); acc[3 * e + 2] = __fmaf_rn(p, g2, acc[3 * e + 2]);
        }
    }
    float *o = grad_coords + ((size_t)b * N + n0) * 3;
    if constexpr (VEC == 1) {
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    } else {
#pragma unroll
        for (int i = 0; i < VEC * 3 / 4; ++i)
            reinterpret_cast<float4 *>(o)[i] = make_float4(acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]);
    }
}

// ---- cuboid route, gradients w.r.t. the pose: one thread per entry of (B, 9 + 3), joints in index order
__global__ void __launch_bounds__(64)
k_sa3d_pose_grad(const float *__restrict__ rot, const float *__restrict__ moment, const float *__restrict__ gk, float *__restrict__ grad_rot,
                 float *__restrict__ grad_center, int B, int J)
{
    const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= (long long)B * 12) return;
    const long long b = idx / 12;
    const int e = (int)(idx % 12);
    float acc = 0.f;
    if (e < 9) {
        if (!grad_rot) return;
        const int r = e / 3, c = e % 3;
        for (int j = 0; j < J; ++j) acc = __fmaf_rn(gk[(b * J + j) * 3 + r], moment[(b * J + j) * 3 + c], acc);
        grad_rot[b * 9 + e] = acc;
    } else {
        if (!grad_center) return;
        const int c = e - 9;
        const float *R = rot + b * 9;
        for (int j = 0; j < J; ++j) {
            const float *g = gk + (b * J + j) * 3;
            const float h = __fmaf_rn(R[6 + c], g[2], __fmaf_rn(R[3 + c], g[1], __fmul_rn(R[c], g[0])));
            acc = __fadd_rn(acc, __fsub_rn(g[c], h));
        }
        grad_center[b * 3 + c] = acc;
    }
}

// the joints of a sample as tiles of 4, then one of 2, then one of 1: `launch(jt_tag, j0, tiles)` per class that occurs
template <typename F> hipError_t for_each_tile_class(int J, F launch)
{
    hipError_t e = hipSuccess;
    int j0 = 0;
    if (J / 4) { e = launch(std::integral_constant<int, 4>(), j0, J / 4); j0 += J / 4 * 4; }
    if (e == hipSuccess && (J & 2)) { e = launch(std::integral_constant<int, 2>(), j0, 1); j0 += 2; }
    if (e == hipSuccess && (J & 1)) e = launch(std::integral_constant<int, 1>(), j0, 1);
    return e;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <typename T, bool TENSOR, int VEC>
hipError_t fwd_partial(const T *vol, const Coords &cs, int B, int J, unsigned N, int S, float c2, float *ws, hipStream_t s)
{
    return for_each_tile_class(J, [&](auto jt, int j0, int tiles) {
        constexpr int JT = decltype(jt)::value;
        hipLaunchKernelGGL((k_sa3d_partial<T, JT, TENSOR, VEC>), dim3((unsigned)((long long)B * tiles * S)), dim3(kSaThreads), 0, s, vol, cs, J, j0,
                           tiles, N, S, c2, ws);
        return hipGetLastError();
    });
}

template <typename T, bool TENSOR, int VEC>
hipError_t bwd_volume(const T *vol, const Coords &cs, int B, int J, unsigned N, float c2, float beta, const float *lse, const float *moment,
                      const float *gk, const float *gl, T *grad_vol, hipStream_t s)
{
    const unsigned nblk = (N / VEC + kSaThreads - 1) / kSaThreads;
    return for_each_tile_class(J, [&](auto jt, int j0, int tiles) {
        constexpr int JT = decltype(jt)::value;
        if ((long long)B * tiles * nblk > 0x7fffffffLL) return hipErrorNotSupported;
        hipLaunchKernelGGL((k_sa3d_bwd<T, JT, TENSOR, VEC>), dim3((unsigned)((long long)B * tiles * nblk)), dim3(kSaThreads), 0, s, vol, cs, J, j0,
                           tiles, N, nblk, c2, beta, lse, moment, gk, gl, grad_vol);
        return hipGetLastError();
    });
}

// dtype and route to template arguments; VEC > 1 only when every slice and every vector of coordinates starts on 16 bytes
template <typename F> hipError_t with_storage(int dtype, bool vec_ok, unsigned N, F f)
{
    switch (dtype) {
    case MVHMR_F32: return vec_ok && N % 4 == 0 ? f((float *)nullptr, std::integral_constant<int, 4>()) : f((float *)nullptr, std::integral_constant<int, 1>());
    case MVHMR_F16: return vec_ok && N % 8 == 0 ? f((__half *)nullptr, std::integral_constant<int, 8>()) : f((__half *)nullptr, std::integral_constant<int, 1>());
    case MVHMR_BF16: return vec_ok && N % 8 == 0 ? f((bf16_t *)nullptr, std::integral_constant<int, 8>()) : f((bf16_t *)nullptr, std::integral_constant<int, 1>());
    }
    return hipErrorNotSupported;
}

}  // namespace

// S = 1 once the tiles alone fill the chip about twice over (2048 blocks: 256 CUs x 4 resident blocks x 2); else enough splits to get
// there, but no block with fewer than 2048 voxels.  A function of the sizes only: results must not depend on the card.
int sa3d_splits(long long B, long long J, long long N)
{
    const long long tiles = B * (J / 4 + ((J & 2) >> 1) + (J & 1)), target = 2048, floor_voxels = 2048;
    if (tiles >= target) return 1;
    const long long want = (target + tiles - 1) / tiles, most = N / floor_voxels;
    return (int)(want < most ? want : (most < 1 ? 1 : most));
}

size_t sa3d_workspace_floats(long long B, long long J, long long N) { return (size_t)(B * J) * (size_t)sa3d_splits(B, J, N) * kSaRec; }

hipError_t launch_sa3d_forward(const void *vol, int dtype, const Coords &cs, int B, int J, int X, float c2, float *keypoints, float *lse,
                               float *moment, float *ws, hipStream_t s)
{
    const unsigned N = (unsigned)((long long)X * cs.Y * cs.Z);
    const int S = sa3d_splits(B, J, N);
    const bool vec_ok = aligned16(vol) && (!cs.ptr || aligned16(cs.ptr));
    hipError_t e = with_storage(dtype, vec_ok, N, [&](auto *tag, auto vec) {
        using T = std::remove_pointer_t<decltype(tag)>;
        constexpr int VEC = decltype(vec)::value;
        return cs.ptr ? fwd_partial<T, true, VEC>(static_cast<const T *>(vol), cs, B, J, N, S, c2, ws, s)
                      : fwd_partial<T, false, VEC>(static_cast<const T *>(vol), cs, B, J, N, S, c2, ws, s);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sa3d_combine, dim3((unsigned)(B * J)), dim3(64), 0, s, ws, cs, J, S, keypoints, lse, moment);
    return hipGetLastError();
}

hipError_t launch_sa3d_backward(const void *vol, int dtype, const Coords &cs, int B, int J, int X, float c2, float beta, const float *lse,
                                const float *moment, const float *grad_kp, const float *grad_lse, void *grad_vol, hipStream_t s)
{
    const unsigned N = (unsigned)((long long)X * cs.Y * cs.Z);
    const bool vec_ok = aligned16(vol) && aligned16(grad_vol) && (!cs.ptr || aligned16(cs.ptr));
    return with_storage(dtype, vec_ok, N, [&](auto *tag, auto vec) {
        using T = std::remove_pointer_t<decltype(tag)>;
        constexpr int VEC = decltype(vec)::value;
        return cs.ptr ? bwd_volume<T, true, VEC>(static_cast<const T *>(vol), cs, B, J, N, c2, beta, lse, moment, grad_kp, grad_lse, static_cast<T *>(grad_vol), s)
                      : bwd_volume<T, false, VEC>(static_cast<const T *>(vol), cs, B, J, N, c2, beta, lse, moment, grad_kp, grad_lse, static_cast<T *>(grad_vol), s);
    });
}

hipError_t launch_sa3d_backward_coords(const void *vol, int dtype, int B, int J, long long N, float c2, const float *lse, const float *grad_kp,
                                       float *grad_coords, hipStream_t s)
{
    const bool vec_ok = aligned16(vol) && aligned16(grad_coords);
    return with_storage(dtype, vec_ok, (unsigned)N, [&](auto *tag, auto vec) {
        using T = std::remove_pointer_t<decltype(tag)>;
        constexpr int VEC = decltype(vec)::value;
        const unsigned nblk = ((unsigned)N / VEC + kSaThreads - 1) / kSaThreads;
        if ((long long)B * nblk > 0x7fffffffLL) return hipErrorNotSupported;
        hipLaunchKernelGGL((k_sa3d_bwd_coords<T, VEC>), dim3((unsigned)((long long)B * nblk)), dim3(kSaThreads), 0, s, static_cast<const T *>(vol), J,
                           (unsigned)N, nblk, c2, lse, grad_kp, grad_coords);
        return hipGetLastError();
    });
}

hipError_t launch_sa3d_backward_pose(const float *rot, const float *moment, const float *grad_kp, float *grad_rot, float *grad_center, int B, int J,
                                     hipStream_t s)
{
    hipLaunchKernelGGL(k_sa3d_pose_grad, dim3((unsigned)(((long long)B * 12 + 63) / 64)), dim3(64), 0, s, rot, moment, grad_kp, grad_rot, grad_center, B, J);
    return hipGetLastError();
}

}  // namespace mvhmr
