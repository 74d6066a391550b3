// 3-D non-maximum suppression and top-K proposals (include/mvhmr_unproject.h: mvhmr_volume_peaks*): the K largest local
// maxima of every (b, j) slice of (B,J,X,Y,Z) heat volumes, in about one read of the volume and O(B J K) numbers written.
//
// Contract (tests/peaks_oracle.py restates it in numpy):
//   key(v)   = 0xffffffff for a NaN; else with u the bits of v and -0 folded onto +0:  u | 0x80000000 for u >= 0,  ~u for u < 0.
//              Integer order of the keys is the order of the reals, -inf (0x007fffff) lowest; outside the volume counts as key 0.
//   box max  = max over z, then over y, then over x of the keys: three separable integer maxima, each exact, so their composition is the
//              maximum of the clipped box whatever the order.  A NaN in the box makes the maximum 0xffffffff, which no peak equals.
//   peak     = key(v_n) != 0xffffffff, key(v_n) == box max, key(v_n) > key(threshold)
//   ranking  = the 64-bit key (key(v_n) << 32) | ~n: descending integer order is value descending, then index ascending; keys of
//              different voxels differ, so the K best of any set do not depend on the order the set was produced in; 0 means "no entry"
// One block owns a strip (kPkXRun planes x kPkTY x kPkTZ) of one slice and marches along X: a plane with its Y/Z halo goes through LDS
// for the in-plane maxima, the 2r+1 planes of in-plane maxima and the r+1 planes of centre keys live in registers (shifted, statically
// indexed).  Peaks better than the block's K-th best so far wait in an LDS buffer; when the buffer could overflow, and at the end, a
// bitonic sort keeps the K best.  k_pk3d_merge does the same over the blocks' lists of a slice and writes scores, index and positions.
#include "device_common.h"
#include "kernels.h"
#include "mvhmr_unproject.h"

namespace mvhmr {

namespace {

constexpr int kPkThreads = 256;
constexpr int kPkXRun = 32, kPkTY = 16, kPkTZ = 64;            // the strip of one block
constexpr int kPkMaxK = 128;
constexpr int kPkPlane = kPkTY * kPkTZ;                        // voxels of one plane of the strip: the most peaks one step can add
constexpr int kPkVpt = kPkPlane / kPkThreads;                  // voxels per lane and plane
constexpr int kPkSortN = 2048;                                 // entries of the sort buffer: the list (K) and the waiting peaks
constexpr int kPkCap = kPkSortN - kPkMaxK;                     // peaks that may wait
constexpr unsigned kPkNanKey = 0xffffffffu;
constexpr long long kPkMaxBlocks = (1LL << 24) - 1;            // a launch holds fewer than 2^32 threads along x: 2^24 - 1 blocks of 256
static_assert(kPkPlane % kPkThreads == 0 && kPkCap >= kPkPlane, "a whole plane of peaks must fit behind the peaks that were left waiting");

typedef unsigned long long u64;

__host__ __device__ inline unsigned pk_key(float v)
{
    unsigned u = __builtin_bit_cast(unsigned, v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return kPkNanKey;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// buf[0, K): the list, sorted descending, 0 = empty; buf[K, K + c): entries in any order (0 = none).  Afterwards buf[0, K) holds the K
// largest of all of them, sorted descending.  Every thread of the block calls it with the same arguments; it ends behind a barrier.
__device__ void pk_absorb(u64 *buf, int K, int c)
{
    const int n = K + c, tid = threadIdx.x;
    int n2 = 2;
    while (n2 < n) n2 <<= 1;
    for (int i = n + tid; i < n2; i += kPkThreads) buf[i] = 0;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += kPkThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const u64 a = buf[i], b = buf[l];
                if ((i & k) == 0 ? a < b : a > b) { buf[i] = b; buf[l] = a; }
            }
            __syncthreads();
        }
}

// ---- first launch: one block per (slice, strip); its K best peaks to ws[(slice * bps + strip) * K ...]
template <typename T, int R>
__global__ void __launch_bounds__(kPkThreads)
k_pk3d_strips(const T *__restrict__ vol, int X, int Y, int Z, int nyt, int nzt, unsigned bps, int K, unsigned tkey, u64 *__restrict__ ws)
{
    constexpr int HY = kPkTY + 2 * R, HZ = kPkTZ + 2 * R;
    constexpr int NPF = (HY * HZ + kPkThreads - 1) / kPkThreads, NZM = (HY * kPkTZ + kPkThreads - 1) / kPkThreads;
    __shared__ unsigned sA[HY * HZ];                           // keys of one plane with halo
    __shared__ unsigned sB[HY * kPkTZ];                        // their maxima along z
    __shared__ u64 buf[kPkSortN];
    __shared__ int cnt;

    const int tid = threadIdx.x;
    const unsigned slice = blockIdx.x / bps, strip = blockIdx.x % bps;
    const int zt = (int)(strip % (unsigned)nzt), yt = (int)((strip / (unsigned)nzt) % (unsigned)nyt), xt = (int)(strip / ((unsigned)nzt * (unsigned)nyt));
    const int x0 = xt * kPkXRun, x1 = min(x0 + kPkXRun, X), y0 = yt * kPkTY, z0 = zt * kPkTZ;
    const size_t plane = (size_t)Y * Z;
    const T *sl = vol + (size_t)slice * plane * X;

    for (int i = tid; i < K; i += kPkThreads) buf[i] = 0;
    if (tid == 0) cnt = 0;

    int off[NPF];                                              // in-plane offset of the halo elements this lane stages, -1 outside
#pragma unroll
    for (int e = 0; e < NPF; ++e) {
        const int idx = tid + e * kPkThreads, yy = idx / HZ, zz = idx % HZ, gy = y0 - R + yy, gz = z0 - R + zz;
        off[e] = (idx < HY * HZ && gy >= 0 && gy < Y && gz >= 0 && gz < Z) ? gy * Z + gz : -1;
    }
    unsigned pf[NPF];
    auto load_plane = [&](int p) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < NPF; ++e) pf[e] = off[e] >= 0 ? pk_key(to_f32<T>(sl[(size_t)p * plane + off[e]])) : 0u;
    };

    unsigned m2[2 * R + 1][kPkVpt], raw[R + 1][kPkVpt];        // planes p - 2R .. p of in-plane maxima, p - R .. p of centre keys
#pragma unroll
    for (int v = 0; v < kPkVpt; ++v) {
#pragma unroll
        for (int i = 0; i <= 2 * R; ++i) m2[i][v] = 0u;
#pragma unroll
        for (int i = 0; i <= R; ++i) raw[i][v] = 0u;
    }

    u64 kth = 0;                                               // the K-th best so far, 0 while the list is not full
    const int pfirst = x0 - R, plast = x1 - 1 + R;
    load_plane(max(pfirst, 0));
    for (int p = pfirst; p <= plast; ++p) {
        const bool in = p >= 0 && p < X;                       // block-uniform
        if (in) {
#pragma unroll
            for (int e = 0; e < NPF; ++e)
                if (tid + e * kPkThreads < HY * HZ) sA[tid + e * kPkThreads] = pf[e];
            if (p + 1 <= plast && p + 1 < X) load_plane(p + 1);                         // the next plane's loads fly under this plane's maxima
        }
        __syncthreads();
        const int waiting = cnt;
        if (waiting > kPkCap - kPkPlane) {                     // the coming plane might not fit: keep the K best (block-uniform)
            pk_absorb(buf, K, waiting);
            kth = buf[K - 1];
            if (tid == 0) cnt = 0;
        }
        unsigned nm[kPkVpt], nr[kPkVpt];
#pragma unroll
        for (int v = 0; v < kPkVpt; ++v) { nm[v] = 0u; nr[v] = 0u; }
        if (in) {
#pragma unroll
            for (int e = 0; e < NZM; ++e) {
                const int idx = tid + e * kPkThreads;
                if (idx < HY * kPkTZ) {
                    const unsigned *row = sA + (idx / kPkTZ) * HZ + idx % kPkTZ;
                    unsigned m = row[0];
#pragma unroll
                    for (int d = 1; d <= 2 * R; ++d) m = max(m, row[d]);
                    sB[idx] = m;
                }
            }
#pragma unroll
            for (int v = 0; v < kPkVpt; ++v) {
                const int idx = tid + v * kPkThreads;
                nr[v] = sA[(idx / kPkTZ + R) * HZ + idx % kPkTZ + R];
            }
        }
        __syncthreads();
        if (in) {
#pragma unroll
            for (int v = 0; v < kPkVpt; ++v) {
                const int idx = tid + v * kPkThreads;
                unsigned m = sB[idx];
#pragma unroll
                for (int d = 1; d <= 2 * R; ++d) m = max(m, sB[idx + d * kPkTZ]);
                nm[v] = m;
            }
        }
        const int xc = p - R;                                  // the plane whose box is complete now
#pragma unroll
        for (int v = 0; v < kPkVpt; ++v) {
#pragma unroll
            for (int i = 0; i < 2 * R; ++i) m2[i][v] = m2[i + 1][v];
            m2[2 * R][v] = nm[v];
#pragma unroll
            for (int i = 0; i < R; ++i) raw[i][v] = raw[i + 1][v];
            raw[R][v] = nr[v];
            if (xc < x0) continue;
            unsigned m3 = m2[0][v];
#pragma unroll
            for (int i = 1; i <= 2 * R; ++i) m3 = max(m3, m2[i][v]);
            const unsigned key = raw[0][v];
            const int idx = tid + v * kPkThreads, gy = y0 + idx / kPkTZ, gz = z0 + idx % kPkTZ;
            if (gy < Y && gz < Z && key != kPkNanKey && key == m3 && key > tkey) {
                const unsigned n = (unsigned)(((size_t)xc * Y + gy) * Z + gz);
                const u64 k64 = ((u64)key << 32) | (u64)(~n);
                if (k64 > kth) buf[K + atomicAdd(&cnt, 1)] = k64;                       // arrival order is sorted away: the keys are distinct
            }
        }
    }
    __syncthreads();
    const int waiting = cnt;
    if (waiting > 0) pk_absorb(buf, K, waiting);
    u64 *o = ws + ((size_t)slice * bps + strip) * K;
    for (int i = tid; i < K; i += kPkThreads) o[i] = buf[i];
}

// ---- second launch: one block per slice keeps the K best of its strips' lists and writes the outputs
template <typename T>
__global__ void __launch_bounds__(kPkThreads)
k_pk3d_merge(const u64 *__restrict__ ws, const T *__restrict__ vol, const Coords cs, int J, long long N, unsigned bps, int K,
             float *__restrict__ scores, int *__restrict__ index, float *__restrict__ positions)
{
    __shared__ u64 buf[kPkSortN];
    const int tid = threadIdx.x;
    const size_t slice = blockIdx.x;
    const long long total = (long long)bps * K;
    const u64 *src = ws + slice * (size_t)total;
    for (int i = tid; i < K; i += kPkThreads) buf[i] = 0;
    u64 kth = 0;
    for (long long base = 0; base < total; base += kPkCap) {
        const int c = (int)min((long long)kPkCap, total - base);
        for (int i = tid; i < c; i += kPkThreads) {
            const u64 k = src[base + i];
            buf[K + i] = k > kth ? k : 0;
        }
        pk_absorb(buf, K, c);
        kth = buf[K - 1];
    }
    for (int s = tid; s < K; s += kPkThreads) {
        const u64 k = buf[s];
        const size_t o = slice * K + s;
        float x = 0.f, y = 0.f, z = 0.f;
        if (k == 0) {
            scores[o] = -__builtin_inff();
            index[o] = -1;
        } else {
            const unsigned n = ~(unsigned)(k & 0xffffffffu);
            scores[o] = to_f32<T>(vol[slice * (size_t)N + n]);                          // the stored bits, -0 included
            index[o] = (int)n;
            if (positions) voxel_xyz(cs, (int)(slice / (size_t)J), N, (long long)n, x, y, z);
        }
        if (positions) { positions[o * 3] = x; positions[o * 3 + 1] = y; positions[o * 3 + 2] = z; }
    }
}

// ---- backward w.r.t. the volume, after the zero fill: one thread per slot, plain stores (the indices of a slice are distinct)
template <typename T>
__global__ void __launch_bounds__(kPkThreads)
k_pk3d_scatter(const int *__restrict__ index, const float *__restrict__ g, long long slots, int K, long long N, T *__restrict__ grad_vol)
{
    const long long i = (long long)blockIdx.x * kPkThreads + threadIdx.x;
    if (i >= slots) return;
    const int n = index[i];
    if (n < 0 || (long long)n >= N) return;
    grad_vol[(size_t)(i / K) * (size_t)N + n] = from_f32<T>(g[i]);
}

// ---- backward of positions w.r.t. the pose: one thread per entry of (B, 9 + 3), the present slots of the sample in (j, slot) order
__global__ void __launch_bounds__(64)
k_pk3d_pose_grad(const int *__restrict__ index, const float *__restrict__ gp, const Coords cs, float *__restrict__ grad_rot,
                 float *__restrict__ grad_center, int B, int JK)
{
    const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= (long long)B * 12) return;
    const int b = (int)(idx / 12), e = (int)(idx % 12);
    const int *ix = index + (size_t)b * JK;
    const float *g = gp + (size_t)b * JK * 3;
    float acc = 0.f;
    if (e < 9) {
        if (!grad_rot) return;
        const int r = e / 3, c = e % 3;
        for (int s = 0; s < JK; ++s) {
            if (ix[s] < 0) continue;
            float d[3];
            cuboid_offset(cs, b, ix[s], d[0], d[1], d[2]);
            acc = __fmaf_rn(g[s * 3 + r], c == 0 ? d[0] : c == 1 ? d[1] : d[2], acc);
        }
        grad_rot[(size_t)b * 9 + e] = acc;
    } else {
        if (!grad_center) return;
        const int c = e - 9;
        const float *Rm = cs.rot + b * 9;
        for (int s = 0; s < JK; ++s) {
            if (ix[s] < 0) continue;
            const float *gs = g + s * 3;
            const float h = __fmaf_rn(Rm[6 + c], gs[2], __fmaf_rn(Rm[3 + c], gs[1], __fmul_rn(Rm[c], gs[0])));
            acc = __fadd_rn(acc, __fsub_rn(gs[c], h));
        }
        grad_center[(size_t)b * 3 + c] = acc;
    }
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

template <typename T>
hipError_t pk_forward(const T *vol, const Coords &cs, int B, int J, int X, int Y, int Z, int K, int radius, unsigned tkey, float *scores, int *index,
                      float *positions, u64 *ws, hipStream_t s)
{
    const int nyt = ceil_div(Y, kPkTY), nzt = ceil_div(Z, kPkTZ);
    const long long bps = pk3d_blocks_per_slice(X, Y, Z), slices = (long long)B * J;
    if (bps > kPkMaxBlocks || slices * bps > kPkMaxBlocks) return hipErrorNotSupported;
    const dim3 grid((unsigned)(slices * bps)), block(kPkThreads);
    switch (radius) {
    case 0: hipLaunchKernelGGL((k_pk3d_strips<T, 0>), grid, block, 0, s, vol, X, Y, Z, nyt, nzt, (unsigned)bps, K, tkey, ws); break;
    case 1: hipLaunchKernelGGL((k_pk3d_strips<T, 1>), grid, block, 0, s, vol, X, Y, Z, nyt, nzt, (unsigned)bps, K, tkey, ws); break;
    case 2: hipLaunchKernelGGL((k_pk3d_strips<T, 2>), grid, block, 0, s, vol, X, Y, Z, nyt, nzt, (unsigned)bps, K, tkey, ws); break;
    case 3: hipLaunchKernelGGL((k_pk3d_strips<T, 3>), grid, block, 0, s, vol, X, Y, Z, nyt, nzt, (unsigned)bps, K, tkey, ws); break;
    default: return hipErrorNotSupported;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_pk3d_merge<T>), dim3((unsigned)slices), block, 0, s, ws, vol, cs, J, (long long)X * Y * Z, (unsigned)bps, K, scores, index,
                       positions);
    return hipGetLastError();
}

template <typename T>
hipError_t pk_backward(const int *index, const float *g, long long slices, long long N, int K, T *grad_vol, hipStream_t s)
{
    const long long slots = slices * K, blocks = (slots + kPkThreads - 1) / kPkThreads;
    if (blocks > kPkMaxBlocks) return hipErrorNotSupported;
    hipError_t e = hipMemsetAsync(grad_vol, 0, (size_t)slices * (size_t)N * sizeof(T), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_pk3d_scatter<T>), dim3((unsigned)blocks), dim3(kPkThreads), 0, s, index, g, slots, K, N, grad_vol);
    return hipGetLastError();
}

}  // namespace

void pk3d_tile(int tile[3]) { tile[0] = kPkXRun; tile[1] = kPkTY; tile[2] = kPkTZ; }
int pk3d_max_k() { return kPkMaxK; }
unsigned pk3d_key(float v) { return pk_key(v); }

long long pk3d_blocks_per_slice(int X, int Y, int Z) { return (long long)ceil_div(X, kPkXRun) * ceil_div(Y, kPkTY) * ceil_div(Z, kPkTZ); }

size_t pk3d_workspace_bytes(long long B, long long J, int X, int Y, int Z, int K)
{
    return (size_t)(B * J) * (size_t)pk3d_blocks_per_slice(X, Y, Z) * (size_t)K * sizeof(u64);
}

hipError_t launch_pk3d_forward(const void *vol, int dtype, const Coords &cs, int B, int J, int X, int Y, int Z, int K, int radius, unsigned tkey,
                               float *scores, int *index, float *positions, void *ws, hipStream_t s)
{
    u64 *w = static_cast<u64 *>(ws);
    switch (dtype) {
    case MVHMR_F32: return pk_forward(static_cast<const float *>(vol), cs, B, J, X, Y, Z, K, radius, tkey, scores, index, positions, w, s);
    case MVHMR_F16: return pk_forward(static_cast<const __half *>(vol), cs, B, J, X, Y, Z, K, radius, tkey, scores, index, positions, w, s);
    case MVHMR_BF16: return pk_forward(static_cast<const bf16_t *>(vol), cs, B, J, X, Y, Z, K, radius, tkey, scores, index, positions, w, s);
    }
    return hipErrorNotSupported;
}

hipError_t launch_pk3d_backward(int dtype, const int *index, const float *grad_scores, long long slices, long long N, int K, void *grad_vol,
                                hipStream_t s)
{
    switch (dtype) {
    case MVHMR_F32: return pk_backward(index, grad_scores, slices, N, K, static_cast<float *>(grad_vol), s);
    case MVHMR_F16: return pk_backward(index, grad_scores, slices, N, K, static_cast<__half *>(grad_vol), s);
    case MVHMR_BF16: return pk_backward(index, grad_scores, slices, N, K, static_cast<bf16_t *>(grad_vol), s);
    }
    return hipErrorNotSupported;
}

hipError_t launch_pk3d_backward_pose(const int *index, const float *grad_pos, const Coords &cs, int B, int J, int K, float *grad_rot,
                                     float *grad_center, hipStream_t s)
{
    hipLaunchKernelGGL(k_pk3d_pose_grad, dim3((unsigned)(((long long)B * 12 + 63) / 64)), dim3(64), 0, s, index, grad_pos, cs, grad_rot, grad_center, B, J * K);
    return hipGetLastError();
}

}  // namespace mvhmr
