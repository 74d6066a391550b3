// Trilinear volume sampling at world points (include/mvhmr_unproject.h: mvhmr_sample_volume_*): reads (B,C,X,Y,Z)
// volumes that live on the cuboid recipe back at N world points per sample, the step after un-projection and soft-argmax.
//
// Arithmetic contract (tests/volsample_oracle.py restates it in numpy, operation for operation; every line one rounded fp32 operation):
//   y_i = fsub(x_i, c_i)
//   d_a = fma(R[2][a], y_2, fma(R[1][a], y_1, fmul(R[0][a], y_0)))          R^T y: voxel_xyz's order mirrored
//   o_a = fsub(c_a, p_a)
//   t_a = fdiv(fadd(d_a, o_a), step_a)                                      the continuous voxel index, the `index` output
//   a point is live iff -1 < t_a < S_a on every axis (a NaN fails); a dead point samples 0 and takes part in no gradient
//   i0 = floor(t),  w1_a = fsub(t_a, i0_a),  w0_a = fsub(fadd(i0_a, 1), t_a),  w(dx,dy,dz) = fmul(fmul(wx, wy), wz)
//   sample = fma chain over the taps in the order dx*4 + dy*2 + dz; a tap outside the grid or of weight exactly 0 is skipped (not read)
// Volume gradient: per chunk of kVsChunk points the live taps are ranked by (voxel, point) through keys staged in LDS (k_vs3d_sort);
// one thread per (segment head, channel) then sums its segment in that order, acc = fma(w, g, acc) from fmul(w, g), and adds the sum
// to the stored value with a plain store (k_vs3d_bwd_vol_sum, one launch per chunk: the stream orders the chunks).  No atomics.
// Geometry gradient: q = dL/dt per point with out-of-grid taps as value 0 (zero-weight taps ARE read here: the slope at a node needs
// its neighbour), channels in index order inside one lane; u = fdiv(q, step); grad_points = R u; grad_rot and grad_center sum over the
// points in index order (k_vs3d_pose_grad).
#include "device_common.h"
#include "kernels.h"
#include "mvhmr_unproject.h"
#include "volume_taps.h"

#include <type_traits>

namespace mvhmr {

namespace {

constexpr int kVsTile = 64;                     // points per block of the per-point kernels: one lane each
constexpr int kVsGroup = 32;                    // channels per block (forward, volume-gradient sum)
constexpr int kVsUnroll = 4;                    // channels per loop trip of the forward: 4 x 8 taps = 32 loads in flight per lane
constexpr int kVsChunk = 256;                   // P: points per sort-and-sum pass; its 2048 8-byte keys take 16 KB of LDS
constexpr int kVsEntries = kVsChunk * 8;
constexpr int kVsHeader = 16;                   // bytes in front of a chunk's table: the number of live taps
constexpr size_t kVsTableBytes = kVsHeader + (size_t)kVsEntries * 12;      // + voxel (int), weight (float), point (int) per entry
constexpr unsigned long long kVsDead = ~0ull;

// (VsTaps, vs_index, vs_live, vs_taps, vs_sample: volume_taps.h, shared with volume_project.hip)

// ---- forward: one lane per point of a tile of 64, a loop over the block's channel group; grid (B * tiles, channel groups)
template <typename T, bool PAIRED>
__global__ void __launch_bounds__(kVsTile)
k_vs3d_fwd(const T *__restrict__ vol, const Coords cs, const float *__restrict__ points, int C, int X, int N, int tiles,
           float *__restrict__ samples, float *__restrict__ index)
{
    const int b = blockIdx.x / tiles, n = (blockIdx.x % tiles) * kVsTile + threadIdx.x;
    if (n >= N) return;
    const int Y = cs.Y, Z = cs.Z;
    const float *x = points + ((size_t)b * N + n) * 3;
    float t[3], y[3];
    vs_index(cs, b, x[0], x[1], x[2], t, y);
    if (blockIdx.y == 0) {
        float *o = index + ((size_t)b * N + n) * 3;
        o[0] = t[0]; o[1] = t[1]; o[2] = t[2];
    }
    VsTaps tp;
    vs_taps(t, vs_live(t, X, Y, Z), X, Y, Z, tp);
    const size_t V = (size_t)X * Y * Z;
    if constexpr (PAIRED) {
        samples[(size_t)b * C + n] = vs_sample<T>(vol + ((size_t)b * C + n) * V, tp);
    } else {
        const int c0 = blockIdx.y * kVsGroup, c1 = min(c0 + kVsGroup, C);
        int c = c0;
        for (; c + kVsUnroll <= c1; c += kVsUnroll) {
            const T *plane = vol + ((size_t)b * C + c) * V;
            float v[kVsUnroll][8];
#pragma unroll
            for (int u = 0; u < kVsUnroll; ++u)
#pragma unroll
                for (int k = 0; k < 8; ++k) v[u][k] = (tp.live >> k) & 1u ? to_f32<T>(plane[u * V + tp.off[k]]) : 0.f;
#pragma unroll
            for (int u = 0; u < kVsUnroll; ++u) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc = (tp.live >> k) & 1u ? __fmaf_rn(tp.w[k], v[u][k], acc) : acc;
                samples[((size_t)b * C + c + u) * N + n] = acc;
            }
        }
        for (; c < c1; ++c) samples[((size_t)b * C + c) * N + n] = vs_sample<T>(vol + ((size_t)b * C + c) * V, tp);
    }
}

// ---- volume gradient, first launch: block (sample, chunk) ranks the chunk's live taps by (voxel, point) and writes them in that order
__global__ void __launch_bounds__(kVsChunk)
k_vs3d_sort(const float *__restrict__ index, int X, int Y, int Z, int N, int chunks, unsigned char *__restrict__ ws)
{
    __shared__ unsigned long long keys[kVsEntries];
    const int b = blockIdx.x / chunks, chunk = blockIdx.x % chunks, p = threadIdx.x, n = chunk * kVsChunk + p;
    float t[3] = {0.f, 0.f, 0.f};
    if (n < N) {
        const float *i = index + ((size_t)b * N + n) * 3;
        t[0] = i[0]; t[1] = i[1]; t[2] = i[2];
    }
    VsTaps tp;
    vs_taps(t, n < N && vs_live(t, X, Y, Z), X, Y, Z, tp);
    unsigned long long mine[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        mine[k] = (tp.live >> k) & 1u ? ((unsigned long long)(unsigned)tp.off[k] << 8) | (unsigned)p : kVsDead;
        keys[p * 8 + k] = mine[k];
    }
    __syncthreads();
    int rank[8] = {0, 0, 0, 0, 0, 0, 0, 0}, count = 0;
    for (int i = 0; i < kVsEntries; ++i) {
        const unsigned long long key = keys[i];
        count += key != kVsDead;
#pragma unroll
        for (int k = 0; k < 8; ++k) rank[k] += key < mine[k];
    }
    unsigned char *table = ws + (size_t)blockIdx.x * kVsTableBytes;
    int *voxel = reinterpret_cast<int *>(table + kVsHeader);
    float *weight = reinterpret_cast<float *>(voxel + kVsEntries);
    int *point = reinterpret_cast<int *>(weight + kVsEntries);
    if (p == 0) *reinterpret_cast<int *>(table) = count;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if ((tp.live >> k) & 1u) { voxel[rank[k]] = tp.off[k]; weight[rank[k]] = tp.w[k]; point[rank[k]] = n; }     // live keys are unique: rank < count
}

// ---- volume gradient, one launch per chunk: thread = sorted position; a segment head sums its segment per channel of the block's
// group and adds the sum to the voxel it alone owns in this launch.  grid (B * kVsEntries / 256, channel groups)
template <typename T>
__global__ void __launch_bounds__(256)
k_vs3d_bwd_vol_sum(const unsigned char *__restrict__ ws, const float *__restrict__ gs, int C, size_t V, int N, int chunks, int chunk,
                   T *__restrict__ grad_vol)
{
    constexpr int per = kVsEntries / 256;
    const int b = blockIdx.x / per, pos = (blockIdx.x % per) * 256 + threadIdx.x;
    const unsigned char *table = ws + ((size_t)b * chunks + chunk) * kVsTableBytes;
    const int count = *reinterpret_cast<const int *>(table);
    if (pos >= count) return;
    const int *voxel = reinterpret_cast<const int *>(table + kVsHeader);
    const float *weight = reinterpret_cast<const float *>(voxel + kVsEntries);
    const int *point = reinterpret_cast<const int *>(weight + kVsEntries);
    const int vox = voxel[pos];
    if (pos > 0 && voxel[pos - 1] == vox) return;
    int end = pos + 1;
    while (end < count && voxel[end] == vox) ++end;
    const int c1 = min((int)(blockIdx.y + 1) * kVsGroup, C);
    for (int c = blockIdx.y * kVsGroup; c < c1; ++c) {
        const float *g = gs + ((size_t)b * C + c) * N;
        float acc = __fmul_rn(weight[pos], g[point[pos]]);
        for (int j = pos + 1; j < end; ++j) acc = __fmaf_rn(weight[j], g[point[j]], acc);
        T *dst = grad_vol + ((size_t)b * C + c) * V + vox;
        *dst = from_f32<T>(__fadd_rn(to_f32<T>(*dst), acc));
    }
}

// ---- volume gradient of a paired call: point j alone writes channel j, nothing collides; one lane per point
template <typename T>
__global__ void __launch_bounds__(kVsTile)
k_vs3d_bwd_vol_paired(const float *__restrict__ index, const float *__restrict__ gs, int X, int Y, int Z, int N, int tiles, T *__restrict__ grad_vol)
{
    const int b = blockIdx.x / tiles, n = (blockIdx.x % tiles) * kVsTile + threadIdx.x;
    if (n >= N) return;
    const float *i = index + ((size_t)b * N + n) * 3;
    const float t[3] = {i[0], i[1], i[2]};
    VsTaps tp;
    vs_taps(t, vs_live(t, X, Y, Z), X, Y, Z, tp);
    const float g = gs[(size_t)b * N + n];
    T *plane = grad_vol + ((size_t)b * N + n) * ((size_t)X * Y * Z);
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if ((tp.live >> k) & 1u) plane[tp.off[k]] = from_f32<T>(__fadd_rn(0.f, __fmul_rn(tp.w[k], g)));
}

// ---- geometry gradient, first launch: one lane per point, the channels in index order inside the lane.  Per channel, with v the eight
// tap values (0 outside the grid) and e = fsub(v[hi], v[lo]) along an axis:  s_x = fma chain over (dy, dz) of fmul(wy, wz) * e, likewise
// s_y over (dx, dz) and s_z over (dx, dy);  q_a = fma(g, s_a, q_a) from 0.  u = fdiv(q, step), (u, live) to ws (B,N,4), grad_points = R u.
template <typename T, bool PAIRED>
__global__ void __launch_bounds__(kVsTile)
k_vs3d_bwd_point(const T *__restrict__ vol, const Coords cs, const float *__restrict__ index, const float *__restrict__ gs, int C, int X, int N,
                 int tiles, float *__restrict__ grad_points, float *__restrict__ ws)
{
    const int b = blockIdx.x / tiles, n = (blockIdx.x % tiles) * kVsTile + threadIdx.x;
    if (n >= N) return;
    const int Y = cs.Y, Z = cs.Z;
    const float *i = index + ((size_t)b * N + n) * 3;
    const float t[3] = {i[0], i[1], i[2]};
    const bool live = vs_live(t, X, Y, Z);
    VsTaps tp;
    vs_taps(t, live, X, Y, Z, tp);
    const size_t V = (size_t)X * Y * Z;
    float q[3] = {0.f, 0.f, 0.f};
    const int c0 = PAIRED ? n : 0, c1 = PAIRED ? n + 1 : C;
    for (int c = c0; c < c1; ++c) {
        const T *plane = vol + ((size_t)b * C + c) * V;
        const float g = PAIRED ? gs[(size_t)b * C + c] : gs[((size_t)b * C + c) * N + n];
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (tp.in >> k) & 1u ? to_f32<T>(plane[tp.off[k]]) : 0.f;
        float s[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int bit = 4 >> a, a1 = a == 0 ? 1 : 0, a2 = a == 2 ? 1 : 2;          // the two other axes, in axis order
            float acc = 0.f;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int d1 = m >> 1, d2 = m & 1, lo = d1 * (4 >> a1) + d2 * (4 >> a2);
                const float e = __fsub_rn(v[lo + bit], v[lo]), w = __fmul_rn(tp.wa[a1][d1], tp.wa[a2][d2]);
                acc = m == 0 ? __fmul_rn(w, e) : __fmaf_rn(w, e, acc);
            }
            s[a] = acc;
        }
        q[0] = __fmaf_rn(g, s[0], q[0]); q[1] = __fmaf_rn(g, s[1], q[1]); q[2] = __fmaf_rn(g, s[2], q[2]);
    }
    const float u0 = live ? __fdiv_rn(q[0], cs.sx) : 0.f, u1 = live ? __fdiv_rn(q[1], cs.sy) : 0.f, u2 = live ? __fdiv_rn(q[2], cs.sz) : 0.f;
    *reinterpret_cast<float4 *>(ws + ((size_t)b * N + n) * 4) = make_float4(u0, u1, u2, live ? 1.f : 0.f);
    if (grad_points) {
        const float *R = cs.rot + b * 9;
        float *o = grad_points + ((size_t)b * N + n) * 3;
        o[0] = __fmaf_rn(R[2], u2, __fmaf_rn(R[1], u1, __fmul_rn(R[0], u0)));
        o[1] = __fmaf_rn(R[5], u2, __fmaf_rn(R[4], u1, __fmul_rn(R[3], u0)));
        o[2] = __fmaf_rn(R[8], u2, __fmaf_rn(R[7], u1, __fmul_rn(R[6], u0)));
    }
}

// ---- geometry gradient, second launch: one thread per entry of (B, 9 + 3), the live points in index order (a dead point is skipped:
// its y may be NaN).  grad_rot[i][a]: acc = fma(fsub(x_i, c_i), u_a, acc);  grad_center[a]: acc = fadd(acc, fsub(u_a, (R u)_a))
__global__ void __launch_bounds__(64)
k_vs3d_pose_grad(const float *__restrict__ points, const float *__restrict__ rot, const float *__restrict__ center, const float *__restrict__ ws,
                 float *__restrict__ grad_rot, float *__restrict__ grad_center, int B, int N)
{
    const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= (long long)B * 12) return;
    const long long b = idx / 12;
    const int e = (int)(idx % 12);
    float acc = 0.f;
    if (e < 9) {
        if (!grad_rot) return;
        const int i = e / 3, a = e % 3;
        const float ci = center[b * 3 + i];
        for (int n = 0; n < N; ++n) {
            const float4 u = *reinterpret_cast<const float4 *>(ws + (b * N + n) * 4);
            if (u.w == 0.f) continue;
            const float ua = a == 0 ? u.x : a == 1 ? u.y : u.z;
            acc = __fmaf_rn(__fsub_rn(points[(b * N + n) * 3 + i], ci), ua, acc);
        }
        grad_rot[b * 9 + e] = acc;
    } else {
        if (!grad_center) return;
        const int a = e - 9;
        const float *R = rot + b * 9 + a * 3;
        for (int n = 0; n < N; ++n) {
            const float4 u = *reinterpret_cast<const float4 *>(ws + (b * N + n) * 4);
            if (u.w == 0.f) continue;
            const float ua = a == 0 ? u.x : a == 1 ? u.y : u.z;
            acc = __fadd_rn(acc, __fsub_rn(ua, __fmaf_rn(R[2], u.z, __fmaf_rn(R[1], u.y, __fmul_rn(R[0], u.x)))));
        }
        grad_center[b * 3 + a] = acc;
    }
}

template <typename F> hipError_t with_storage(int dtype, F f)
{
    switch (dtype) {
    case MVHMR_F32: return f((float *)nullptr);
    case MVHMR_F16: return f((__half *)nullptr);
    case MVHMR_BF16: return f((bf16_t *)nullptr);
    }
    return hipErrorNotSupported;
}

int vs_tiles(int N) { return (N + kVsTile - 1) / kVsTile; }
int vs_chunks(long long N) { return (int)((N + kVsChunk - 1) / kVsChunk); }
int vs_groups(int C) { return (C + kVsGroup - 1) / kVsGroup; }
bool vs_grid_ok(long long x, long long y) { return x <= 0x7fffffffLL && y <= 65535; }

}  // namespace

int vs3d_chunk_points() { return kVsChunk; }

// the sorted tap tables of every (sample, chunk); the geometry gradient's (B,N,4) floats fit in front of them
size_t vs3d_workspace_bytes(long long B, long long N) { return (size_t)B * (size_t)vs_chunks(N) * kVsTableBytes; }

hipError_t launch_vs3d_forward(const void *vol, int dtype, const Coords &cs, const float *points, int B, int C, int X, int N, int paired,
                               float *samples, float *index, hipStream_t s)
{
    const int tiles = vs_tiles(N), groups = paired ? 1 : vs_groups(C);
    if (!vs_grid_ok((long long)B * tiles, groups)) return hipErrorNotSupported;
    return with_storage(dtype, [&](auto *tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        const dim3 grid((unsigned)(B * tiles), (unsigned)groups);
        if (paired)
            hipLaunchKernelGGL((k_vs3d_fwd<T, true>), grid, dim3(kVsTile), 0, s, static_cast<const T *>(vol), cs, points, C, X, N, tiles, samples, index);
        else
            hipLaunchKernelGGL((k_vs3d_fwd<T, false>), grid, dim3(kVsTile), 0, s, static_cast<const T *>(vol), cs, points, C, X, N, tiles, samples, index);
        return hipGetLastError();
    });
}

hipError_t launch_vs3d_backward_volumes(int dtype, const float *index, const float *grad_samples, int B, int C, int X, int Y, int Z, int N, int paired,
                                        void *grad_vol, void *ws, hipStream_t s)
{
    const size_t V = (size_t)X * Y * Z;
    const int tiles = vs_tiles(N), chunks = vs_chunks(N), groups = vs_groups(C);
    if (!vs_grid_ok((long long)B * tiles, 1) || !vs_grid_ok((long long)B * chunks, groups) || !vs_grid_ok((long long)B * (kVsEntries / 256), groups))
        return hipErrorNotSupported;
    return with_storage(dtype, [&](auto *tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        hipError_t e = hipMemsetAsync(grad_vol, 0, (size_t)B * C * V * sizeof(T), s);
        if (e != hipSuccess) return e;
        if (paired) {
            hipLaunchKernelGGL((k_vs3d_bwd_vol_paired<T>), dim3((unsigned)(B * tiles)), dim3(kVsTile), 0, s, index, grad_samples, X, Y, Z, N, tiles,
                               static_cast<T *>(grad_vol));
            return hipGetLastError();
        }
        hipLaunchKernelGGL(k_vs3d_sort, dim3((unsigned)(B * chunks)), dim3(kVsChunk), 0, s, index, X, Y, Z, N, chunks, static_cast<unsigned char *>(ws));
        if ((e = hipGetLastError()) != hipSuccess) return e;
        for (int chunk = 0; chunk < chunks; ++chunk) {
            hipLaunchKernelGGL((k_vs3d_bwd_vol_sum<T>), dim3((unsigned)(B * (kVsEntries / 256)), (unsigned)groups), dim3(256), 0, s,
                               static_cast<const unsigned char *>(ws), grad_samples, C, V, N, chunks, chunk, static_cast<T *>(grad_vol));
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        return hipSuccess;
    });
}

hipError_t launch_vs3d_backward_geometry(const void *vol, int dtype, const Coords &cs, const float *points, const float *index, const float *grad_samples,
                                         int B, int C, int X, int N, int paired, float *grad_points, float *grad_rot, float *grad_center, float *ws,
                                         hipStream_t s)
{
    const int tiles = vs_tiles(N);
    if (!vs_grid_ok((long long)B * tiles, 1)) return hipErrorNotSupported;
    hipError_t e = with_storage(dtype, [&](auto *tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        if (paired)
            hipLaunchKernelGGL((k_vs3d_bwd_point<T, true>), dim3((unsigned)(B * tiles)), dim3(kVsTile), 0, s, static_cast<const T *>(vol), cs, index,
                               grad_samples, C, X, N, tiles, grad_points, ws);
        else
            hipLaunchKernelGGL((k_vs3d_bwd_point<T, false>), dim3((unsigned)(B * tiles)), dim3(kVsTile), 0, s, static_cast<const T *>(vol), cs, index,
                               grad_samples, C, X, N, tiles, grad_points, ws);
        return hipGetLastError();
    });
    if (e != hipSuccess || (!grad_rot && !grad_center)) return e;
    hipLaunchKernelGGL(k_vs3d_pose_grad, dim3((unsigned)(((long long)B * 12 + 63) / 64)), dim3(64), 0, s, points, cs.rot, cs.center, ws, grad_rot,
                       grad_center, B, N);
    return hipGetLastError();
}

}  // namespace mvhmr
