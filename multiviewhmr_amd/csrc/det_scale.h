// Deterministic mode: the fixed-point format of the feature gradient and the helpers of the scale pass that chooses it.
// The pass itself -- every kernel, the layout of its scratch and its one launcher -- is unproject_det.hip.
//
// One power-of-two exponent K[b][c] per sample and channel, chosen before any tap is added so that N * bound * 2^K < 2^62, where N is the
// voxels per sample and bound an upper limit of |ds| over the sample's voxels and views.  A pixel receives at most one tap per voxel and
// view, so no int64 sum can overflow.  Every contribution llrint(ds * w * 2^K) is exact whenever it is at least 2^-41 of the bound, and
// integer addition is associative: the sums carry the same bits in any arrival order.  A (b, c) whose bound is not finite is poisoned
// (K = kDetPoison): it adds nothing and its gradient is NaN.
//
// The bound, by what the call selects (k_det_exponent; the same table with its reasons is DESIGN.md 5.7).  g = max |grad_out| of the (b, c)
// row, F = max |feature| of (b, c), n_b / wmax_b / cmax_b the sample's present views / largest view weight / largest confidence pixel:
//
//     selection          softmax                     sum          mean                max
//     plain, lens        g (1 + 2F), F: all pixels   g            g / V               g
//     view mask          as plain                    g            g / max(n_b, 1)     g
//     view weights       as plain                    g wmax_b     g                   g
//     visible            F: marked pixels            g            g                   g
//     confidence         F: marked pixels            g cmax_b     g
//     shared             plain's, then K -= ceil log2 cnt_b (cnt_b volumes name sample b; cnt_b = 0: K = 0 whatever the tables hold)
//     moments            g_m + 4 g_v F (g_m, g_v: the mean and variance halves of grad_out), F: marked pixels
//
// (moments: ds = (2 g_v / n) (s_v - mu) + g_m / n with n >= 1 and |s_v - mu| <= 2F.)  The marked pixels are those a voxel-view that takes
// part taps (k_det_mark): a non-finite value elsewhere must neither poison the (b, c) nor widen its scale.
#pragma once
#include <hip/hip_runtime.h>
#include "device_common.h"

namespace mvhmr {

constexpr int kDetPoison = 0x7fffffff;

// ds * w (fp32, as the default route rounds it) scaled by 2^k (exact) and rounded to the nearest integer, as the u64 an atomic adds
__device__ __forceinline__ unsigned long long det_fixed(float x, int k)
{
    return (unsigned long long)(long long)__builtin_rintf(__builtin_ldexpf(x, k));
}

// an accumulated sum back as fp32: the one rounding of the deterministic gradient (NaN for a poisoned (b, c))
__device__ __forceinline__ float det_value(unsigned long long acc, int k)
{
    if (k == kDetPoison) return __builtin_nanf("");
    return (float)ldexp((double)(long long)acc, -k);
}

// Maxima are taken with integer atomicMax on the bits of |x|: non-negative floats order as integers, and Inf / NaN sort above every finite
// value, so the result does not depend on the order and a non-finite input is seen
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

inline int log2_ceil(long long N) { return N > 1 ? 64 - __builtin_clzll((unsigned long long)(N - 1)) : 0; }   // N <= 2^log2_ceil(N)
// blocks along a row of N elements for the grid-stride maxima: 2048 elements each, at most 64
inline unsigned chunks_of(long long N)
{
    const long long c = (N + 2047) / 2048;
    return (unsigned)(c < 1 ? 1 : c > 64 ? 64 : c);
}

// Which row of grad_out block x of k_det_gmax reads and which slot of the table it raises; false: the block has nothing to do.
// Identity: row x of a (rows, N) tensor into slot x.
struct DetRowsIdentity {
    __device__ __forceinline__ bool map(long long x, long long &src, long long &dst) const { src = dst = x; return true; }
};
// Cross-view variance: x = (b * C + c) * halves + h over the (B, halves * C, N) gradient; the last half is the variance half and goes to
// the second table, which lies BC slots behind the first.  One half: the variance alone (the first table stays 0).
struct DetRowsMoments {
    int C, halves;
    long long BC;
    __device__ __forceinline__ bool map(long long x, long long &src, long long &dst) const
    {
        const long long row = x / halves, b = row / C, c = row % C;
        const int h = (int)(x % halves);
        src = (b * halves + h) * C + c;
        dst = (h == halves - 1 ? BC : 0) + row;
        return true;
    }
};
// Shared feature maps: x = m * C + c over the (M, C, N) gradient, reduced over the volumes of a sample into slot feature_index[m] * C + c;
// an index outside [0, B) names no sample
struct DetRowsShared {
    const int *fidx;
    int B, C;
    __device__ __forceinline__ bool map(long long x, long long &src, long long &dst) const
    {
        const int m = (int)(x / C), fb = uniform(fidx[m]);
        src = x;
        dst = (long long)fb * C + (x - (long long)m * C);
        return (unsigned)fb < (unsigned)B;
    }
};

// Camera-view maps: x = (b * V + v) * C + c over the (B, V, C, N) gradient of a projected volume, reduced over the views into slot b * C + c
struct DetRowsViews {
    int V, C;
    __device__ __forceinline__ bool map(long long x, long long &src, long long &dst) const
    {
        src = x;
        dst = x / ((long long)V * C) * C + x % C;
        return true;
    }
};

// max |grad_out| of each row of a (rows, N) tensor: block (row, chunk).  Also the row maxima of the grad_confidence stream
// (unproject_confidence.hip), hence in this header.  The map's fields are the kernel's trailing arguments, so the identity instances take
// exactly the three arguments they always took.
template <typename TO, typename ROWS, typename... FIELDS>
__global__ void __launch_bounds__(256) k_det_gmax(const TO *__restrict__ grad_out, unsigned *__restrict__ gmax, long long N, FIELDS... fields)
{
    const ROWS rows{fields...};
    long long src, dst;
    if (!rows.map(blockIdx.x, src, dst)) return;
    const TO *g = grad_out + src * N;
    unsigned m = 0;
    for (long long n = (long long)blockIdx.y * 256 + threadIdx.x; n < N; n += (long long)gridDim.y * 256) {
        const unsigned a = abs_bits(to_f32<TO>(g[n]));
        m = a > m ? a : m;
    }
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(gmax + dst, m);
}

}  // namespace mvhmr
