// Deterministic mode: the fixed-point format of the feature gradient (unproject_det.hip).
//
// One power-of-two exponent K[b][c] per sample and channel, chosen before any tap is added so that N * bound * 2^K < 2^62, where bound is an
// upper limit of |ds| over the sample's voxels and views (softmax max|g| * (1 + 2 Fmax), sum and max max|g|, mean max|g| / V; visibility-aware mean max|g|; per-pixel confidence: sum max|g| * the sample's largest confidence pixel, mean max|g|;
// cross-view variance (unproject_moments.hip): max|g_m| + 4 max|g_v| Fmax with g_m, g_v the mean and variance halves of grad_out and Fmax the
// largest |feature| a participating view taps -- ds = (2 g_v / n) (s_v - mu) + g_m / n with n >= 1 and |s_v - mu| <= 2 Fmax) and N the
// voxels per sample: a pixel receives at most one tap per voxel and view, so no int64 sum can overflow.  Every contribution
// llrint(ds * w * 2^K) is exact whenever it is at least 2^-41 of the bound, and integer addition is associative: the sums carry the same bits
// in any arrival order.  A (b, c) whose bound is not finite is poisoned (K = kDetPoison): it adds nothing and its gradient is NaN.
#pragma once
#include <hip/hip_runtime.h>

namespace mvhmr {

constexpr int kDetPoison = 0x7fffffff;

// ds * w (fp32, as the default route rounds it) scaled by 2^k (exact) and rounded to the nearest integer, as the u64 an atomic adds
__device__ __forceinline__ unsigned long long det_fixed(float x, int k)
{
    return (unsigned long long)(long long)__builtin_rintf(__builtin_ldexpf(x, k));
}

}  // namespace mvhmr
