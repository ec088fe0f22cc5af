// log Phi and the log of a difference of two normal cumulatives, as the fused likelihood kernels take them
// (noisy_normal_bits.hip, mixture_bits.hip).  The operation order is the reference's: the difference is taken on the
// side of the median where it does not cancel (survival functions right of it), in log space; log Phi as torch / TF
// do it: log(erfcx(-z / sqrt 2) / 2) - z^2 / 2 for z < -1, log1p(-erfc(z / sqrt 2) / 2) otherwise.
#pragma once
#include <hip/hip_runtime.h>

namespace tfc {

constexpr float kInvSqrt2 = 0.70710678118654752f;
constexpr float kLogSqrt2Pi = 0.91893853320467274f;

__device__ inline float log_ndtr(float z) {
  if (z < -1.f) return __logf(0.5f * erfcxf(-z * kInvSqrt2)) - 0.5f * z * z;
  return log1pf(-0.5f * erfcf(z * kInvSqrt2));
}

// log( Phi(zu) - Phi(zl) ), zu > zl
__device__ inline float log_interval_normal(float zu, float zl) {
  const bool right = zu > 0.f;                         // logsf(zu) < logcdf(zu)
  const float big = right ? log_ndtr(-zl) : log_ndtr(zu);
  const float small = right ? log_ndtr(-zu) : log_ndtr(zl);
  return log1pf(-__expf(small - big)) + big;
}

}  // namespace tfc
