// The quantised CDF of a discretized Gaussian mixture, evaluated where it is coded: ONE definition for
// the encoder, the decoder and the table dump of mixture_coder.hip.
//
//   window [lo, lo + L - 1], 1 <= L <= MIX_MAX_WINDOW;  boundaries b = 0 .. L;  S = 2^16 - MIX_RESERVE * L
//   c_0 = 0,  c_L = 2^16,  c_b = MIX_RESERVE * b + floor(F(lo + b - 1/2) * S)  in between
//   F(t) = sum_k w_k Phi((t - mu_k) / sigma_k),  w = softmax(logits)
//
// F is float32 in a fixed operation order: every step below is a single correctly rounded operation (or a library
// function of one argument), written with the rounding intrinsics and with contraction off, so that the three callers
// get the same bits whatever surrounds the inlined code.  F is clamped to [0, 1] (a NaN goes to 0), so every c_b is in
// [MIX_RESERVE * b, 2^16 - MIX_RESERVE * (L - b)] whatever the parameters are.
#pragma once
#include <hip/hip_runtime.h>

namespace tfc {

constexpr int MIX_PRECISION = 16;
constexpr int MIX_RESERVE = 2;            // counts every symbol keeps: a float32 F that steps back costs at most one
constexpr int MIX_MAX_WINDOW = 4096;      // so that symbol - lo fits the legacy op's int16
constexpr int MIX_MAX_COMPONENTS = 4;
constexpr int MIX_MAX_ABS_LO = 4194304;   // 2^22: lo + b - 1/2 is exact in float32

template <int K>
struct MixElem {
  float w[K], mu[K], sigma[K];
};

// One element's parameters from the planes [K][n] (element `at`), the weights by a softmax in ascending k.
template <int K>
__device__ inline MixElem<K> mix_load(const float* logits, const float* loc, const float* scale, long long n,
                                      long long at) {
#pragma clang fp contract(off)
  MixElem<K> e;
  float l[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    l[k] = logits[k * n + at];
    e.mu[k] = loc[k * n + at];
    e.sigma[k] = scale[k * n + at];
  }
  float m = l[0];
#pragma unroll
  for (int k = 1; k < K; ++k) m = fmaxf(m, l[k]);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    e.w[k] = expf(__fsub_rn(l[k], m));
    sum = __fadd_rn(sum, e.w[k]);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) e.w[k] = __fdiv_rn(e.w[k], sum);
  return e;
}

// F(t), clamped to [0, 1].  The quotient, not a product with 1 / sigma: a positive finite sigma then gives no NaN
// ((t - mu) / sigma is 0, finite or an infinity of the right sign).
template <int K>
__device__ inline float mix_cumulative(const MixElem<K>& e, float t) {
#pragma clang fp contract(off)
  float f = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float z = __fdiv_rn(__fsub_rn(t, e.mu[k]), e.sigma[k]);
    const float phi = __fmul_rn(0.5f, erfcf(__fmul_rn(z, -0.70710678118654752f)));
    f = __fadd_rn(f, __fmul_rn(e.w[k], phi));
  }
  return fminf(fmaxf(f, 0.f), 1.f);
}

// c_b; any b (below 0 counts as 0, above L as L).
template <int K>
__device__ inline int mix_boundary(const MixElem<K>& e, int lo, int len, int b) {
#pragma clang fp contract(off)
  if (b <= 0) return 0;
  if (b >= len) return 1 << MIX_PRECISION;
  const float t = __fsub_rn(static_cast<float>(lo + b), 0.5f);
  const float s = static_cast<float>((1 << MIX_PRECISION) - MIX_RESERVE * len);
  return MIX_RESERVE * b + static_cast<int>(__fmul_rn(mix_cumulative<K>(e, t), s));
}

}  // namespace tfc
