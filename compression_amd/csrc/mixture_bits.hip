// Training-time likelihood of the discretized Gaussian mixture (Cheng, Sun, Takeuchi, Katto, CVPR 2020), fused: what
// distributions/uniform_noise.py NoisyNormalMixture computes as a tensor-op composition over [..., K],
//   y_hat = y + u
//   lp_k  = log( Phi((y_hat + .5 - mu_k) / sigma_k) - Phi((y_hat - .5 - mu_k) / sigma_k) )
//   log p = logsumexp_k( log_softmax(logits)_k + lp_k )
//   bits[unit] = - sum_unit log p / ln 2
// as one forward kernel (y, u, 3 K parameter planes -> y_hat, block partial sums) and one backward kernel that writes
// dy, dlogits, dloc and dscale through the responsibilities r_k = softmax_k(logits_k + lp_k); no [N, K] temporary goes
// to memory.  The parameters are float32 planes [K][units * elems]: a wave's loads of one plane are contiguous.
// lp_k is noisy_normal_bits.hip's (normal_log_cdf.h); the block sum and the second-stage sum are bits_common.h's.
// The Laplace tail and expected gradients of the single-Gaussian kernel are not offered here.
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "../../include/tfc_hip.h"
#include "bf16_io.h"
#include "bits_common.h"
#include "mixture_cdf.h"
#include "normal_log_cdf.h"

namespace tfc {
namespace {

struct MixBitsParams {
  const void* y;
  const void* noise;
  const float* logits;       // planes [K][units * elems]
  const float* loc;
  const float* scale;
  void* y_hat;
  long long units, elems;
  float* partial;            // [units][blocks_per_unit]
  int blocks_per_unit;
  const float* gbits;        // backward
  void* dy;
  float* dlogits;
  float* dloc;
  float* dscale;
};

constexpr int kThreads = 256;

// log p of one element, and what the backward pass needs beside it
template <int K>
struct MixTerms {
  float a[K];                // logits_k + lp_k
  float zu[K], zl[K], inv[K], lp[K];
  float amax, asum;          // max_k a_k, sum_k exp(a_k - amax)
  float lmax, lsum;          // the same of the logits
};

template <int K>
__device__ inline float mix_log_prob(const MixBitsParams& p, long long at, float v, MixTerms<K>& m) {
  const long long n = p.units * p.elems;
  float l[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    l[k] = p.logits[k * n + at];
    m.inv[k] = 1.f / p.scale[k * n + at];
    const float d = v - p.loc[k * n + at];
    m.zu[k] = (d + 0.5f) * m.inv[k];
    m.zl[k] = (d - 0.5f) * m.inv[k];
    m.lp[k] = log_interval_normal(m.zu[k], m.zl[k]);
    m.a[k] = l[k] + m.lp[k];
  }
  m.amax = m.a[0];
  m.lmax = l[0];
#pragma unroll
  for (int k = 1; k < K; ++k) {
    m.amax = fmaxf(m.amax, m.a[k]);
    m.lmax = fmaxf(m.lmax, l[k]);
  }
  m.asum = 0.f;
  m.lsum = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    m.asum += __expf(m.a[k] - m.amax);
    m.lsum += __expf(l[k] - m.lmax);
    m.a[k] = l[k];           // the backward pass reads the logits back from here
  }
  return (m.amax - m.lmax) + (__logf(m.asum) - __logf(m.lsum));
}

template <typename T, int K>
__global__ void __launch_bounds__(kThreads) mixture_bits_forward_kernel(MixBitsParams p) {
  const int t = threadIdx.x;
  const long long unit = blockIdx.x / p.blocks_per_unit;
  const int blk = blockIdx.x % p.blocks_per_unit;
  const T* y = static_cast<const T*>(p.y) + unit * p.elems;
  const T* nz = p.noise ? static_cast<const T*>(p.noise) + unit * p.elems : nullptr;
  T* yh = static_cast<T*>(p.y_hat) + unit * p.elems;
  float acc = 0.f;
  for (long long e = static_cast<long long>(blk) * kThreads + t; e < p.elems;
       e += static_cast<long long>(p.blocks_per_unit) * kThreads) {
    float v = load_as_float(y, e);
    if (nz) v += load_as_float(nz, e);
    store_from_float(yh, e, v);
    v = load_as_float(yh, e);                         // the value later passes see (dtype-rounded)
    MixTerms<K> m;
    acc += mix_log_prob<K>(p, unit * p.elems + e, v, m);
  }
  __shared__ float wsum[kThreads / 64];              // the block sum: its own copy (bits_common.h says why)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
  if ((t & 63) == 0) wsum[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    float s = 0.f;
    for (int w = 0; w < kThreads / 64; ++w) s += wsum[w];     // fixed order
    p.partial[blockIdx.x] = s;
  }
}

template <typename T, int K>
__global__ void __launch_bounds__(kThreads) mixture_bits_backward_kernel(MixBitsParams p) {
  const long long unit = blockIdx.x / p.blocks_per_unit;
  const int blk = blockIdx.x % p.blocks_per_unit;
  const T* yh = static_cast<const T*>(p.y_hat) + unit * p.elems;
  T* dy = static_cast<T*>(p.dy) + unit * p.elems;
  const long long n = p.units * p.elems;
  const float g = p.gbits[unit] * -1.4426950408889634f;     // dL/d(sum log p) of this unit
  for (long long e = static_cast<long long>(blk) * kThreads + threadIdx.x; e < p.elems;
       e += static_cast<long long>(p.blocks_per_unit) * kThreads) {
    const long long at = unit * p.elems + e;
    const float v = load_as_float(yh, e);
    MixTerms<K> m;
    mix_log_prob<K>(p, at, v, m);
    const float inv_asum = 1.f / m.asum, inv_lsum = 1.f / m.lsum;
    float dv = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float l = m.a[k];
      const float r = __expf(l + m.lp[k] - m.amax) * inv_asum;        // responsibility
      const float w = __expf(l - m.lmax) * inv_lsum;                  // softmax(logits)_k
      // d lp / d zu = phi(zu) / P, d lp / d zl = -phi(zl) / P, with P = exp(lp): ratios in log space
      const float gu = __expf(-0.5f * m.zu[k] * m.zu[k] - kLogSqrt2Pi - m.lp[k]);
      const float gl = -__expf(-0.5f * m.zl[k] * m.zl[k] - kLogSqrt2Pi - m.lp[k]);
      const float dz = r * (gu + gl) * m.inv[k];                      // r_k d lp_k / d y_hat
      dv += dz;
      p.dlogits[k * n + at] = g * (r - w);
      p.dloc[k * n + at] = -g * dz;
      p.dscale[k * n + at] = -g * r * (gu * m.zu[k] + gl * m.zl[k]) * m.inv[k];
    }
    store_from_float(dy, e, g * dv);
  }
}

int plan(long long units, long long elems, int* blocks_per_unit) {
  *blocks_per_unit = bits_blocks_per_unit(units, elems, kThreads);
  if (units * *blocks_per_unit > kMaxGridX) return fail("tfc_mixture_bits: problem too large");
  return 0;
}

int check(const char* who, int dtype, int k, const void* logits, const void* loc, const void* scale) {
  if (int rc = check_dtype(who, dtype)) return rc;
  if (k < 1 || k > MIX_MAX_COMPONENTS) return fail("%s: k must be in [1, %d] (got %d)", who, MIX_MAX_COMPONENTS, k);
  if (!logits || !loc || !scale) return fail("%s: null parameter pointer", who);
  return 0;
}

template <template <typename, int> class Launcher>
void dispatch(int dtype, int k, dim3 grid, hipStream_t st, const MixBitsParams& p) {
  if (dtype == 0) {
    switch (k) {
      case 1: Launcher<float, 1>::go(grid, st, p); break;
      case 2: Launcher<float, 2>::go(grid, st, p); break;
      case 3: Launcher<float, 3>::go(grid, st, p); break;
      default: Launcher<float, 4>::go(grid, st, p); break;
    }
  } else {
    switch (k) {
      case 1: Launcher<__hip_bfloat16, 1>::go(grid, st, p); break;
      case 2: Launcher<__hip_bfloat16, 2>::go(grid, st, p); break;
      case 3: Launcher<__hip_bfloat16, 3>::go(grid, st, p); break;
      default: Launcher<__hip_bfloat16, 4>::go(grid, st, p); break;
    }
  }
}

template <typename T, int K>
struct Forward {
  static void go(dim3 grid, hipStream_t st, const MixBitsParams& p) {
    hipLaunchKernelGGL((mixture_bits_forward_kernel<T, K>), grid, dim3(kThreads), 0, st, p);
  }
};
template <typename T, int K>
struct Backward {
  static void go(dim3 grid, hipStream_t st, const MixBitsParams& p) {
    hipLaunchKernelGGL((mixture_bits_backward_kernel<T, K>), grid, dim3(kThreads), 0, st, p);
  }
};

}  // namespace
}  // namespace tfc

extern "C" int tfc_mixture_bits_forward(const void* y, const void* noise, const float* logits, const float* loc,
                                        const float* scale, int k, void* y_hat, int dtype, int64_t units,
                                        int64_t elems, float* bits, void* stream) {
  using namespace tfc;
  if (int rc = check("tfc_mixture_bits_forward", dtype, k, logits, loc, scale)) return rc;
  if (units == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  MixBitsParams p{};
  p.y = y; p.noise = noise; p.logits = logits; p.loc = loc; p.scale = scale; p.y_hat = y_hat;
  p.units = units; p.elems = elems;
  if (int rc = plan(units, elems, &p.blocks_per_unit)) return rc;
  DevBuf partial;
  TFC_HIP(partial.alloc(sizeof(float) * units * p.blocks_per_unit, st));
  p.partial = partial.as<float>();
  {
    KernelTimer timer("mixture_bits_forward", st);
    dispatch<Forward>(dtype, k, dim3(static_cast<unsigned>(units * p.blocks_per_unit)), st, p);
  }
  launch_bits_reduce(p.partial, p.blocks_per_unit, units, bits, st);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_mixture_bits_backward(const void* y_hat, const float* logits, const float* loc, const float* scale,
                                         int k, int dtype, int64_t units, int64_t elems, const float* gbits, void* dy,
                                         float* dlogits, float* dloc, float* dscale, void* stream) {
  using namespace tfc;
  if (int rc = check("tfc_mixture_bits_backward", dtype, k, logits, loc, scale)) return rc;
  if (units == 0 || elems == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  MixBitsParams p{};
  p.y_hat = const_cast<void*>(y_hat); p.logits = logits; p.loc = loc; p.scale = scale;
  p.units = units; p.elems = elems; p.gbits = gbits; p.dy = dy; p.dlogits = dlogits; p.dloc = dloc; p.dscale = dscale;
  if (int rc = plan(units, elems, &p.blocks_per_unit)) return rc;
  KernelTimer timer("mixture_bits_backward", st);
  dispatch<Backward>(dtype, k, dim3(static_cast<unsigned>(units * p.blocks_per_unit)), st, p);
  TFC_HIP(hipGetLastError());
  return 0;
}
