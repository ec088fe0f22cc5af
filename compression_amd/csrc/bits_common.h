// What the two bits-per-unit units share (noisy_normal_bits.hip, factorized_bits.hip): a unit's elements go to
// blocks_per_unit blocks, each leaves one partial sum of log p, and a second kernel adds a unit's partials in a fixed
// order and scales by -1 / ln 2.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launch.h"

namespace tfc {

// Blocks per unit: about 8 per CU over all units, no more than the unit has rows of `threads` elements.
inline int bits_blocks_per_unit(long long units, long long elems, int threads) {
  const long long rows = ceil_div(elems, threads);
  const long long want = ceil_div(static_cast<long long>(device_cus()) * 8, std::max<long long>(units, 1));
  return static_cast<int>(std::max<long long>(1, std::min<long long>(rows, want)));
}

// The block sum that ends both forward kernels (wave shuffles, then lane 0 of each wave through LDS) stays written out
// in each: as a shared inline function it compiled to the same instructions in another order (the LDS address before
// the last add instead of behind it), and this header moves no instruction.

static __global__ void bits_reduce_kernel(const float* partial, int blocks_per_unit, long long units, float* bits) {
  const long long u = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
  if (u >= units) return;
  float s = 0.f;
  for (int b = 0; b < blocks_per_unit; ++b) s += partial[u * blocks_per_unit + b];
  bits[u] = s * -1.4426950408889634f;          // / -ln 2
}

static inline void launch_bits_reduce(const float* partial, int blocks_per_unit, long long units, float* bits,
                                      hipStream_t st) {
  hipLaunchKernelGGL(bits_reduce_kernel, dim3(static_cast<unsigned>(ceil_div(units, 256))), dim3(256), 0, st, partial,
                     blocks_per_unit, units, bits);
}

}  // namespace tfc
