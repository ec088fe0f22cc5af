// Element conversion and element I/O of the kernels, once: float <-> bfloat16 bits, a 16-byte granule of a float32 or
// bfloat16 tensor <-> floats, one element by index, and the non-temporal granule store.  A new kernel file includes
// this header instead of defining its own.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "mfma_types.h"

namespace tfc {

// v_cvt_pk_bf16_f32: two floats -> packed bf16 pair, round-to-nearest-even.
__device__ inline unsigned int pack_bf16(f32x2 v) { return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf16x2)); }
__device__ inline unsigned int pack_bf16(float lo, float hi) { return pack_bf16(f32x2{lo, hi}); }
// one float, the same instruction
__device__ inline unsigned short float_to_bf16_bits(float f) { return __builtin_bit_cast(unsigned short, static_cast<__bf16>(f)); }
__device__ inline float bf16_bits_to_float(unsigned int bits16) { return __uint_as_float(bits16 << 16); }

// A granule (16 bytes) of a tensor <-> its 8 (bfloat16) or 4 (float32) elements.
template <bool BF16>
__device__ inline void unpack(const u32x4 raw, float* v) {
  if (BF16) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      v[2 * w] = __uint_as_float(raw[w] << 16);
      v[2 * w + 1] = __uint_as_float(raw[w] & 0xFFFF0000u);
    }
  } else {
#pragma unroll
    for (int w = 0; w < 4; ++w) v[w] = __uint_as_float(raw[w]);
  }
}

template <bool BF16>
__device__ inline u32x4 repack(const float* v) {
  u32x4 out;
  if (BF16) {
#pragma unroll
    for (int w = 0; w < 4; ++w) out[w] = pack_bf16(v[2 * w], v[2 * w + 1]);
  } else {
#pragma unroll
    for (int w = 0; w < 4; ++w) out[w] = __float_as_uint(v[w]);
  }
  return out;
}

// Element `at` of a tensor whose dtype is a template flag ...
template <bool BF16>
__device__ inline float load(const void* base, long long at) {
  if (BF16) return bf16_bits_to_float(static_cast<const unsigned short*>(base)[at]);
  return static_cast<const float*>(base)[at];
}

template <bool BF16>
__device__ inline void store(void* base, long long at, float v) {
  if (BF16) static_cast<unsigned short*>(base)[at] = float_to_bf16_bits(v);
  else static_cast<float*>(base)[at] = v;
}

// ... or an element type; unsigned short is bfloat16 as its 16 bits.
template <typename T> __device__ inline float load_as_float(const T* p, long long i);
template <> __device__ inline float load_as_float<float>(const float* p, long long i) { return p[i]; }
template <> __device__ inline float load_as_float<__hip_bfloat16>(const __hip_bfloat16* p, long long i) { return __bfloat162float(p[i]); }
template <> __device__ inline float load_as_float<_Float16>(const _Float16* p, long long i) { return static_cast<float>(p[i]); }
template <> __device__ inline float load_as_float<unsigned char>(const unsigned char* p, long long i) { return p[i]; }
template <> __device__ inline float load_as_float<unsigned short>(const unsigned short* p, long long i) { return bf16_bits_to_float(p[i]); }

template <typename T> __device__ inline void store_from_float(T* p, long long i, float v);
template <> __device__ inline void store_from_float<float>(float* p, long long i, float v) { p[i] = v; }
template <> __device__ inline void store_from_float<__hip_bfloat16>(__hip_bfloat16* p, long long i, float v) { p[i] = __float2bfloat16(v); }

// A granule to memory, non-temporal if `nt`.  (As an instruction by hand: with __builtin_nontemporal_store in one branch
// and a plain store in the other the optimiser merges the two into ONE plain store.)
__device__ inline void store_granule(u32x4* dst, u32x4 v, int nt) {
  if (nt) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(dst), "v"(v) : "memory");
  else *dst = v;
}

}  // namespace tfc
