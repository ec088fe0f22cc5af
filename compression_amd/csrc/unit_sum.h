// Sums over the 2^k consecutive lanes of a wave64 that share a row (ChannelNorm, the LPIPS distance head), without
// LDS memory: DPP (quad_perm, row_half_mirror, row_mirror), ds_swizzle (lane ^ 16) and v_permlane32_swap.
#pragma once
#include <hip/hip_runtime.h>

namespace tfc {

template <int CTRL>
__device__ inline float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// Sum over the 2^lpr_log2 lanes of a unit, the result in every one of them with the same bits (each step adds the
// same two numbers on both sides).  lpr_log2 is wave-uniform.
__device__ inline float unit_sum(float v, int lpr_log2) {
  if (lpr_log2 >= 1) v = dpp_add<0xB1>(v);          // quad_perm [1,0,3,2]
  if (lpr_log2 >= 2) v = dpp_add<0x4E>(v);          // quad_perm [2,3,0,1]
  if (lpr_log2 >= 3) v = dpp_add<0x141>(v);         // row_half_mirror: the other quad of 8
  if (lpr_log2 >= 4) v = dpp_add<0x140>(v);         // row_mirror: the other 8 of 16
  if (lpr_log2 >= 5) v += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));   // lane ^ 16
  if (lpr_log2 >= 6) {
    const unsigned int b = __float_as_uint(v);
    const auto r = __builtin_amdgcn_permlane32_swap(b, b, false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  return v;
}

}  // namespace tfc
