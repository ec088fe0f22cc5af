// What context_model.hip and ckb_engine.h share beyond context_params.h, which stays free of device types and of
// the library's error state: the two element-wise device helpers and the size checks every entry point opens with.
#pragma once
#include "common.h"
#include "context_params.h"

namespace tfc {

__device__ __forceinline__ float ctx_lrelu(float v) { return v > 0.f ? v : 0.2f * v; }

// tfc_index_prepare's value (csrc/elementwise.hip)
__device__ __forceinline__ int32_t ctx_index(float v, float hi) { return static_cast<int32_t>(fminf(fmaxf(v, 0.f), hi)); }

// ctx_layout, then ctx_check_shape: 0 with `L` filled, or fail() under the entry point's name.  `weights` is false for
// tfc_context_workspace, which takes neither num_scales nor a packed buffer and names neither in its message.
inline int ctx_check_args(const char* name, int m, int p, int h1, int h2, int64_t batch, int64_t hl, int64_t wl,
                          bool weights, int num_scales, int64_t packed_floats, ContextLayout* L) {
  if (const char* e = ctx_layout(m, p, h1, h2, L)) return fail("%s: %s (M %d, P %d, H1 %d, H2 %d)", name, e, m, p, h1, h2);
  const long long b = batch, h = hl, w = wl;
  if (!weights) {
    if (const char* e = ctx_check_shape(batch, hl, wl, 1, L->total, *L))
      return fail("%s: %s (batch %lld, Hl %lld, Wl %lld)", name, e, b, h, w);
  } else if (const char* e = ctx_check_shape(batch, hl, wl, num_scales, packed_floats, *L)) {
    return fail("%s: %s (batch %lld, Hl %lld, Wl %lld, num_scales %d, %lld packed floats)", name, e, b, h, w, num_scales,
                static_cast<long long>(packed_floats));
  }
  return 0;
}

}  // namespace tfc
