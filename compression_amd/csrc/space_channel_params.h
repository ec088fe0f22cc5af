// Packed weights and launch plan of the space-channel context model (space_channel.hip, "SCCTX"), shared by the
// kernels, the host entry points and ops/scctx_ops.py, which reads the constants below from this file and restates
// scctx_layout().  Plain C++: no device types.
//
// The model is ELIC's (He, Yang, Peng, Mao, Qin, Wang, CVPR 2022) channel groups with the checkerboard inside every
// group.  The reference tree holds no program text for it: the definition, the stream format and the layer shapes are
// this project's own, and parity with anyone's checkpoints is unpinned.
//
// One packed float32 buffer PER GROUP g of M_g channels that start at channel c_g of the latent:
//
//   ctx_layout(M_g, P, H1, H2) of context_params.h, whose wc [CTX_TAPS][Mgp][2 M_g] holds the own-group kernel Wsp_g on
//       the 12 checkerboard taps (packed tap k is element 2 k + 1 of the 5x5 window), followed at its `total` by
//   wch  [SCCTX_TAPS][cgp][2 M_g]   the earlier-group kernel Wch_g on ALL taps of the window, row-major: packed tap k
//                                   is element k, (di, dj) = (k / 5 - 2, k % 5 - 2); cgp = c_g padded to CTX_KPAD with
//                                   zero rows; absent (0 floats) for c_g = 0
//
// so the buffer of a single group (c_g = 0) is the checkerboard model's buffer, float for float: tfc_checkerboard_params
// is tfc_scctx_params with c_g = 0 and M_g = M (space_channel.hip).
#pragma once
#include "context_params.h"

namespace tfc {

constexpr int SCCTX_TAPS = 25;          // the whole 5x5 window over the earlier groups
constexpr int SCCTX_STREAM = 64;        // default positions of one code stream (ops/scctx_ops.py)

struct ScctxLayout {
  ContextLayout L;                      // of (M_g, P, H1, H2)
  int m, cg, cgp;                       // latent depth, first channel of the group, c_g padded
  int64_t wch, total;                   // offsets in floats
};

// Fills `S`; returns null, or the text of what is wrong with the sizes.
inline const char* scctx_layout(int64_t m, int64_t cg, int64_t mg, int64_t p, int64_t h1, int64_t h2, ScctxLayout* S) {
  // a group that is the whole latent (the checkerboard model) has no bounds beyond ctx_layout's on M_g = M, and gets
  // them in ctx_layout's words
  if (cg != 0 || mg != m) {
    if (m < 1 || m > CTX_MAX_DIM) return "M must be in [1, 65536]";
    if (cg < 0 || mg < 1 || cg > m - mg) return "the group must lie inside the latent: c_g >= 0, M_g >= 1, c_g + M_g <= M";
  }
  if (const char* e = ctx_layout(mg, p, h1, h2, &S->L)) return e;
  S->m = static_cast<int>(m);
  S->cg = static_cast<int>(cg);
  S->cgp = ctx_pad(S->cg);
  S->wch = S->L.total;
  const int64_t n = static_cast<int64_t>(SCCTX_TAPS) * S->cgp * S->L.c2;
  S->total = S->wch + (n + CTX_KPAD - 1) / CTX_KPAD * CTX_KPAD;
  return nullptr;
}

// The checks of tfc_scctx_params beyond scctx_layout that need no device; null, or the text.
inline const char* scctx_check(int pass, int64_t batch, int64_t hl, int64_t wl, int64_t num_scales,
                               int64_t packed_floats, const ScctxLayout& S) {
  if (const char* e = ctx_check_shape(batch, hl, wl, num_scales, S.L.total, S.L)) return e;
  if (packed_floats != S.total) return "the packed weights do not have the size of this c_g, M_g, P, H1, H2";
  return ckb_check(pass, batch, hl, wl, S.L);      // pass, the LDS fit of this group's widths, the grid
}

}  // namespace tfc
