// Packed weights and launch plan of the context-model kernels (context_model.hip), shared by the kernels, the host
// entry points and ops/context_ops.py, which reads the constants below from this file and restates ctx_layout().
// Plain C++: no device types, so that host tools can include it on their own.
//
// The packed buffer is float32.  A weight matrix is stored [K padded][O]: row k holds the O outputs of input k,
// K is padded to a multiple of CTX_KPAD with zero rows, and every section starts at a multiple of CTX_KPAD floats:
//
//   wc   [CTX_TAPS][Mp][2M]   the causal taps of the 5x5 kernel, mask applied: tap = (di + 2) * 5 + (dj + 2)
//   bc   [2M]
//   w1c  [C2p][H1]            first layer, rows of the context features (C2 = 2M)
//   w1p  [Pp][H1]             first layer, rows of the hyperprior features
//   b1   [H1]
//   w2   [H1p][H2]     b2 [H2]
//   w3   [H2p][2M]     b3 [2M]
#pragma once
#include <cstdint>

namespace tfc {

constexpr int CTX_TAPS = 12;            // (di, dj) with di < 0, or di == 0 and dj < 0, of a 5x5 window
constexpr int CTX_KPAD = 4;             // the kernels sum K in four interleaved partial sums
constexpr int CTX_THREADS = 512;        // one workgroup per image
constexpr int CTX_MAX_WAVES = 8;        // positions of a wavefront step that are in flight together
constexpr int CTX_LDS_FLOATS = 15360;   // 60 KiB of activations
constexpr int CTX_MAX_DIM = 65536;      // bound of M, P, H1, H2 (keeps every offset inside int64 by far)

struct ContextLayout {
  int m, p, h1, h2;
  int mp, c2, c2p, pp, h1p, h2p;        // padded K extents; c2 = 2M
  int64_t wc, bc, w1c, w1p, b1, w2, b2, w3, b3, total;   // offsets in floats
  int a_floats, b_floats;               // per position: buffer A holds ctx then h2, buffer B holds h1 then the output
  int pos_floats;                       // LDS floats per position in flight
  int waves;                            // positions in flight
};

inline int ctx_pad(int v) { return (v + CTX_KPAD - 1) / CTX_KPAD * CTX_KPAD; }

// Fills `L`; returns null, or the text of what is wrong with the sizes.
inline const char* ctx_layout(int64_t m, int64_t p, int64_t h1, int64_t h2, ContextLayout* L) {
  if (m < 1 || p < 1 || h1 < 1 || h2 < 1) return "M, P, H1 and H2 must be at least 1";
  if (m > CTX_MAX_DIM || p > CTX_MAX_DIM || h1 > CTX_MAX_DIM || h2 > CTX_MAX_DIM)
    return "M, P, H1 and H2 must be at most 65536";
  L->m = static_cast<int>(m);
  L->p = static_cast<int>(p);
  L->h1 = static_cast<int>(h1);
  L->h2 = static_cast<int>(h2);
  L->mp = ctx_pad(L->m);
  L->c2 = 2 * L->m;
  L->c2p = ctx_pad(L->c2);
  L->pp = ctx_pad(L->p);
  L->h1p = ctx_pad(L->h1);
  L->h2p = ctx_pad(L->h2);
  int64_t at = 0;
  auto take = [&at](int64_t n) {
    const int64_t start = at;
    at += (n + CTX_KPAD - 1) / CTX_KPAD * CTX_KPAD;
    return start;
  };
  L->wc = take(static_cast<int64_t>(CTX_TAPS) * L->mp * L->c2);
  L->bc = take(L->c2);
  L->w1c = take(static_cast<int64_t>(L->c2p) * L->h1);
  L->w1p = take(static_cast<int64_t>(L->pp) * L->h1);
  L->b1 = take(L->h1);
  L->w2 = take(static_cast<int64_t>(L->h1p) * L->h2);
  L->b2 = take(L->h2);
  L->w3 = take(static_cast<int64_t>(L->h2p) * L->c2);
  L->b3 = take(L->c2);
  L->total = at;
  L->a_floats = L->c2p > L->h2p ? L->c2p : L->h2p;
  L->b_floats = L->h1p > L->c2p ? L->h1p : L->c2p;
  const int64_t ab = static_cast<int64_t>(L->a_floats) + L->b_floats;
  const int64_t pos = ab > L->pp ? ab : L->pp;
  if (pos > CTX_LDS_FLOATS) return "the activations of one position do not fit 60 KiB of LDS";
  L->pos_floats = static_cast<int>(pos);
  const int64_t waves = CTX_LDS_FLOATS / pos;
  L->waves = static_cast<int>(waves < CTX_MAX_WAVES ? waves : CTX_MAX_WAVES);
  return nullptr;
}

// The shape checks of tfc_context_scan / tfc_context_decode that need no device; null, or the text.
inline const char* ctx_check_shape(int64_t batch, int64_t hl, int64_t wl, int64_t num_scales, int64_t packed_floats,
                                   const ContextLayout& L) {
  if (batch < 0) return "the batch size must not be negative";
  if (hl < 1 || wl < 1) return "Hl and Wl must be at least 1";
  if (batch > 0x7fffffffll) return "the batch size must be below 2^31";
  if (hl > (1 << 24) || wl > (1 << 24)) return "Hl and Wl must be at most 2^24";
  if (num_scales < 1 || num_scales > (1 << 24)) return "num_scales must be in [1, 2^24]";
  if (packed_floats != L.total) return "the packed weights do not have the size of this M, P, H1, H2";
  // global offsets are int64: positions * 65536 floats stay below 2^58 bytes; the wavefront steps
  // Wl - 1 + 3 (Hl - 1) < 2^26 are counted in int
  if (batch > 0 && hl * wl > (1ll << 40) / batch) return "batch * Hl * Wl must be at most 2^40";
  return nullptr;
}

// Bytes of the workspace: the hyperprior half of the first layer for every position, then one coder state
// (16 bytes) per row stream.
inline int64_t ctx_workspace_bytes(int64_t batch, int64_t hl, int64_t wl, int64_t h1) {
  const int64_t pre = batch * hl * wl * h1 * 4;
  return (pre + 15) / 16 * 16 + batch * hl * 16;
}

// ---- the checkerboard context model (ckb_engine.h, space_channel.hip) ----------------------------------------------
// Same packed buffer (ctx_layout), the same CTX_TAPS x Mp rows of wc; only the tap list differs: the 12 offsets of the
// 5x5 window with di + dj odd, row-major.  Those are the odd elements of the window counted row-major, so packed tap k
// is element 2 k + 1: (di, dj) = (ckb_tap_di(k), ckb_tap_dj(k)) = (-2,-1) (-2,1) (-1,-2) (-1,0) (-1,2) (0,-1) (0,1) ...

constexpr int CKB_TILE = 32;            // positions of one workgroup: the 32 rows of v_mfma_f32_32x32x2_f32
constexpr int CKB_THREADS = 256;        // four waves, each owns 32-column blocks of a layer's output
constexpr int CKB_BLOCKS = 5;           // column blocks a wave accumulates side by side (5 x 16 registers)
constexpr int CKB_GROUP = 8;            // k-steps (of two input rows) whose weights a wave loads ahead
constexpr int CKB_STAGE_K = 64;         // input rows of one staged chunk of gathered y_hat or psi
constexpr int CKB_LDS_FLOATS = 40960;   // 160 KiB: gfx950's whole LDS, declared on purpose

constexpr int ckb_tap_di(int k) { return (2 * k + 1) / 5 - 2; }
constexpr int ckb_tap_dj(int k) { return (2 * k + 1) % 5 - 2; }
static_assert(ckb_tap_di(0) == -2 && ckb_tap_dj(0) == -1 && ckb_tap_di(CTX_TAPS - 1) == 2 && ckb_tap_dj(CTX_TAPS - 1) == 1,
              "the checkerboard taps are the odd elements of the 5x5 window");

// Positions of a pass: anchors (i + j even) are pass 0
inline int64_t ckb_positions(int64_t hl, int64_t wl, int pass) { return (hl * wl + (pass == 0 ? 1 : 0)) / 2; }

// LDS rows (of CKB_TILE floats) of the two activation buffers: A holds ctx then h2, B holds h1 then the output
inline int ckb_rows_a(const ContextLayout& L) { return L.a_floats; }
inline int ckb_rows_b(const ContextLayout& L) { return L.b_floats; }

// The checks of tfc_checkerboard_params / tfc_scctx_params beyond ctx_layout / ctx_check_shape; null, or the text.
inline const char* ckb_check(int pass, int64_t batch, int64_t hl, int64_t wl, const ContextLayout& L) {
  if (pass != 0 && pass != 1) return "pass must be 0 or 1";
  const int64_t rows = static_cast<int64_t>(ckb_rows_a(L)) + ckb_rows_b(L);
  if (rows * CKB_TILE + CKB_STAGE_K * CKB_TILE > CKB_LDS_FLOATS)
    return "the activations of one tile of 32 positions do not fit 160 KiB of LDS";
  const int64_t tiles = (ckb_positions(hl, wl, pass) + CKB_TILE - 1) / CKB_TILE;
  if (batch > 0 && tiles > 0x7fffffffll / batch) return "batch * tiles of 32 positions must be below 2^31";
  return nullptr;
}

}  // namespace tfc
