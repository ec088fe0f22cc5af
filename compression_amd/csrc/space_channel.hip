// The space-channel context model ("SCCTX") after He, Yang, Peng, Mao, Qin and Wang, "ELIC: efficient learned image
// compression with unevenly grouped space-channel contextual adaptive coding" (CVPR 2022) on gfx950: the latent's
// channels are cut into groups, the checkerboard of He, Zheng, Sun, Wang and Qin (CVPR 2021) runs inside every group,
// and a group sees all earlier groups through a full 5x5 window.  ONE launch per (group, pass) computes, for all
// positions of the pass, the masked correlation, the group's pointwise entropy-parameter network and the quantisation
// (scctx_params_kernel); scctx_place_kernel is the decoder's store of a decoded (group, pass).  include/tfc_hip.h
// states the definition.  The checkerboard model itself is the one-group case, c_g = 0 and M_g = M:
// tfc_checkerboard_params and tfc_checkerboard_place below run these kernels.
//
// The reference tree holds no program text for this model: the definition, the stream format and the layer shapes are
// this project's own, and parity with anyone's checkpoints is unpinned.
//
// The plan is the one at the head of ckb_engine.h: a workgroup of CKB_THREADS threads owns CKB_TILE = 32 consecutive
// compact positions of one image, the four layers run on v_mfma_f32_32x32x2_f32 with the activations k-major in LDS
// and the weights loaded straight to registers a group of k-steps ahead.  The staged source of the correlation is a
// channel range of the full y_hat (row stride M; the earlier groups [0, c_g), then the own group [c_g, c_g + M_g)),
// there are two tap lists (all 25 taps over the earlier groups, the 12 checkerboard taps over the own group) and the
// context chain has up to two segments, the first of which exists in pass 0 as well when g > 0.
//
// Every output element stays one chain: its bias, then one fmaf per input row in ascending k: the earlier-group taps
// (row-major, channels ascending), the own-group taps, for the first layer the 2 M_g context rows and then the P
// hyperprior rows.  A neighbour outside the latent and a padded row enter as zeros, never skipped.  There is no split
// of K across waves: a 16-channel group has one block of 32 output columns, so three of the four waves of its
// workgroup repeat that block and drop it.  The rule costs speed there and wins.
//
// Nothing waits on another workgroup; every loop bound comes from the shapes.  A launch reads the channels below c_g
// everywhere and, in pass 1, the own group at anchors; it writes the own group at the pass's positions only, so two
// workgroups never touch the same element.
#include "ckb_engine.h"
#include "space_channel_params.h"

#include "../../include/tfc_hip.h"

namespace tfc {
namespace {

struct ScxArgs {
  ScctxLayout S;
  int pass, hl, wl, num_scales;
  int64_t positions;        // of this pass, per image
  int64_t tiles;            // per image
  const float* packed;
  const float* psi;         // [B, Hl, Wl, P]
  const float* y;           // [B, Hl, Wl, M] or null
  float* y_hat;             // [B, Hl, Wl, M]
  float* mu;                // [B, positions, M_g]
  float* index_float;
  int32_t* idx;
  int32_t* sym;
};

template <int PASS>
__global__ void __launch_bounds__(CKB_THREADS) scctx_params_kernel(const ScxArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[CKB_LDS_FLOATS];
  const ContextLayout& L = a.S.L;
  const int Mg = L.m, M = a.S.m, cg = a.S.cg;
  const int b = static_cast<int>(blockIdx.x / a.tiles);
  const int64_t slot0 = (blockIdx.x - static_cast<int64_t>(b) * a.tiles) * CKB_TILE;
  float* bufA = lds;
  float* bufB = bufA + static_cast<size_t>(L.a_floats) * CKB_TILE;
  float* stage = bufB + static_cast<size_t>(L.b_floats) * CKB_TILE;

  CkbTile t;
  t.b = b;
  t.hl = a.hl;
  t.wl = a.wl;
  t.np = static_cast<int>(min<int64_t>(CKB_TILE, a.positions - slot0));
  {
    const int sp = threadIdx.x & (CKB_TILE - 1);
    t.pi = -1;
    t.pj = 0;
    if (sp < t.np) ckb_position(slot0 + sp, PASS, a.wl, &t.pi, &t.pj);
  }

  // ctx -> A: the bias, then all taps over the earlier groups (g > 0), then the 12 taps over the own group (pass 1)
  const CkbSeg earlier = {a.y_hat, a.packed + a.S.wch, M, cg, a.S.cgp, SCCTX_TAPS, 0, 1};
  const CkbSeg own = {a.y_hat + cg, a.packed + L.wc, M, Mg, L.mp, CTX_TAPS, 1, 2};
  const CkbSeg none = {};
  const int nseg = (cg > 0 ? 1 : 0) + PASS;
  if (nseg == 0) {
    const float* bc = a.packed + L.bc;
    for (int e = threadIdx.x; e < L.c2p * CKB_TILE; e += CKB_THREADS) {
      const int k = e / CKB_TILE;
      bufA[e] = k < L.c2 ? bc[k] : 0.f;
    }
  } else if (cg > 0) {
    ckb_layer_n(t, stage, nullptr, 0, a.packed, nseg, earlier, PASS ? own : none, a.packed + L.bc, L.c2, L.c2p,
                ckb_store_to(bufA, false));
  } else {
    ckb_layer_n(t, stage, nullptr, 0, a.packed, 1, own, none, a.packed + L.bc, L.c2, L.c2p, ckb_store_to(bufA, false));
  }
  __syncthreads();
  ckb_network(t, L, a.packed, a.psi, bufA, bufB, stage);

  // the outputs of the tile, the group's channels innermost
  const float hi = static_cast<float>(a.num_scales - 1);
  for (int e = threadIdx.x; e < t.np * Mg; e += CKB_THREADS) {
    const int p = e / Mg, m = e - p * Mg;
    const float mu = bufB[static_cast<size_t>(m) * CKB_TILE + p];
    const float fi = bufB[static_cast<size_t>(Mg + m) * CKB_TILE + p];
    const int64_t at = (static_cast<int64_t>(b) * a.positions + slot0 + p) * Mg + m;
    a.mu[at] = mu;
    a.index_float[at] = fi;
    a.idx[at] = ctx_index(fi, hi);
    if (a.y) {
      int i, j;
      ckb_position(slot0 + p, PASS, a.wl, &i, &j);
      const int64_t full = ((static_cast<int64_t>(b) * a.hl + i) * a.wl + j) * M + cg + m;
      const int32_t s = static_cast<int32_t>(rintf(a.y[full] - mu));
      a.sym[at] = s;
      a.y_hat[full] = static_cast<float>(s) + mu;
    }
  }
}

struct ScxPlace {
  int pass, hl, wl, m, cg, mg;
  int64_t positions, total;     // per image; batch * positions * M_g
  const float* sym;
  const float* mu;
  float* y_hat;
};

__global__ void __launch_bounds__(256) scctx_place_kernel(const ScxPlace a) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < a.total; e += stride) {
    const int64_t s = e / a.mg;
    const int m = static_cast<int>(e - s * a.mg);
    const int64_t b = s / a.positions;
    int i, j;
    ckb_position(s - b * a.positions, a.pass, a.wl, &i, &j);
    a.y_hat[((b * a.hl + i) * a.wl + j) * a.m + a.cg + m] = a.sym[e] + a.mu[e];
  }
}

// tfc_scctx_params, and tfc_checkerboard_params with c_g = 0 and M_g = M: errors go by the `name` that was called,
// profiles by its `label`.
int params_entry(const char* name, const char* label, int pass, const float* y, float* y_hat, const float* psi,
                 const float* packed, int64_t packed_floats, int64_t batch, int64_t hl, int64_t wl, int m, int cg, int mg,
                 int p, int h1, int h2, int num_scales, float* mu, float* index_float, int32_t* idx, int32_t* sym,
                 void* stream) {
  ScxArgs a = {};
  const char* e = scctx_layout(m, cg, mg, p, h1, h2, &a.S);
  if (!e) e = scctx_check(pass, batch, hl, wl, num_scales, packed_floats, a.S);
  if (e)
    return fail("%s: %s (pass %d, batch %lld, Hl %lld, Wl %lld, M %d, c_g %d, M_g %d, P %d, H1 %d, H2 %d, num_scales %d, "
                "%lld packed floats)", name, e, pass, static_cast<long long>(batch), static_cast<long long>(hl),
                static_cast<long long>(wl), m, cg, mg, p, h1, h2, num_scales, static_cast<long long>(packed_floats));
  a.positions = ckb_positions(hl, wl, pass);
  if (batch == 0 || a.positions == 0) return 0;
  if (!y_hat || !psi || !packed || !mu || !index_float || !idx)
    return fail("%s: y_hat, psi, packed, mu, index_float and idx must not be null", name);
  if (y && !sym) return fail("%s: sym must not be null when y is given", name);
  a.pass = pass;
  a.hl = static_cast<int>(hl);
  a.wl = static_cast<int>(wl);
  a.num_scales = num_scales;
  a.tiles = (a.positions + CKB_TILE - 1) / CKB_TILE;
  a.packed = packed;
  a.psi = psi;
  a.y = y;
  a.y_hat = y_hat;
  a.mu = mu;
  a.index_float = index_float;
  a.idx = idx;
  a.sym = sym;
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer(label, st);
  const dim3 grid(static_cast<unsigned>(a.tiles * batch));
  if (pass == 0)
    hipLaunchKernelGGL(scctx_params_kernel<0>, grid, dim3(CKB_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL(scctx_params_kernel<1>, grid, dim3(CKB_THREADS), 0, st, a);
  TFC_HIP(hipGetLastError());
  return 0;
}

// tfc_scctx_place, and tfc_checkerboard_place with c_g = 0 and M_g = M.
int place_entry(const char* name, const char* label, int pass, const float* sym, const float* mu, float* y_hat,
                int64_t batch, int64_t hl, int64_t wl, int m, int cg, int mg, void* stream) {
  if (pass != 0 && pass != 1) return fail("%s: pass must be 0 or 1, got %d", name, pass);
  if (m < 1 || m > CTX_MAX_DIM) return fail("%s: M must be in [1, 65536], got %d", name, m);
  if (cg < 0 || mg < 1 || cg > m - mg)
    return fail("%s: the group must lie inside the latent: c_g >= 0, M_g >= 1, c_g + M_g <= M (M %d, c_g %d, M_g %d)",
                name, m, cg, mg);
  if (batch < 0) return fail("%s: the batch size must not be negative", name);
  if (hl < 1 || wl < 1 || hl > (1 << 24) || wl > (1 << 24))
    return fail("%s: Hl and Wl must be in [1, 2^24] (Hl %lld, Wl %lld)", name, static_cast<long long>(hl),
                static_cast<long long>(wl));
  if (batch > 0 && hl * wl > (1ll << 40) / batch) return fail("%s: batch * Hl * Wl must be at most 2^40", name);
  ScxPlace a = {};
  a.positions = ckb_positions(hl, wl, pass);
  a.total = batch * a.positions * mg;
  if (a.total == 0) return 0;
  if (!sym || !mu || !y_hat) return fail("%s: sym, mu and y_hat must not be null", name);
  a.pass = pass;
  a.hl = static_cast<int>(hl);
  a.wl = static_cast<int>(wl);
  a.m = m;
  a.cg = cg;
  a.mg = mg;
  a.sym = sym;
  a.mu = mu;
  a.y_hat = y_hat;
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer(label, st);
  const int64_t blocks = (a.total + 255) / 256;
  hipLaunchKernelGGL(scctx_place_kernel, dim3(static_cast<unsigned>(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st,
                     a);
  TFC_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_scctx_params(int pass, const float* y, float* y_hat, const float* psi, const float* packed,
                                int64_t packed_floats, int64_t batch, int64_t hl, int64_t wl, int m, int cg, int mg,
                                int p, int h1, int h2, int num_scales, float* mu, float* index_float, int32_t* idx,
                                int32_t* sym, void* stream) {
  return tfc::params_entry("tfc_scctx_params", "scctx_params", pass, y, y_hat, psi, packed, packed_floats, batch, hl, wl,
                           m, cg, mg, p, h1, h2, num_scales, mu, index_float, idx, sym, stream);
}

extern "C" int tfc_scctx_place(int pass, const float* sym, const float* mu, float* y_hat, int64_t batch, int64_t hl,
                               int64_t wl, int m, int cg, int mg, void* stream) {
  return tfc::place_entry("tfc_scctx_place", "scctx_place", pass, sym, mu, y_hat, batch, hl, wl, m, cg, mg, stream);
}

// The checkerboard model: one group that is the whole latent.
extern "C" int tfc_checkerboard_params(int pass, const float* y, float* y_hat, const float* psi, const float* packed,
                                       int64_t packed_floats, int64_t batch, int64_t hl, int64_t wl, int m, int p,
                                       int h1, int h2, int num_scales, float* mu, float* index_float, int32_t* idx,
                                       int32_t* sym, void* stream) {
  return tfc::params_entry("tfc_checkerboard_params", "checkerboard_params", pass, y, y_hat, psi, packed, packed_floats,
                           batch, hl, wl, m, 0, m, p, h1, h2, num_scales, mu, index_float, idx, sym, stream);
}

extern "C" int tfc_checkerboard_place(int pass, const float* sym, const float* mu, float* y_hat, int64_t batch,
                                      int64_t hl, int64_t wl, int m, void* stream) {
  return tfc::place_entry("tfc_checkerboard_place", "checkerboard_place", pass, sym, mu, y_hat, batch, hl, wl, m, 0, m,
                          stream);
}

