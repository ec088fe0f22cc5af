// The engine of the checkerboard kernels (space_channel.hip; the checkerboard context model of He, Zheng, Sun, Wang and
// Qin, CVPR 2021, is their one-group case): the compact order of a pass, the MFMA walk over K with the weights a group
// of k-steps ahead (ckb_mma) and the layer driver for one tile of CKB_TILE positions (ckb_layer).  The constants are
// those of context_params.h.  The plan:
//
// A workgroup of CKB_THREADS threads owns CKB_TILE = 32 consecutive compact positions of one image and runs the four
// dense layers on v_mfma_f32_32x32x2_f32: the 32 positions are the rows of the A operand, 32 output columns the
// columns of B, and a wave accumulates up to CKB_BLOCKS column blocks side by side (16 accumulator registers each)
// while it walks K.  That instruction is bit for bit D = fmaf(a[k+1], b[k+1], fmaf(a[k], b[k], C)), so every output
// element is ONE chain: its bias, then one fmaf per input row in ascending k (for the correlation: taps in row-major
// order, the channels of a tap ascending, a neighbour outside the latent contributing fmaf(0, w, acc); for the first
// layer: the context features, then the P hyperprior features).  Rows and columns of an MFMA do not interact, and
// nothing here splits K across waves, so the chain depends on the sizes alone: not on the batch, the tile, the slot in
// the tile or the neighbours that exist.  Encoder and decoder run the same kernel.
//
// Activations stay in LDS between the layers, k-major: row k holds the 32 positions' values of feature k, so the A
// operand of k-step s is the 64 consecutive floats at row 2 s, one ds_read_b32 without a bank conflict, and an
// accumulator column goes back as four 16-byte stores.  Buffer A holds ctx, then h2; buffer B holds h1, then the
// output; a third region stages the gathered inputs (a tap's y_hat rows, psi) CKB_STAGE_K rows at a time, the next
// chunk's global loads in flight while the current one is multiplied.  [ctx, psi] are two K ranges of the first layer.
// With the checkerboard model's widths A is 64 KiB and B 80 KiB: the kernel declares gfx950's whole 160 KiB of LDS, on
// purpose (one workgroup of four waves per CU, one wave per SIMD, which is what the f32 MFMA needs to reach its rate).
//
// Weights: no two waves of a workgroup use the same weight element (a wave owns its columns for all 32 positions),
// so a trip through LDS would add traffic and save none; each lane loads its B operand, one float of the packed
// buffer, straight into a register, 128 contiguous bytes per half wave, eight k-steps ahead.  The whole packed buffer
// is read once per tile of 32 positions.
//
// A layer's chain takes the LDS-resident rows first and then up to two staged segments in the order given: a segment
// is a channel range of a [B, Hl, Wl, stride] tensor seen through a list of taps of the 5x5 window, taps in ascending
// order, the channels of a tap ascending, a neighbour outside the latent and a padded row entering as zeros (never
// skipped).
#pragma once
#include "context_shared.h"
#include "mfma_types.h"

namespace tfc {

// Compact slot -> raster index i * Wl + j of the position
__device__ __forceinline__ void ckb_position(int64_t slot, int pass, int wl, int* i, int* j) {
  if (wl & 1) {
    const int64_t n = 2 * slot + pass;
    *i = static_cast<int>(n / wl);
    *j = static_cast<int>(n - static_cast<int64_t>(*i) * wl);
  } else {
    const int half = wl >> 1;
    *i = static_cast<int>(slot / half);
    const int c = static_cast<int>(slot - static_cast<int64_t>(*i) * half);
    *j = 2 * c + ((*i + pass) & 1);
  }
}

// acc[q] += in[0 .. Kp) x w[0 .. Kp)[col q], k ascending.  `in` is LDS, k-major rows of CKB_TILE floats; `wq[q]` points
// at w[lane >> 5][column of block q for this lane]; Kp is a multiple of CTX_KPAD, so it is even.
template <int NQ>
__device__ __forceinline__ void ckb_mma(f32x16 (&acc)[NQ], const float* in, int Kp, const float* (&wq)[NQ], int O) {
  constexpr int G = CKB_GROUP;
  const int lane = threadIdx.x & 63;
  const float* a = in + lane;
  const size_t step = 2 * static_cast<size_t>(O);
  const int steps = Kp >> 1, groups = steps / G;
  // whole groups of G k-steps: the next group's weights are on their way while this one is multiplied
  float next[G][NQ];
  auto load = [&](int g) {
#pragma unroll
    for (int u = 0; u < G; ++u)
#pragma unroll
      for (int q = 0; q < NQ; ++q) next[u][q] = wq[q][static_cast<size_t>(g * G + u) * step];
  };
  if (groups > 0) load(0);
  for (int g = 0; g < groups; ++g) {
    float av[G], bv[G][NQ];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      av[u] = a[static_cast<size_t>(g * G + u) * (2 * CKB_TILE)];
#pragma unroll
      for (int q = 0; q < NQ; ++q) bv[u][q] = next[u][q];
    }
    if (g + 1 < groups) load(g + 1);
#pragma unroll
    for (int u = 0; u < G; ++u)
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u][q], acc[q], 0, 0, 0);
  }
  for (int s = groups * G; s < steps; ++s) {
    const float av = a[static_cast<size_t>(s) * (2 * CKB_TILE)];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wq[q][static_cast<size_t>(s) * step], acc[q], 0, 0, 0);
  }
}
static_assert(CTX_KPAD % 2 == 0, "a k-step of the MFMA is two input rows");

// What a thread fetches of one staged chunk: position (tid & 31) of the tile, 8 consecutive input rows.
constexpr int CKB_STAGE_PER_THREAD = CKB_STAGE_K * CKB_TILE / CKB_THREADS;
static_assert(CKB_STAGE_PER_THREAD * (CKB_THREADS / CKB_TILE) == CKB_STAGE_K, "a chunk is 8 row groups of 32 positions");

struct CkbTile {
  int b, np;                // image, live positions of the tile
  int pi, pj;               // this thread's staged position (tid & 31), or pi < 0 when it is beyond the pass
  int hl, wl;               // the latent
};

// One staged segment of a layer's chain: rows [0, Cp) of src[the position moved by the tap][C channels], C <= Cp, against
// w + tap * Cp * O.  `src` points at the segment's first channel of a [B, Hl, Wl, stride] tensor.  Tap t is element
// first + step * t of the 5x5 window counted row-major: (12, 0) is the position itself, (1, 2) the 12 checkerboard taps,
// (0, 1) all 25.
struct CkbSeg {
  const float* src;
  const float* w;
  int stride, C, Cp, taps, first, step;
};
constexpr int CKB_WINDOW_CENTRE = 12;

// One layer for the tile: out (k-major, LDS) = act(bias + chain).  The chain takes the LDS-resident rows [0, Kl) of
// `in` against wl first, then the `nseg` staged segments s0, s1 in that order.  A wave accumulates NQ column blocks side
// by side (blocks wave, wave + 4, ...); NQ is the same for the whole workgroup, and a block beyond the layer's width
// computes a live column again and drops it.  All threads of the workgroup call it together.  `store` receives
// (column, first of four positions, the four values).
template <int NQ, typename Store>
__device__ __forceinline__ void ckb_layer(const CkbTile& t, float* stage, const float* in, int Kl, const float* wl,
                                          int nseg, const CkbSeg& s0, const CkbSeg& s1, const float* bias, int O, int Op,
                                          Store store) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int col = lane & 31, kk = lane >> 5;
  const int nblk = (Op + 31) >> 5;
  const int spos = threadIdx.x & (CKB_TILE - 1), sk = (threadIdx.x / CKB_TILE) * CKB_STAGE_PER_THREAD;
  const int chunks0 = nseg > 0 ? s0.taps * ((s0.Cp + CKB_STAGE_K - 1) / CKB_STAGE_K) : 0;
  const int chunks = chunks0 + (nseg > 1 ? s1.taps * ((s1.Cp + CKB_STAGE_K - 1) / CKB_STAGE_K) : 0);

  for (int base = 0; base < nblk; base += (CKB_THREADS / 64) * NQ) {
    f32x16 acc[NQ];
    const float* wq[NQ];
    int cq[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      cq[q] = (base + wave + 4 * q) * 32 + col;
      const int c = min(cq[q], O - 1);
      const float bv = bias[c];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = bv;
      wq[q] = wl + static_cast<size_t>(kk) * O + c;
    }
    if (Kl > 0) ckb_mma<NQ>(acc, in, Kl, wq, O);
    if (chunks > 0) {
      float r[CKB_STAGE_PER_THREAD];
      auto fetch = [&](int c) {
        const bool second = c >= chunks0;
        const CkbSeg& s = second ? s1 : s0;
        const int cc = second ? c - chunks0 : c;
        const int per_tap = (s.Cp + CKB_STAGE_K - 1) / CKB_STAGE_K;
        const int tap = cc / per_tap, k0 = (cc - tap * per_tap) * CKB_STAGE_K + sk;
        const int el = s.first + s.step * tap;
        const int ii = t.pi + el / 5 - 2, jj = t.pj + el % 5 - 2;
        const bool live = t.pi >= 0 && ii >= 0 && ii < t.hl && jj >= 0 && jj < t.wl;
        const float* row =
            s.src + ((static_cast<int64_t>(t.b) * t.hl + (live ? ii : 0)) * t.wl + (live ? jj : 0)) * s.stride;
#pragma unroll
        for (int e = 0; e < CKB_STAGE_PER_THREAD; ++e) r[e] = (live && k0 + e < s.C) ? row[k0 + e] : 0.f;
      };
      fetch(0);
      for (int c = 0; c < chunks; ++c) {
        const bool second = c >= chunks0;
        const CkbSeg& s = second ? s1 : s0;
        const int cc = second ? c - chunks0 : c;
        const int per_tap = (s.Cp + CKB_STAGE_K - 1) / CKB_STAGE_K;
        const int tap = cc / per_tap, k0 = (cc - tap * per_tap) * CKB_STAGE_K;
        const int kn = min(CKB_STAGE_K, s.Cp - k0);
#pragma unroll
        for (int e = 0; e < CKB_STAGE_PER_THREAD; ++e) stage[(sk + e) * CKB_TILE + spos] = r[e];
        __syncthreads();
        if (c + 1 < chunks) fetch(c + 1);
        const float* wb = s.w + (static_cast<size_t>(tap) * s.Cp + k0 + kk) * O;
#pragma unroll
        for (int q = 0; q < NQ; ++q) wq[q] = wb + min(cq[q], O - 1);
        ckb_mma<NQ>(acc, stage, kn, wq, O);
        __syncthreads();
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (cq[q] < Op) {
        const bool live = cq[q] < O;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = live ? acc[q][4 * g + e] : 0.f;
          store(cq[q], 8 * g + 4 * kk, v);
        }
      }
    }
  }
}

// ckb_layer with the block count of the layer's width: ceil(blocks / 4), at most CKB_BLOCKS (wider layers take turns)
template <typename Store>
__device__ __forceinline__ void ckb_layer_n(const CkbTile& t, float* stage, const float* in, int Kl, const float* wl,
                                            int nseg, const CkbSeg& s0, const CkbSeg& s1, const float* bias, int O,
                                            int Op, Store store) {
  const int per_wave = (((Op + 31) >> 5) + 3) >> 2;
  switch (per_wave) {                 // the same for every thread of the grid
    case 1: ckb_layer<1>(t, stage, in, Kl, wl, nseg, s0, s1, bias, O, Op, store); break;
    case 2: ckb_layer<2>(t, stage, in, Kl, wl, nseg, s0, s1, bias, O, Op, store); break;
    case 3: ckb_layer<3>(t, stage, in, Kl, wl, nseg, s0, s1, bias, O, Op, store); break;
    case 4: ckb_layer<4>(t, stage, in, Kl, wl, nseg, s0, s1, bias, O, Op, store); break;
    default: ckb_layer<CKB_BLOCKS>(t, stage, in, Kl, wl, nseg, s0, s1, bias, O, Op, store); break;
  }
}
static_assert(CKB_BLOCKS == 5, "ckb_layer_n lists the block counts");

// The store of a layer into an LDS buffer, k-major, with or without the leaky ReLU
__device__ __forceinline__ auto ckb_store_to(float* buf, bool lrelu) {
  return [buf, lrelu](int col, int pos, f32x4 v) {
    if (lrelu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ctx_lrelu(v[e]);
    }
    *reinterpret_cast<f32x4*>(buf + static_cast<size_t>(col) * CKB_TILE + pos) = v;
  };
}

// The three dense layers after ctx (in bufA, rows [0, c2p)): h1 -> B (context rows, then the hyperprior rows staged
// from psi), h2 -> A, out -> B.  `packed` and L are one group's ctx_layout sections.
__device__ __forceinline__ void ckb_network(const CkbTile& t, const ContextLayout& L, const float* packed,
                                            const float* psi, float* bufA, float* bufB, float* stage) {
  const CkbSeg none = {};
  const CkbSeg hyper = {psi, packed + L.w1p, L.p, L.p, L.pp, 1, CKB_WINDOW_CENTRE, 0};
  ckb_layer_n(t, stage, bufA, L.c2p, packed + L.w1c, 1, hyper, none, packed + L.b1, L.h1, L.h1p, ckb_store_to(bufB, true));
  __syncthreads();
  ckb_layer_n(t, stage, bufB, L.h1p, packed + L.w2, 0, none, none, packed + L.b2, L.h2, L.h2p, ckb_store_to(bufA, true));
  __syncthreads();
  ckb_layer_n(t, stage, bufA, L.h2p, packed + L.w3, 0, none, none, packed + L.b3, L.c2, L.c2, ckb_store_to(bufB, false));
  __syncthreads();
}

}  // namespace tfc
