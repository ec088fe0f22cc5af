// Shifted-window attention (the Swin block's attention, here by this project's own definition: include/tfc_hip.h,
// tfc_window_attention_forward) for gfx950, channels last: qkv [B, H, W, 3 C] -> out [B, H, W, C], C = heads * D.
//
// As tensor ops this is a roll, a window-partition copy, two batched matmuls on tiny operands, a [windows, heads, T, T]
// score tensor written and read three times, a reverse copy and a roll back.  Here qkv is read once and out written
// once: no padded, rolled or partitioned tensor and no score tensor exists in memory.
//
// Layout.  T = ws * ws tokens per window.  A lane owns ONE token of ONE window for ONE head (blockIdx.y): it works out
// its source pixel from (window, token, shift) itself — that is the whole of "roll" and "partition" — keeps its q row
// (D floats) in registers and writes its k and v rows to LDS as float32.  After one barrier it walks the T keys of its
// window: every lane of a window reads the same k_j / v_j address (an LDS broadcast, no bank conflicts), the T scores
// stay in registers (the key loops are fully unrolled, so every index is a constant), and the softmax is the lane's
// own: no cross-lane reduction in the forward.  A key takes part iff it is valid and in the query's wrap class; any
// other key is skipped — weight exactly 0, whatever its k and v hold — and invalid tokens are neither read nor
// written.  A window's result is a function of that window's tokens and the table only, in a fixed order of
// summation: bit-identical whatever else is in the image or the batch.
//
// Precision.  float32 (and both dtypes in the backward) runs the products as float32 `fmaf` chains in key / channel
// order: the float32-input MFMA has the VALU's rate and the bits of exactly such a chain, and with one lane per query
// no operand has to cross lanes.  Softmax in float32: out_i = (sum_j p_ij v_j) / (sum_j p_ij), p_ij = exp(S_ij - max_j
// S_ij), one correctly rounded division at the end.  bfloat16 forward: both products on the bf16 MFMA with float32
// accumulation (wa_forward_mfma_kernel below), softmax in float32, p_ij (IN (0, 1], NOT YET NORMALISED) IS ROUNDED TO
// BFLOAT16 BEFORE P.V, the row sum uses the unrounded p, and out is rounded once on the store.  bfloat16 backward:
// inputs widened on load, float32 throughout (P is not rounded), dqkv rounded once.
//
// Backward (S and P recomputed, nothing saved by the forward), with dP = dO V^T, delta_i = dO_i . out_i
// (= rowsum(dP o P)) and dS = P o (dP - delta):
//   dV = P^T dO,   dQ = D^-1/2 dS K,   dK = D^-1/2 dS^T Q,   dtable[head, rel] = sum of dS over batches, windows, pairs.
// Row phase: lane i recomputes its row of P, out_i and delta_i, then dS (registers) and dQ_i.  Column phase: P, then
// dS, go through a [T][T + 1] LDS tile (the pad keeps a lane's row writes off one bank) and lane j sums its column in
// query order against dO / q rows staged over the k / v tiles.  dtable: a workgroup walks its window groups in a fixed
// order, every thread owning table entries whose dS it sums from the tile in (window, key) order, and writes ONE
// partial per workgroup; wa_dtable_merge_kernel adds the partials in workgroup order.  No float atomics: two calls
// give identical bits.  dqkv or dtable may be null: what nobody needs is not computed.
#include <hip/hip_runtime.h>

#include <cmath>
#include <initializer_list>

#include "../../include/tfc_hip.h"
#include "bf16_io.h"
#include "common.h"
#include "window_attention_params.h"

namespace tfc {
namespace {

struct WaParams {
  const void* qkv;
  const float* table;      // [heads, (2 ws - 1)^2]
  void* out;               // forward
  const void* dout;        // backward
  void* dqkv;              // backward, or null
  float* part;             // backward: [heads, gridDim.x, (2 ws - 1)^2] partial dtable, or null
  long long windows;       // B * nwy * nwx
  long long groups;        // backward: ceil(windows / windows per workgroup)
  int H, W, heads, shift;
  int nwy, nwx;            // windows down and across the padded grid
  float scale;             // D^-1/2
};

// Token t of window `win`: its wrap class (0..3), or -1 if it lies in the padding; `pix` = its pixel in [B, H, W].
template <int WS>
__device__ __forceinline__ int wa_token(const WaParams& p, long long win, int t, long long* pix) {
  const int per = p.nwy * p.nwx;
  const long long b = win / per;
  const int wi = static_cast<int>(win - b * per);
  const int wy = wi / p.nwx, wx = wi - wy * p.nwx;
  const int Hp = p.nwy * WS, Wp = p.nwx * WS;
  int y = wy * WS + t / WS + p.shift, x = wx * WS + t % WS + p.shift;
  const int fy = y >= Hp, fx = x >= Wp;
  y -= fy ? Hp : 0;
  x -= fx ? Wp : 0;
  *pix = (b * p.H + y) * p.W + x;
  return y < p.H && x < p.W ? fy * 2 + fx : -1;
}

// D consecutive elements from element `at` (a multiple of 16 bytes) <-> floats.
template <int D, bool BF16>
__device__ __forceinline__ void wa_load_row(const void* base, long long at, float* v) {
  constexpr int EPG = BF16 ? 8 : 4;
  const u32x4* src = reinterpret_cast<const u32x4*>(static_cast<const char*>(base) + at * (BF16 ? 2 : 4));
#pragma unroll
  for (int g = 0; g < D / EPG; ++g) unpack<BF16>(src[g], v + g * EPG);
}

template <int D, bool BF16>
__device__ __forceinline__ void wa_store_row(void* base, long long at, const float* v) {
  constexpr int EPG = BF16 ? 8 : 4;
  u32x4* dst = reinterpret_cast<u32x4*>(static_cast<char*>(base) + at * (BF16 ? 2 : 4));
#pragma unroll
  for (int g = 0; g < D / EPG; ++g) dst[g] = repack<BF16>(v + g * EPG);
}

template <int D>
__device__ __forceinline__ void wa_lds_put(float* row, const float* v) {
#pragma unroll
  for (int c = 0; c < D; c += 4) *reinterpret_cast<f32x4*>(row + c) = f32x4{v[c], v[c + 1], v[c + 2], v[c + 3]};
}

// a . row, in channel order
template <int D>
__device__ __forceinline__ float wa_dot(const float* a, const float* row) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < D; c += 4) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(row + c);
    s = fmaf(a[c], r[0], s);
    s = fmaf(a[c + 1], r[1], s);
    s = fmaf(a[c + 2], r[2], s);
    s = fmaf(a[c + 3], r[3], s);
  }
  return s;
}

// acc += w * row
template <int D>
__device__ __forceinline__ void wa_axpy(float w, const float* row, float* acc) {
#pragma unroll
  for (int c = 0; c < D; c += 4) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(row + c);
    acc[c] = fmaf(w, r[0], acc[c]);
    acc[c + 1] = fmaf(w, r[1], acc[c + 1]);
    acc[c + 2] = fmaf(w, r[2], acc[c + 2]);
    acc[c + 3] = fmaf(w, r[3], acc[c + 3]);
  }
}

// The row of query t: p[j] = exp(S_tj - max) for the keys that take part, 0 for the others -> the row sum.
template <int WS, int D>
__device__ __forceinline__ float wa_row(const float* q, const float* sk, const int* scls, const float* stab, int cls,
                                        int t, float scale, float* p) {
  constexpr int T = WS * WS, SPAN = 2 * WS - 1;
  const int rel0 = (t / WS + WS - 1) * SPAN + t % WS + WS - 1;
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const bool take = scls[j] == cls;
    const float s = fmaf(scale, wa_dot<D>(q, sk + j * D), stab[rel0 - (j / WS) * SPAN - j % WS]);
    p[j] = take ? s : -INFINITY;
    m = take ? fmaxf(m, s) : m;
  }
  float l = 0.f;
#pragma unroll
  for (int j = 0; j < T; ++j) {
    // (the query is a key of its own class, so m is finite unless a score is not)
    const float e = p[j] == -INFINITY ? 0.f : expf(p[j] - m);
    p[j] = e;
    l += e;
  }
  return l;
}

template <int WS, int D, bool BF16, int NWIN>
__global__ void __launch_bounds__(NWIN* WS* WS) wa_forward_kernel(WaParams p) {
  constexpr int T = WS * WS, R = (2 * WS - 1) * (2 * WS - 1), NT = NWIN * T;
  __shared__ __align__(16) float sk[NWIN * T * D];
  __shared__ __align__(16) float sv[NWIN * T * D];
  __shared__ float stab[R];
  __shared__ int scls[NWIN * T];
  const int tid = threadIdx.x, w = tid / T, t = tid % T;
  const int head = blockIdx.y, C = p.heads * D;
  for (int r = tid; r < R; r += NT) stab[r] = p.table[head * R + r];
  const long long win = static_cast<long long>(blockIdx.x) * NWIN + w;
  long long pix = 0;
  const int cls = win < p.windows ? wa_token<WS>(p, win, t, &pix) : -1;
  const long long at = pix * 3 * C + head * D;
  float q[D];
  if (cls >= 0) {
    float row[D];
    wa_load_row<D, BF16>(p.qkv, at, q);
    wa_load_row<D, BF16>(p.qkv, at + C, row);
    wa_lds_put<D>(sk + tid * D, row);
    wa_load_row<D, BF16>(p.qkv, at + 2 * C, row);
    wa_lds_put<D>(sv + tid * D, row);
  }
  scls[tid] = cls;
  __syncthreads();
  if (cls < 0) return;      // (the only barrier is behind us)

  float pr[T];
  const float l = wa_row<WS, D>(q, sk + w * T * D, scls + w * T, stab, cls, t, p.scale, pr);
  float acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = 0.f;
#pragma unroll
  for (int j = 0; j < T; ++j) {
    if (pr[j] != 0.f) {
      const float pj = BF16 ? bf16_bits_to_float(float_to_bf16_bits(pr[j])) : pr[j];
      wa_axpy<D>(pj, sv + (w * T + j) * D, acc);
    }
  }
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = acc[c] / l;
  wa_store_row<D, BF16>(p.out, pix * C + head * D, acc);
}

// The bfloat16 forward on the matrix cores.  One wave takes G = 32 NT tokens: one window of 64 (NT = 2) or
// WA_MFMA_WINDOWS_WS4 = 2 windows of 16 (NT = 1; the window slot is part of a token's class, so the cross-window pairs
// of the shared tile are excluded keys like any other).  With v_mfma_f32_32x32x16_bf16 (lane l, r = l & 31, h = l >> 5:
// A[row r][k = 8h + e], B[k = 8h + e][col r], C[row (reg & 3) + 8 (reg >> 2) + 4h][col r]):
//   S^T = K Q^T   A: 16 bytes of token r's k row, B: 16 bytes of token r's q row, both straight from qkv;
//                 the accumulator holds query r's scores against the tile's keys: softmax is per lane plus one
//                 exchange with lane r + 32;
//   O^T = V^T P^T the accumulator registers 8s .. 8s + 7, rounded to bfloat16, ARE the B fragment of key step s (keys
//                 16s + 8 (e >> 2) + 4h + (e & 3)), so P never moves between lanes; A gathers v of those keys at
//                 channel r (zero rows where D = 16).
// Float32 accumulation, softmax in float32, exp(S - max) rounded to bfloat16 before P.V, the row sum from the unrounded
// values, one division, out rounded once: the same roundings as the VALU kernel, in the MFMA's order of summation.
template <int WS, int D>
__global__ void __launch_bounds__(64) wa_forward_mfma_kernel(WaParams p) {
  constexpr int T = WS * WS, SPAN = 2 * WS - 1, R = SPAN * SPAN;
  constexpr int NW = WS == 8 ? WA_MFMA_WINDOWS_WS8 : WA_MFMA_WINDOWS_WS4, NT = NW * T / 32, G = 32 * NT, KS = D / 16;
  static_assert(NW * T % 32 == 0 && G <= 64, "a wave's tokens fill whole 32-row tiles");
  __shared__ float stab[R];
  __shared__ int scls[G];
  __shared__ long long spix[G];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, C = p.heads * D;
  for (int i = lane; i < R; i += 64) stab[i] = p.table[head * R + i];
  if (lane < G) {
    const int slot = lane / T;
    const long long win = static_cast<long long>(blockIdx.x) * NW + slot;
    long long pix = 0;
    const int cls = win < p.windows ? wa_token<WS>(p, win, lane % T, &pix) : -1;
    scls[lane] = cls < 0 ? -1 : cls + 4 * slot;
    spix[lane] = pix;
  }
  __syncthreads();
  const unsigned short* const base = static_cast<const unsigned short*>(p.qkv);

  // S^T: key tiles down, query tiles across
  bf16x8 qf[NT][KS], kf[NT][KS];
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
    const int g = 32 * tt + r;
    const bool on = scls[g] >= 0;
    const unsigned short* row = base + spix[g] * 3 * C + head * D + 8 * h;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      u32x4 qa = {0u, 0u, 0u, 0u}, ka = {0u, 0u, 0u, 0u};
      if (on) {
        qa = *reinterpret_cast<const u32x4*>(row + 16 * ks);
        ka = *reinterpret_cast<const u32x4*>(row + C + 16 * ks);
      }
      qf[tt][ks] = __builtin_bit_cast(bf16x8, qa);
      kf[tt][ks] = __builtin_bit_cast(bf16x8, ka);
    }
  }
  f32x16 sacc[NT][NT];
#pragma unroll
  for (int jt = 0; jt < NT; ++jt)
#pragma unroll
    for (int it = 0; it < NT; ++it) {
#pragma unroll
      for (int e = 0; e < 16; ++e) sacc[jt][it][e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        sacc[jt][it] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[jt][ks], qf[it][ks], sacc[jt][it], 0, 0, 0);
    }

  // V^T fragments: element e of key step (jt, s) is key 32 jt + 16 s + 8 (e >> 2) + 4h + (e & 3), channel r
  bf16x8 vf[NT][2];
#pragma unroll
  for (int jt = 0; jt < NT; ++jt)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
      u16x8 raw;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = 32 * jt + 16 * s + 8 * (e >> 2) + 4 * h + (e & 3);
        unsigned short bits = 0;
        if (r < D && scls[j] >= 0) bits = base[spix[j] * 3 * C + 2 * C + head * D + r];
        raw[e] = bits;
      }
      vf[jt][s] = __builtin_bit_cast(bf16x8, raw);
    }

#pragma unroll
  for (int it = 0; it < NT; ++it) {
    const int i = 32 * it + r, ti = i % T;
    const int cls = scls[i];
    const int rel0 = (ti / WS + WS - 1) * SPAN + ti % WS + WS - 1;
    float m = -INFINITY;
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int j = 32 * jt + (e & 3) + 8 * (e >> 2) + 4 * h, tj = j % T;
        const bool take = cls >= 0 && scls[j] == cls;
        const float sc = fmaf(p.scale, sacc[jt][it][e], stab[rel0 - (tj / WS) * SPAN - tj % WS]);
        sacc[jt][it][e] = take ? sc : -INFINITY;
        m = take ? fmaxf(m, sc) : m;
      }
    m = fmaxf(m, __shfl_xor(m, 32));
    float l = 0.f;
    f32x16 oacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[e] = 0.f;
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float sc = sacc[jt][it][e];
        const float pe = sc == -INFINITY ? 0.f : expf(sc - m);
        sacc[jt][it][e] = pe;
        l += pe;
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        u32x4 packed;
#pragma unroll
        for (int w = 0; w < 4; ++w) packed[w] = pack_bf16(sacc[jt][it][8 * s + 2 * w], sacc[jt][it][8 * s + 2 * w + 1]);
        oacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[jt][s], __builtin_bit_cast(bf16x8, packed), oacc, 0, 0, 0);
      }
    }
    l += __shfl_xor(l, 32);
    if (cls >= 0) {
      unsigned short* const dst = static_cast<unsigned short*>(p.out) + spix[i] * C + head * D;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int dd = 8 * q4 + 4 * h;
        if (dd < D) {
          u32x2 two;
          two[0] = pack_bf16(oacc[4 * q4] / l, oacc[4 * q4 + 1] / l);
          two[1] = pack_bf16(oacc[4 * q4 + 2] / l, oacc[4 * q4 + 3] / l);
          *reinterpret_cast<u32x2*>(dst + dd) = two;
        }
      }
    }
  }
}

template <int WS, int D, bool BF16, int NWIN>
__global__ void __launch_bounds__(NWIN* WS* WS) wa_backward_kernel(WaParams p) {
  constexpr int T = WS * WS, SPAN = 2 * WS - 1, R = SPAN * SPAN, NT = NWIN * T, NR = (R + NT - 1) / NT;
  __shared__ __align__(16) float sa[NWIN * T * D];        // k rows, then q rows
  __shared__ __align__(16) float sb[NWIN * T * D];        // v rows, then dO rows
  __shared__ float sm[NWIN * T * (T + 1)];                // P, then dS: [window][query][key], rows padded by one
  __shared__ float stab[R];
  __shared__ int scls[NWIN * T];
  const int tid = threadIdx.x, w = tid / T, t = tid % T;
  const int head = blockIdx.y, C = p.heads * D;
  for (int r = tid; r < R; r += NT) stab[r] = p.table[head * R + r];
  float dt[NR];
#pragma unroll
  for (int n = 0; n < NR; ++n) dt[n] = 0.f;
  float* const mrow = sm + (w * T + t) * (T + 1);         // this query's row
  const float* const mcol = sm + w * T * (T + 1) + t;     // this key's column

  for (long long g = blockIdx.x; g < p.groups; g += gridDim.x) {
    const long long win = g * NWIN + w;
    long long pix = 0;
    const int cls = win < p.windows ? wa_token<WS>(p, win, t, &pix) : -1;
    const long long at = pix * 3 * C + head * D;
    __syncthreads();                                      // the last group's readers are done
    float q[D], go[D], acc[D], pr[T];
#pragma unroll
    for (int c = 0; c < D; ++c) q[c] = go[c] = acc[c] = 0.f;
    if (cls >= 0) {
      float row[D];
      wa_load_row<D, BF16>(p.qkv, at, q);
      wa_load_row<D, BF16>(p.qkv, at + C, row);
      wa_lds_put<D>(sa + tid * D, row);
      wa_load_row<D, BF16>(p.qkv, at + 2 * C, row);
      wa_lds_put<D>(sb + tid * D, row);
      wa_load_row<D, BF16>(p.dout, pix * C + head * D, go);
    }
    scls[tid] = cls;
    __syncthreads();

    // row phase: P_i, out_i, delta_i; then dS_i and dQ_i
    if (cls >= 0) {
      const float l = wa_row<WS, D>(q, sa + w * T * D, scls + w * T, stab, cls, t, p.scale, pr);
      const float inv = 1.f / l;
#pragma unroll
      for (int j = 0; j < T; ++j) {
        pr[j] *= inv;
        if (pr[j] != 0.f) wa_axpy<D>(pr[j], sb + (w * T + j) * D, acc);
      }
    } else {
#pragma unroll
      for (int j = 0; j < T; ++j) pr[j] = 0.f;
    }
    float delta = 0.f;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      delta = fmaf(go[c], acc[c], delta);
      acc[c] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < T; ++j) mrow[j] = pr[j];
#pragma unroll
    for (int j = 0; j < T; ++j) {
      if (pr[j] != 0.f) {                                 // an excluded key: dS = 0 whatever its k and v hold
        const float ds = pr[j] * (wa_dot<D>(go, sb + (w * T + j) * D) - delta);
        pr[j] = ds;
        if (p.dqkv) wa_axpy<D>(ds, sa + (w * T + j) * D, acc);
      }
    }
    if (p.dqkv && cls >= 0) {
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] *= p.scale;
      wa_store_row<D, BF16>(p.dqkv, at, acc);
    }
    __syncthreads();                                      // k and v are read, P is written

    // column phase: dV_j = sum_i P_ij dO_i, then dK_j = D^-1/2 sum_i dS_ij q_i
    if (p.dqkv) {
      wa_lds_put<D>(sa + tid * D, q);
      wa_lds_put<D>(sb + tid * D, go);
      __syncthreads();
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = 0.f;
#pragma unroll 4
      for (int i = 0; i < T; ++i) wa_axpy<D>(mcol[i * (T + 1)], sb + (w * T + i) * D, acc);
      if (cls >= 0) wa_store_row<D, BF16>(p.dqkv, at + 2 * C, acc);
      __syncthreads();                                    // P is read
    }
#pragma unroll
    for (int j = 0; j < T; ++j) mrow[j] = pr[j];
    __syncthreads();
    if (p.dqkv) {
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = 0.f;
#pragma unroll 4
      for (int i = 0; i < T; ++i) wa_axpy<D>(mcol[i * (T + 1)], sa + (w * T + i) * D, acc);
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] *= p.scale;
      if (cls >= 0) wa_store_row<D, BF16>(p.dqkv, at + C, acc);
    }
    if (p.part) {
      // entry r = (dy, dx): the pairs (query = key + (dy, dx), key) of every window of the group, in (window, key) order
#pragma unroll
      for (int n = 0; n < NR; ++n) {
        const int r = tid + n * NT;
        if (r < R) {
          const int dy = r / SPAN - (WS - 1), dx = r % SPAN - (WS - 1);
          float s = dt[n];
          for (int ww = 0; ww < NWIN; ++ww)
            for (int j = 0; j < T; ++j) {
              const int iy = j / WS + dy, ix = j % WS + dx;
              if (iy >= 0 && iy < WS && ix >= 0 && ix < WS) s += sm[(ww * T + iy * WS + ix) * (T + 1) + j];
            }
          dt[n] = s;
        }
      }
    }
  }
  if (p.part) {
#pragma unroll
    for (int n = 0; n < NR; ++n) {
      const int r = tid + n * NT;
      if (r < R) p.part[(static_cast<long long>(head) * gridDim.x + blockIdx.x) * R + r] = dt[n];
    }
  }
}

// dtable[head][r] = the workgroups' partials in workgroup order.  grid (ceil(R / WA_MERGE_THREADS), heads).
__global__ void __launch_bounds__(WA_MERGE_THREADS) wa_dtable_merge_kernel(const float* part, int parts, int R,
                                                                          float* dtable) {
  const int r = blockIdx.x * WA_MERGE_THREADS + threadIdx.x;
  if (r >= R) return;
  const float* src = part + static_cast<long long>(blockIdx.y) * parts * R + r;
  float s = 0.f;
  for (int b = 0; b < parts; ++b) s += src[static_cast<long long>(b) * R];
  dtable[blockIdx.y * R + r] = s;
}

int wa_validate(const char* name, int dtype, int64_t batch, int64_t height, int64_t width, int heads, int head_dim,
                int window, int shift) {
  if (int rc = check_dtype(name, dtype)) return rc;
  if (window != 4 && window != 8) return fail("%s: window must be one of {4, 8}, got %d", name, window);
  if (head_dim != 16 && head_dim != 32) return fail("%s: head_dim must be one of {16, 32}, got %d", name, head_dim);
  if (shift != 0 && shift != window / 2)
    return fail("%s: shift must be 0 or window / 2 = %d, got %d", name, window / 2, shift);
  if (heads < 1 || heads > 65535) return fail("%s: heads must be in [1, 65535], got %d", name, heads);
  if (batch < 1 || height < 1 || width < 1)
    return fail("%s: batch, height and width must be at least 1, got %lld, %lld, %lld", name,
                static_cast<long long>(batch), static_cast<long long>(height), static_cast<long long>(width));
  if (height > (1 << 24) || width > (1 << 24)) return fail("%s: height and width must be at most 2^24", name);
  return 0;
}

bool wa_aligned(std::initializer_list<const void*> tensors) {
  for (const void* t : tensors)
    if (reinterpret_cast<uintptr_t>(t) % 16 != 0) return false;
  return true;
}

WaParams wa_params(int64_t batch, int64_t height, int64_t width, int heads, int head_dim, int window, int shift) {
  WaParams p = {};
  p.H = static_cast<int>(height); p.W = static_cast<int>(width);
  p.heads = heads; p.shift = shift;
  p.nwy = static_cast<int>(ceil_div(height, window)); p.nwx = static_cast<int>(ceil_div(width, window));
  p.windows = batch * p.nwy * p.nwx;
  p.scale = head_dim == 16 ? 0.25f : 0.17677669529663689f;       // D^-1/2 rounded to float32
  return p;
}

// float32: the VALU kernel; bfloat16: the MFMA kernel
template <int WS, int D, bool BF>
int wa_launch_forward(const WaParams& p, int heads, hipStream_t st, const char* name) {
  constexpr int NWIN = BF ? (WS == 8 ? WA_MFMA_WINDOWS_WS8 : WA_MFMA_WINDOWS_WS4)
                          : (WS == 8 ? WA_FWD_WINDOWS_WS8 : WA_FWD_WINDOWS_WS4);
  const long long blocks = ceil_div(p.windows, NWIN);
  if (blocks > 0x7fffffffll) return fail("%s: too many windows", name);
  const dim3 grid(static_cast<unsigned>(blocks), heads);
  if constexpr (BF) hipLaunchKernelGGL((wa_forward_mfma_kernel<WS, D>), grid, dim3(64), 0, st, p);
  else hipLaunchKernelGGL((wa_forward_kernel<WS, D, false, NWIN>), grid, dim3(NWIN * WS * WS), 0, st, p);
  return 0;
}

}  // namespace
}  // namespace tfc

#define TFC_WA_ROUTES(LAUNCH)                                                                           \
  if (window == 8 && head_dim == 16 && dtype == 0) LAUNCH(8, 16, false)                                 \
  else if (window == 8 && head_dim == 32 && dtype == 0) LAUNCH(8, 32, false)                            \
  else if (window == 4 && head_dim == 16 && dtype == 0) LAUNCH(4, 16, false)                            \
  else if (window == 4 && head_dim == 32 && dtype == 0) LAUNCH(4, 32, false)                            \
  else if (window == 8 && head_dim == 16) LAUNCH(8, 16, true)                                           \
  else if (window == 8 && head_dim == 32) LAUNCH(8, 32, true)                                           \
  else if (window == 4 && head_dim == 16) LAUNCH(4, 16, true)                                           \
  else LAUNCH(4, 32, true)

extern "C" int tfc_window_attention_forward(const void* qkv, const float* table, void* out, int dtype, int64_t batch,
                                            int64_t height, int64_t width, int heads, int head_dim, int window,
                                            int shift, void* stream) {
  using namespace tfc;
  const char* name = "tfc_window_attention_forward";
  if (int rc = wa_validate(name, dtype, batch, height, width, heads, head_dim, window, shift)) return rc;
  if (!qkv || !table || !out) return fail("%s: qkv, table and out must not be null", name);
  if (!wa_aligned({qkv, out})) return fail("%s: qkv and out must be 16-byte aligned", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  WaParams p = wa_params(batch, height, width, heads, head_dim, window, shift);
  p.qkv = qkv; p.table = table; p.out = out;
  KernelTimer timer("window_attention_forward", st);
#define TFC_WA_FWD(WS, D, BF)                                                      \
  {                                                                                \
    if (int rc = wa_launch_forward<WS, D, BF>(p, heads, st, name)) return rc;      \
  }
  TFC_WA_ROUTES(TFC_WA_FWD)
#undef TFC_WA_FWD
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_window_attention_backward(const void* qkv, const float* table, const void* dout, void* dqkv,
                                             float* dtable, int dtype, int64_t batch, int64_t height, int64_t width,
                                             int heads, int head_dim, int window, int shift, void* stream) {
  using namespace tfc;
  const char* name = "tfc_window_attention_backward";
  if (int rc = wa_validate(name, dtype, batch, height, width, heads, head_dim, window, shift)) return rc;
  if (!dqkv && !dtable) return 0;
  if (!qkv || !table || !dout) return fail("%s: qkv, table and dout must not be null", name);
  if (!wa_aligned({qkv, dout, dqkv})) return fail("%s: qkv, dout and dqkv must be 16-byte aligned", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  WaParams p = wa_params(batch, height, width, heads, head_dim, window, shift);
  p.qkv = qkv; p.table = table; p.dout = dout; p.dqkv = dqkv;
  const int R = (2 * window - 1) * (2 * window - 1);
  const int nwin = window == 8 ? WA_BWD_WINDOWS_WS8 : WA_BWD_WINDOWS_WS4;
  p.groups = ceil_div(p.windows, nwin);
  // the workgroup count, and with it the order of every sum, is a function of the shape alone
  const int blocks = static_cast<int>(std::min<long long>(p.groups, WA_DTABLE_PARTIALS));
  DevBuf part;
  if (dtable) {
    TFC_HIP(part.alloc(sizeof(float) * static_cast<size_t>(heads) * blocks * R, st));
    p.part = part.as<float>();
  }
  KernelTimer timer("window_attention_backward", st);
#define TFC_WA_BWD(WS, D, BF)                                                                             \
  {                                                                                                       \
    constexpr int NWIN = WS == 8 ? WA_BWD_WINDOWS_WS8 : WA_BWD_WINDOWS_WS4;                               \
    hipLaunchKernelGGL((wa_backward_kernel<WS, D, BF, NWIN>), dim3(blocks, heads), dim3(NWIN * WS * WS), \
                       0, st, p);                                                                         \
  }
  TFC_WA_ROUTES(TFC_WA_BWD)
#undef TFC_WA_BWD
  if (dtable)
    hipLaunchKernelGGL(wa_dtable_merge_kernel, dim3(static_cast<unsigned>(ceil_div(R, WA_MERGE_THREADS)), heads),
                       dim3(WA_MERGE_THREADS), 0, st, p.part, blocks, R, dtable);
  TFC_HIP(hipGetLastError());
  return 0;
}
