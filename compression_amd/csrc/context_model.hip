// The spatially autoregressive context model of Minnen, Ballé and Toderici, "Joint autoregressive and hierarchical
// priors for learned image compression" (NeurIPS 2018) on gfx950: masked 5x5 correlation, the pointwise
// entropy-parameter network and the per-element coding of every latent position in ONE launch, encoder side
// (context_scan_kernel) and decoder side (context_decode_kernel).  include/tfc_hip.h states the definition.
//
// One workgroup of CTX_THREADS threads per image.  Position (i, j) belongs to step t = j + 3 i; every position of a step
// depends on earlier steps only (the latest causal neighbour, (i - 1, j + 2), is of step t - 1), so a step's positions
// go through the network together, `waves` of them at a time (what fits CTX_LDS_FLOATS; rows beyond that are taken in
// turns), and are then coded side by side, one wave per position: each latent row is a code stream of its own.
//
// The network of a chunk is four dense layers over the chunk's positions, computed by the whole workgroup: a thread
// owns one output column for four positions and sums K in four interleaved partial sums (k mod 4), combined as
// (a0 + a1) + (a2 + a3) and added to the bias.  ctx_network() is that code for both kernels: the decoder reproduces
// the encoder's y_hat bit for bit because it runs the same instructions on the same inputs in the same order.  The
// hyperprior half of the first layer depends on no decoded value; it is computed for all positions of the image
// before the serial part (ctx_precompute) and read back as the first layer's starting value.
//
// The decoded values travel through global memory (y_hat is an output anyway): a step reads the rows above and the
// positions to the left that earlier steps of the SAME workgroup stored, ordered by __syncthreads().  Nothing waits
// on another workgroup.  Every loop bound comes from the shapes; the unary part of an escape is bounded by
// dec_escape() and reads past a string's end yield zeros (window_load), so damaged input ends the kernel as any other.
#include "context_shared.h"
#include "range_tables.h"
#include "range_wave.h"

#include "../../include/tfc_hip.h"

namespace tfc {
namespace {

struct CtxArgs {
  ContextLayout L;
  int batch, hl, wl, num_scales;
  const float* packed;
  const float* psi;         // [B, Hl, Wl, P]
  float* pre1;              // workspace [B, Hl * Wl, H1]
  uint4* state;             // workspace [B * Hl]: base, span_m1, window, pulls of a row's decoder
  float* y_hat;             // [B, Hl, Wl, M]
  // scan
  const float* y;
  int32_t* sym;
  int32_t* idx;
  float* mu;
  float* index_float;
  // decode
  TableView tab;
  const uint8_t* blob;
  const long long* off;     // [B * Hl + 1]
  const int32_t* cdf_offset;
  uint8_t* ok;
};

// out(p, o) = act(init(p, o) + sum_k in[p][k] w[k][o]) for p < np, o < O; out(p, o) = 0 for O <= o < Op (the next
// layer's K padding).  `in` is LDS, [np][ldin], Kp a multiple of CTX_KPAD, w [Kp][O] with zero rows behind K.
template <typename Init, typename Store>
__device__ __forceinline__ void ctx_dense(const float* in, int ldin, int Kp, const float* __restrict__ w, int O, int Op,
                                          int np, bool lrelu, Init init, Store store) {
  const int groups = (np + 3) >> 2;
  for (int item = threadIdx.x; item < groups * Op; item += CTX_THREADS) {
    const int g = item / Op, o = item - g * Op;
    const int p0 = g * 4;
    if (o >= O) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (p0 + q < np) store(p0 + q, o, 0.f);
      continue;
    }
    const float* row[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) row[q] = in + static_cast<size_t>(min(p0 + q, np - 1)) * ldin;
    float acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[q][r] = 0.f;
    const float* wk = w + o;
#pragma unroll 2
    for (int k = 0; k < Kp; k += 4) {
      const float w0 = wk[static_cast<size_t>(k) * O], w1 = wk[static_cast<size_t>(k + 1) * O],
                  w2 = wk[static_cast<size_t>(k + 2) * O], w3 = wk[static_cast<size_t>(k + 3) * O];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 x = *reinterpret_cast<const float4*>(row[q] + k);
        acc[q][0] = fmaf(x.x, w0, acc[q][0]);
        acc[q][1] = fmaf(x.y, w1, acc[q][1]);
        acc[q][2] = fmaf(x.z, w2, acc[q][2]);
        acc[q][3] = fmaf(x.w, w3, acc[q][3]);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (p0 + q < np) {
        float v = init(p0 + q, o) + ((acc[q][0] + acc[q][1]) + (acc[q][2] + acc[q][3]));
        if (lrelu) v = ctx_lrelu(v);
        store(p0 + q, o, v);
      }
    }
  }
}

// The masked correlation of a chunk: position p of the chunk is (i0 + p, t - 3 (i0 + p)) of image b.  Neighbours come
// from y_hat in global memory (this workgroup's own earlier stores); the ones outside the latent are skipped, which
// is adding zeros.  Same partial sums as ctx_dense, over k = the channel inside each tap.  A wave owns four positions
// and 64 output columns at a time: 64 channels of a neighbour arrive with one coalesced load, a channel per lane, and
// reach the FMAs through v_readlane (the load unit takes as long for 64 lanes reading one address as for a row).
__device__ __forceinline__ void ctx_taps(const CtxArgs& a, int b, int t, int i0, int np, float* bufA) {
  const ContextLayout& L = a.L;
  const int O = L.c2, Op = L.c2p, M = L.m;
  const float* __restrict__ wc = a.packed + L.wc;
  const float* bc = a.packed + L.bc;
  const float* yh = a.y_hat;
  const int groups = (np + 3) >> 2;
  const int ocols = (Op + 63) >> 6;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  for (int unit = wave; unit < groups * ocols; unit += CTX_THREADS / 64) {
    const int g = unit / ocols;
    const int o = (unit - g * ocols) * 64 + lane;
    const int p0 = g * 4;
    const bool live = o < O;
    int pi[4], pj[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pi[q] = i0 + min(p0 + q, np - 1);
      pj[q] = t - 3 * pi[q];
    }
    float acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[q][r] = 0.f;
    for (int tap = 0; tap < CTX_TAPS; ++tap) {
      const int di = tap / 5 - 2, dj = tap % 5 - 2;
      int64_t xoff[4];
      bool in[4];
      bool any = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ii = pi[q] + di, jj = pj[q] + dj;
        in[q] = ii >= 0 && jj >= 0 && jj < a.wl;
        xoff[q] = in[q] ? ((static_cast<int64_t>(b) * a.hl + ii) * a.wl + jj) * M : 0;
        any |= in[q];
      }
      if (!any) continue;
      const float* wk = wc + static_cast<size_t>(tap) * L.mp * O + (live ? o : 0);
      for (int k0 = 0; k0 < M; k0 += 64) {
        const int kn = min(64, M - k0);
        int xv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) xv[q] = (in[q] && lane < kn) ? __float_as_int(yh[xoff[q] + k0 + lane]) : 0;
        const float* wb = wk + static_cast<size_t>(k0) * O;
        const int kfull = kn & ~3;
        for (int kk = 0; kk < kfull; kk += 4) {
          const float w0 = wb[static_cast<size_t>(kk) * O], w1 = wb[static_cast<size_t>(kk + 1) * O],
                      w2 = wb[static_cast<size_t>(kk + 2) * O], w3 = wb[static_cast<size_t>(kk + 3) * O];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (in[q]) {
              acc[q][0] = fmaf(__int_as_float(__builtin_amdgcn_readlane(xv[q], kk)), w0, acc[q][0]);
              acc[q][1] = fmaf(__int_as_float(__builtin_amdgcn_readlane(xv[q], kk + 1)), w1, acc[q][1]);
              acc[q][2] = fmaf(__int_as_float(__builtin_amdgcn_readlane(xv[q], kk + 2)), w2, acc[q][2]);
              acc[q][3] = fmaf(__int_as_float(__builtin_amdgcn_readlane(xv[q], kk + 3)), w3, acc[q][3]);
            }
          }
        }
        const int rest = kn & 3;          // only behind the last full block of a tap, where M is no multiple of 4
        if (rest) {
          const float w0 = wb[static_cast<size_t>(kfull) * O];
          const float w1 = rest > 1 ? wb[static_cast<size_t>(kfull + 1) * O] : 0.f;
          const float w2 = rest > 2 ? wb[static_cast<size_t>(kfull + 2) * O] : 0.f;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (in[q]) {
              acc[q][0] = fmaf(__int_as_float(__builtin_amdgcn_readlane(xv[q], kfull)), w0, acc[q][0]);
              if (rest > 1) acc[q][1] = fmaf(__int_as_float(__builtin_amdgcn_readlane(xv[q], kfull + 1)), w1, acc[q][1]);
              if (rest > 2) acc[q][2] = fmaf(__int_as_float(__builtin_amdgcn_readlane(xv[q], kfull + 2)), w2, acc[q][2]);
            }
          }
        }
      }
    }
    if (o < Op) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (p0 + q < np)
          bufA[static_cast<size_t>(p0 + q) * L.a_floats + o] =
              live ? bc[o] + ((acc[q][0] + acc[q][1]) + (acc[q][2] + acc[q][3])) : 0.f;
    }
  }
}

// pre1[pos][o] = b1[o] + sum_k psi[pos][k] w1p[k][o] for every position of image b, `per` positions at a time.
__device__ __forceinline__ void ctx_precompute(const CtxArgs& a, int b, float* lds) {
  const ContextLayout& L = a.L;
  const int64_t positions = static_cast<int64_t>(a.hl) * a.wl;
  const int per = CTX_LDS_FLOATS / L.pp;
  const float* b1 = a.packed + L.b1;
  for (int64_t base = 0; base < positions; base += per) {
    const int np = static_cast<int>(min<int64_t>(per, positions - base));
    const float* src = a.psi + (static_cast<int64_t>(b) * positions + base) * L.p;
    for (int e = threadIdx.x; e < np * L.pp; e += CTX_THREADS) {
      const int p = e / L.pp, k = e - p * L.pp;
      lds[e] = k < L.p ? src[static_cast<int64_t>(p) * L.p + k] : 0.f;
    }
    __syncthreads();
    float* dst = a.pre1 + (static_cast<int64_t>(b) * positions + base) * L.h1;
    ctx_dense(lds, L.pp, L.pp, a.packed + L.w1p, L.h1, L.h1, np, false,
              [&](int, int o) { return b1[o]; },
              [&](int p, int o, float v) { dst[static_cast<int64_t>(p) * L.h1 + o] = v; });
    __syncthreads();
  }
}

// The network of one chunk (np positions from row i0 of step t): afterwards bufB[p] holds the 2M outputs of
// position p, means first.  Shared by both kernels.
__device__ __forceinline__ void ctx_network(const CtxArgs& a, int b, int t, int i0, int np, float* bufA, float* bufB) {
  const ContextLayout& L = a.L;
  const int la = L.a_floats, lb = L.b_floats;
  ctx_taps(a, b, t, i0, np, bufA);
  __syncthreads();
  const float* b2 = a.packed + L.b2;
  const float* b3 = a.packed + L.b3;
  const float* pre = a.pre1 + static_cast<int64_t>(b) * a.hl * a.wl * L.h1;
  ctx_dense(bufA, la, L.c2p, a.packed + L.w1c, L.h1, L.h1p, np, true,
            [&](int p, int o) {
              const int i = i0 + p;
              return o < L.h1 ? pre[(static_cast<int64_t>(i) * a.wl + (t - 3 * i)) * L.h1 + o] : 0.f;
            },
            [&](int p, int o, float v) { bufB[static_cast<size_t>(p) * lb + o] = v; });
  __syncthreads();
  ctx_dense(bufB, lb, L.h1p, a.packed + L.w2, L.h2, L.h2p, np, true, [&](int, int o) { return b2[o]; },
            [&](int p, int o, float v) { bufA[static_cast<size_t>(p) * la + o] = v; });
  __syncthreads();
  ctx_dense(bufA, la, L.h2p, a.packed + L.w3, L.c2, L.c2, np, false, [&](int, int o) { return b3[o]; },
            [&](int p, int o, float v) { bufB[static_cast<size_t>(p) * lb + o] = v; });
  __syncthreads();
}

// Rows of step t: i0 .. i0 + n - 1 (n <= 0: none)
__device__ __forceinline__ void ctx_step_rows(int t, int hl, int wl, int* i0, int* n) {
  const int hi = min(t / 3, hl - 1);
  const int lo = t - (wl - 1) > 0 ? (t - (wl - 1) + 2) / 3 : 0;
  *i0 = lo;
  *n = hi - lo + 1;
}

template <bool DECODE>
__global__ void __launch_bounds__(CTX_THREADS) context_kernel(const CtxArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[CTX_LDS_FLOATS];
  const ContextLayout& L = a.L;
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int M = L.m;
  const float hi = static_cast<float>(a.num_scales - 1);
  float* bufA = lds;
  float* bufB = lds + static_cast<size_t>(L.waves) * L.a_floats;

  if (DECODE) {
    // every row stream of the image opens
    for (int i = threadIdx.x; i < a.hl; i += CTX_THREADS) {
      const int64_t s = static_cast<int64_t>(b) * a.hl + i;
      a.state[s] = dec_open_state(a.blob + a.off[s], a.off[s + 1] - a.off[s]);
    }
  }
  ctx_precompute(a, b, lds);        // ends with __syncthreads()

  const int steps = (a.wl - 1) + 3 * (a.hl - 1) + 1;
  for (int t = 0; t < steps; ++t) {
    int row0, rows;
    ctx_step_rows(t, a.hl, a.wl, &row0, &rows);
    for (int c0 = 0; c0 < rows; c0 += L.waves) {
      const int np = min(L.waves, rows - c0);
      const int i0 = row0 + c0;
      ctx_network(a, b, t, i0, np, bufA, bufB);
      if (wave < np) {
        const int i = i0 + wave, j = t - 3 * i;
        const int64_t pos = (static_cast<int64_t>(b) * a.hl + i) * a.wl + j;
        const float* out = bufB + static_cast<size_t>(wave) * L.b_floats;
        if (!DECODE) {
          for (int m = lane; m < M; m += 64) {
            const float mu = out[m], fi = out[M + m];
            const float yv = a.y[pos * M + m];
            const int32_t s = static_cast<int32_t>(rintf(yv - mu));
            a.sym[pos * M + m] = s;
            a.idx[pos * M + m] = ctx_index(fi, hi);
            a.mu[pos * M + m] = mu;
            a.index_float[pos * M + m] = fi;
            a.y_hat[pos * M + m] = static_cast<float>(s) + mu;
          }
        } else {
          const int64_t s = static_cast<int64_t>(b) * a.hl + i;
          auto T = [&](int k) -> int32_t { return a.tab.data[k]; };
          const uint4 st0 = a.state[s];
          DecoderState st;
          st.base = __builtin_amdgcn_readfirstlane(st0.x);
          st.span_m1 = __builtin_amdgcn_readfirstlane(st0.y);
          st.window = __builtin_amdgcn_readfirstlane(st0.z);
          DigitWindow w;
          const long long o0 = a.off[s];
          w.src = a.blob + o0;
          w.len = a.off[s + 1] - o0;
          w.pulls = __builtin_amdgcn_readfirstlane(st0.w);
          w.base = w.pulls;
          window_load(w, lane);
          for (int m0 = 0; m0 < M; m0 += 64) {
            const int m = m0 + lane;
            int tb = 0;
            float mu = 0.f;
            if (m < M) {
              mu = out[m];
              tb = ctx_index(out[M + m], hi);
            }
            const int cnt = min(64, M - m0);
            int outv = 0;
            for (int n = 0; n < cnt; ++n) {
              const int tn = __builtin_amdgcn_readlane(tb, n);
              const int2 row = a.tab.rows[tn];
              const int start = __builtin_amdgcn_readfirstlane(row.x);
              const int nints = __builtin_amdgcn_readfirstlane(row.y);
              const int sp = __builtin_amdgcn_readfirstlane(T(start));
              const int prec = sp < 0 ? -sp : sp;
              int v = dec_symbol(T, st, start + 1, nints - 1, prec, w, lane);
              if (sp < 0 && v == nints - 3) v = dec_escape(st, w, lane, nints);
              outv = tfc_writelane(v, n, outv);
            }
            if (m < M) a.y_hat[pos * M + m] = static_cast<float>(outv + a.cdf_offset[tb]) + mu;
          }
          if (lane == 0) {
            a.state[s] = make_uint4(st.base, st.span_m1, st.window, w.pulls);
            if (j == a.wl - 1) a.ok[s] = dec_finalize_ok(st.base, st.span_m1, st.window, w.pulls, w.len) ? 1 : 0;
          }
        }
      }
      __syncthreads();
    }
  }
}

bool ctx_aligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

int ctx_prepare(const char* name, const float* psi, const float* packed, int64_t packed_floats, int64_t batch,
                int64_t hl, int64_t wl, int m, int p, int h1, int h2, int num_scales, void* workspace, float* y_hat,
                CtxArgs* a) {
  if (int rc = ctx_check_args(name, m, p, h1, h2, batch, hl, wl, true, num_scales, packed_floats, &a->L)) return rc;
  if (batch == 0) return 0;
  if (!psi || !packed || !workspace || !y_hat) return fail("%s: psi, packed, workspace and y_hat must not be null", name);
  if (!ctx_aligned(packed) || !ctx_aligned(workspace)) return fail("%s: packed and workspace must be 16-byte aligned", name);
  a->batch = static_cast<int>(batch);
  a->hl = static_cast<int>(hl);
  a->wl = static_cast<int>(wl);
  a->num_scales = num_scales;
  a->packed = packed;
  a->psi = psi;
  a->pre1 = static_cast<float*>(workspace);
  const int64_t pre = batch * hl * wl * h1 * 4;
  a->state = reinterpret_cast<uint4*>(static_cast<char*>(workspace) + (pre + 15) / 16 * 16);
  a->y_hat = y_hat;
  return 0;
}

}  // namespace
}  // namespace tfc

extern "C" int64_t tfc_context_workspace(int64_t batch, int64_t hl, int64_t wl, int m, int p, int h1, int h2) {
  using namespace tfc;
  ContextLayout L;
  if (ctx_check_args("tfc_context_workspace", m, p, h1, h2, batch, hl, wl, false, 0, 0, &L)) return -1;
  return ctx_workspace_bytes(batch, hl, wl, h1);
}

extern "C" int tfc_context_scan(const float* y, const float* psi, const float* packed, int64_t packed_floats,
                                int64_t batch, int64_t hl, int64_t wl, int m, int p, int h1, int h2, int num_scales,
                                void* workspace, int32_t* sym, int32_t* idx, float* mu, float* index_float,
                                float* y_hat, void* stream) {
  using namespace tfc;
  CtxArgs a = {};
  if (int rc = ctx_prepare("tfc_context_scan", psi, packed, packed_floats, batch, hl, wl, m, p, h1, h2, num_scales,
                           workspace, y_hat, &a))
    return rc;
  if (batch == 0) return 0;
  if (!y || !sym || !idx || !mu || !index_float)
    return fail("tfc_context_scan: y, sym, idx, mu and index_float must not be null");
  a.y = y;
  a.sym = sym;
  a.idx = idx;
  a.mu = mu;
  a.index_float = index_float;
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer("context_scan", st);
  hipLaunchKernelGGL(context_kernel<false>, dim3(static_cast<unsigned>(batch)), dim3(CTX_THREADS), 0, st, a);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_context_decode(const tfc_tables* tables, const uint8_t* blob, const int64_t* offsets,
                                  const float* psi, const float* packed, int64_t packed_floats,
                                  const int32_t* cdf_offset, int64_t batch, int64_t hl, int64_t wl, int m, int p,
                                  int h1, int h2, int num_scales, void* workspace, float* y_hat, uint8_t* ok,
                                  void* stream) {
  using namespace tfc;
  CtxArgs a = {};
  if (int rc = ctx_prepare("tfc_context_decode", psi, packed, packed_floats, batch, hl, wl, m, p, h1, h2, num_scales,
                           workspace, y_hat, &a))
    return rc;
  if (!tables) return fail("tfc_context_decode: tables must not be null");
  if (static_cast<int64_t>(tables->rows.size()) != num_scales)
    return fail("tfc_context_decode: the tables hold %lld rows, num_scales is %d",
                static_cast<long long>(tables->rows.size()), num_scales);
  if (batch == 0) return 0;
  if (!blob || !offsets || !cdf_offset || !ok)
    return fail("tfc_context_decode: blob, offsets, cdf_offset and ok must not be null");
  a.tab = view_of(tables);
  a.blob = blob;
  a.off = reinterpret_cast<const long long*>(offsets);
  a.cdf_offset = cdf_offset;
  a.ok = ok;
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer("context_decode", st);
  hipLaunchKernelGGL(context_kernel<true>, dim3(static_cast<unsigned>(batch)), dim3(CTX_THREADS), 0, st, a);
  TFC_HIP(hipGetLastError());
  return 0;
}
