// ChannelNorm of HiFiC (models/hific/archs.py:214-297) for gfx950, channels last: x [pixels, C].
//
//   mean_p = sum_c x[p,c] / C
//   var_p  = sum_c (x[p,c] - mean_p)^2 / (C - 1)                 archs.py:262-273: N - 1, not N
//   y[p,c] = (x[p,c] - mean_p) * rsqrt(var_p + epsilon) * gamma[c] + beta[c]     (tf.nn.batch_normalization, :258)
//   y = relu(y) if relu;   y += residual[p,c] if residual       (the layers HiFiC puts behind 22 of its 24 norms)
//
// The reference runs this as mean, squared_difference, sum, divide, batch_normalization (+ ReLU / add): six launches
// and about five round trips over the activation.  Here it is one pass over HBM: x is read once, y written once.
//
// Layout (vector path, row bytes a multiple of 8, at most 256 (bfloat16) / 512 (float32) granules per unit):
//   * A granule is 16 bytes (8 bfloat16 / 4 float32).  A UNIT is one row, or — where a row is an odd number of
//     8-byte halves (C = 60 or 220 bfloat16: 120 / 440 bytes) — TWO consecutive rows, so that a unit starts on a
//     16-byte boundary and is V whole granules.  Of a pair's granules only the middle one holds both rows: its low
//     half ends row 0, its high half starts row 1.
//   * LPR = min(64, next power of two >= V) lanes share a unit, 64 / LPR units go through a wave at once, and lane
//     l of a unit holds granules l, l + LPR, ... (NG of them, a template parameter; slots >= V are masked).  A row of
//     960 bfloat16 values is 120 granules: LPR = 64, NG = 2, 120 of 128 slots in use; 60 bfloat16 values: pairs of
//     15 granules, LPR = 16, eight rows (960 contiguous bytes) per wave instruction.
//     Consecutive lanes hold consecutive granules, so eight lanes write one 128-byte line.
//   * The row stays in registers (float32) between the reductions and the epilogue.  Both moments are taken from
//     those registers, mean first, then sum (x - mean)^2: no E[x^2] - E[x]^2.  Sums cross lanes by DPP
//     (quad_perm, row_half_mirror, row_mirror), ds_swizzle (lane ^ 16) and v_permlane32_swap: the row reductions use no
//     LDS memory.
//   * A lane's channels are the same in every unit it visits: gamma and beta are read once into registers (a wave
//     takes at least four steps where there are enough, so that these reads stay a fraction of the x traffic).
//   * The next unit's x is requested before the current one is reduced.
// Any other C >= 2 (odd byte counts, rows longer than 8 KB) takes the wave-per-row kernel below, which re-reads the
// row from the caches for every pass; so does the last row of an odd number of paired rows.
//
// Backward (the reference relies on TF autodiff), with xhat = (x - mean) rstd and g' = g [y_pre_relu > 0]:
//   dx = rstd ( g' gamma - sum_c(g' gamma) / C - xhat sum_c(g' gamma xhat) / (C - 1) )
//   dgamma[c] = sum_p g' xhat,   dbeta[c] = sum_p g'
// archs.py:267 takes the variance through tf.stop_gradient(mean).  That changes no gradient: the term it removes is
// d var / d mean = -2 sum_c (x - mean) / (C - 1), and sum_c (x - mean) is zero.
// dx is one pass (the statistics are recomputed from x).  dgamma / dbeta: every wave keeps its sums in registers,
// adds those of its units once at the end (__shfl_xor), writes them to a workspace, and cnorm_param_sum_kernel adds the
// partials in a fixed order (16 slice sums per channel staged in LDS): no float atomics, two calls give identical bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <initializer_list>

#include "../../include/tfc_hip.h"
#include "bf16_io.h"
#include "launch.h"
#include "unit_sum.h"

namespace tfc {
namespace {

struct CnormParams {
  const void* x;
  const void* g;        // backward: dL/dy
  const void* res;      // forward: residual or null
  void* y;              // forward: y; backward: dx
  const float* gamma;   // or null: 1
  const float* beta;    // or null: 0
  float* part;          // backward: [parts][2][C] partial (dgamma, dbeta)
  long long pixels;     // wave-per-row kernel: rows it covers
  long long units;      // vector path: rows or row pairs
  long long row0;       // wave-per-row kernel: first row
  long long part0;      // wave-per-row kernel: first partial it owns
  int C;
  int V;                // granules per unit
  int lpr_log2;         // lanes per unit
  float eps, cf, cm1f;  // epsilon, C, C - 1
  int relu;
  int nt;               // non-temporal stores
};

// NG granules per lane; PAIR: a unit is two rows; BWD: dx and the parameter partials instead of y.
template <int NG, bool BF16, bool PAIR, bool BWD>
__global__ void __launch_bounds__(256) cnorm_vec_kernel(CnormParams p) {
  constexpr int EPG = BF16 ? 8 : 4;
  constexpr int HALF = EPG / 2;
  constexpr int NE = NG * EPG;
  const int lane = threadIdx.x & 63;
  const int lpr = 1 << p.lpr_log2;
  const int l = lane & (lpr - 1);
  const int grp = lane >> p.lpr_log2;
  const int rw = 64 >> p.lpr_log2;                 // units per wave instruction
  const long long wave = static_cast<long long>(blockIdx.x) * (blockDim.x >> 6) +
                         __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const long long nwaves = static_cast<long long>(gridDim.x) * (blockDim.x >> 6);
  const long long steps = (p.units + rw - 1) / rw;
  const int mid = p.V >> 1;                        // PAIR: the granule that holds both rows

  // this lane's slots: which exist, which row each half belongs to, its channels' gamma and beta
  bool on[NG], lo1[NG], hi1[NG];
  float gam[NE], bet[NE];
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int gr = j * lpr + l;
    on[j] = gr < p.V;
    lo1[j] = PAIR && gr > mid;
    hi1[j] = PAIR && gr >= mid;
    // (one 8- or 16-byte load per half granule: its channels are consecutive and start on a multiple of HALF)
    typedef __attribute__((ext_vector_type(HALF))) float halfvec;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int c0 = gr * EPG + hf * HALF - ((hf ? hi1[j] : lo1[j]) ? p.C : 0);
      halfvec gv, bv;
#pragma unroll
      for (int e = 0; e < HALF; ++e) { gv[e] = on[j] ? 1.f : 0.f; bv[e] = 0.f; }
      if (on[j] && p.gamma) gv = *reinterpret_cast<const halfvec*>(p.gamma + c0);
      if (on[j] && p.beta) bv = *reinterpret_cast<const halfvec*>(p.beta + c0);
#pragma unroll
      for (int e = 0; e < HALF; ++e) {
        gam[j * EPG + hf * HALF + e] = gv[e];
        bet[j * EPG + hf * HALF + e] = bv[e];
      }
    }
  }
  float dgam[BWD ? NE : 1], dbet[BWD ? NE : 1];
  if (BWD) {
#pragma unroll
    for (int k = 0; k < NE; ++k) dgam[k] = dbet[k] = 0.f;
  }

  const u32x4* const xg = static_cast<const u32x4*>(p.x);
  auto fetch = [&](const u32x4* base, long long step, u32x4* raw) {
    const long long u = step * rw + grp;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      raw[j] = u32x4{0u, 0u, 0u, 0u};
      if (on[j] && u < p.units) raw[j] = base[u * p.V + j * lpr + l];
    }
  };
  u32x4 xn[NG];
  if (wave < steps) fetch(xg, wave, xn);

  for (long long step = wave; step < steps; step += nwaves) {
    const long long u = step * rw + grp;
    const bool live = u < p.units;
    float v[NE];
#pragma unroll
    for (int j = 0; j < NG; ++j) unpack<BF16>(xn[j], v + j * EPG);
    u32x4 extra[NG];                            // forward: the residual; backward: g
    if (BWD) fetch(static_cast<const u32x4*>(p.g), step, extra);
    else if (p.res) fetch(static_cast<const u32x4*>(p.res), step, extra);
    if (step + nwaves < steps) fetch(xg, step + nwaves, xn);

    // mean (masked slots hold zeros)
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < NG; ++j)
#pragma unroll
      for (int e = 0; e < EPG; ++e) {
        const bool r1 = e < HALF ? lo1[j] : hi1[j];
        if (PAIR) { s0 += r1 ? 0.f : v[j * EPG + e]; s1 += r1 ? v[j * EPG + e] : 0.f; }
        else s0 += v[j * EPG + e];
      }
    const float m0 = unit_sum(s0, p.lpr_log2) / p.cf;
    const float m1 = PAIR ? unit_sum(s1, p.lpr_log2) / p.cf : 0.f;
    // variance from the centred values
    float q0 = 0.f, q1 = 0.f;
#pragma unroll
    for (int j = 0; j < NG; ++j)
#pragma unroll
      for (int e = 0; e < EPG; ++e) {
        const bool r1 = e < HALF ? lo1[j] : hi1[j];
        const float d = on[j] ? v[j * EPG + e] - (PAIR && r1 ? m1 : m0) : 0.f;
        v[j * EPG + e] = d;
        if (PAIR) { q0 = r1 ? q0 : fmaf(d, d, q0); q1 = r1 ? fmaf(d, d, q1) : q1; }
        else q0 = fmaf(d, d, q0);
      }
    // (a lane group past the last unit holds zeros: with epsilon = 0 its rsqrt(0) = inf must not reach the backward's
    // register sums as 0 * inf, so its rstd is 0 and everything it accumulates is 0; the sums themselves are taken by
    // all lanes)
    const float var0 = unit_sum(q0, p.lpr_log2) / p.cm1f;
    const float var1 = PAIR ? unit_sum(q1, p.lpr_log2) / p.cm1f : 0.f;
    const float rstd0 = live ? __builtin_amdgcn_rsqf(var0 + p.eps) : 0.f;
    const float rstd1 = PAIR && live ? __builtin_amdgcn_rsqf(var1 + p.eps) : 0.f;

    if (!BWD) {
#pragma unroll
      for (int j = 0; j < NG; ++j) {
        float r[EPG];
        if (p.res) unpack<BF16>(extra[j], r);
#pragma unroll
        for (int e = 0; e < EPG; ++e) {
          const bool r1 = e < HALF ? lo1[j] : hi1[j];
          float yv = v[j * EPG + e] * (PAIR && r1 ? rstd1 : rstd0) * gam[j * EPG + e] + bet[j * EPG + e];
          if (p.relu) yv = fmaxf(yv, 0.f);
          if (p.res) yv += r[e];
          v[j * EPG + e] = yv;
        }
        if (on[j] && live) store_granule(static_cast<u32x4*>(p.y) + u * p.V + j * lpr + l, repack<BF16>(v + j * EPG), p.nt);
      }
    } else {
      float gg[NE];
      float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
#pragma unroll
      for (int j = 0; j < NG; ++j) {
        float gv[EPG];
        unpack<BF16>(extra[j], gv);
#pragma unroll
        for (int e = 0; e < EPG; ++e) {
          const int k = j * EPG + e;
          const bool r1 = e < HALF ? lo1[j] : hi1[j];
          const float xh = v[k] * (PAIR && r1 ? rstd1 : rstd0);
          v[k] = xh;
          float gp = gv[e];
          if (p.relu) gp = xh * gam[k] + bet[k] > 0.f ? gp : 0.f;
          dgam[k] = fmaf(gp, xh, dgam[k]);
          dbet[k] += gp;
          const float t = gp * gam[k];
          gg[k] = t;
          if (PAIR) {
            a0 += r1 ? 0.f : t; a1 += r1 ? t : 0.f;
            b0 = r1 ? b0 : fmaf(t, xh, b0); b1 = r1 ? fmaf(t, xh, b1) : b1;
          } else {
            a0 += t; b0 = fmaf(t, xh, b0);
          }
        }
      }
      a0 = unit_sum(a0, p.lpr_log2) / p.cf;
      b0 = unit_sum(b0, p.lpr_log2) / p.cm1f;
      if (PAIR) {
        a1 = unit_sum(a1, p.lpr_log2) / p.cf;
        b1 = unit_sum(b1, p.lpr_log2) / p.cm1f;
      }
#pragma unroll
      for (int j = 0; j < NG; ++j) {
#pragma unroll
        for (int e = 0; e < EPG; ++e) {
          const int k = j * EPG + e;
          const bool r1 = PAIR && (e < HALF ? lo1[j] : hi1[j]);
          v[k] = (r1 ? rstd1 : rstd0) * (gg[k] - (r1 ? a1 : a0) - v[k] * (r1 ? b1 : b0));
        }
        if (on[j] && live) store_granule(static_cast<u32x4*>(p.y) + u * p.V + j * lpr + l, repack<BF16>(v + j * EPG), 0);
      }
    }
  }

  if (BWD) {
    // the wave's units hold the same channels in the same slots: add them up (lanes l, l + LPR, ...), then the
    // lanes of the first unit write the wave's partial: rows [wave][row of the pair]
    for (int off = lpr; off < 64; off <<= 1) {
#pragma unroll
      for (int k = 0; k < NE; ++k) {
        dgam[k] += __shfl_xor(dgam[k], off);
        dbet[k] += __shfl_xor(dbet[k], off);
      }
    }
    if (grp == 0) {
#pragma unroll
      for (int j = 0; j < NG; ++j)
#pragma unroll
        for (int e = 0; e < EPG; ++e) {
          const bool r1 = e < HALF ? lo1[j] : hi1[j];
          const int c = (j * lpr + l) * EPG + e - (r1 ? p.C : 0);
          float* const row = p.part + ((wave * (PAIR ? 2 : 1) + (r1 ? 1 : 0)) * 2) * p.C;
          if (on[j]) {
            row[c] = dgam[j * EPG + e];
            row[p.C + c] = dbet[j * EPG + e];
          }
        }
    }
  }
}

// Any C >= 2: one wave per row, lane l takes channels l, l + 64, ...; the passes re-read the row (from the caches).
// Backward: wave w adds into its own partial rows (zeroed by the host), always the same lane into the same word.
template <bool BF16, bool BWD>
__global__ void __launch_bounds__(256) cnorm_row_kernel(CnormParams p) {
  const int lane = threadIdx.x & 63;
  const long long wave = static_cast<long long>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long long nwaves = static_cast<long long>(gridDim.x) * (blockDim.x >> 6);
  float* const mine = BWD ? p.part + (p.part0 + wave) * 2 * p.C : nullptr;
  for (long long r = wave; r < p.pixels; r += nwaves) {
    const long long at = (p.row0 + r) * p.C;
    float s = 0.f;
    for (int c = lane; c < p.C; c += 64) s += load<BF16>(p.x, at + c);
    const float mean = unit_sum(s, 6) / p.cf;
    float q = 0.f;
    for (int c = lane; c < p.C; c += 64) {
      const float d = load<BF16>(p.x, at + c) - mean;
      q = fmaf(d, d, q);
    }
    const float rstd = __builtin_amdgcn_rsqf(unit_sum(q, 6) / p.cm1f + p.eps);
    if (!BWD) {
      for (int c = lane; c < p.C; c += 64) {
        float yv = (load<BF16>(p.x, at + c) - mean) * rstd * (p.gamma ? p.gamma[c] : 1.f) + (p.beta ? p.beta[c] : 0.f);
        if (p.relu) yv = fmaxf(yv, 0.f);
        if (p.res) yv += load<BF16>(p.res, at + c);
        store<BF16>(p.y, at + c, yv);
      }
    } else {
      float a = 0.f, b = 0.f;
      for (int c = lane; c < p.C; c += 64) {
        const float xh = (load<BF16>(p.x, at + c) - mean) * rstd;
        const float gm = p.gamma ? p.gamma[c] : 1.f;
        float gp = load<BF16>(p.g, at + c);
        if (p.relu) gp = xh * gm + (p.beta ? p.beta[c] : 0.f) > 0.f ? gp : 0.f;
        mine[c] = fmaf(gp, xh, mine[c]);
        mine[p.C + c] += gp;
        a += gp * gm;
        b = fmaf(gp * gm, xh, b);
      }
      a = unit_sum(a, 6) / p.cf;
      b = unit_sum(b, 6) / p.cm1f;
      for (int c = lane; c < p.C; c += 64) {
        const float xh = (load<BF16>(p.x, at + c) - mean) * rstd;
        const float gm = p.gamma ? p.gamma[c] : 1.f;
        float gp = load<BF16>(p.g, at + c);
        if (p.relu) gp = xh * gm + (p.beta ? p.beta[c] : 0.f) > 0.f ? gp : 0.f;
        store<BF16>(p.y, at + c, rstd * (gp * gm - a - xh * b));
      }
    }
  }
}

// dgamma[c] / dbeta[c] = sum of the partials in a fixed order: 16 strided slices per channel, then the 16 slice sums.
// grid (ceil(C / 64), 2: gamma, beta), block (64, 16).
__global__ void __launch_bounds__(1024) cnorm_param_sum_kernel(const float* part, long long parts, int C, float* dgamma,
                                                               float* dbeta) {
  __shared__ float slices[16][64];
  float* const out = blockIdx.y ? dbeta : dgamma;
  const int c = blockIdx.x * 64 + threadIdx.x;
  float s = 0.f;
  if (c < C)
    for (long long q = threadIdx.y; q < parts; q += 16) s += part[(q * 2 + blockIdx.y) * C + c];
  slices[threadIdx.y][threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.y == 0 && c < C && out) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += slices[k][threadIdx.x];
    out[c] = t;
  }
}

struct CnormPlan {
  bool vec = false, pair = false;
  int V = 0, lpr_log2 = 0, ng = 0;
  long long units = 0;
};

// How the rows of [pixels, C] go onto waves (see the top of the file).
CnormPlan cnorm_plan(int dtype, long long pixels, long long C, std::initializer_list<const void*> tensors) {
  CnormPlan plan;
  const long long row_bytes = C * dtype_bytes(dtype);
  bool aligned = true;
  for (const void* t : tensors) aligned = aligned && reinterpret_cast<uintptr_t>(t) % 16 == 0;
  if (!aligned || row_bytes % 8 != 0) return plan;
  plan.pair = row_bytes % 16 != 0;
  const long long V = (plan.pair ? 2 : 1) * row_bytes / 16;
  if (V > (dtype == 1 ? 256 : 512)) return plan;
  plan.vec = true;
  plan.V = static_cast<int>(V);
  while ((1 << plan.lpr_log2) < V && plan.lpr_log2 < 6) ++plan.lpr_log2;
  const int need = static_cast<int>((V + (1 << plan.lpr_log2) - 1) >> plan.lpr_log2);
  plan.ng = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 8;
  plan.units = plan.pair ? pixels / 2 : pixels;
  return plan;
}

template <bool BWD>
void cnorm_launch_vec(const CnormPlan& plan, int dtype, unsigned blocks, hipStream_t st, const CnormParams& p) {
#define TFC_CNORM_CASE(NGV, BF, PR)                                                                            \
  if (plan.ng == NGV && (dtype == 1) == BF && plan.pair == PR) {                                               \
    hipLaunchKernelGGL((cnorm_vec_kernel<NGV, BF, PR, BWD>), dim3(blocks), dim3(256), 0, st, p);               \
    return;                                                                                                    \
  }
  TFC_CNORM_CASE(1, false, false) TFC_CNORM_CASE(2, false, false) TFC_CNORM_CASE(4, false, false)
  TFC_CNORM_CASE(8, false, false) TFC_CNORM_CASE(1, false, true) TFC_CNORM_CASE(2, false, true)
  TFC_CNORM_CASE(4, false, true) TFC_CNORM_CASE(8, false, true)
  TFC_CNORM_CASE(1, true, false) TFC_CNORM_CASE(2, true, false) TFC_CNORM_CASE(4, true, false)
  TFC_CNORM_CASE(1, true, true) TFC_CNORM_CASE(2, true, true) TFC_CNORM_CASE(4, true, true)
#undef TFC_CNORM_CASE
}

int cnorm_validate(const char* name, int dtype, int64_t pixels, int64_t channels, float epsilon, bool biased) {
  if (int rc = check_dtype(name, dtype)) return rc;
  if (pixels < 0) return fail("%s: pixels must be non-negative, got %lld", name, static_cast<long long>(pixels));
  if (biased && (channels < 1 || channels > (1 << 24)))
    return fail("%s: channels must be in [1, 2^24], got %lld", name, static_cast<long long>(channels));
  if (!biased && (channels < 2 || channels > (1 << 24)))
    return fail("%s: channels must be at least 2 (the variance divides by channels - 1), got %lld", name,
                static_cast<long long>(channels));
  if (!std::isfinite(epsilon) || epsilon < 0.f) return fail("%s: epsilon must be finite and non-negative", name);
  return 0;
}

// Both norms: `biased` (layer norm) divides the sum of squares by C, ChannelNorm by C - 1; nothing else differs.
int cnorm_forward(const char* name, const void* x, const float* gamma, const float* beta, const void* residual, void* y,
                  int dtype, int64_t pixels, int64_t channels, float epsilon, int relu, bool biased, void* stream) {
  if (int rc = cnorm_validate(name, dtype, pixels, channels, epsilon, biased)) return rc;
  if (pixels == 0) return 0;
  if (!x || !y) return fail("%s: x and y must not be null", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int cus = device_cus();
  CnormParams p = {};
  p.x = x; p.res = residual; p.y = y; p.gamma = gamma; p.beta = beta;
  p.C = static_cast<int>(channels);
  p.eps = epsilon; p.cf = static_cast<float>(channels); p.cm1f = static_cast<float>(channels - (biased ? 0 : 1));
  p.relu = relu ? 1 : 0;
  // x + y beyond the cache: y goes out non-temporal — the rule and the figure of the GDN kernels (TFC_GDN_NT),
  // inherited, not measured here.  TFC_CNORM_NT = 0 / 1: never / always.
  static const int nt_env = env_switch("TFC_CNORM_NT");
  const long long bytes = pixels * channels * dtype_bytes(dtype);
  p.nt = beyond_cache(2 * bytes, nt_env);
  const CnormPlan plan = cnorm_plan(dtype, pixels, channels, {x, y, residual, gamma, beta});
  KernelTimer timer("channel_norm_forward", st);
  long long done = 0;
  if (plan.vec && plan.units > 0) {
    p.V = plan.V; p.lpr_log2 = plan.lpr_log2; p.units = plan.units;
    const long long steps = ceil_div(plan.units, 64 >> plan.lpr_log2);
    // a wave reads gamma and beta for its lanes once (4 bytes per byte of a bfloat16 row): four steps per wave at least,
    // so that this stays a fraction of the x traffic, and 32 waves per CU at most
    const unsigned blocks = static_cast<unsigned>(std::max<long long>(1, std::min<long long>(ceil_div(steps, 16), 8ll * cus)));
    cnorm_launch_vec<false>(plan, dtype, blocks, st, p);
    done = plan.units * (plan.pair ? 2 : 1);
  }
  if (done < pixels) {
    p.row0 = done; p.pixels = pixels - done;
    const unsigned blocks = static_cast<unsigned>(std::min<long long>(ceil_div(p.pixels, 4), 8ll * cus));
    if (dtype == 1) hipLaunchKernelGGL((cnorm_row_kernel<true, false>), dim3(blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((cnorm_row_kernel<false, false>), dim3(blocks), dim3(256), 0, st, p);
  }
  TFC_HIP(hipGetLastError());
  return 0;
}

int cnorm_backward(const char* name, const void* x, const void* g, const float* gamma, const float* beta, void* dx,
                   float* dgamma, float* dbeta, int dtype, int64_t pixels, int64_t channels, float epsilon, int relu,
                   bool biased, void* stream) {
  if (int rc = cnorm_validate(name, dtype, pixels, channels, epsilon, biased)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (pixels == 0) {
    if (dgamma) TFC_HIP(hipMemsetAsync(dgamma, 0, sizeof(float) * channels, st));
    if (dbeta) TFC_HIP(hipMemsetAsync(dbeta, 0, sizeof(float) * channels, st));
    return 0;
  }
  if (!x || !g || !dx) return fail("%s: x, g and dx must not be null", name);
  const int cus = device_cus();
  CnormParams p = {};
  p.x = x; p.g = g; p.y = dx; p.gamma = gamma; p.beta = beta;
  p.C = static_cast<int>(channels);
  p.eps = epsilon; p.cf = static_cast<float>(channels); p.cm1f = static_cast<float>(channels - (biased ? 0 : 1));
  p.relu = relu ? 1 : 0;
  const CnormPlan plan = cnorm_plan(dtype, pixels, channels, {x, g, dx, gamma, beta});
  unsigned vblocks = 0, rblocks = 0;
  long long done = 0;
  if (plan.vec && plan.units > 0) {
    const long long steps = ceil_div(plan.units, 64 >> plan.lpr_log2);
    vblocks = static_cast<unsigned>(std::min<long long>(ceil_div(steps, 4), 2ll * cus));
    done = plan.units * (plan.pair ? 2 : 1);
  }
  if (done < pixels) rblocks = static_cast<unsigned>(std::min<long long>(ceil_div(pixels - done, 4), 2ll * cus));
  const long long vparts = 4ll * vblocks * (plan.pair ? 2 : 1), rparts = 4ll * rblocks;
  DevBuf part;
  TFC_HIP(part.alloc(sizeof(float) * 2 * channels * (vparts + rparts), st));
  p.part = part.as<float>();
  KernelTimer timer("channel_norm_backward", st);
  if (vblocks) {
    p.V = plan.V; p.lpr_log2 = plan.lpr_log2; p.units = plan.units;
    cnorm_launch_vec<true>(plan, dtype, vblocks, st, p);
  }
  if (rblocks) {
    p.row0 = done; p.pixels = pixels - done; p.part0 = vparts;
    TFC_HIP(hipMemsetAsync(p.part + 2 * channels * vparts, 0, sizeof(float) * 2 * channels * rparts, st));
    if (dtype == 1) hipLaunchKernelGGL((cnorm_row_kernel<true, true>), dim3(rblocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((cnorm_row_kernel<false, true>), dim3(rblocks), dim3(256), 0, st, p);
  }
  if (dgamma || dbeta)
    hipLaunchKernelGGL(cnorm_param_sum_kernel, dim3(static_cast<unsigned>(ceil_div(channels, 64)), 2), dim3(64, 16), 0,
                       st, p.part, vparts + rparts, p.C, dgamma, dbeta);
  TFC_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_channel_norm_forward(const void* x, const float* gamma, const float* beta, const void* residual,
                                        void* y, int dtype, int64_t pixels, int64_t channels, float epsilon, int relu,
                                        void* stream) {
  return tfc::cnorm_forward("tfc_channel_norm_forward", x, gamma, beta, residual, y, dtype, pixels, channels, epsilon,
                            relu, false, stream);
}

extern "C" int tfc_channel_norm_backward(const void* x, const void* g, const float* gamma, const float* beta, void* dx,
                                         float* dgamma, float* dbeta, int dtype, int64_t pixels, int64_t channels,
                                         float epsilon, int relu, void* stream) {
  return tfc::cnorm_backward("tfc_channel_norm_backward", x, g, gamma, beta, dx, dgamma, dbeta, dtype, pixels, channels,
                             epsilon, relu, false, stream);
}

extern "C" int tfc_layer_norm_forward(const void* x, const float* gamma, const float* beta, const void* residual,
                                      void* y, int dtype, int64_t pixels, int64_t channels, float epsilon,
                                      void* stream) {
  return tfc::cnorm_forward("tfc_layer_norm_forward", x, gamma, beta, residual, y, dtype, pixels, channels, epsilon, 0,
                            true, stream);
}

extern "C" int tfc_layer_norm_backward(const void* x, const void* g, const float* gamma, const float* beta, void* dx,
                                       float* dgamma, float* dbeta, int dtype, int64_t pixels, int64_t channels,
                                       float epsilon, void* stream) {
  return tfc::cnorm_backward("tfc_layer_norm_backward", x, g, gamma, beta, dx, dgamma, dbeta, dtype, pixels, channels,
                             epsilon, 0, true, stream);
}
