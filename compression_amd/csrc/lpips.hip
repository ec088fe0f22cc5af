// LPIPS (Zhang et al. 2018, the AlexNet variant HiFiC trains with: models/hific/model.py:840-872) for gfx950: what the
// network needs beyond this library's convolutions — the distance head and the max-pool, channels last.
//
// Distance head, per tap, features f0, f1 [N, P, C], weights w [C] >= 0:
//   n0 = sqrt(sum_c f0^2), n1 likewise;   a = 1 / (n0 + eps), b = 1 / (n1 + eps)
//   d[image] = 1/P sum_p sum_c w[c] (a f0[p,c] - b f1[p,c])^2
// The difference is taken FIRST.  a^2 sum w f0^2 - 2ab sum w f0 f1 + b^2 sum w f1^2 would need no second look at the
// row, but cancels where f0 ~ f1, which is where a codec trains (2.4e-2 relative error in float32 at f1 = f0 (1 + 1e-3
// noise) against 3e-6 for the difference form).  So a pixel's two rows stay in registers between the norms and the
// weighted sum: one pass over HBM.
//
// Layout (vector path, row bytes a multiple of 16, at most 128 granules of 16 bytes): as csrc/channel_norm.hip.
// LPR = min(64, next power of two >= V) lanes share a pixel, 64 / LPR pixels go through a wave at once, lane l holds
// granules l, l + LPR (NG = 1 or 2 of them); sums cross lanes by DPP / swizzle / permlane (unit_sum.h), no LDS.  A lane's
// channels are the same for every pixel it visits: w is read once.  The next pixel's rows are requested before the
// current ones are reduced.  Any other C, or unaligned tensors: one wave per pixel, lanes stride the channels and the
// passes re-read the rows from the caches.
// Reduction: lane 0 of a pixel's lanes adds the pixel's value to its own running sum; a wave's lanes, then a
// workgroup's four waves, are added in a fixed order into part[image][workgroup]; lpips_final_kernel adds an image's
// partials in a fixed order.  No float atomics: two calls give the same bits.
//
// Backward, with e = 2 g[image] / P * w (u - v), u = a f0, v = b f1:
//   df0 =  e a - f0 (f0 . e) a^2 / n0      (second term 0 where n0 = 0)
//   df1 = -e b + f1 (f1 . e) b^2 / n1
// the explicit derivative of f / (|f| + eps), finite at an all-zero pixel where sqrt's own derivative is not.  The
// norms are recomputed; nothing but d leaves the forward.
//
// Max-pool, x [N, H, W, C], window k, stride s, no padding, out = (in - k) / s + 1 (floor): 16 bytes per thread along
// C where the row allows.  The forward stores y only.  The backward is a gather: an input element visits the at most
// ceil(k / s)^2 windows that hold it, finds each window's winner from x again — the FIRST maximum in row-major order —
// and adds the window's gradient where it is the winner, windows in row-major order.  No atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <initializer_list>

#include "../../include/tfc_hip.h"
#include "bf16_io.h"
#include "launch.h"
#include "unit_sum.h"

namespace tfc {
namespace {

constexpr int kLpWaves = 4;            // waves per workgroup of the distance kernels

struct LpipsParams {
  const void* f0;
  const void* f1;
  const float* w;
  const float* g;       // backward: dL/dd [N]
  void* df0;            // backward: or null
  void* df1;            // backward: or null
  float* part;          // forward: [N][B]
  long long P;          // pixels of an image
  int B;                // workgroups per image
  int C;
  int V;                // granules per row
  int lpr_log2;         // lanes per row
  float eps, inv_p;
};

// The wave's running sum -> part[blockIdx.x], every step adding the same operands in the same order.
__device__ inline void lp_block_partial(float acc, float* part) {
  __shared__ float ws[kLpWaves];
  acc = unit_sum(acc, 6);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// NG granules per lane; BWD: df0 / df1 instead of the partial sums.  grid N * B, block 256.
template <int NG, bool BF16, bool BWD>
__global__ void __launch_bounds__(64 * kLpWaves) lpips_vec_kernel(LpipsParams p) {
  constexpr int EPG = BF16 ? 8 : 4;
  constexpr int NE = NG * EPG;
  const int lane = threadIdx.x & 63;
  const int lpr = 1 << p.lpr_log2;
  const int l = lane & (lpr - 1);
  const int grp = lane >> p.lpr_log2;
  const int rw = 64 >> p.lpr_log2;                 // pixels per wave instruction
  const long long img = blockIdx.x / p.B;
  const long long wave = static_cast<long long>(blockIdx.x % p.B) * kLpWaves +
                         __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const long long nwaves = static_cast<long long>(p.B) * kLpWaves;
  const long long steps = (p.P + rw - 1) / rw;

  bool on[NG];
  float wgt[NE];
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int gr = j * lpr + l;
    on[j] = gr < p.V;
#pragma unroll
    for (int q = 0; q < EPG / 4; ++q) {
      f32x4 wv = {0.f, 0.f, 0.f, 0.f};
      if (on[j]) wv = *reinterpret_cast<const f32x4*>(p.w + gr * EPG + q * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) wgt[j * EPG + q * 4 + e] = wv[e];
    }
  }

  const u32x4* const b0 = static_cast<const u32x4*>(p.f0) + img * p.P * p.V;
  const u32x4* const b1 = static_cast<const u32x4*>(p.f1) + img * p.P * p.V;
  auto fetch = [&](const u32x4* base, long long step, u32x4* raw) {
    const long long u = step * rw + grp;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      raw[j] = u32x4{0u, 0u, 0u, 0u};
      if (on[j] && u < p.P) raw[j] = base[u * p.V + j * lpr + l];
    }
  };
  u32x4 n0[NG], n1[NG];
  if (wave < steps) {
    fetch(b0, wave, n0);
    fetch(b1, wave, n1);
  }
  const float ge = BWD ? 2.f * p.g[img] * p.inv_p : 0.f;
  float acc = 0.f;

  for (long long step = wave; step < steps; step += nwaves) {
    const long long u = step * rw + grp;
    const bool live = u < p.P;
    float a[NE], b[NE];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      unpack<BF16>(n0[j], a + j * EPG);
      unpack<BF16>(n1[j], b + j * EPG);
    }
    if (step + nwaves < steps) {
      fetch(b0, step + nwaves, n0);
      fetch(b1, step + nwaves, n1);
    }
    // (masked slots and pixels past the last one hold zeros)
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
      s0 = fmaf(a[k], a[k], s0);
      s1 = fmaf(b[k], b[k], s1);
    }
    const float nrm0 = sqrtf(unit_sum(s0, p.lpr_log2)), nrm1 = sqrtf(unit_sum(s1, p.lpr_log2));
    const float ia = live ? 1.f / (nrm0 + p.eps) : 0.f, ib = live ? 1.f / (nrm1 + p.eps) : 0.f;
    if (!BWD) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < NE; ++k) {
        const float d = a[k] * ia - b[k] * ib;
        t = fmaf(wgt[k] * d, d, t);
      }
      t = unit_sum(t, p.lpr_log2);
      if (live && l == 0) acc += t;
    } else {
      float e[NE];
      float d0 = 0.f, d1 = 0.f;
#pragma unroll
      for (int k = 0; k < NE; ++k) {
        e[k] = ge * wgt[k] * (a[k] * ia - b[k] * ib);
        d0 = fmaf(a[k], e[k], d0);
        d1 = fmaf(b[k], e[k], d1);
      }
      d0 = unit_sum(d0, p.lpr_log2);
      d1 = unit_sum(d1, p.lpr_log2);
      const float c0 = nrm0 > 0.f ? d0 * ia * ia / nrm0 : 0.f;
      const float c1 = nrm1 > 0.f ? d1 * ib * ib / nrm1 : 0.f;
#pragma unroll
      for (int j = 0; j < NG; ++j) {
        float o[EPG];
        if (p.df0) {
#pragma unroll
          for (int q = 0; q < EPG; ++q) o[q] = e[j * EPG + q] * ia - a[j * EPG + q] * c0;
          if (on[j] && live) static_cast<u32x4*>(p.df0)[(img * p.P + u) * p.V + j * lpr + l] = repack<BF16>(o);
        }
        if (p.df1) {
#pragma unroll
          for (int q = 0; q < EPG; ++q) o[q] = b[j * EPG + q] * c1 - e[j * EPG + q] * ib;
          if (on[j] && live) static_cast<u32x4*>(p.df1)[(img * p.P + u) * p.V + j * lpr + l] = repack<BF16>(o);
        }
      }
    }
  }
  if (!BWD) lp_block_partial(acc, p.part);
}

// Any C: one wave per pixel, lane l takes channels l, l + 64, ...; the passes re-read the rows (from the caches).
template <bool BF16, bool BWD>
__global__ void __launch_bounds__(64 * kLpWaves) lpips_row_kernel(LpipsParams p) {
  const int lane = threadIdx.x & 63;
  const long long img = blockIdx.x / p.B;
  const long long wave = static_cast<long long>(blockIdx.x % p.B) * kLpWaves + (threadIdx.x >> 6);
  const long long nwaves = static_cast<long long>(p.B) * kLpWaves;
  const float ge = BWD ? 2.f * p.g[img] * p.inv_p : 0.f;
  float acc = 0.f;
  for (long long r = wave; r < p.P; r += nwaves) {
    const long long at = (img * p.P + r) * p.C;
    float s0 = 0.f, s1 = 0.f;
    for (int c = lane; c < p.C; c += 64) {
      const float a = load<BF16>(p.f0, at + c), b = load<BF16>(p.f1, at + c);
      s0 = fmaf(a, a, s0);
      s1 = fmaf(b, b, s1);
    }
    const float nrm0 = sqrtf(unit_sum(s0, 6)), nrm1 = sqrtf(unit_sum(s1, 6));
    const float ia = 1.f / (nrm0 + p.eps), ib = 1.f / (nrm1 + p.eps);
    if (!BWD) {
      float t = 0.f;
      for (int c = lane; c < p.C; c += 64) {
        const float d = load<BF16>(p.f0, at + c) * ia - load<BF16>(p.f1, at + c) * ib;
        t = fmaf(p.w[c] * d, d, t);
      }
      acc += unit_sum(t, 6);                         // the same in all lanes; lane 0's is kept below
    } else {
      float d0 = 0.f, d1 = 0.f;
      for (int c = lane; c < p.C; c += 64) {
        const float a = load<BF16>(p.f0, at + c), b = load<BF16>(p.f1, at + c);
        const float e = ge * p.w[c] * (a * ia - b * ib);
        d0 = fmaf(a, e, d0);
        d1 = fmaf(b, e, d1);
      }
      d0 = unit_sum(d0, 6);
      d1 = unit_sum(d1, 6);
      const float c0 = nrm0 > 0.f ? d0 * ia * ia / nrm0 : 0.f;
      const float c1 = nrm1 > 0.f ? d1 * ib * ib / nrm1 : 0.f;
      for (int c = lane; c < p.C; c += 64) {
        const float a = load<BF16>(p.f0, at + c), b = load<BF16>(p.f1, at + c);
        const float e = ge * p.w[c] * (a * ia - b * ib);
        if (p.df0) store<BF16>(p.df0, at + c, e * ia - a * c0);
        if (p.df1) store<BF16>(p.df1, at + c, b * c1 - e * ib);
      }
    }
  }
  if (!BWD) lp_block_partial(lane == 0 ? acc : 0.f, p.part);
}

// d[image] = inv_p * sum of the image's B partials: lane l adds partials l, l + 64, ..., then the lanes are added.
// grid N, block 64.
__global__ void __launch_bounds__(64) lpips_final_kernel(const float* part, int B, float inv_p, float* d) {
  const float* const row = part + static_cast<long long>(blockIdx.x) * B;
  float s = 0.f;
  for (int i = threadIdx.x; i < B; i += 64) s += row[i];
  s = unit_sum(s, 6);
  if (threadIdx.x == 0) d[blockIdx.x] = s * inv_p;
}

struct LpipsPlan {
  bool vec = false;
  int V = 0, lpr_log2 = 0, ng = 1;
};

LpipsPlan lpips_plan(int dtype, long long C, std::initializer_list<const void*> tensors) {
  LpipsPlan plan;
  const long long row_bytes = C * dtype_bytes(dtype);
  bool aligned = true;
  for (const void* t : tensors) aligned = aligned && reinterpret_cast<uintptr_t>(t) % 16 == 0;
  if (!aligned || row_bytes % 16 != 0 || row_bytes / 16 > 128) return plan;
  plan.vec = true;
  plan.V = static_cast<int>(row_bytes / 16);
  while ((1 << plan.lpr_log2) < plan.V && plan.lpr_log2 < 6) ++plan.lpr_log2;
  plan.ng = plan.V > 64 ? 2 : 1;
  return plan;
}

// Workgroups per image: two steps per wave where there are enough, about 32 waves per CU over all images at most.
int lpips_blocks(const LpipsPlan& plan, long long N, long long P) {
  const long long steps = plan.vec ? ceil_div(P, 64 >> plan.lpr_log2) : P;
  const long long cap = std::max<long long>(1, 8ll * device_cus() / N);
  return static_cast<int>(std::max<long long>(1, std::min<long long>(ceil_div(steps, 2 * kLpWaves), cap)));
}

template <bool BWD>
void lpips_launch(const LpipsPlan& plan, int dtype, long long N, hipStream_t st, const LpipsParams& p) {
  const dim3 grid(static_cast<unsigned>(N * p.B)), block(64 * kLpWaves);
  if (!plan.vec) {
    if (dtype == 1) hipLaunchKernelGGL((lpips_row_kernel<true, BWD>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((lpips_row_kernel<false, BWD>), grid, block, 0, st, p);
  } else if (plan.ng == 1) {
    if (dtype == 1) hipLaunchKernelGGL((lpips_vec_kernel<1, true, BWD>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((lpips_vec_kernel<1, false, BWD>), grid, block, 0, st, p);
  } else {
    if (dtype == 1) hipLaunchKernelGGL((lpips_vec_kernel<2, true, BWD>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((lpips_vec_kernel<2, false, BWD>), grid, block, 0, st, p);
  }
}

int lpips_validate(const char* name, int dtype, int64_t N, int64_t P, int64_t C, float eps) {
  if (int rc = check_dtype(name, dtype)) return rc;
  if (N < 0 || N >= (1 << 20)) return fail("%s: images must be in [0, 2^20), got %lld", name, static_cast<long long>(N));
  if (P < 1) return fail("%s: pixels must be positive, got %lld", name, static_cast<long long>(P));
  if (C < 1 || C > (1 << 24)) return fail("%s: channels must be in [1, 2^24], got %lld", name, static_cast<long long>(C));
  if (!std::isfinite(eps) || eps < 0.f) return fail("%s: epsilon must be finite and non-negative", name);
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------

struct PoolParams {
  const void* x;
  const void* g;        // backward: dL/dy
  void* y;              // forward: y; backward: dx
  long long total;      // threads that have work
  int H, W, OH, OW;
  int CV;               // granules (vector kernels) or channels of a pixel
  int k, s;
};

// torch's rule: a later element replaces the running maximum if it is greater or a NaN.
__device__ inline bool pool_takes(float v, float m) { return v > m || v != v; }

// One thread per output pixel and granule (VEC) or channel.  Row stride in elements of this kernel: CV.
template <bool BF16, bool VEC>
__global__ void __launch_bounds__(256) maxpool_fwd_kernel(PoolParams p) {
  constexpr int EPG = VEC ? (BF16 ? 8 : 4) : 1;
  for (long long idx = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; idx < p.total;
       idx += static_cast<long long>(gridDim.x) * 256) {
    const int cv = static_cast<int>(idx % p.CV);
    long long q = idx / p.CV;
    const int ow = static_cast<int>(q % p.OW);
    q /= p.OW;
    const int oh = static_cast<int>(q % p.OH);
    const long long n = q / p.OH;
    float m[EPG];
#pragma unroll
    for (int e = 0; e < EPG; ++e) m[e] = 0.f;
    for (int i = 0; i < p.k; ++i)
      for (int j = 0; j < p.k; ++j) {
        const long long at = ((n * p.H + oh * p.s + i) * p.W + ow * p.s + j) * p.CV + cv;
        float v[EPG];
        if (VEC) unpack<BF16>(static_cast<const u32x4*>(p.x)[at], v);
        else v[0] = load<BF16>(p.x, at);
#pragma unroll
        for (int e = 0; e < EPG; ++e) m[e] = (i == 0 && j == 0) || pool_takes(v[e], m[e]) ? v[e] : m[e];
      }
    // (m holds input values: the conversion back is exact)
    if (VEC) static_cast<u32x4*>(p.y)[idx] = repack<BF16>(m);
    else store<BF16>(p.y, idx, m[0]);
  }
}

// One thread per INPUT pixel and granule / channel.
template <bool BF16, bool VEC>
__global__ void __launch_bounds__(256) maxpool_bwd_kernel(PoolParams p) {
  constexpr int EPG = VEC ? (BF16 ? 8 : 4) : 1;
  for (long long idx = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; idx < p.total;
       idx += static_cast<long long>(gridDim.x) * 256) {
    const int cv = static_cast<int>(idx % p.CV);
    long long q = idx / p.CV;
    const int w = static_cast<int>(q % p.W);
    q /= p.W;
    const int h = static_cast<int>(q % p.H);
    const long long n = q / p.H;
    // windows o with o s <= h <= o s + k - 1
    const int oh0 = h < p.k ? 0 : (h - p.k + p.s) / p.s, oh1 = min(p.OH - 1, h / p.s);
    const int ow0 = w < p.k ? 0 : (w - p.k + p.s) / p.s, ow1 = min(p.OW - 1, w / p.s);
    float acc[EPG];
#pragma unroll
    for (int e = 0; e < EPG; ++e) acc[e] = 0.f;
    for (int oh = oh0; oh <= oh1; ++oh)
      for (int ow = ow0; ow <= ow1; ++ow) {
        const int mine = (h - oh * p.s) * p.k + (w - ow * p.s);
        float m[EPG];
        int win[EPG];
#pragma unroll
        for (int e = 0; e < EPG; ++e) { m[e] = 0.f; win[e] = 0; }
        for (int i = 0; i < p.k; ++i)
          for (int j = 0; j < p.k; ++j) {
            const long long at = ((n * p.H + oh * p.s + i) * p.W + ow * p.s + j) * p.CV + cv;
            float v[EPG];
            if (VEC) unpack<BF16>(static_cast<const u32x4*>(p.x)[at], v);
            else v[0] = load<BF16>(p.x, at);
#pragma unroll
            for (int e = 0; e < EPG; ++e) {
              const bool take = (i == 0 && j == 0) || pool_takes(v[e], m[e]);
              m[e] = take ? v[e] : m[e];
              win[e] = take ? i * p.k + j : win[e];
            }
          }
        const long long gat = ((n * p.OH + oh) * p.OW + ow) * p.CV + cv;
        float gv[EPG];
        if (VEC) unpack<BF16>(static_cast<const u32x4*>(p.g)[gat], gv);
        else gv[0] = load<BF16>(p.g, gat);
#pragma unroll
        for (int e = 0; e < EPG; ++e) acc[e] += win[e] == mine ? gv[e] : 0.f;
      }
    if (VEC) static_cast<u32x4*>(p.y)[idx] = repack<BF16>(acc);
    else store<BF16>(p.y, idx, acc[0]);
  }
}

int pool_validate(const char* name, int dtype, int64_t n, int64_t h, int64_t w, int64_t c, int k, int s) {
  if (int rc = check_dtype(name, dtype)) return rc;
  if (n < 0 || c < 1 || c > (1 << 24)) return fail("%s: bad batch or channel count", name);
  if (k < 1 || s < 1 || k > 64) return fail("%s: window must be in [1, 64] and stride positive", name);
  if (h < k || w < k || h >= (1 << 30) || w >= (1 << 30))
    return fail("%s: a %lld x %lld image holds no %d x %d window", name, static_cast<long long>(h),
                static_cast<long long>(w), k, k);
  return 0;
}

template <bool BWD>
int pool_launch(const void* x, const void* g, void* out, int dtype, int64_t n, int64_t h, int64_t w, int64_t c, int k,
                int s, hipStream_t st) {
  PoolParams p = {};
  p.x = x; p.g = g; p.y = out;
  p.H = static_cast<int>(h); p.W = static_cast<int>(w);
  p.OH = static_cast<int>((h - k) / s + 1); p.OW = static_cast<int>((w - k) / s + 1);
  p.k = k; p.s = s;
  const long long row_bytes = c * dtype_bytes(dtype);
  bool vec = row_bytes % 16 == 0;
  for (const void* t : {x, g, static_cast<const void*>(out)}) vec = vec && reinterpret_cast<uintptr_t>(t) % 16 == 0;
  p.CV = static_cast<int>(vec ? row_bytes / 16 : c);
  p.total = n * (BWD ? h * w : static_cast<long long>(p.OH) * p.OW) * p.CV;
  if (p.total == 0) return 0;
  const unsigned blocks = static_cast<unsigned>(std::min<long long>(ceil_div(p.total, 256), 1 << 20));
#define TFC_POOL_CASE(BF, VC)                                                                                   \
  if ((dtype == 1) == BF && vec == VC) {                                                                        \
    if (BWD) hipLaunchKernelGGL((maxpool_bwd_kernel<BF, VC>), dim3(blocks), dim3(256), 0, st, p);               \
    else hipLaunchKernelGGL((maxpool_fwd_kernel<BF, VC>), dim3(blocks), dim3(256), 0, st, p);                   \
  }
  TFC_POOL_CASE(false, false) TFC_POOL_CASE(false, true) TFC_POOL_CASE(true, false) TFC_POOL_CASE(true, true)
#undef TFC_POOL_CASE
  TFC_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_lpips_distance_forward(const void* f0, const void* f1, const float* w, float* d, int dtype,
                                          int64_t images, int64_t pixels, int64_t channels, float epsilon,
                                          void* stream) {
  using namespace tfc;
  if (int rc = lpips_validate("tfc_lpips_distance_forward", dtype, images, pixels, channels, epsilon)) return rc;
  if (images == 0) return 0;
  if (!f0 || !f1 || !w || !d) return fail("tfc_lpips_distance_forward: f0, f1, w and d must not be null");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LpipsPlan plan = lpips_plan(dtype, channels, {f0, f1, w});
  LpipsParams p = {};
  p.f0 = f0; p.f1 = f1; p.w = w;
  p.P = pixels; p.C = static_cast<int>(channels); p.V = plan.V; p.lpr_log2 = plan.lpr_log2;
  p.eps = epsilon; p.inv_p = 1.f / static_cast<float>(pixels);
  p.B = lpips_blocks(plan, images, pixels);
  DevBuf part;
  TFC_HIP(part.alloc(sizeof(float) * images * p.B, st));
  p.part = part.as<float>();
  KernelTimer timer("lpips_distance_forward", st);
  lpips_launch<false>(plan, dtype, images, st, p);
  hipLaunchKernelGGL(lpips_final_kernel, dim3(static_cast<unsigned>(images)), dim3(64), 0, st, p.part, p.B, p.inv_p, d);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_lpips_distance_backward(const float* g, const void* f0, const void* f1, const float* w, void* df0,
                                           void* df1, int dtype, int64_t images, int64_t pixels, int64_t channels,
                                           float epsilon, int mask, void* stream) {
  using namespace tfc;
  if (int rc = lpips_validate("tfc_lpips_distance_backward", dtype, images, pixels, channels, epsilon)) return rc;
  if (mask < 0 || mask > 3) return fail("tfc_lpips_distance_backward: mask must be in [0, 3]");
  if (images == 0 || mask == 0) return 0;
  if (!g || !f0 || !f1 || !w) return fail("tfc_lpips_distance_backward: g, f0, f1 and w must not be null");
  if (((mask & 1) && !df0) || ((mask & 2) && !df1))
    return fail("tfc_lpips_distance_backward: a gradient the mask asks for has no buffer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  LpipsParams p = {};
  p.f0 = f0; p.f1 = f1; p.w = w; p.g = g;
  p.df0 = (mask & 1) ? df0 : nullptr;
  p.df1 = (mask & 2) ? df1 : nullptr;
  const LpipsPlan plan = lpips_plan(dtype, channels, {f0, f1, w, p.df0, p.df1});
  p.P = pixels; p.C = static_cast<int>(channels); p.V = plan.V; p.lpr_log2 = plan.lpr_log2;
  p.eps = epsilon; p.inv_p = 1.f / static_cast<float>(pixels);
  p.B = lpips_blocks(plan, images, pixels);
  KernelTimer timer("lpips_distance_backward", st);
  lpips_launch<true>(plan, dtype, images, st, p);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_maxpool2d_forward(const void* x, void* y, int dtype, int64_t n, int64_t h, int64_t w, int64_t c,
                                     int k, int s, void* stream) {
  using namespace tfc;
  if (int rc = pool_validate("tfc_maxpool2d_forward", dtype, n, h, w, c, k, s)) return rc;
  if (n == 0) return 0;
  if (!x || !y) return fail("tfc_maxpool2d_forward: x and y must not be null");
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer("maxpool2d_forward", st);
  return pool_launch<false>(x, nullptr, y, dtype, n, h, w, c, k, s, st);
}

extern "C" int tfc_maxpool2d_backward(const void* x, const void* g, void* dx, int dtype, int64_t n, int64_t h,
                                      int64_t w, int64_t c, int k, int s, void* stream) {
  using namespace tfc;
  if (int rc = pool_validate("tfc_maxpool2d_backward", dtype, n, h, w, c, k, s)) return rc;
  if (n == 0) return 0;
  if (!x || !g || !dx) return fail("tfc_maxpool2d_backward: x, g and dx must not be null");
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer("maxpool2d_backward", st);
  return pool_launch<true>(x, g, dx, dtype, n, h, w, c, k, s, st);
}
