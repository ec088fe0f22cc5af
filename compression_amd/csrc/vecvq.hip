// Entropy-constrained vector quantisation (models/toy_sources/vecvq.py:53-71, compression_model.py:88-95):
// for every row of x the codeword that minimises rates[k] + lmbda * dist(x, c_k), its rate and its distortion, in
// one pass that never writes the [N, K] cost matrix; and the gradients for codebook, rates and x as a gather with
// a fixed order of summation (no float atomics).
//
// The distance is always the difference form sum_d (x - c)^2: the expansion |c|^2 - 2 x.c cancels where x ~ c_k,
// which is where a trained codebook sits.  Ties go to the lowest k: every lane walks k upwards and replaces its
// best only on a strictly smaller cost, and the split merge walks the splits upwards under the same rule.  A NaN
// cost never wins, so `index` stays in [0, K) whatever the inputs.
#include "common.h"
#include "vecvq_params.h"

#include <cmath>

namespace tfc {
namespace {

struct VqParams {
  const float* x;
  const float* c;
  const float* rates;
  int* index;
  float* rate;
  float* dist;
  int* counts;
  float* pcost;            // [splits, N] each, only with splits > 1
  float* pdist;
  int* pidx;
  long long N;
  int K, D;
  int splits, k_per_split;
  int vec;                 // rows of x are 16-byte aligned and D % 4 == 0
  float lmbda, scale;
};

__device__ __forceinline__ void vq_finish(const VqParams& p, long long n, int idx, float dist) {
  p.index[n] = idx;
  p.rate[n] = p.rates[idx];
  p.dist[n] = dist;
  if (p.counts) atomicAdd(p.counts + idx, 1);
}

__device__ __forceinline__ void vq_emit(const VqParams& p, long long n, float cost, int idx, float dist) {
  if (n >= p.N) return;
  if (p.splits == 1) {
    vq_finish(p, n, idx, dist);
  } else {
    const long long at = static_cast<long long>(blockIdx.y) * p.N + n;
    p.pcost[at] = cost;
    p.pdist[at] = dist;
    p.pidx[at] = idx;
  }
}

// Narrow route: D <= DP <= VQ_NARROW_MAX_D.  A lane keeps its row (zero-padded to DP) in registers; a chunk of
// codewords, padded alike, is staged in LDS and every lane reads the same address (a broadcast, no bank conflicts).
template <int DP>
__global__ void __launch_bounds__(VQ_ROWS) vecvq_assign_narrow_kernel(VqParams p) {
  __shared__ __align__(16) float sc[VQ_NARROW_CHUNK * DP];
  __shared__ float sr[VQ_NARROW_CHUNK];
  const int tid = threadIdx.x;
  const long long n = static_cast<long long>(blockIdx.x) * VQ_ROWS + tid;
  const long long nl = n < p.N ? n : p.N - 1;
  float xr[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) xr[d] = d < p.D ? p.x[nl * p.D + d] : 0.f;
  const int kbeg = blockIdx.y * p.k_per_split;
  const int kend = min(p.K, kbeg + p.k_per_split);
  float best = INFINITY, bdist = 0.f;
  int bidx = kbeg;
  for (int k0 = kbeg; k0 < kend; k0 += VQ_NARROW_CHUNK) {
    const int kc = min(VQ_NARROW_CHUNK, kend - k0);
    __syncthreads();
    for (int i = tid; i < kc * DP; i += VQ_ROWS) {
      const int kk = i / DP, d = i % DP;
      sc[i] = d < p.D ? p.c[static_cast<long long>(k0 + kk) * p.D + d] : 0.f;
    }
    for (int i = tid; i < kc; i += VQ_ROWS) sr[i] = p.rates[k0 + i];
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < kc; ++kk) {
      const float* cr = sc + kk * DP;
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        const float t = xr[d] - cr[d];
        s = fmaf(t, t, s);
      }
      const float dist = s * p.scale;
      const float cost = fmaf(p.lmbda, dist, sr[kk]);
      if (cost < best) {
        best = cost;
        bdist = dist;
        bidx = k0 + kk;
      }
    }
  }
  vq_emit(p, n, best, bidx, bdist);
}

// Wide route: D > VQ_NARROW_MAX_D.  A lane holds partial sums for a block of VQ_WIDE_KB codewords and walks D in
// tiles of VQ_WIDE_DT: its own x tile in registers, the codebook tile in LDS (broadcast reads again).
__global__ void __launch_bounds__(VQ_ROWS) vecvq_assign_wide_kernel(VqParams p) {
  __shared__ __align__(16) float sc[VQ_WIDE_KB * VQ_WIDE_DT];
  const int tid = threadIdx.x;
  const long long n = static_cast<long long>(blockIdx.x) * VQ_ROWS + tid;
  const long long nl = n < p.N ? n : p.N - 1;
  const float* xrow = p.x + nl * p.D;
  const int kbeg = blockIdx.y * p.k_per_split;
  const int kend = min(p.K, kbeg + p.k_per_split);
  float best = INFINITY, bdist = 0.f;
  int bidx = kbeg;
  for (int k0 = kbeg; k0 < kend; k0 += VQ_WIDE_KB) {
    const int kc = min(VQ_WIDE_KB, kend - k0);
    float acc[VQ_WIDE_KB];
#pragma unroll
    for (int kk = 0; kk < VQ_WIDE_KB; ++kk) acc[kk] = 0.f;
    for (int d0 = 0; d0 < p.D; d0 += VQ_WIDE_DT) {
      __syncthreads();
      for (int i = tid; i < VQ_WIDE_KB * VQ_WIDE_DT; i += VQ_ROWS) {
        const int kk = i / VQ_WIDE_DT, d = d0 + i % VQ_WIDE_DT;
        sc[i] = (kk < kc && d < p.D) ? p.c[static_cast<long long>(k0 + kk) * p.D + d] : 0.f;
      }
      __syncthreads();
      float xr[VQ_WIDE_DT];
      if (p.vec && d0 + VQ_WIDE_DT <= p.D) {
        const float4* xv = reinterpret_cast<const float4*>(xrow + d0);
#pragma unroll
        for (int j = 0; j < VQ_WIDE_DT / 4; ++j) {
          const float4 v = xv[j];
          xr[4 * j] = v.x; xr[4 * j + 1] = v.y; xr[4 * j + 2] = v.z; xr[4 * j + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < VQ_WIDE_DT; ++j) xr[j] = d0 + j < p.D ? xrow[d0 + j] : 0.f;
      }
#pragma unroll
      for (int kk = 0; kk < VQ_WIDE_KB; ++kk) {
        float s = acc[kk];
#pragma unroll
        for (int j = 0; j < VQ_WIDE_DT; ++j) {
          const float t = xr[j] - sc[kk * VQ_WIDE_DT + j];
          s = fmaf(t, t, s);
        }
        acc[kk] = s;
      }
    }
#pragma unroll
    for (int kk = 0; kk < VQ_WIDE_KB; ++kk) {
      const float dist = acc[kk] * p.scale;
      const float cost = fmaf(p.lmbda, dist, p.rates[k0 + min(kk, kc - 1)]);
      if (kk < kc && cost < best) {
        best = cost;
        bdist = dist;
        bidx = k0 + kk;
      }
    }
  }
  vq_emit(p, n, best, bidx, bdist);
}

// The splits of a row in ascending k, the same strict comparison: the lowest k of the smallest cost.
__global__ void __launch_bounds__(256) vecvq_assign_merge_kernel(VqParams p) {
  const long long n = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (n >= p.N) return;
  float best = p.pcost[n], bdist = p.pdist[n];
  int bidx = p.pidx[n];
  for (int z = 1; z < p.splits; ++z) {
    const long long at = static_cast<long long>(z) * p.N + n;
    const float cost = p.pcost[at];
    if (cost < best) {
      best = cost;
      bdist = p.pdist[at];
      bidx = p.pidx[at];
    }
  }
  vq_finish(p, n, bidx, bdist);
}

struct VqCall {
  VqParams p;
  hipStream_t st;
  DevBuf* work;
};

// Splits the codebook over grid.y (whole chunks each) when the row tiles alone would leave most of the chip idle,
// as a training batch does.  A pure function of (N, K, chunk): the result does not depend on it anyway.
int vq_plan_splits(VqCall& k, int chunk) {
  VqParams& p = k.p;
  const long long row_tiles = ceil_div(p.N, VQ_ROWS);
  const long long chunks = ceil_div(p.K, chunk);
  long long splits = 1;
  if (row_tiles < VQ_TARGET_BLOCKS)
    splits = std::min<long long>({chunks, ceil_div(VQ_TARGET_BLOCKS, row_tiles), VQ_MAX_SPLITS});
  const long long per = ceil_div(chunks, splits);
  p.splits = static_cast<int>(ceil_div(chunks, per));
  p.k_per_split = static_cast<int>(std::min<long long>(per * chunk, p.K));
  if (p.splits > 1) {
    const size_t slab = sizeof(float) * static_cast<size_t>(p.splits) * static_cast<size_t>(p.N);
    TFC_HIP(k.work->alloc(3 * slab, k.st));
    p.pcost = k.work->as<float>();
    p.pdist = p.pcost + static_cast<size_t>(p.splits) * p.N;
    p.pidx = reinterpret_cast<int*>(p.pdist + static_cast<size_t>(p.splits) * p.N);
  }
  return 0;
}

dim3 vq_grid(const VqParams& p) {
  return dim3(static_cast<unsigned>(ceil_div(p.N, VQ_ROWS)), static_cast<unsigned>(p.splits));
}

// A route returns -1 for a shape it does not take, else its status.
int route_narrow(VqCall& k) {
  if (k.p.D > VQ_NARROW_MAX_D) return -1;
  if (int rc = vq_plan_splits(k, VQ_NARROW_CHUNK)) return rc;
  const VqParams& p = k.p;
#define TFC_VQ_NARROW(DP)                                                                                         \
  if (p.D <= DP) {                                                                                                \
    hipLaunchKernelGGL((vecvq_assign_narrow_kernel<DP>), vq_grid(p), dim3(VQ_ROWS), 0, k.st, p);                  \
    return 0;                                                                                                     \
  }
  TFC_VQ_NARROW(1) TFC_VQ_NARROW(2) TFC_VQ_NARROW(4) TFC_VQ_NARROW(8) TFC_VQ_NARROW(12) TFC_VQ_NARROW(16)
  TFC_VQ_NARROW(24) TFC_VQ_NARROW(32)
#undef TFC_VQ_NARROW
  static_assert(VQ_NARROW_MAX_D == 32, "the narrow route's widths end at VQ_NARROW_MAX_D");
  return fail("tfc_vecvq_assign: no narrow kernel for D = %d", p.D);
}

int route_wide(VqCall& k) {
  if (int rc = vq_plan_splits(k, VQ_WIDE_KB)) return rc;
  hipLaunchKernelGGL(vecvq_assign_wide_kernel, vq_grid(k.p), dim3(VQ_ROWS), 0, k.st, k.p);
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Backward

struct VqBwdParams {
  const float* x;
  const float* c;
  const int* index;
  const float* g_rate;     // null: d_rates is not accumulated here
  const float* g_dist;     // null: d_codebook is not accumulated here
  float* d_rates;          // with splits > 1: the partials [splits, K]
  float* d_codebook;       // with splits > 1: the partials [splits, K, D]
  float* d_x;
  long long N;
  int K, D;
  int splits;
  long long rows_per_split;
  float two_s;
};

// d_x[n, :] = 2 s g_dist[n] (x_n - c_index[n]).
__global__ void __launch_bounds__(256) vecvq_bwd_x_kernel(VqBwdParams p) {
  const long long total = p.N * p.D;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < total;
       i += static_cast<long long>(gridDim.x) * 256) {
    const long long n = i / p.D;
    const int d = static_cast<int>(i - n * p.D);
    const int k = p.index[n];
    float v = 0.f;
    if (static_cast<unsigned>(k) < static_cast<unsigned>(p.K))
      v = p.two_s * p.g_dist[n] * (p.x[i] - p.c[static_cast<long long>(k) * p.D + d]);
    p.d_x[i] = v;
  }
}

// A workgroup owns VQ_BWD_KT codewords and VQ_BWD_DT columns, and the rows [z rows_per_split, (z + 1) rows_per_split)
// of its n-split z.  Each wave scans one contiguous quarter of those rows 64 at a time, takes the rows whose index
// falls in the tile by ballot in ascending n, and adds g (c_k - x_n) into its own accumulators in LDS, lanes across D.
// The waves' sums are then added in wave order.  The order of every sum is thus fixed by n and this geometry.
__global__ void __launch_bounds__(VQ_BWD_WAVES * VQ_WAVE) vecvq_bwd_gather_kernel(VqBwdParams p) {
  constexpr int CPL = VQ_BWD_DT / VQ_WAVE;             // columns per lane
  __shared__ float sacc[VQ_BWD_WAVES][VQ_BWD_KT][VQ_BWD_DT];
  __shared__ float srate[VQ_BWD_WAVES][VQ_BWD_KT];
  __shared__ float sc[VQ_BWD_KT][VQ_BWD_DT];
  const int tid = threadIdx.x, lane = tid % VQ_WAVE, w = tid / VQ_WAVE;
  const int k0 = blockIdx.x * VQ_BWD_KT, d0 = blockIdx.y * VQ_BWD_DT;
  const int kt = min(VQ_BWD_KT, p.K - k0);
  const bool do_cb = p.g_dist != nullptr;
  const bool do_r = p.g_rate != nullptr && blockIdx.y == 0;
  for (int i = tid; i < VQ_BWD_WAVES * VQ_BWD_KT * VQ_BWD_DT; i += VQ_BWD_WAVES * VQ_WAVE) (&sacc[0][0][0])[i] = 0.f;
  if (tid < VQ_BWD_WAVES * VQ_BWD_KT) (&srate[0][0])[tid] = 0.f;
  for (int i = tid; i < VQ_BWD_KT * VQ_BWD_DT; i += VQ_BWD_WAVES * VQ_WAVE) {
    const int kk = i / VQ_BWD_DT, d = d0 + i % VQ_BWD_DT;
    (&sc[0][0])[i] = (do_cb && kk < kt && d < p.D) ? p.c[static_cast<long long>(k0 + kk) * p.D + d] : 0.f;
  }
  __syncthreads();

  const long long zbeg = static_cast<long long>(blockIdx.z) * p.rows_per_split;
  const long long zend = min(p.N, zbeg + p.rows_per_split);
  const long long per_wave = p.rows_per_split / VQ_BWD_WAVES;     // a multiple of VQ_WAVE
  const long long wbeg = zbeg + w * per_wave;
  const long long wend = min(zend, wbeg + per_wave);
  for (long long base = wbeg; base < wend; base += VQ_WAVE) {
    const long long n = base + lane;
    int kk = -1;
    if (n < wend) {
      const unsigned r = static_cast<unsigned>(p.index[n] - k0);
      if (r < static_cast<unsigned>(kt)) kk = static_cast<int>(r);
    }
    unsigned long long mask = __ballot(kk >= 0);
    while (mask) {
      // up to VQ_BWD_BATCH matching rows: every load first, then the sums in ascending n
      int src[VQ_BWD_BATCH], kv[VQ_BWD_BATCH];
      float gd[VQ_BWD_BATCH], gr[VQ_BWD_BATCH], xv[VQ_BWD_BATCH][CPL];
#pragma unroll
      for (int u = 0; u < VQ_BWD_BATCH; ++u) {
        src[u] = -1;
        if (mask) {
          src[u] = __ffsll(static_cast<long long>(mask)) - 1;
          mask &= mask - 1;
        }
      }
#pragma unroll
      for (int u = 0; u < VQ_BWD_BATCH; ++u) {
        kv[u] = 0; gd[u] = 0.f; gr[u] = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) xv[u][j] = 0.f;
        if (src[u] >= 0) {
          const long long nn = base + src[u];
          kv[u] = __shfl(kk, src[u]);
          if (do_r) gr[u] = p.g_rate[nn];
          if (do_cb) {
            gd[u] = p.g_dist[nn];
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
              const int d = d0 + lane + VQ_WAVE * j;
              if (d < p.D) xv[u][j] = p.x[nn * p.D + d];
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < VQ_BWD_BATCH; ++u) {
        if (src[u] < 0) continue;
        if (do_cb) {
#pragma unroll
          for (int j = 0; j < CPL; ++j) {
            const int dl = lane + VQ_WAVE * j;
            sacc[w][kv[u]][dl] += gd[u] * (sc[kv[u]][dl] - xv[u][j]);
          }
        }
        if (do_r && lane == 0) srate[w][kv[u]] += gr[u];
      }
    }
  }
  __syncthreads();

  const bool direct = p.splits == 1;
  if (do_cb) {
    for (int i = tid; i < VQ_BWD_KT * VQ_BWD_DT; i += VQ_BWD_WAVES * VQ_WAVE) {
      const int kk = i / VQ_BWD_DT, dl = i % VQ_BWD_DT, d = d0 + dl;
      if (kk >= kt || d >= p.D) continue;
      float s = sacc[0][kk][dl];
#pragma unroll
      for (int v = 1; v < VQ_BWD_WAVES; ++v) s += sacc[v][kk][dl];
      const long long at = (static_cast<long long>(blockIdx.z) * p.K + k0 + kk) * p.D + d;
      p.d_codebook[at] = direct ? p.two_s * s : s;
    }
  }
  if (do_r && tid < kt) {
    float s = srate[0][tid];
#pragma unroll
    for (int v = 1; v < VQ_BWD_WAVES; ++v) s += srate[v][tid];
    p.d_rates[static_cast<long long>(blockIdx.z) * p.K + k0 + tid] = s;
  }
}

// out[i] = factor * (part[0][i] + part[1][i] + ...), the n-splits in ascending order.
__global__ void __launch_bounds__(256) vecvq_bwd_merge_kernel(const float* part, float* out, long long count, int splits,
                                                              float factor) {
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < count;
       i += static_cast<long long>(gridDim.x) * 256) {
    float s = part[i];
    for (int z = 1; z < splits; ++z) s += part[static_cast<long long>(z) * count + i];
    out[i] = factor * s;
  }
}

int vq_validate(const char* name, int64_t n, int64_t k, int64_t d, int distortion) {
  if (d < 1 || d > (1 << 20)) return fail("%s: D must be in [1, 2^20], got %lld", name, static_cast<long long>(d));
  if (k < 1 || k > (1 << 24)) return fail("%s: K must be in [1, 2^24], got %lld", name, static_cast<long long>(k));
  if (n < 0 || n > (1ll << 36)) return fail("%s: N must be in [0, 2^36], got %lld", name, static_cast<long long>(n));
  if (distortion != 0 && distortion != 1) return fail("%s: distortion must be 0 (sse) or 1 (mse), got %d", name, distortion);
  return 0;
}

unsigned vq_flat_blocks(long long count) {
  return static_cast<unsigned>(std::min<long long>(ceil_div(count, 256), 1 << 20));
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_vecvq_assign(const float* x, const float* codebook, const float* rates, int64_t n, int64_t k,
                                int64_t d, float lmbda, int distortion, int* index, float* rate, float* dist,
                                int* counts, void* stream) {
  using namespace tfc;
  if (int rc = vq_validate("tfc_vecvq_assign", n, k, d, distortion)) return rc;
  if (!std::isfinite(lmbda)) return fail("tfc_vecvq_assign: lmbda must be finite");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (counts) TFC_HIP(hipMemsetAsync(counts, 0, sizeof(int) * static_cast<size_t>(k), st));
  if (n == 0) return 0;
  if (!x || !codebook || !rates || !index || !rate || !dist)
    return fail("tfc_vecvq_assign: x, codebook, rates, index, rate and distortion must not be null");
  DevBuf work;
  VqCall call = {};
  call.st = st;
  call.work = &work;
  VqParams& p = call.p;
  p.x = x; p.c = codebook; p.rates = rates;
  p.index = index; p.rate = rate; p.dist = dist; p.counts = counts;
  p.N = n; p.K = static_cast<int>(k); p.D = static_cast<int>(d);
  p.vec = d % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
  p.lmbda = lmbda;
  p.scale = distortion == 1 ? 1.f / static_cast<float>(d) : 1.f;
  KernelTimer timer("vecvq_assign", st);
  // the first route that takes the shape runs it; route_wide takes every D the narrow one leaves
  static int (*const routes[])(VqCall&) = {route_narrow, route_wide};
  int rc = -1;
  for (auto route : routes)
    if ((rc = route(call)) >= 0) break;
  if (rc) return rc;
  if (p.splits > 1)
    hipLaunchKernelGGL(vecvq_assign_merge_kernel, dim3(static_cast<unsigned>(ceil_div(n, 256))), dim3(256), 0, st, p);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_vecvq_backward(const float* x, const float* codebook, const int* index, const float* g_rate,
                                  const float* g_dist, int64_t n, int64_t k, int64_t d, int distortion,
                                  float* d_rates, float* d_codebook, float* d_x, void* stream) {
  using namespace tfc;
  if (int rc = vq_validate("tfc_vecvq_backward", n, k, d, distortion)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool need_cb = d_codebook && g_dist && n > 0, need_r = d_rates && g_rate && n > 0;
  const bool need_x = d_x && g_dist && n > 0;
  if ((need_cb || need_r || need_x) && !index) return fail("tfc_vecvq_backward: index must not be null");
  if ((need_cb || need_x) && (!x || !codebook)) return fail("tfc_vecvq_backward: x and codebook must not be null");
  // what no row contributes to is exactly zero
  if (d_rates && !need_r) TFC_HIP(hipMemsetAsync(d_rates, 0, sizeof(float) * static_cast<size_t>(k), st));
  if (d_codebook && !need_cb) TFC_HIP(hipMemsetAsync(d_codebook, 0, sizeof(float) * static_cast<size_t>(k * d), st));
  if (d_x && !need_x && n > 0) TFC_HIP(hipMemsetAsync(d_x, 0, sizeof(float) * static_cast<size_t>(n * d), st));
  if (!need_cb && !need_r && !need_x) return 0;

  VqBwdParams p = {};
  p.x = x; p.c = codebook; p.index = index;
  p.N = n; p.K = static_cast<int>(k); p.D = static_cast<int>(d);
  p.two_s = distortion == 1 ? 2.f / static_cast<float>(d) : 2.f;
  KernelTimer timer("vecvq_backward", st);
  if (need_x) {
    VqBwdParams q = p;
    q.g_dist = g_dist; q.d_x = d_x;
    hipLaunchKernelGGL(vecvq_bwd_x_kernel, dim3(vq_flat_blocks(n * d)), dim3(256), 0, st, q);
  }
  if (need_cb || need_r) {
    const long long ktiles = ceil_div(k, VQ_BWD_KT), dtiles = need_cb ? ceil_div(d, VQ_BWD_DT) : 1;
    // n-splits: a pure function of (N, K, D), so that the order of the sums is too
    long long splits = std::min<long long>({ceil_div(VQ_BWD_TARGET_BLOCKS, ktiles * dtiles),
                                            ceil_div(n, VQ_BWD_SPLIT_ROWS), VQ_BWD_MAX_SPLITS});
    splits = std::max<long long>(splits, 1);
    constexpr long long kGrain = VQ_BWD_WAVES * VQ_WAVE;
    p.rows_per_split = ceil_div(ceil_div(n, splits), kGrain) * kGrain;
    p.splits = static_cast<int>(ceil_div(n, p.rows_per_split));
    p.g_rate = need_r ? g_rate : nullptr;
    p.g_dist = need_cb ? g_dist : nullptr;
    DevBuf part;
    const size_t cb_count = static_cast<size_t>(k * d), r_count = static_cast<size_t>(k);
    if (p.splits == 1) {
      p.d_rates = d_rates; p.d_codebook = d_codebook;
    } else {
      TFC_HIP(part.alloc(sizeof(float) * p.splits * ((need_cb ? cb_count : 0) + (need_r ? r_count : 0)), st));
      p.d_codebook = part.as<float>();
      p.d_rates = part.as<float>() + (need_cb ? p.splits * cb_count : 0);
    }
    hipLaunchKernelGGL(vecvq_bwd_gather_kernel,
                       dim3(static_cast<unsigned>(ktiles), static_cast<unsigned>(dtiles), static_cast<unsigned>(p.splits)),
                       dim3(VQ_BWD_WAVES * VQ_WAVE), 0, st, p);
    if (p.splits > 1) {
      if (need_cb)
        hipLaunchKernelGGL(vecvq_bwd_merge_kernel, dim3(vq_flat_blocks(k * d)), dim3(256), 0, st, p.d_codebook,
                           d_codebook, static_cast<long long>(k * d), p.splits, p.two_s);
      if (need_r)
        hipLaunchKernelGGL(vecvq_bwd_merge_kernel, dim3(vq_flat_blocks(k)), dim3(256), 0, st, p.d_rates, d_rates,
                           static_cast<long long>(k), p.splits, 1.f);
    }
  }
  TFC_HIP(hipGetLastError());
  return 0;
}
