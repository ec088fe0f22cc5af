// LVAC (learned volumetric attribute compression) on gfx950: the two halves of its training step that had no kernel.
//
// Part one, inverse RAHT.  A level turns parent rows into child rows, child[c] = parent[p(c)] + w(c) ac[k(c)]; the
// children of a node are adjacent, so forward and backward are gathers: no atomics, one writer per element, the same
// bits from call to call.  A level without a two-child node is the identity and launches nothing; consecutive levels
// of at most RAHT_HEAD_ITEMS elements run in ONE single-workgroup launch with a barrier between them.
//
// Part two, the per-point decoder recon = A (W2^T relu(W1^T [pos; Z[idx]] + b1) + b2) + o with its squared error.  A
// workgroup owns PM_TILE points; the hidden layer is produced PM_HC units at a time in registers (8 points x 4 units
// per thread, float32 FMA on the vector unit) and contracted at once, so no [N, H] tensor exists.  The backward
// recomputes it per tile: one kernel for the per-point latent gradient (summed per block by a second, every block's
// points being contiguous), one for the parameter gradients (a fixed number of tile groups, each with its own partial,
// merged in ascending order).
#include "common.h"
#include "lvac_params.h"

#include <cmath>

namespace tfc {
namespace {

// ------------------------------------------------------------------------------------------------------------------
// inverse RAHT
// ------------------------------------------------------------------------------------------------------------------

// descriptor of a level, RAHT_DESC int64: child rows, parent rows, AC rows, then the offsets (in 4-byte words of the
// table buffer) of child_parent, child_ac, child_weight, parent_first, parent_count, ac_left, ac_coeff
struct RahtRun {
  float* ac[RAHT_MAX_LEVELS];      // forward: the level's AC rows (read); backward: their gradient (written)
  int level[RAHT_MAX_LEVELS];      // the levels of this launch in execution order
  int count;
};

__device__ __forceinline__ const float* raht_in(int s, const float* src, const float* tmp0, const float* tmp1) {
  return s == 0 ? src : (((s - 1) & 1) ? tmp1 : tmp0);
}

__device__ __forceinline__ float* raht_out(int s, int count, float* dst, float* tmp0, float* tmp1) {
  return s == count - 1 ? dst : ((s & 1) ? tmp1 : tmp0);
}

// more than one level per launch only with gridDim.x == 1 (the barrier is the workgroup's)
__global__ void __launch_bounds__(RAHT_THREADS) lvac_raht_forward_kernel(RahtRun run, const long long* desc,
                                                                        const int* tab, const float* src, float* dst,
                                                                        float* tmp0, float* tmp1, int C) {
  for (int s = 0; s < run.count; ++s) {
    const long long* d = desc + static_cast<long long>(RAHT_DESC) * run.level[s];
    const long long nc = d[0], np = d[1], na = d[2];
    const int* child_parent = tab + d[3];
    const int* child_ac = tab + d[4];
    const float* child_w = reinterpret_cast<const float*>(tab + d[5]);
    const float* in = raht_in(s, src, tmp0, tmp1);
    float* out = raht_out(s, run.count, dst, tmp0, tmp1);
    const float* ac = run.ac[s];
    const long long items = nc * C;
    for (long long i = static_cast<long long>(blockIdx.x) * RAHT_THREADS + threadIdx.x; i < items;
         i += static_cast<long long>(gridDim.x) * RAHT_THREADS) {
      const long long c = i / C;
      const int ch = static_cast<int>(i - c * C);
      const int p = child_parent[c], k = child_ac[c];
      float v = (p >= 0 && p < np) ? in[static_cast<long long>(p) * C + ch] : 0.f;
      if (k >= 0 && k < na) v = fmaf(child_w[c], ac[static_cast<long long>(k) * C + ch], v);
      out[i] = v;
    }
    if (s + 1 < run.count) __syncthreads();
  }
}

__global__ void __launch_bounds__(RAHT_THREADS) lvac_raht_backward_kernel(RahtRun run, const long long* desc,
                                                                         const int* tab, const float* src, float* dst,
                                                                         float* tmp0, float* tmp1, int C) {
  for (int s = 0; s < run.count; ++s) {
    const long long* d = desc + static_cast<long long>(RAHT_DESC) * run.level[s];
    const long long nc = d[0], np = d[1], na = d[2];
    const int* parent_first = tab + d[6];
    const int* parent_count = tab + d[7];
    const int* ac_left = tab + d[8];
    const float* ac_coeff = reinterpret_cast<const float*>(tab + d[9]);
    const float* g = raht_in(s, src, tmp0, tmp1);
    float* out = raht_out(s, run.count, dst, tmp0, tmp1);
    float* d_ac = run.ac[s];
    const long long items = (np + na) * C;
    for (long long i = static_cast<long long>(blockIdx.x) * RAHT_THREADS + threadIdx.x; i < items;
         i += static_cast<long long>(gridDim.x) * RAHT_THREADS) {
      const long long row = i / C;
      const int ch = static_cast<int>(i - row * C);
      if (row < np) {
        const long long f = parent_first[row];
        const int n = parent_count[row];
        float v = 0.f;
        if (f >= 0 && f < nc) v = g[f * C + ch];
        if (n == 2 && f >= 0 && f + 1 < nc) v += g[(f + 1) * C + ch];
        out[i] = v;
      } else {
        const long long k = row - np;
        const long long l = ac_left[k];
        float v = 0.f;
        if (l >= 0 && l + 1 < nc) v = fmaf(ac_coeff[k], g[l * C + ch], g[(l + 1) * C + ch]);
        d_ac[k * C + ch] = v;
      }
    }
    if (s + 1 < run.count) __syncthreads();
  }
}

struct RahtPlan {
  int levels = 0;
  long long nc[RAHT_MAX_LEVELS], np[RAHT_MAX_LEVELS], na[RAHT_MAX_LEVELS];
  int active[RAHT_MAX_LEVELS];     // levels with AC rows, ascending
  int n_active = 0;
};

int raht_plan(const char* name, const int64_t* desc, int64_t table_words, int levels, int64_t channels, int64_t n_root,
              int64_t n_out, RahtPlan* plan) {
  if (levels < 0 || levels > RAHT_MAX_LEVELS)
    return fail("%s: levels must be in [0, %d], got %d", name, RAHT_MAX_LEVELS, levels);
  if (channels < 1 || channels > (1 << 16))
    return fail("%s: channels must be in [1, 65536], got %lld", name, static_cast<long long>(channels));
  if (n_root < 0 || n_out < 0) return fail("%s: negative row count", name);
  if (levels > 0 && !desc) return fail("%s: the level descriptors must not be null", name);
  plan->levels = levels;
  long long rows = n_root;
  for (int l = 0; l < levels; ++l) {
    const int64_t* d = desc + static_cast<int64_t>(RAHT_DESC) * l;
    const long long nc = d[0], np = d[1], na = d[2];
    if (nc < 0 || np < 0 || na < 0 || nc > 0x7fffffffll || nc != np + na || np != rows)
      return fail("%s: level %d has %lld children, %lld parents and %lld AC rows after %lld rows", name, l, nc, np, na,
                  rows);
    const long long need[7] = {nc, nc, nc, np, np, na, na};
    for (int j = 0; j < 7; ++j)
      if (d[3 + j] < 0 || d[3 + j] + need[j] > table_words)
        return fail("%s: table %d of level %d lies outside the table buffer", name, j, l);
    plan->nc[l] = nc; plan->np[l] = np; plan->na[l] = na;
    if (na > 0) plan->active[plan->n_active++] = l;
    rows = nc;
  }
  if (rows != n_out)
    return fail("%s: the tree ends in %lld rows, the output has %lld", name, rows, static_cast<long long>(n_out));
  return 0;
}

bool raht_is_head(const RahtPlan& plan, int level, int64_t channels) {
  return plan.nc[level] * channels <= RAHT_HEAD_ITEMS;
}

unsigned raht_blocks(long long items) {
  return static_cast<unsigned>(std::max<long long>(1, std::min<long long>(ceil_div(items, RAHT_THREADS), RAHT_MAX_BLOCKS)));
}

// The launches of one direction.  `order` lists the active levels in execution order; the head levels (small ones) are
// a prefix of it in the forward and a suffix in the backward, and share one launch.
template <typename Kernel>
int raht_run(Kernel kernel, const RahtPlan& plan, const int* order, int n, bool head_first, float* const* ac,
             const int64_t* desc_dev, const int32_t* tables, int64_t channels, const float* src, float* dst,
             hipStream_t st) {
  int n_head = 0;
  if (head_first) {
    while (n_head < n && raht_is_head(plan, order[n_head], channels)) ++n_head;
  } else {
    while (n_head < n && raht_is_head(plan, order[n - 1 - n_head], channels)) ++n_head;
  }
  // workspace: two buffers for the one-level launches, two small ones for the steps inside the head launch
  long long big = 0;
  for (int i = 0; i < n; ++i) big = std::max(big, plan.nc[order[i]] * channels);
  DevBuf work;
  TFC_HIP(work.alloc(sizeof(float) * static_cast<size_t>(2 * big + 2 * RAHT_HEAD_ITEMS), st));
  float* bufs[2] = {work.as<float>(), work.as<float>() + big};
  float* tmp0 = work.as<float>() + 2 * big;
  float* tmp1 = tmp0 + RAHT_HEAD_ITEMS;
  const float* cur = src;
  int flip = 0, i = 0;
  while (i < n) {
    const bool in_head = head_first ? i < n_head : i >= n - n_head;
    const int take = in_head && n_head > 0 ? (head_first ? n_head - i : n - i) : 1;
    RahtRun run = {};
    run.count = take;
    long long items = 0;
    for (int j = 0; j < take; ++j) {
      run.level[j] = order[i + j];
      run.ac[j] = ac[order[i + j]];
      if (!run.ac[j]) return fail("tfc_raht: level %d has AC rows and a null pointer", order[i + j]);
      items = head_first ? plan.nc[order[i + j]] * channels
                         : (plan.np[order[i + j]] + plan.na[order[i + j]]) * channels;
    }
    float* out = i + take == n ? dst : bufs[flip];
    flip ^= 1;
    const unsigned blocks = take > 1 ? 1u : raht_blocks(items);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(RAHT_THREADS), 0, st, run,
                       reinterpret_cast<const long long*>(desc_dev), tables, cur, out, tmp0, tmp1,
                       static_cast<int>(channels));
    cur = out;
    i += take;
  }
  TFC_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// the point decoder
// ------------------------------------------------------------------------------------------------------------------

struct PmParams {
  const float* z;          // [n_blocks, C]
  const int* index;        // [N]
  const long long* block_offset;   // [n_blocks + 1] (backward)
  const float* pos;        // [N, 3] or null
  const float* w1;         // [K, H]
  const float* b1;         // [H]
  const float* w2;         // [H, 3]
  const float* b2;         // [3]
  const float* target;     // [N, 3]
  const float* g;          // [1], the upstream gradient of the sum (backward)
  float* recon;            // [N, 3] or null
  float* gerr;             // [N, 3]: recon - target where the gradient flows, 0 where the clip cut it
  float* partial;          // forward: [tiles] sums; backward: [groups, total] parameter gradients
  float* dzp;              // [N, C]
  long long N;
  long long tiles;
  long long total;         // K H + H + 3 H + 3
  int n_blocks, C, H, PD, K, clip, groups;
  float A[9], o[3];
};

// the tile's inputs as Xs[k][point]: position rows first, then the block's latent
__device__ __forceinline__ void pm_stage_x(const PmParams& p, long long tile, float* Xs) {
  for (int e = threadIdx.x; e < p.K * PM_TILE; e += PM_THREADS) {
    const int k = e / PM_TILE, pt = e - k * PM_TILE;
    const long long n = tile * PM_TILE + pt;
    float v = 0.f;
    if (n < p.N) {
      if (k < p.PD) {
        v = p.pos[n * 3 + k];
      } else {
        const int b = p.index[n];
        if (b >= 0 && b < p.n_blocks) v = p.z[static_cast<long long>(b) * p.C + (k - p.PD)];
      }
    }
    Xs[e] = v;
  }
}

// a chunk of the weights: W1s[k][PM_HC], b1s[PM_HC], W2s[PM_HC][3], zero past H
__device__ __forceinline__ void pm_stage_w(const PmParams& p, int chunk, float* W1s, float* b1s, float* W2s) {
  const int hbase = chunk * PM_HC;
  for (int e = threadIdx.x; e < p.K * PM_HC; e += PM_THREADS) {
    const int k = e / PM_HC, h = hbase + (e - k * PM_HC);
    W1s[e] = h < p.H ? p.w1[static_cast<long long>(k) * p.H + h] : 0.f;
  }
  if (threadIdx.x < PM_HC) {
    const int h = hbase + threadIdx.x;
    b1s[threadIdx.x] = h < p.H ? p.b1[h] : 0.f;
  }
  if (threadIdx.x < PM_HC * 3) {
    const int h = hbase + threadIdx.x / 3;
    W2s[threadIdx.x] = h < p.H ? p.w2[static_cast<long long>(hbase) * 3 + threadIdx.x] : 0.f;
  }
}

// pre-activations of 8 points x 4 hidden units
__device__ __forceinline__ void pm_hidden(const float* Xs, const float* W1s, const float* b1s, int K, int p0, int h0,
                                          float (&pre)[8][4]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) pre[i][j] = 0.f;
  for (int k = 0; k < K; ++k) {
    const float4 xa = *reinterpret_cast<const float4*>(Xs + k * PM_TILE + p0);
    const float4 xb = *reinterpret_cast<const float4*>(Xs + k * PM_TILE + p0 + 4);
    const float4 w = *reinterpret_cast<const float4*>(W1s + k * PM_HC + h0);
    const float x[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
    const float ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) pre[i][j] = fmaf(x[i], ww[j], pre[i][j]);
  }
  const float4 b = *reinterpret_cast<const float4*>(b1s + h0);
  const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) pre[i][j] += bb[j];
}

__global__ void __launch_bounds__(PM_THREADS) lvac_point_mlp_forward_kernel(PmParams p) {
  __shared__ __attribute__((aligned(16))) float Xs[PM_MAX_K * PM_TILE];
  __shared__ __attribute__((aligned(16))) float W1s[PM_MAX_K * PM_HC];
  __shared__ __attribute__((aligned(16))) float b1s[PM_HC];
  __shared__ float W2s[PM_HC * 3];
  __shared__ float red[PM_THREADS / 16];
  const int t = threadIdx.x, hg = t & 15, pg = t >> 4, p0 = pg * 8, h0 = hg * 4;
  const long long tile = blockIdx.x;
  pm_stage_x(p, tile, Xs);
  float y[8][3];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) y[i][c] = 0.f;
  const int chunks = (p.H + PM_HC - 1) / PM_HC;
  for (int chunk = 0; chunk < chunks; ++chunk) {
    if (chunk) __syncthreads();
    pm_stage_w(p, chunk, W1s, b1s, W2s);
    __syncthreads();
    float pre[8][4];
    pm_hidden(Xs, W1s, b1s, p.K, p0, h0, pre);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float w0 = W2s[(h0 + j) * 3], w1 = W2s[(h0 + j) * 3 + 1], w2 = W2s[(h0 + j) * 3 + 2];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float h = fmaxf(pre[i][j], 0.f);
        y[i][0] = fmaf(h, w0, y[i][0]);
        y[i][1] = fmaf(h, w1, y[i][1]);
        y[i][2] = fmaf(h, w2, y[i][2]);
      }
    }
  }
  // the 16 hidden groups of a point group are 16 adjacent lanes: a butterfly leaves the same sum in each
#pragma unroll
  for (int m = 1; m < 16; m <<= 1)
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) y[i][c] += __shfl_xor(y[i][c], m);
  float sse = 0.f;
  if (hg == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const long long n = tile * PM_TILE + p0 + i;
      if (n < p.N) {
        const float y0 = y[i][0] + p.b2[0], y1 = y[i][1] + p.b2[1], y2 = y[i][2] + p.b2[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          float v = fmaf(p.A[r * 3 + 2], y2, fmaf(p.A[r * 3 + 1], y1, fmaf(p.A[r * 3], y0, p.o[r])));
          bool open = true;
          if (p.clip) {
            open = v >= 0.f && v <= 255.f;
            v = fminf(fmaxf(v, 0.f), 255.f);
          }
          const float e = v - p.target[n * 3 + r];
          if (p.recon) p.recon[n * 3 + r] = v;
          if (p.gerr) p.gerr[n * 3 + r] = open ? e : 0.f;
          sse = fmaf(e, e, sse);
        }
      }
    }
    red[pg] = sse;
  }
  __syncthreads();
  if (t == 0) {
    float s = 0.f;
    for (int i = 0; i < PM_THREADS / 16; ++i) s += red[i];
    p.partial[tile] = s;
  }
}

// out[i] = scale * sum_g part[g * stride + i], g ascending; one element per thread
__global__ void __launch_bounds__(PM_SUM_THREADS) lvac_point_mlp_merge_kernel(const float* part, float* out,
                                                                             long long count, long long stride,
                                                                             int groups) {
  const long long i = static_cast<long long>(blockIdx.x) * PM_SUM_THREADS + threadIdx.x;
  if (i >= count) return;
  float s = 0.f;
  for (int g = 0; g < groups; ++g) s += part[g * stride + i];
  out[i] = s;
}

// out[0] = sum of part[0 .. count): each thread a strided sum in ascending order, then a fixed tree
__global__ void __launch_bounds__(PM_SUM_THREADS) lvac_point_mlp_sum_kernel(const float* part, long long count,
                                                                           float* out) {
  __shared__ float red[PM_SUM_THREADS];
  float s = 0.f;
  for (long long i = threadIdx.x; i < count; i += PM_SUM_THREADS) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = PM_SUM_THREADS / 2; w > 0; w >>= 1) {
    if (static_cast<int>(threadIdx.x) < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

// dy = A^T (2 g gerr) of the tile's points as dYs[c][point]
__device__ __forceinline__ void pm_stage_dy(const PmParams& p, long long tile, float gs, float* dYs, float (&dy)[3]) {
  dy[0] = dy[1] = dy[2] = 0.f;
  if (threadIdx.x < PM_TILE) {
    const long long n = tile * PM_TILE + threadIdx.x;
    if (n < p.N) {
      const float d0 = 2.f * gs * p.gerr[n * 3], d1 = 2.f * gs * p.gerr[n * 3 + 1], d2 = 2.f * gs * p.gerr[n * 3 + 2];
#pragma unroll
      for (int c = 0; c < 3; ++c) dy[c] = fmaf(p.A[6 + c], d2, fmaf(p.A[3 + c], d1, p.A[c] * d0));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dYs[c * PM_TILE + threadIdx.x] = dy[c];
  }
}

// dh of 8 points x 4 hidden units (through the ReLU) into dHs[point][PM_DH]; h is left in `pre`
__device__ __forceinline__ void pm_dhidden(const float* dYs, const float* W2s, int p0, int h0, float (&pre)[8][4],
                                           float (&dh)[8][4]) {
  float dy[3][8];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float4 a = *reinterpret_cast<const float4*>(dYs + c * PM_TILE + p0);
    const float4 b = *reinterpret_cast<const float4*>(dYs + c * PM_TILE + p0 + 4);
    dy[c][0] = a.x; dy[c][1] = a.y; dy[c][2] = a.z; dy[c][3] = a.w;
    dy[c][4] = b.x; dy[c][5] = b.y; dy[c][6] = b.z; dy[c][7] = b.w;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float w0 = W2s[(h0 + j) * 3], w1 = W2s[(h0 + j) * 3 + 1], w2 = W2s[(h0 + j) * 3 + 2];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float v = fmaf(w2, dy[2][i], fmaf(w1, dy[1][i], w0 * dy[0][i]));
      dh[i][j] = pre[i][j] > 0.f ? v : 0.f;
      pre[i][j] = fmaxf(pre[i][j], 0.f);
    }
  }
}

// the per-point gradient of the latent: dzp[n, c] = sum_h W1[PD + c, h] dh[n, h]
__global__ void __launch_bounds__(PM_THREADS) lvac_point_mlp_bwd_input_kernel(PmParams p) {
  __shared__ __attribute__((aligned(16))) float Xs[PM_MAX_K * PM_TILE];
  __shared__ __attribute__((aligned(16))) float W1s[PM_MAX_K * PM_HC];
  __shared__ __attribute__((aligned(16))) float dHs[PM_TILE * PM_DH];
  __shared__ __attribute__((aligned(16))) float dYs[3 * PM_TILE];
  __shared__ __attribute__((aligned(16))) float b1s[PM_HC];
  __shared__ float W2s[PM_HC * 3];
  const int t = threadIdx.x, hg = t & 15, pg = t >> 4, p0 = pg * 8, h0 = hg * 4;
  const int pt = t & (PM_TILE - 1), kk = t / PM_TILE;      // second mapping: a point and every other channel
  const long long tile = blockIdx.x;
  const float gs = p.g[0];
  pm_stage_x(p, tile, Xs);
  float dy_own[3];
  pm_stage_dy(p, tile, gs, dYs, dy_own);
  float dx[PM_MAX_C / 2];
#pragma unroll
  for (int i = 0; i < PM_MAX_C / 2; ++i) dx[i] = 0.f;
  const int mine = (p.C - kk + 1) / 2;                      // channels kk, kk + 2, ... below C
  const int chunks = (p.H + PM_HC - 1) / PM_HC;
  for (int chunk = 0; chunk < chunks; ++chunk) {
    if (chunk) __syncthreads();
    pm_stage_w(p, chunk, W1s, b1s, W2s);
    __syncthreads();
    float pre[8][4], dh[8][4];
    pm_hidden(Xs, W1s, b1s, p.K, p0, h0, pre);
    pm_dhidden(dYs, W2s, p0, h0, pre, dh);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      *reinterpret_cast<float4*>(dHs + (p0 + i) * PM_DH + h0) = make_float4(dh[i][0], dh[i][1], dh[i][2], dh[i][3]);
    __syncthreads();
    for (int h4 = 0; h4 < PM_HC; h4 += 4) {
      const float4 d = *reinterpret_cast<const float4*>(dHs + pt * PM_DH + h4);
#pragma unroll
      for (int i = 0; i < PM_MAX_C / 2; ++i) {
        if (i < mine) {
          const float4 w = *reinterpret_cast<const float4*>(W1s + (p.PD + kk + 2 * i) * PM_HC + h4);
          dx[i] = fmaf(d.w, w.w, fmaf(d.z, w.z, fmaf(d.y, w.y, fmaf(d.x, w.x, dx[i]))));
        }
      }
    }
  }
  __syncthreads();
  // through LDS so that the rows leave as whole lines
#pragma unroll
  for (int i = 0; i < PM_MAX_C / 2; ++i)
    if (i < mine) dHs[pt * PM_DH + kk + 2 * i] = dx[i];
  __syncthreads();
  for (int e = t; e < PM_TILE * p.C; e += PM_THREADS) {
    const int row = e / p.C, c = e - row * p.C;
    const long long n = tile * PM_TILE + row;
    if (n < p.N) p.dzp[n * p.C + c] = dHs[row * PM_DH + c];
  }
}

// dz[b, c] = sum of dzp over the block's points: 256 / CP row lanes, each in ascending order, combined in lane order
__global__ void __launch_bounds__(PM_THREADS) lvac_point_mlp_bwd_blocks_kernel(const float* dzp,
                                                                               const long long* block_offset, float* dz,
                                                                               long long N, int n_blocks, int C, int CP) {
  __shared__ float red[PM_THREADS];
  const int c = threadIdx.x & (CP - 1), r = threadIdx.x / CP, lanes = PM_THREADS / CP;
  for (long long b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    long long lo = block_offset[b], hi = block_offset[b + 1];
    lo = lo < 0 ? 0 : (lo > N ? N : lo);
    hi = hi < lo ? lo : (hi > N ? N : hi);
    float s = 0.f;
    if (c < C)
      for (long long n = lo + r; n < hi; n += lanes) s += dzp[n * C + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (r == 0 && c < C) {
      float v = 0.f;
      for (int q = 0; q < lanes; ++q) v += red[q * CP + c];
      dz[b * C + c] = v;
    }
    __syncthreads();
  }
}

// parameter gradients: workgroup (g, chunk) owns PM_HC hidden units and the tiles g, g + groups, ...
__global__ void __launch_bounds__(PM_THREADS) lvac_point_mlp_bwd_param_kernel(PmParams p) {
  __shared__ __attribute__((aligned(16))) float Xs[PM_MAX_K * PM_TILE];
  __shared__ __attribute__((aligned(16))) float W1s[PM_MAX_K * PM_HC];
  __shared__ __attribute__((aligned(16))) float dHs[PM_TILE * PM_DH];
  __shared__ __attribute__((aligned(16))) float dYs[3 * PM_TILE];
  __shared__ __attribute__((aligned(16))) float b1s[PM_HC];
  __shared__ float W2s[PM_HC * 3];
  __shared__ float db2s[2 * 3];
  const int t = threadIdx.x, hg = t & 15, pg = t >> 4, p0 = pg * 8, h0 = hg * 4;
  const int kg = pg;                                       // second mapping: 4 hidden units x rows kg, kg + 16, ...
  const int chunk = blockIdx.y, hbase = chunk * PM_HC;
  const float gs = p.g[0];
  pm_stage_w(p, chunk, W1s, b1s, W2s);
  float dw1[PM_KG][4], dw2[4][3], db1[4], db2[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    db1[j] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) dw2[j][c] = 0.f;
#pragma unroll
    for (int i = 0; i < PM_KG; ++i) dw1[i][j] = 0.f;
  }
  int krow[PM_KG];
#pragma unroll
  for (int i = 0; i < PM_KG; ++i) krow[i] = min(kg + 16 * i, p.K - 1);
  for (long long tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    __syncthreads();
    pm_stage_x(p, tile, Xs);
    float dy_own[3];
    pm_stage_dy(p, tile, gs, dYs, dy_own);
    if (chunk == 0 && t < PM_TILE) {
#pragma unroll
      for (int m = 1; m < PM_WAVE; m <<= 1)
#pragma unroll
        for (int c = 0; c < 3; ++c) dy_own[c] += __shfl_xor(dy_own[c], m);
#pragma unroll
      for (int c = 0; c < 3; ++c) db2[c] += dy_own[c];
    }
    __syncthreads();
    float pre[8][4], dh[8][4];
    pm_hidden(Xs, W1s, b1s, p.K, p0, h0, pre);
    pm_dhidden(dYs, W2s, p0, h0, pre, dh);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      *reinterpret_cast<float4*>(dHs + (p0 + i) * PM_DH + h0) = make_float4(dh[i][0], dh[i][1], dh[i][2], dh[i][3]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        db1[j] += dh[i][j];
#pragma unroll
        for (int c = 0; c < 3; ++c) dw2[j][c] = fmaf(pre[i][j], dYs[c * PM_TILE + p0 + i], dw2[j][c]);
      }
    }
    __syncthreads();
    for (int q4 = 0; q4 < PM_TILE; q4 += 4) {
      float4 d[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) d[q] = *reinterpret_cast<const float4*>(dHs + (q4 + q) * PM_DH + h0);
#pragma unroll
      for (int i = 0; i < PM_KG; ++i) {
        if (16 * i < p.K) {
          const float4 x = *reinterpret_cast<const float4*>(Xs + krow[i] * PM_TILE + q4);
          dw1[i][0] = fmaf(x.w, d[3].x, fmaf(x.z, d[2].x, fmaf(x.y, d[1].x, fmaf(x.x, d[0].x, dw1[i][0]))));
          dw1[i][1] = fmaf(x.w, d[3].y, fmaf(x.z, d[2].y, fmaf(x.y, d[1].y, fmaf(x.x, d[0].y, dw1[i][1]))));
          dw1[i][2] = fmaf(x.w, d[3].z, fmaf(x.z, d[2].z, fmaf(x.y, d[1].z, fmaf(x.x, d[0].z, dw1[i][2]))));
          dw1[i][3] = fmaf(x.w, d[3].w, fmaf(x.z, d[2].w, fmaf(x.y, d[1].w, fmaf(x.x, d[0].w, dw1[i][3]))));
        }
      }
    }
  }
  float* out = p.partial + static_cast<long long>(blockIdx.x) * p.total;
  const long long off_b1 = static_cast<long long>(p.K) * p.H, off_w2 = off_b1 + p.H, off_b2 = off_w2 + 3ll * p.H;
#pragma unroll
  for (int i = 0; i < PM_KG; ++i) {
    const int k = kg + 16 * i;
    if (k < p.K) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (hbase + h0 + j < p.H) out[static_cast<long long>(k) * p.H + hbase + h0 + j] = dw1[i][j];
    }
  }
  // dW2 and db1 of a hidden unit are spread over the 16 point groups: through LDS, summed in group order
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int c = 0; c < 3; ++c) dHs[(pg * PM_HC + h0 + j) * 4 + c] = dw2[j][c];
    dHs[(pg * PM_HC + h0 + j) * 4 + 3] = db1[j];
  }
  if (chunk == 0 && t < PM_TILE && (t & (PM_WAVE - 1)) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) db2s[(t / PM_WAVE) * 3 + c] = db2[c];
  }
  __syncthreads();
  {
    const int hl = t >> 2, c = t & 3;
    float s = 0.f;
    for (int q = 0; q < PM_THREADS / 16; ++q) s += dHs[(q * PM_HC + hl) * 4 + c];
    const int h = hbase + hl;
    if (h < p.H) {
      if (c < 3) out[off_w2 + 3ll * h + c] = s;
      else out[off_b1 + h] = s;
    }
  }
  if (chunk == 0 && t < 3) out[off_b2 + t] = db2s[t] + db2s[3 + t];
}

int pm_validate(const char* name, int64_t n, int64_t n_blocks, int channels, int hidden) {
  if (channels < PM_MIN_C || channels > PM_MAX_C)
    return fail("%s: channels must be in [%d, %d], got %d", name, PM_MIN_C, PM_MAX_C, channels);
  if (hidden < PM_MIN_H || hidden > PM_MAX_H)
    return fail("%s: hidden must be in [%d, %d], got %d", name, PM_MIN_H, PM_MAX_H, hidden);
  if (n < 0 || n > (1ll << 36)) return fail("%s: N must be in [0, 2^36], got %lld", name, static_cast<long long>(n));
  if (n_blocks < 0 || n_blocks > 0x7fffffffll)
    return fail("%s: n_blocks must be in [0, 2^31), got %lld", name, static_cast<long long>(n_blocks));
  if (n > 0 && n_blocks == 0) return fail("%s: points without a block", name);
  if (ceil_div(n, PM_TILE) > 0x7fffffffll) return fail("%s: too many point tiles", name);
  return 0;
}

void pm_fill(PmParams* p, const float* z, const int32_t* index, const float* position, const float* w1,
             const float* b1, const float* w2, const float* b2, const float* affine, int64_t n, int64_t n_blocks,
             int channels, int hidden) {
  p->z = z; p->index = index; p->pos = position; p->w1 = w1; p->b1 = b1; p->w2 = w2; p->b2 = b2;
  p->N = n; p->n_blocks = static_cast<int>(n_blocks); p->C = channels; p->H = hidden;
  p->PD = position ? 3 : 0;
  p->K = channels + p->PD;
  p->tiles = ceil_div(n, PM_TILE);
  p->total = static_cast<long long>(p->K) * hidden + hidden + 3ll * hidden + 3;
  for (int i = 0; i < 9; ++i) p->A[i] = affine[i];
  for (int i = 0; i < 3; ++i) p->o[i] = affine[9 + i];
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_raht_forward(const float* dc, int64_t n_root, const float* const* ac, const int64_t* desc,
                                const int64_t* desc_dev, const int32_t* tables, int64_t table_words, int levels,
                                int64_t channels, float* out, int64_t n_out, void* stream) {
  using namespace tfc;
  RahtPlan plan;
  if (int rc = raht_plan("tfc_raht_forward", desc, table_words, levels, channels, n_root, n_out, &plan)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_out == 0) return 0;
  if (!dc || !out) return fail("tfc_raht_forward: dc and out must not be null");
  KernelTimer timer("raht_forward", st);
  if (plan.n_active == 0) {
    TFC_HIP(hipMemcpyAsync(out, dc, sizeof(float) * static_cast<size_t>(n_out * channels), hipMemcpyDeviceToDevice, st));
    return 0;
  }
  if (!ac || !desc_dev || !tables) return fail("tfc_raht_forward: ac, descriptors and tables must not be null");
  return raht_run(lvac_raht_forward_kernel, plan, plan.active, plan.n_active, true, const_cast<float* const*>(ac),
                  desc_dev, tables, channels, dc, out, st);
}

extern "C" int tfc_raht_backward(const float* d_out, int64_t n_out, float* const* d_ac, const int64_t* desc,
                                 const int64_t* desc_dev, const int32_t* tables, int64_t table_words, int levels,
                                 int64_t channels, float* d_dc, int64_t n_root, void* stream) {
  using namespace tfc;
  RahtPlan plan;
  if (int rc = raht_plan("tfc_raht_backward", desc, table_words, levels, channels, n_root, n_out, &plan)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_out == 0) return 0;
  if (!d_out || !d_dc) return fail("tfc_raht_backward: d_out and d_dc must not be null");
  KernelTimer timer("raht_backward", st);
  if (plan.n_active == 0) {
    TFC_HIP(hipMemcpyAsync(d_dc, d_out, sizeof(float) * static_cast<size_t>(n_out * channels), hipMemcpyDeviceToDevice,
                           st));
    return 0;
  }
  if (!d_ac || !desc_dev || !tables) return fail("tfc_raht_backward: d_ac, descriptors and tables must not be null");
  int order[RAHT_MAX_LEVELS];
  for (int i = 0; i < plan.n_active; ++i) order[i] = plan.active[plan.n_active - 1 - i];
  return raht_run(lvac_raht_backward_kernel, plan, order, plan.n_active, false, d_ac, desc_dev, tables, channels,
                  d_out, d_dc, st);
}

extern "C" int tfc_point_mlp_forward(const float* z, const int32_t* index, const float* position, const float* w1,
                                     const float* b1, const float* w2, const float* b2, const float* affine,
                                     const float* target, int64_t n, int64_t n_blocks, int channels, int hidden,
                                     int clip, float* recon, float* gerr, float* sse, void* stream) {
  using namespace tfc;
  if (int rc = pm_validate("tfc_point_mlp_forward", n, n_blocks, channels, hidden)) return rc;
  if (!sse || !affine) return fail("tfc_point_mlp_forward: sse and affine must not be null");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) {
    TFC_HIP(hipMemsetAsync(sse, 0, sizeof(float), st));
    return 0;
  }
  if (!z || !index || !w1 || !b1 || !w2 || !b2 || !target)
    return fail("tfc_point_mlp_forward: z, index, the weights and target must not be null");
  PmParams p = {};
  pm_fill(&p, z, index, position, w1, b1, w2, b2, affine, n, n_blocks, channels, hidden);
  p.target = target; p.clip = clip; p.recon = recon; p.gerr = gerr;
  DevBuf part;
  TFC_HIP(part.alloc(sizeof(float) * static_cast<size_t>(p.tiles), st));
  p.partial = part.as<float>();
  KernelTimer timer("point_mlp_forward", st);
  hipLaunchKernelGGL(lvac_point_mlp_forward_kernel, dim3(static_cast<unsigned>(p.tiles)), dim3(PM_THREADS), 0, st, p);
  hipLaunchKernelGGL(lvac_point_mlp_sum_kernel, dim3(1), dim3(PM_SUM_THREADS), 0, st, p.partial, p.tiles, sse);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_point_mlp_backward(const float* z, const int32_t* index, const int64_t* block_offset,
                                      const float* position, const float* w1, const float* b1, const float* w2,
                                      const float* b2, const float* affine, const float* gerr, const float* g_sse,
                                      int64_t n, int64_t n_blocks, int channels, int hidden, float* d_params,
                                      float* d_z, void* stream) {
  using namespace tfc;
  if (int rc = pm_validate("tfc_point_mlp_backward", n, n_blocks, channels, hidden)) return rc;
  if (!affine) return fail("tfc_point_mlp_backward: affine must not be null");
  hipStream_t st = static_cast<hipStream_t>(stream);
  PmParams p = {};
  pm_fill(&p, z, index, position, w1, b1, w2, b2, affine, n, n_blocks, channels, hidden);
  if (n == 0) {
    if (d_params) TFC_HIP(hipMemsetAsync(d_params, 0, sizeof(float) * static_cast<size_t>(p.total), st));
    if (d_z && n_blocks) TFC_HIP(hipMemsetAsync(d_z, 0, sizeof(float) * static_cast<size_t>(n_blocks * channels), st));
    return 0;
  }
  if (!d_params && !d_z) return 0;
  if (!z || !index || !w1 || !b1 || !w2 || !b2 || !gerr || !g_sse)
    return fail("tfc_point_mlp_backward: z, index, the weights, gerr and g_sse must not be null");
  if (d_z && !block_offset) return fail("tfc_point_mlp_backward: block_offset must not be null");
  p.block_offset = reinterpret_cast<const long long*>(block_offset);
  p.gerr = const_cast<float*>(gerr); p.g = g_sse;
  KernelTimer timer("point_mlp_backward", st);
  if (d_z) {
    DevBuf dzp;
    TFC_HIP(dzp.alloc(sizeof(float) * static_cast<size_t>(n * channels), st));
    PmParams q = p;
    q.dzp = dzp.as<float>();
    hipLaunchKernelGGL(lvac_point_mlp_bwd_input_kernel, dim3(static_cast<unsigned>(p.tiles)), dim3(PM_THREADS), 0, st, q);
    int cp = 1;
    while (cp < channels) cp <<= 1;
    const unsigned blocks = static_cast<unsigned>(std::min<int64_t>(n_blocks, 1 << 22));
    hipLaunchKernelGGL(lvac_point_mlp_bwd_blocks_kernel, dim3(blocks), dim3(PM_THREADS), 0, st, q.dzp,
                       p.block_offset, d_z, static_cast<long long>(n), static_cast<int>(n_blocks), channels, cp);
  }
  if (d_params) {
    PmParams q = p;
    q.groups = static_cast<int>(std::min<long long>(p.tiles, PM_PARAM_GROUPS));
    DevBuf part;
    TFC_HIP(part.alloc(sizeof(float) * static_cast<size_t>(q.groups * p.total), st));
    q.partial = part.as<float>();
    const unsigned chunks = static_cast<unsigned>(ceil_div(hidden, PM_HC));
    hipLaunchKernelGGL(lvac_point_mlp_bwd_param_kernel, dim3(static_cast<unsigned>(q.groups), chunks), dim3(PM_THREADS),
                       0, st, q);
    hipLaunchKernelGGL(lvac_point_mlp_merge_kernel, dim3(static_cast<unsigned>(ceil_div(p.total, PM_SUM_THREADS))),
                       dim3(PM_SUM_THREADS), 0, st, q.partial, d_params, p.total, p.total, q.groups);
  }
  TFC_HIP(hipGetLastError());
  return 0;
}
