// The scale-space warp of "Scale-space flow for end-to-end optimized video compression" (Agustsson et al., CVPR 2020,
// section 3.1) on gfx950: the Gaussian scale-space volume of a frame, its trilinear sampling by a (dx, dy, s) field, and
// both gradients.  include/tfc_hip.h states the definition in full.
//
// Volume.  Two launches for all planes.  The row pass loads one segment of an image row (with the widest plane's halo)
// into LDS once and writes plane 0 and the M row-blurred planes of it; the column pass has the plane as a grid
// dimension and stages a SS_COL_TILE_H x SS_COL_TILE_X tile of the W * C row-major plane with that plane's own halo.
// The taps exp(-t^2 / 2 sigma^2) and their running sums (from which the norm of a border pixel follows as
// cum[min(R, i)] + cum[min(R, n - 1 - i)] - 1) are computed on the host in double and travel in the kernel arguments.
// The adjoint is the same pair of passes in the other order on g / norm: a gather, no scatter.
//
// Warp.  One output pixel per lane, the C channels of a corner loaded together.  The backward computes the flow
// gradient as a gather (differences of corners first, channels summed in ascending order) and scatters g * weight
// into the volume gradient in 64-bit fixed point: integer addition is associative, so the sums are the same bits
// whatever order the atomics arrive in.  The scale 2^(SS_FIXED_BITS - e), e = floor(log2 max|g|) + 1, comes from a
// two-stage reduction that stays on the device; with H * W <= 2^22 contributions below 2^40 each a sum cannot
// overflow.  The volume adjoint reads the integer planes directly, so the prediction's backward never holds the float
// volume gradient.
#include "common.h"
#include "scale_space_params.h"

#include <cmath>

namespace tfc {
namespace {

struct SsShape {
  int n, h, w, c, m;          // m blurred planes: the volume has m + 1
};

// taps of plane p + 1: w[off[p] + t], t = 0 .. radius[p]; cum[off[p] + t] = w_0 + ... + w_t
struct SsTaps {
  int off[SS_MAX_LEVELS];
  int radius[SS_MAX_LEVELS];
  float w[SS_MAX_TAPS];
  float cum[SS_MAX_TAPS];
};

// the sum of the taps that fall inside [0, n) around position i
__device__ __forceinline__ float ss_norm(const float* cum, int r, int i, int n) {
  return cum[min(r, i)] + cum[min(r, n - 1 - i)] - 1.0f;
}

struct SsFixed {
  int e;
  bool bad;                   // max|g| is not finite: every gradient is NaN
};

__device__ __forceinline__ SsFixed ss_fixed_init(const float* gmax) {
  SsFixed f;
  const float g = *gmax;
  f.bad = !(g < INFINITY);
  f.e = 0;
  if (!f.bad && g > 0.0f) (void)frexpf(g, &f.e);       // g = m 2^e, m in [0.5, 1): e = floor(log2 g) + 1
  return f;
}

__device__ __forceinline__ float ss_fixed_to_float(long long v, SsFixed f) {
  return f.bad ? NAN : static_cast<float>(ldexp(static_cast<double>(v), f.e - SS_FIXED_BITS));
}

// ------------------------------------------------------------------------------------------------------------------
// the volume and its adjoint
// ------------------------------------------------------------------------------------------------------------------

constexpr int SS_ROW_SEG = (SS_ROW_TILE + 2 * SS_MAX_RADIUS) * SS_MAX_C;       // floats
constexpr int SS_ROW_ITEMS = SS_ROW_TILE * SS_MAX_C / SS_THREADS;              // (pixel, channel) items of a thread
constexpr int SS_COL_ROWS = SS_COL_TILE_H + 2 * SS_MAX_RADIUS;
constexpr int SS_COL_GROUPS = SS_THREADS / SS_COL_TILE_X;                      // row groups of a column workgroup

__device__ __forceinline__ void ss_block_row(long long b, int tiles_w, int h, int* n, int* i, int* jt) {
  *jt = static_cast<int>(b % tiles_w);
  b /= tiles_w;
  *i = static_cast<int>(b % h);
  *n = static_cast<int>(b / h);
}

// x [N, H, W, C] -> plane 0 of vol [N, M + 1, H, W, C] and the row-blurred planes tmp [N, M, H, W, C]
__global__ __launch_bounds__(SS_THREADS) void scale_space_row_forward_kernel(
    const float* __restrict__ x, float* __restrict__ vol, float* __restrict__ tmp, SsShape s, SsTaps taps,
    int tiles_w) {
  __shared__ float seg[SS_ROW_SEG];
  __shared__ float sw[SS_MAX_TAPS];
  __shared__ float scum[SS_MAX_TAPS];
  const int tid = threadIdx.x;
  int n, i, jt;
  ss_block_row(blockIdx.x, tiles_w, s.h, &n, &i, &jt);
  const int rmax = taps.radius[s.m - 1];
  const int ntaps = taps.off[s.m - 1] + rmax + 1;
  for (int k = tid; k < ntaps; k += SS_THREADS) {
    sw[k] = taps.w[k];
    scum[k] = taps.cum[k];
  }
  const int len_row = s.w * s.c;
  const int j0 = jt * SS_ROW_TILE;
  const int f0 = (j0 - rmax) * s.c;                       // the row's flattened index of seg[0]
  const int len = (SS_ROW_TILE + 2 * rmax) * s.c;
  const long long plane = static_cast<long long>(s.h) * len_row;
  const float* row = x + (static_cast<long long>(n) * s.h + i) * len_row;
  for (int k = tid; k < len; k += SS_THREADS) {
    const int f = f0 + k;
    seg[k] = (f >= 0 && f < len_row) ? row[f] : 0.0f;
  }
  __syncthreads();
  const int items = min(SS_ROW_TILE, s.w - j0) * s.c;
  const long long at = static_cast<long long>(i) * len_row + static_cast<long long>(j0) * s.c;
  float* v0 = vol + static_cast<long long>(n) * (s.m + 1) * plane + at;
  float* t0 = tmp + static_cast<long long>(n) * s.m * plane + at;
  for (int idx = tid; idx < items; idx += SS_THREADS) {
    const int j = j0 + idx / s.c;
    const int center = rmax * s.c + idx;
    v0[idx] = seg[center];
    for (int p = 0; p < s.m; ++p) {
      const int r = taps.radius[p];
      const float* w = sw + taps.off[p];
      const int lo = max(-r, -j), hi = min(r, s.w - 1 - j);
      float acc = 0.0f;
      for (int t = lo; t <= hi; ++t) acc = fmaf(w[abs(t)], seg[center + t * s.c], acc);
      t0[p * plane + idx] = acc / ss_norm(scum + taps.off[p], r, j, s.w);
    }
  }
}

// ADJ = false: tmp plane p -> vol plane p + 1, blurred along H and divided by the column norm.
// ADJ = true: plane p + 1 of the volume gradient (float, or FIXED: the integer sums), divided by the norm of its own
// pixel, correlated along H -> tmp plane p.
template <bool ADJ, bool FIXED>
__global__ __launch_bounds__(SS_THREADS) void scale_space_col_kernel(
    const void* __restrict__ src, float* __restrict__ dst, const float* __restrict__ gmax, SsShape s, SsTaps taps,
    int tiles_x, int tiles_h) {
  __shared__ float tile[SS_COL_ROWS * SS_COL_TILE_X];
  __shared__ float sw[SS_MAX_RADIUS + 1];
  __shared__ float scum[SS_MAX_RADIUS + 1];
  const int tid = threadIdx.x;
  long long b = blockIdx.x;
  const int xt = static_cast<int>(b % tiles_x);
  b /= tiles_x;
  const int it = static_cast<int>(b % tiles_h);
  b /= tiles_h;
  const int p = static_cast<int>(b % s.m);
  const int n = static_cast<int>(b / s.m);
  const int r = taps.radius[p];
  const int off = taps.off[p];
  for (int k = tid; k <= r; k += SS_THREADS) {
    sw[k] = taps.w[off + k];
    scum[k] = taps.cum[off + k];
  }
  __syncthreads();
  const int len_row = s.w * s.c;
  const int xl = tid % SS_COL_TILE_X, rg = tid / SS_COL_TILE_X;
  const int x = xt * SS_COL_TILE_X + xl;
  const int i0 = it * SS_COL_TILE_H;
  const int rows = SS_COL_TILE_H + 2 * r;
  const long long plane = static_cast<long long>(s.h) * len_row;
  const long long src_at = (ADJ ? static_cast<long long>(n) * (s.m + 1) + p + 1 : static_cast<long long>(n) * s.m + p) * plane;
  const long long dst_at = (ADJ ? static_cast<long long>(n) * s.m + p : static_cast<long long>(n) * (s.m + 1) + p + 1) * plane;
  SsFixed fx = {0, false};
  if (FIXED) fx = ss_fixed_init(gmax);
  float nrow = 1.0f;
  if (ADJ && x < len_row) nrow = ss_norm(scum, r, x / s.c, s.w);
  for (int rr = rg; rr < rows; rr += SS_COL_GROUPS) {
    const int ii = i0 - r + rr;
    float v = 0.0f;
    if (ii >= 0 && ii < s.h && x < len_row) {
      const long long at = src_at + static_cast<long long>(ii) * len_row + x;
      if (!ADJ) {
        v = static_cast<const float*>(src)[at];
      } else {
        const float g = FIXED ? ss_fixed_to_float(static_cast<const long long*>(src)[at], fx)
                              : static_cast<const float*>(src)[at];
        v = g / (nrow * ss_norm(scum, r, ii, s.h));
      }
    }
    tile[rr * SS_COL_TILE_X + xl] = v;
  }
  __syncthreads();
  if (x >= len_row) return;
  for (int rr = rg; rr < SS_COL_TILE_H; rr += SS_COL_GROUPS) {
    const int i = i0 + rr;
    if (i >= s.h) break;
    const int lo = max(-r, -i), hi = min(r, s.h - 1 - i);
    float acc = 0.0f;
    for (int t = lo; t <= hi; ++t) acc = fmaf(sw[abs(t)], tile[(rr + r + t) * SS_COL_TILE_X + xl], acc);
    dst[dst_at + static_cast<long long>(i) * len_row + x] = ADJ ? acc : acc / ss_norm(scum, r, i, s.h);
  }
}

// gx = plane 0 of the volume gradient + sum over p (ascending) of the row correlation of tmp plane p
template <bool FIXED>
__global__ __launch_bounds__(SS_THREADS) void scale_space_row_adjoint_kernel(
    const void* __restrict__ gvol, const float* __restrict__ tmp, float* __restrict__ gx,
    const float* __restrict__ gmax, SsShape s, SsTaps taps, int tiles_w) {
  __shared__ float seg[SS_ROW_SEG];
  __shared__ float sw[SS_MAX_TAPS];
  const int tid = threadIdx.x;
  int n, i, jt;
  ss_block_row(blockIdx.x, tiles_w, s.h, &n, &i, &jt);
  const int ntaps = taps.off[s.m - 1] + taps.radius[s.m - 1] + 1;
  for (int k = tid; k < ntaps; k += SS_THREADS) sw[k] = taps.w[k];
  const int len_row = s.w * s.c;
  const int j0 = jt * SS_ROW_TILE;
  const int items = min(SS_ROW_TILE, s.w - j0) * s.c;
  const long long plane = static_cast<long long>(s.h) * len_row;
  const long long row_at = static_cast<long long>(i) * len_row;
  const long long at = row_at + static_cast<long long>(j0) * s.c;
  SsFixed fx = {0, false};
  if (FIXED) fx = ss_fixed_init(gmax);
  float out[SS_ROW_ITEMS];
#pragma unroll
  for (int q = 0; q < SS_ROW_ITEMS; ++q) {
    const int idx = tid + q * SS_THREADS;
    out[q] = 0.0f;
    if (idx < items) {
      const long long g0 = static_cast<long long>(n) * (s.m + 1) * plane + at + idx;
      out[q] = FIXED ? ss_fixed_to_float(static_cast<const long long*>(gvol)[g0], fx)
                     : static_cast<const float*>(gvol)[g0];
    }
  }
  for (int p = 0; p < s.m; ++p) {
    const int r = taps.radius[p];
    const float* w = sw + taps.off[p];
    const int f0 = (j0 - r) * s.c;
    const int len = (SS_ROW_TILE + 2 * r) * s.c;
    const float* row = tmp + (static_cast<long long>(n) * s.m + p) * plane + row_at;
    __syncthreads();                                      // the taps (first round), the previous plane's readers
    for (int k = tid; k < len; k += SS_THREADS) {
      const int f = f0 + k;
      seg[k] = (f >= 0 && f < len_row) ? row[f] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SS_ROW_ITEMS; ++q) {
      const int idx = tid + q * SS_THREADS;
      if (idx < items) {
        const int j = j0 + idx / s.c;
        const int center = r * s.c + idx;
        const int lo = max(-r, -j), hi = min(r, s.w - 1 - j);
        float acc = 0.0f;
        for (int t = lo; t <= hi; ++t) acc = fmaf(w[abs(t)], seg[center + t * s.c], acc);
        out[q] += acc;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < SS_ROW_ITEMS; ++q) {
    const int idx = tid + q * SS_THREADS;
    if (idx < items) gx[static_cast<long long>(n) * plane + at + idx] = out[q];
  }
}

// ------------------------------------------------------------------------------------------------------------------
// the warp
// ------------------------------------------------------------------------------------------------------------------

// One axis of the sampling position: clamped into [0, last], so that whatever `raw` holds (NaN goes to 0 through
// fmaxf) both cells lie inside the volume.  `inside`: the coordinate was not clamped, its gradient is not zero.
__device__ __forceinline__ void ss_axis(float raw, int last, int* a0, int* a1, float* wa, bool* inside) {
  const float hi = static_cast<float>(last);
  const float p = fminf(fmaxf(raw, 0.0f), hi);
  *inside = raw > 0.0f && raw < hi;
  const int f = static_cast<int>(floorf(p));
  *a0 = max(0, min(f, max(last - 1, 0)));
  *a1 = min(*a0 + 1, last);
  *wa = p - static_cast<float>(*a0);
}

template <int C>
__device__ __forceinline__ void ss_load(const float* p, float (&v)[C]) {
  if constexpr (C % 4 == 0) {
#pragma unroll
    for (int k = 0; k < C / 4; ++k) {
      const float4 q = reinterpret_cast<const float4*>(p)[k];
      v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
    }
  } else if constexpr (C % 2 == 0) {
#pragma unroll
    for (int k = 0; k < C / 2; ++k) {
      const float2 q = reinterpret_cast<const float2*>(p)[k];
      v[2 * k] = q.x; v[2 * k + 1] = q.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < C; ++k) v[k] = p[k];
  }
}

template <int C>
__device__ __forceinline__ void ss_store(float* p, const float (&v)[C]) {
  if constexpr (C % 4 == 0) {
#pragma unroll
    for (int k = 0; k < C / 4; ++k)
      reinterpret_cast<float4*>(p)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
  } else if constexpr (C % 2 == 0) {
#pragma unroll
    for (int k = 0; k < C / 2; ++k) reinterpret_cast<float2*>(p)[k] = make_float2(v[2 * k], v[2 * k + 1]);
  } else {
#pragma unroll
    for (int k = 0; k < C; ++k) p[k] = v[k];
  }
}

struct SsSample {
  int n;
  int a0[3], a1[3];           // x, y, z cells
  float wa[3];
  bool inside[3];
};

__device__ __forceinline__ SsSample ss_sample(const float* flow, long long pix, SsShape s) {
  SsSample q;
  const long long hw = static_cast<long long>(s.h) * s.w;
  q.n = static_cast<int>(pix / hw);
  const int rem = static_cast<int>(pix - q.n * hw);
  const int i = rem / s.w, j = rem - i * s.w;
  const float dx = flow[pix * 3], dy = flow[pix * 3 + 1], sz = flow[pix * 3 + 2];
  ss_axis(static_cast<float>(j) + dx, s.w - 1, &q.a0[0], &q.a1[0], &q.wa[0], &q.inside[0]);
  ss_axis(static_cast<float>(i) + dy, s.h - 1, &q.a0[1], &q.a1[1], &q.wa[1], &q.inside[1]);
  ss_axis(sz, s.m, &q.a0[2], &q.a1[2], &q.wa[2], &q.inside[2]);
  return q;
}

// corner k: bit 0 picks x1, bit 1 y1, bit 2 z1
__device__ __forceinline__ long long ss_corner(const SsSample& q, int k, SsShape s, int channels) {
  const int x = (k & 1) ? q.a1[0] : q.a0[0], y = (k & 2) ? q.a1[1] : q.a0[1], z = (k & 4) ? q.a1[2] : q.a0[2];
  return (((static_cast<long long>(q.n) * (s.m + 1) + z) * s.h + y) * s.w + x) * channels;
}

__device__ __forceinline__ float ss_weight(const SsSample& q, int k) {
  const float wx = (k & 1) ? q.wa[0] : 1.0f - q.wa[0];
  const float wy = (k & 2) ? q.wa[1] : 1.0f - q.wa[1];
  const float wz = (k & 4) ? q.wa[2] : 1.0f - q.wa[2];
  return (wz * wy) * wx;
}

template <int C>
__global__ __launch_bounds__(SS_WARP_TILE) void scale_space_warp_forward_kernel(
    const float* __restrict__ vol, const float* __restrict__ flow, float* __restrict__ out, SsShape s) {
  const long long pix = static_cast<long long>(blockIdx.x) * SS_WARP_TILE + threadIdx.x;
  if (pix >= static_cast<long long>(s.n) * s.h * s.w) return;
  const SsSample q = ss_sample(flow, pix, s);
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float v[C];
    ss_load<C>(vol + ss_corner(q, k, s, C), v);
    const float w = ss_weight(q, k);
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = fmaf(w, v[c], acc[c]);
  }
  ss_store<C>(out + pix * C, acc);
}

// max |g| in two stages of fixed shape; a NaN or an infinity anywhere makes the result NaN
__device__ __forceinline__ void ss_absmax_block(float m, bool bad, float* result) {
  __shared__ float sm[SS_THREADS];
  __shared__ int sb[SS_THREADS];
  const int tid = threadIdx.x;
  sm[tid] = m;
  sb[tid] = bad ? 1 : 0;
  __syncthreads();
  for (int k = SS_THREADS / 2; k > 0; k >>= 1) {
    if (tid < k) {
      sm[tid] = fmaxf(sm[tid], sm[tid + k]);
      sb[tid] |= sb[tid + k];
    }
    __syncthreads();
  }
  if (tid == 0) *result = sb[0] ? NAN : sm[0];
}

__global__ __launch_bounds__(SS_THREADS) void scale_space_absmax_kernel(const float* __restrict__ g, long long total,
                                                                        float* __restrict__ parts) {
  float m = 0.0f;
  bool bad = false;
  const long long step = static_cast<long long>(gridDim.x) * SS_THREADS;
  for (long long k = static_cast<long long>(blockIdx.x) * SS_THREADS + threadIdx.x; k < total; k += step) {
    const float a = fabsf(g[k]);
    bad |= !(a < INFINITY);
    m = fmaxf(m, a);
  }
  ss_absmax_block(m, bad, parts + blockIdx.x);
}

__global__ __launch_bounds__(SS_THREADS) void scale_space_absmax_final_kernel(const float* __restrict__ parts, int count,
                                                                              float* __restrict__ gmax) {
  float m = 0.0f;
  bool bad = false;
  for (int k = threadIdx.x; k < count; k += SS_THREADS) {
    const float a = parts[k];
    bad |= !(a < INFINITY);
    m = fmaxf(m, a);
  }
  ss_absmax_block(m, bad, gmax);
}

// gflow (when asked for) and the fixed-point scatter of g * weight into acc [N, M + 1, H, W, C] (when asked for)
template <int C>
__global__ __launch_bounds__(SS_WARP_TILE) void scale_space_warp_backward_kernel(
    const float* __restrict__ g, const float* __restrict__ vol, const float* __restrict__ flow,
    float* __restrict__ gflow, long long* __restrict__ acc, const float* __restrict__ gmax, SsShape s) {
  const long long pix = static_cast<long long>(blockIdx.x) * SS_WARP_TILE + threadIdx.x;
  if (pix >= static_cast<long long>(s.n) * s.h * s.w) return;
  const float gm = *gmax;
  if (!(gm > 0.0f && gm < INFINITY)) {                   // all of g is zero, or some of it is not finite
    if (gflow) {
      const float fill = gm == 0.0f ? 0.0f : NAN;
      gflow[pix * 3] = fill;
      gflow[pix * 3 + 1] = fill;
      gflow[pix * 3 + 2] = fill;
    }
    return;
  }
  const SsSample q = ss_sample(flow, pix, s);
  float gv[C];
  ss_load<C>(g + pix * C, gv);
  if (gflow) {
    float v[8][C];
#pragma unroll
    for (int k = 0; k < 8; ++k) ss_load<C>(vol + ss_corner(q, k, s, C), v[k]);
    const float wx[2] = {1.0f - q.wa[0], q.wa[0]}, wy[2] = {1.0f - q.wa[1], q.wa[1]}, wz[2] = {1.0f - q.wa[2], q.wa[2]};
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float ddx = 0.0f, ddy = 0.0f, ddz = 0.0f;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          ddx = fmaf(wz[a] * wy[b], v[4 * a + 2 * b + 1][c] - v[4 * a + 2 * b][c], ddx);
          ddy = fmaf(wz[a] * wx[b], v[4 * a + 2 + b][c] - v[4 * a + b][c], ddy);
          ddz = fmaf(wy[a] * wx[b], v[4 + 2 * a + b][c] - v[2 * a + b][c], ddz);
        }
      }
      gx = fmaf(gv[c], ddx, gx);
      gy = fmaf(gv[c], ddy, gy);
      gz = fmaf(gv[c], ddz, gz);
    }
    gflow[pix * 3] = q.inside[0] ? gx : 0.0f;
    gflow[pix * 3 + 1] = q.inside[1] ? gy : 0.0f;
    gflow[pix * 3 + 2] = q.inside[2] ? gz : 0.0f;
  }
  if (acc) {
    int e = 0;
    (void)frexpf(gm, &e);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float w = ss_weight(q, k);
      unsigned long long* dst = reinterpret_cast<unsigned long long*>(acc + ss_corner(q, k, s, C));
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const long long add = llrint(ldexp(static_cast<double>(gv[c] * w), SS_FIXED_BITS - e));
        if (add != 0) atomicAdd(dst + c, static_cast<unsigned long long>(add));
      }
    }
  }
}

__global__ __launch_bounds__(SS_THREADS) void scale_space_fixed_to_float_kernel(const long long* __restrict__ acc,
                                                                                float* __restrict__ out, long long total,
                                                                                const float* __restrict__ gmax) {
  const long long k = static_cast<long long>(blockIdx.x) * SS_THREADS + threadIdx.x;
  if (k >= total) return;
  out[k] = ss_fixed_to_float(acc[k], ss_fixed_init(gmax));
}

// ------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------

int ss_validate(const char* name, int64_t n, int64_t h, int64_t w, int channels, int levels, SsShape* s) {
  if (channels < 1 || channels > SS_MAX_C) return fail("%s: channels must be in [1, %d], got %d", name, SS_MAX_C, channels);
  if (levels < 1 || levels > SS_MAX_LEVELS)
    return fail("%s: num_levels must be in [1, %d], got %d", name, SS_MAX_LEVELS, levels);
  if (h < 1 || h > SS_MAX_DIM || w < 1 || w > SS_MAX_DIM)
    return fail("%s: H and W must be in [1, %d], got %lld x %lld", name, SS_MAX_DIM, static_cast<long long>(h),
                static_cast<long long>(w));
  if (n < 0) return fail("%s: N must not be negative, got %lld", name, static_cast<long long>(n));
  const int64_t per = (levels + 1) * h * w * channels;        // < 9 * 2^28 * 8
  if (n > 0 && n >= ((1ll << 31) + per - 1) / per)
    return fail("%s: the volume must hold fewer than 2^31 elements, got %lld x %d x %lld x %lld x %d", name,
                static_cast<long long>(n), levels + 1, static_cast<long long>(h), static_cast<long long>(w), channels);
  *s = SsShape{static_cast<int>(n), static_cast<int>(h), static_cast<int>(w), channels, levels};
  return 0;
}

int ss_taps(const char* name, int levels, double sigma0, SsTaps* t) {
  if (!(sigma0 > 0.0) || !(sigma0 * static_cast<double>(1 << (levels - 1)) <= SS_MAX_SIGMA))
    return fail("%s: sigma0 must be positive and sigma0 * 2^(num_levels - 1) at most %d, got %g with %d levels", name,
                SS_MAX_SIGMA, sigma0, levels);
  *t = SsTaps{};
  int at = 0;
  for (int p = 0; p < levels; ++p) {
    const double sigma = sigma0 * static_cast<double>(1 << p);
    const int r = static_cast<int>(std::ceil(3.0 * sigma));
    if (r > SS_MAX_RADIUS || at + r + 1 > SS_MAX_TAPS) return fail("%s: the taps of %d levels do not fit", name, levels);
    t->off[p] = at;
    t->radius[p] = r;
    double cum = 0.0;
    for (int k = 0; k <= r; ++k) {
      const double w = std::exp(-static_cast<double>(k) * k / (2.0 * sigma * sigma));
      cum += w;
      t->w[at + k] = static_cast<float>(w);
      t->cum[at + k] = static_cast<float>(cum);
    }
    at += r + 1;
  }
  return 0;
}

bool ss_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int ss_volume_forward(const float* x, float* vol, SsShape s, const SsTaps& taps, hipStream_t st) {
  const int64_t per = static_cast<int64_t>(s.h) * s.w * s.c;
  DevBuf tmp;
  TFC_HIP(tmp.alloc(sizeof(float) * static_cast<size_t>(per * s.m * s.n), st));
  const int tiles_w = static_cast<int>(ceil_div(s.w, SS_ROW_TILE));
  const int tiles_x = static_cast<int>(ceil_div(static_cast<int64_t>(s.w) * s.c, SS_COL_TILE_X));
  const int tiles_h = static_cast<int>(ceil_div(s.h, SS_COL_TILE_H));
  const int64_t row_blocks = static_cast<int64_t>(s.n) * s.h * tiles_w;
  const int64_t col_blocks = static_cast<int64_t>(s.n) * s.m * tiles_h * tiles_x;
  if (row_blocks > 0x7fffffffll || col_blocks > 0x7fffffffll) return fail("tfc_scale_space_volume: too many tiles");
  KernelTimer timer("scale_space_volume", st);
  hipLaunchKernelGGL(scale_space_row_forward_kernel, dim3(static_cast<unsigned>(row_blocks)), dim3(SS_THREADS), 0, st, x,
                     vol, tmp.as<float>(), s, taps, tiles_w);
  hipLaunchKernelGGL((scale_space_col_kernel<false, false>), dim3(static_cast<unsigned>(col_blocks)), dim3(SS_THREADS), 0,
                     st, static_cast<const void*>(tmp.as<float>()), vol, static_cast<const float*>(nullptr), s, taps,
                     tiles_x, tiles_h);
  TFC_HIP(hipGetLastError());
  return 0;
}

// gsrc: the volume gradient as float (fixed = false) or as the integer sums with their max|g| (fixed = true)
int ss_volume_adjoint(const void* gsrc, bool fixed, const float* gmax, float* gx, SsShape s, const SsTaps& taps,
                      hipStream_t st) {
  const int64_t per = static_cast<int64_t>(s.h) * s.w * s.c;
  DevBuf tmp;
  TFC_HIP(tmp.alloc(sizeof(float) * static_cast<size_t>(per * s.m * s.n), st));
  const int tiles_w = static_cast<int>(ceil_div(s.w, SS_ROW_TILE));
  const int tiles_x = static_cast<int>(ceil_div(static_cast<int64_t>(s.w) * s.c, SS_COL_TILE_X));
  const int tiles_h = static_cast<int>(ceil_div(s.h, SS_COL_TILE_H));
  const int64_t row_blocks = static_cast<int64_t>(s.n) * s.h * tiles_w;
  const int64_t col_blocks = static_cast<int64_t>(s.n) * s.m * tiles_h * tiles_x;
  if (row_blocks > 0x7fffffffll || col_blocks > 0x7fffffffll)
    return fail("tfc_scale_space_volume_backward: too many tiles");
  KernelTimer timer("scale_space_volume_backward", st);
  const dim3 cg(static_cast<unsigned>(col_blocks)), rg(static_cast<unsigned>(row_blocks)), th(SS_THREADS);
  if (fixed) {
    hipLaunchKernelGGL((scale_space_col_kernel<true, true>), cg, th, 0, st, gsrc, tmp.as<float>(), gmax, s, taps, tiles_x,
                       tiles_h);
    hipLaunchKernelGGL(scale_space_row_adjoint_kernel<true>, rg, th, 0, st, gsrc,
                       static_cast<const float*>(tmp.as<float>()), gx, gmax, s, taps, tiles_w);
  } else {
    hipLaunchKernelGGL((scale_space_col_kernel<true, false>), cg, th, 0, st, gsrc, tmp.as<float>(), gmax, s, taps,
                       tiles_x, tiles_h);
    hipLaunchKernelGGL(scale_space_row_adjoint_kernel<false>, rg, th, 0, st, gsrc,
                       static_cast<const float*>(tmp.as<float>()), gx, gmax, s, taps, tiles_w);
  }
  TFC_HIP(hipGetLastError());
  return 0;
}

template <int C>
void ss_launch_warp_forward(const float* vol, const float* flow, float* out, SsShape s, unsigned blocks, hipStream_t st) {
  hipLaunchKernelGGL(scale_space_warp_forward_kernel<C>, dim3(blocks), dim3(SS_WARP_TILE), 0, st, vol, flow, out, s);
}

template <int C>
void ss_launch_warp_backward(const float* g, const float* vol, const float* flow, float* gflow, long long* acc,
                             const float* gmax, SsShape s, unsigned blocks, hipStream_t st) {
  hipLaunchKernelGGL(scale_space_warp_backward_kernel<C>, dim3(blocks), dim3(SS_WARP_TILE), 0, st, g, vol, flow, gflow,
                     acc, gmax, s);
}

#define SS_DISPATCH_C(channels, call) \
  switch (channels) {                 \
    case 1: call(1); break;           \
    case 2: call(2); break;           \
    case 3: call(3); break;           \
    case 4: call(4); break;           \
    case 5: call(5); break;           \
    case 6: call(6); break;           \
    case 7: call(7); break;           \
    default: call(8); break;          \
  }

}  // namespace
}  // namespace tfc

extern "C" int64_t tfc_scale_space_workspace(int64_t n, int64_t h, int64_t w, int channels, int num_levels) {
  using namespace tfc;
  SsShape s;
  if (ss_validate("tfc_scale_space_workspace", n, h, w, channels, num_levels, &s)) return -1;
  return 8 * n * (num_levels + 1) * h * w * channels;
}

extern "C" int tfc_scale_space_volume(const float* x, float* volume, int64_t n, int64_t h, int64_t w, int channels,
                                      int num_levels, double sigma0, void* stream) {
  using namespace tfc;
  SsShape s;
  SsTaps taps;
  if (int rc = ss_validate("tfc_scale_space_volume", n, h, w, channels, num_levels, &s)) return rc;
  if (int rc = ss_taps("tfc_scale_space_volume", num_levels, sigma0, &taps)) return rc;
  if (n == 0) return 0;
  if (!x || !volume) return fail("tfc_scale_space_volume: x and volume must not be null");
  if (!ss_aligned(x) || !ss_aligned(volume)) return fail("tfc_scale_space_volume: x and volume must be 16-byte aligned");
  return ss_volume_forward(x, volume, s, taps, static_cast<hipStream_t>(stream));
}

extern "C" int tfc_scale_space_volume_backward(const float* g_volume, float* g_x, int64_t n, int64_t h, int64_t w,
                                               int channels, int num_levels, double sigma0, void* stream) {
  using namespace tfc;
  SsShape s;
  SsTaps taps;
  if (int rc = ss_validate("tfc_scale_space_volume_backward", n, h, w, channels, num_levels, &s)) return rc;
  if (int rc = ss_taps("tfc_scale_space_volume_backward", num_levels, sigma0, &taps)) return rc;
  if (n == 0) return 0;
  if (!g_volume || !g_x) return fail("tfc_scale_space_volume_backward: g_volume and g_x must not be null");
  if (!ss_aligned(g_volume) || !ss_aligned(g_x))
    return fail("tfc_scale_space_volume_backward: g_volume and g_x must be 16-byte aligned");
  return ss_volume_adjoint(g_volume, false, nullptr, g_x, s, taps, static_cast<hipStream_t>(stream));
}

extern "C" int tfc_scale_space_warp_forward(const float* volume, const float* flow, float* out, int64_t n, int64_t h,
                                            int64_t w, int channels, int num_levels, void* stream) {
  using namespace tfc;
  SsShape s;
  if (int rc = ss_validate("tfc_scale_space_warp_forward", n, h, w, channels, num_levels, &s)) return rc;
  if (n == 0) return 0;
  if (!volume || !flow || !out) return fail("tfc_scale_space_warp_forward: volume, flow and out must not be null");
  if (!ss_aligned(volume) || !ss_aligned(flow) || !ss_aligned(out))
    return fail("tfc_scale_space_warp_forward: volume, flow and out must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned blocks = static_cast<unsigned>(ceil_div(n * h * w, SS_WARP_TILE));
  KernelTimer timer("scale_space_warp_forward", st);
#define SS_CALL(CC) ss_launch_warp_forward<CC>(volume, flow, out, s, blocks, st)
  SS_DISPATCH_C(channels, SS_CALL)
#undef SS_CALL
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_scale_space_warp_backward(const float* g, const float* volume, const float* flow, float* g_flow,
                                             float* g_volume, float* g_x, double sigma0, int64_t n, int64_t h, int64_t w,
                                             int channels, int num_levels, void* stream) {
  using namespace tfc;
  SsShape s;
  SsTaps taps;
  const char* name = "tfc_scale_space_warp_backward";
  if (int rc = ss_validate(name, n, h, w, channels, num_levels, &s)) return rc;
  if (g_x)
    if (int rc = ss_taps(name, num_levels, sigma0, &taps)) return rc;
  const bool scatter = g_volume || g_x;
  if (scatter && h * w > (1ll << SS_MAX_HW_LOG2))
    return fail("%s: the volume gradient needs H * W <= 2^%d (a 64-bit sum of H * W contributions below 2^%d), got "
                "%lld x %lld", name, SS_MAX_HW_LOG2, SS_FIXED_BITS, static_cast<long long>(h), static_cast<long long>(w));
  if (n == 0 || (!g_flow && !scatter)) return 0;
  if (!g || !flow) return fail("%s: g and flow must not be null", name);
  if (g_flow && !volume) return fail("%s: the flow gradient needs the volume", name);
  if (!ss_aligned(g) || !ss_aligned(flow) || !ss_aligned(volume) || !ss_aligned(g_flow) || !ss_aligned(g_volume) ||
      !ss_aligned(g_x))
    return fail("%s: every tensor must be 16-byte aligned", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t pixels = n * h * w;
  const int64_t total = pixels * (num_levels + 1) * channels;
  DevBuf red, fixed;
  TFC_HIP(red.alloc(sizeof(float) * (SS_MAX_PARTS + 1), st));
  float* parts = red.as<float>();
  float* gmax = parts + SS_MAX_PARTS;
  if (scatter) {
    TFC_HIP(fixed.alloc(sizeof(long long) * static_cast<size_t>(total), st));
    TFC_HIP(hipMemsetAsync(fixed.p, 0, sizeof(long long) * static_cast<size_t>(total), st));
  }
  const int nparts = static_cast<int>(std::min<int64_t>(SS_MAX_PARTS, ceil_div(pixels * channels, 4 * SS_THREADS)));
  const unsigned blocks = static_cast<unsigned>(ceil_div(pixels, SS_WARP_TILE));
  {
    KernelTimer timer("scale_space_warp_backward", st);
    hipLaunchKernelGGL(scale_space_absmax_kernel, dim3(static_cast<unsigned>(nparts)), dim3(SS_THREADS), 0, st, g,
                       static_cast<long long>(pixels * channels), parts);
    hipLaunchKernelGGL(scale_space_absmax_final_kernel, dim3(1), dim3(SS_THREADS), 0, st,
                       static_cast<const float*>(parts), nparts, gmax);
#define SS_CALL(CC) \
  ss_launch_warp_backward<CC>(g, volume, flow, g_flow, fixed.as<long long>(), static_cast<const float*>(gmax), s, blocks, st)
    SS_DISPATCH_C(channels, SS_CALL)
#undef SS_CALL
    if (g_volume)
      hipLaunchKernelGGL(scale_space_fixed_to_float_kernel, dim3(static_cast<unsigned>(ceil_div(total, SS_THREADS))),
                         dim3(SS_THREADS), 0, st, static_cast<const long long*>(fixed.as<long long>()), g_volume,
                         static_cast<long long>(total), static_cast<const float*>(gmax));
    TFC_HIP(hipGetLastError());
  }
  if (g_x) return ss_volume_adjoint(fixed.p, true, gmax, g_x, s, taps, st);
  return 0;
}
