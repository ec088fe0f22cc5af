// What HiFiC's discriminator (models/hific/archs.py:300-372) and its GAN loss need around the convolutions, for gfx950:
// spectral normalisation of a kernel, the latent-conditioning front end, leaky ReLU with its backward, and the
// non-saturating loss.  compare_gan, where the reference takes these from, is not part of the reference tree; the
// definitions are the ones include/tfc_hip.h states at each entry point.
//
// Everything here is float32 arithmetic on float32 or bfloat16 activations, any size, wave64, and has no float atomics:
// every sum is taken in an order that depends only on the shapes (per-thread strided sums, a fixed LDS tree, ordered
// partials through reduce_rows.h), so two calls on the same input give the same bits.
//
// Spectral norm, W [R, C] row-major, u [R]:
//   t = W^T u    sn_wtu_kernel: a workgroup owns 16 rows and all columns, partial [R / 16, C]; sum_rows_kernel adds them
//   s = W v      sn_rowdot_kernel: v = t rsqrt(max(|t|^2, eps)) is formed by every workgroup from t (C values, the same
//                order everywhere, hence the same bits); one wave per row
//   W / sigma    sn_scale_kernel: u' = s rsqrt(max(|s|^2, eps)) and sigma = u'^T s (= u'^T W v) are formed by every
//                workgroup from s (R values), then the division
// The chain v -> u' -> sigma needs ALL of W before each next step, so W is read three times; it is at most 8 MB, and
// only the first read comes from HBM (the other two find it in the 256 MB Infinity Cache).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/tfc_hip.h"
#include "bf16_io.h"
#include "common.h"
#include "reduce_rows.h"

namespace tfc {
namespace {

constexpr float kSnEps = 1e-12f;
constexpr float kSlope = 0.2f;
constexpr int kSnRows = 16;          // rows of W per workgroup of sn_wtu_kernel

// max(x, 0.2 x): a positive slope keeps the sign
__device__ inline float lrelu(float v) { return fmaxf(v, kSlope * v); }

// Sum of one value per thread over a workgroup of 256, the same bits in every thread and for every workgroup that holds
// the same values: lanes by xor shuffles (both sides add the same two numbers), then the four wave sums in order.
__device__ inline float block_sum_256(float v, float* lds4) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();                    // lds4 may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// sum_i a[i] * b[i], i < n, by a workgroup of 256: thread k takes i = k, k + 256, ... in order.
__device__ inline float block_dot_256(const float* a, const float* b, long long n, float* lds4) {
  float s = 0.f;
  for (long long i = threadIdx.x; i < n; i += 256) s = fmaf(a[i], b[i], s);
  return block_sum_256(s, lds4);
}

// part[blockIdx.x][c] = sum over the workgroup's 16 rows of W[r, c] u[r]; block (64, 4): 64 columns x 4 row phases.
__global__ void __launch_bounds__(256) sn_wtu_kernel(const float* w, const float* u, long long R, int C, float* part) {
  __shared__ float lds[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long long r0 = static_cast<long long>(blockIdx.x) * kSnRows;
  for (int c0 = 0; c0 < C; c0 += 64) {
    const int c = c0 + tx;
    float s = 0.f;
    if (c < C) {
#pragma unroll
      for (int k = 0; k < kSnRows / 4; ++k) {
        const long long r = r0 + ty + 4 * k;
        if (r < R) s = fmaf(w[r * C + c], u[r], s);
      }
    }
    __syncthreads();
    lds[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && c < C) part[static_cast<long long>(blockIdx.x) * C + c] = ((lds[0][tx] + lds[1][tx]) + lds[2][tx]) + lds[3][tx];
  }
}

// s[r] = sum_c W[r, c] v[c], v = t rsqrt(max(sum t^2, eps)); workgroup 0 also writes v.
__global__ void __launch_bounds__(256) sn_rowdot_kernel(const float* w, const float* t, long long R, int C, float* v_out,
                                                        float* s) {
  __shared__ float lds4[4];
  const float tt = block_dot_256(t, t, C, lds4);
  const float inv = rsqrtf(fmaxf(tt, kSnEps));
  if (blockIdx.x == 0)
    for (int c = threadIdx.x; c < C; c += 256) v_out[c] = t[c] * inv;
  const int lane = threadIdx.x & 63;
  const long long wave = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const long long nwaves = static_cast<long long>(gridDim.x) * 4;
  for (long long r = wave; r < R; r += nwaves) {
    float a = 0.f;
    for (int c = lane; c < C; c += 64) a = fmaf(w[r * C + c], t[c] * inv, a);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);
    if (lane == 0) s[r] = a;
  }
}

// out = W / sigma; workgroup 0 also writes u' and sigma.
__global__ void __launch_bounds__(256) sn_scale_kernel(const float* w, const float* s, long long R, int C, float* out,
                                                       float* u_out, float* sigma_out) {
  __shared__ float lds4[4];
  const float ss = block_dot_256(s, s, R, lds4);
  const float inv = rsqrtf(fmaxf(ss, kSnEps));
  float part = 0.f;                                       // sigma = sum_r u'[r] s[r]
  for (long long r = threadIdx.x; r < R; r += 256) part = fmaf(s[r] * inv, s[r], part);
  const float sigma = block_sum_256(part, lds4);
  if (blockIdx.x == 0) {
    for (long long r = threadIdx.x; r < R; r += 256) u_out[r] = s[r] * inv;
    if (threadIdx.x == 0) *sigma_out = sigma;
  }
  const long long n = R * C, stride = static_cast<long long>(gridDim.x) * 256;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) out[i] = w[i] / sigma;
}

// part[blockIdx.x] = the workgroup's share of <G, W>: element i = (blockIdx.x * 256 + thread) + k * stride, in order.
__global__ void __launch_bounds__(256) sn_inner_kernel(const float* g, const float* w, long long n, float* part) {
  __shared__ float lds4[4];
  float a = 0.f;
  const long long stride = static_cast<long long>(gridDim.x) * 256;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) a = fmaf(g[i], w[i], a);
  a = block_sum_256(a, lds4);
  if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// dW = G / sigma - (<G, W> / sigma^2) u' v^T; every workgroup adds the `parts` partials in the same order.
__global__ void __launch_bounds__(256) sn_backward_kernel(const float* g, const float* part, int parts, const float* u,
                                                          const float* v, const float* sigma_p, long long R, int C,
                                                          float* dw) {
  __shared__ float lds4[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < parts; i += 256) a += part[i];
  const float inner = block_sum_256(a, lds4);
  const float sigma = *sigma_p;
  const float k = inner / (sigma * sigma);
  const long long n = R * C, stride = static_cast<long long>(gridDim.x) * 256;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) {
    const long long r = i / C;
    const int c = static_cast<int>(i - r * C);
    dw[i] = g[i] / sigma - k * (u[r] * v[c]);
  }
}

// Nearest-neighbour source index: min(floor((2 d + 1) in / (2 out)), in - 1).  Axes are at most 2^15 long (checked on the
// host), so the products stay below 2^32.
__device__ inline int nearest_src(int d, int in, int out) {
  const unsigned int q = (2u * d + 1u) * static_cast<unsigned int>(in) / (2u * out);
  return static_cast<int>(q < static_cast<unsigned int>(in - 1) ? q : in - 1);
}
// The first destination index whose source is >= s (s = in gives out).
__device__ inline int nearest_first(int s, int in, int out) {
  if (s <= 0) return 0;
  const unsigned int d = (2u * out * s + static_cast<unsigned int>(in) - 1u) / (2u * in);   // ceil((2 out s - in) / (2 in))
  return static_cast<int>(d > static_cast<unsigned int>(out) ? out : d);
}

struct FrontParams {
  const void* x;       // [N, H, W, cx]
  const void* lat;     // [N, h, w, cl]: the latent branch's convolution output (before the leaky ReLU)
  void* out;           // forward: [N, H, W, P]
  const void* g;       // backward: [N, H, W, P]
  void* dx;            // backward: [N, H, W, cx]
  void* dlat;          // backward: [N, h, w, cl]
  long long N;
  int H, W, h, w, cx, cl, P;
};

// One thread per (destination pixel, group of four channels): one 16-byte (float32) or 8-byte (bfloat16) store.
// grid.x covers a row's W * P / 4 stores, grid.y walks the N * H rows: the column's source index is computed once per
// thread, the row's once per workgroup, and no 64-bit division is left per element.
template <bool BF16>
__global__ void __launch_bounds__(256) front_forward_kernel(FrontParams p) {
  const unsigned int groups = p.P >> 2;
  const unsigned int per_row = p.W * groups;
  const unsigned int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= per_row) return;
  const unsigned int xw = j / groups;
  const int c0 = static_cast<int>(j - xw * groups) * 4;
  const int sx = nearest_src(static_cast<int>(xw), p.w, p.W);
  const long long rows = p.N * p.H;
  for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
    const long long n = row / p.H;
    const int yh = static_cast<int>(row - n * p.H);
    const long long src = (n * p.h + nearest_src(yh, p.h, p.H)) * p.w + sx;
    const long long pix = row * p.W + xw;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c0 + e;
      if (c < p.cx) v[e] = load<BF16>(p.x, pix * p.cx + c);
      else if (c < p.cx + p.cl) v[e] = lrelu(load<BF16>(p.lat, src * p.cl + (c - p.cx)));
      else v[e] = 0.f;
    }
    const long long at = row * per_row + j;
    if (BF16) {
      uint2 o;
      o.x = float_to_bf16_bits(v[0]) | (static_cast<unsigned int>(float_to_bf16_bits(v[1])) << 16);
      o.y = float_to_bf16_bits(v[2]) | (static_cast<unsigned int>(float_to_bf16_bits(v[3])) << 16);
      static_cast<uint2*>(p.out)[at] = o;
    } else {
      static_cast<float4*>(p.out)[at] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// One wave per SOURCE pixel.  Lane = (phase q = lane / 16, channel c = lane % 16): the wave walks the pixel's replicas
// (a rectangle of the destination, row-major) four at a time, phase q taking replicas q, q + 4, ...; lanes c < cx copy
// dx, lanes cx <= c < cx + cl add up.  The four phase sums are combined as (q0 + q2) + (q1 + q3).  cx + cl <= 16.
template <bool BF16>
__global__ void __launch_bounds__(256) front_backward_kernel(FrontParams p) {
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const long long wave = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const long long nwaves = static_cast<long long>(gridDim.x) * 4;
  const long long sources = p.N * p.h * p.w;
  const bool is_x = c < p.cx, is_lat = c >= p.cx && c < p.cx + p.cl;
  for (long long sp = wave; sp < sources; sp += nwaves) {
    const int sx = static_cast<int>(sp % p.w);
    const long long t = sp / p.w;
    const int sy = static_cast<int>(t % p.h);
    const long long n = t / p.h;
    const int y0 = nearest_first(sy, p.h, p.H), y1 = nearest_first(sy + 1, p.h, p.H);
    const int x0 = nearest_first(sx, p.w, p.W), x1 = nearest_first(sx + 1, p.w, p.W);
    const int ww = x1 - x0, count = (y1 - y0) * ww;
    float acc = 0.f;
    for (int k = q; k < count; k += 4) {
      const int dy = k / ww, dxx = k - dy * ww;
      const long long pix = (n * p.H + y0 + dy) * p.W + x0 + dxx;
      if (is_x || is_lat) {
        const float gv = load<BF16>(p.g, pix * p.P + c);
        if (is_x) store<BF16>(p.dx, pix * p.cx + c, gv);
        else acc += gv;
      }
    }
    acc += __shfl_xor(acc, 32);
    acc += __shfl_xor(acc, 16);
    if (is_lat && q == 0) {
      const long long at = sp * p.cl + (c - p.cx);
      const float lv = load<BF16>(p.lat, at);
      store<BF16>(p.dlat, at, acc * (lv > 0.f ? 1.f : kSlope));
    }
  }
}

template <bool BF16>
__global__ void __launch_bounds__(256) lrelu_forward_kernel(void* y, long long n) {
  const long long stride = static_cast<long long>(gridDim.x) * 256;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride)
    store<BF16>(y, i, lrelu(load<BF16>(y, i)));
}

// The same, 16 bytes per thread and step (y 16-byte aligned, `groups` whole groups of 4 float32 / 8 bfloat16 values).
template <bool BF16>
__global__ void __launch_bounds__(256) lrelu_forward_vec_kernel(uint4* y, long long groups) {
  const long long stride = static_cast<long long>(gridDim.x) * 256;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < groups; i += stride) {
    uint4 raw = y[i];
    unsigned int w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (BF16) {
        const float lo = lrelu(__uint_as_float(w[k] << 16)), hi = lrelu(__uint_as_float(w[k] & 0xFFFF0000u));
        w[k] = float_to_bf16_bits(lo) | (static_cast<unsigned int>(float_to_bf16_bits(hi)) << 16);
      } else {
        w[k] = __float_as_uint(lrelu(__uint_as_float(w[k])));
      }
    }
    y[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// gm = gy * (masked && y <= 0 ? 0.2 : 1) and part[blockIdx.x][c] = the sum of gm over the workgroup's pixels.
// Block (64 channels, 4 pixel phases); a workgroup owns `rows` consecutive pixels; phase j takes pixels j, j + 4, ...
template <bool BF16>
__global__ void __launch_bounds__(256) lrelu_backward_kernel(const void* gy, const void* y, void* gm, float* part,
                                                             long long pixels, int C, int rows, int masked) {
  __shared__ float lds[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long long p0 = static_cast<long long>(blockIdx.x) * rows;
  const long long p1 = p0 + rows < pixels ? p0 + rows : pixels;
  for (int c0 = 0; c0 < C; c0 += 64) {
    const int c = c0 + tx;
    float s = 0.f;
    if (c < C) {
      for (long long px = p0 + ty; px < p1; px += 4) {
        const long long at = px * C + c;
        float g = load<BF16>(gy, at);
        if (masked) g = g * (load<BF16>(y, at) > 0.f ? 1.f : kSlope);
        if (gm) store<BF16>(gm, at, g);
        s += g;
      }
    }
    __syncthreads();
    lds[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && c < C && part) part[static_cast<long long>(blockIdx.x) * C + c] = ((lds[0][tx] + lds[1][tx]) + lds[2][tx]) + lds[3][tx];
  }
}

// The same with 16 bytes per thread and step: C is a power of two times VEC (4 float32 / 8 bfloat16 values) with at most
// 256 such groups per row, pointers 16-byte aligned.  Thread t owns channel group t % groups and row phase t / groups;
// the phases' sums meet in LDS and are added in phase order.
template <bool BF16>
__global__ void __launch_bounds__(256) lrelu_backward_vec_kernel(const uint4* gy, const uint4* y, uint4* gm, float* part,
                                                                 long long pixels, int C, int rows, int masked) {
  constexpr int VEC = BF16 ? 8 : 4;
  __shared__ float lds[256][VEC + 1];
  const int groups = C / VEC;
  const int cg = threadIdx.x % groups, phase = threadIdx.x / groups, phases = 256 / groups;
  const long long p0 = static_cast<long long>(blockIdx.x) * rows;
  const long long p1 = p0 + rows < pixels ? p0 + rows : pixels;
  float acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
  for (long long px = p0 + phase; px < p1; px += phases) {
    const long long at = px * groups + cg;
    const uint4 graw = gy[at];
    const unsigned int gw[4] = {graw.x, graw.y, graw.z, graw.w};
    unsigned int yw[4] = {0u, 0u, 0u, 0u};
    if (masked) {
      const uint4 yraw = y[at];
      yw[0] = yraw.x; yw[1] = yraw.y; yw[2] = yraw.z; yw[3] = yraw.w;
    }
    unsigned int ow[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (BF16) {
        float lo = __uint_as_float(gw[k] << 16), hi = __uint_as_float(gw[k] & 0xFFFF0000u);
        if (masked) {
          lo = lo * (__uint_as_float(yw[k] << 16) > 0.f ? 1.f : kSlope);
          hi = hi * (__uint_as_float(yw[k] & 0xFFFF0000u) > 0.f ? 1.f : kSlope);
        }
        acc[2 * k] += lo;
        acc[2 * k + 1] += hi;
        ow[k] = float_to_bf16_bits(lo) | (static_cast<unsigned int>(float_to_bf16_bits(hi)) << 16);
      } else {
        float g = __uint_as_float(gw[k]);
        if (masked) g = g * (__uint_as_float(yw[k]) > 0.f ? 1.f : kSlope);
        acc[k] += g;
        ow[k] = __float_as_uint(g);
      }
    }
    if (gm) gm[at] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
  }
  if (!part) return;
#pragma unroll
  for (int e = 0; e < VEC; ++e) lds[threadIdx.x][e] = acc[e];
  __syncthreads();
  if (phase == 0) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float t = 0.f;
      for (int r = 0; r < phases; ++r) t += lds[r * groups + cg][e];
      part[static_cast<long long>(blockIdx.x) * C + cg * VEC + e] = t;
    }
  }
}

__device__ inline float sigmoid_stable(float x) {
  if (x >= 0.f) return 1.f / (1.f + expf(-x));
  const float e = expf(x);
  return e / (1.f + e);
}
__device__ inline float softplus_neg_abs(float x) { return log1pf(expf(-fabsf(x))); }

// One workgroup of 1024: out = {d_loss, g_loss, mean sigmoid(real), mean sigmoid(fake)}; logits [2 M], real first.
template <bool BF16>
__global__ void __launch_bounds__(1024) gan_loss_forward_kernel(const void* logits, long long M, float* out) {
  __shared__ float lds[4][16];
  float a[4] = {0.f, 0.f, 0.f, 0.f};      // sce(real, 1), sce(fake, 0), sce(fake, 1), (unused)
  float pr = 0.f, pf = 0.f;
  for (long long i = threadIdx.x; i < M; i += 1024) {
    const float r = load<BF16>(logits, i), f = load<BF16>(logits, M + i);
    a[0] += fmaxf(r, 0.f) - r + softplus_neg_abs(r);
    a[1] += fmaxf(f, 0.f) + softplus_neg_abs(f);
    a[2] += fmaxf(f, 0.f) - f + softplus_neg_abs(f);
    pr += 1.f / (1.f + expf(-r));
    pf += 1.f / (1.f + expf(-f));
  }
  float vals[4] = {a[0] + a[1], a[2], pr, pf};
  // d_loss = (sum sce(real, 1) + sum sce(fake, 0)) / M: the two means have the same count
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v = vals[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) lds[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += lds[threadIdx.x][k];
    out[threadIdx.x] = t / static_cast<float>(M);
  }
}

// grad[i] = *scale * (sigmoid(x) - z) / M; mode 0 (d_loss): real z = 1, fake z = 0; mode 1 (g_loss): real 0, fake z = 1.
// sigmoid(x) - 1 is taken as -sigmoid(-x).
template <bool BF16>
__global__ void __launch_bounds__(256) gan_loss_backward_kernel(const void* logits, const float* scale, long long M,
                                                                int mode, void* grad) {
  const float k = *scale / static_cast<float>(M);
  const long long stride = static_cast<long long>(gridDim.x) * 256;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < 2 * M; i += stride) {
    const float x = load<BF16>(logits, i);
    const bool real = i < M;
    float gsc;
    if (mode == 0) gsc = real ? -sigmoid_stable(-x) : sigmoid_stable(x);
    else gsc = real ? 0.f : -sigmoid_stable(-x);
    store<BF16>(grad, i, k * gsc);
  }
}

unsigned hg_blocks(long long items, long long per_block) {
  return static_cast<unsigned>(std::max<long long>(1, std::min<long long>(ceil_div(items, per_block), 2048)));
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_spectral_norm_forward(const float* w, const float* u, int64_t rows, int64_t cols, float* w_sn,
                                         float* u_out, float* v_out, float* sigma, void* stream) {
  using namespace tfc;
  if (rows < 1 || rows > (1ll << 24)) return fail("tfc_spectral_norm_forward: rows must be in [1, 2^24], got %lld", static_cast<long long>(rows));
  if (cols < 1 || cols > (1 << 16)) return fail("tfc_spectral_norm_forward: cols must be in [1, 65536], got %lld", static_cast<long long>(cols));
  if (!w || !u || !w_sn || !u_out || !v_out || !sigma) return fail("tfc_spectral_norm_forward: null tensor");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int C = static_cast<int>(cols);
  const long long nblk = ceil_div(rows, kSnRows);
  DevBuf work;                                            // partials [nblk, C], t [C], s [rows]
  TFC_HIP(work.alloc(sizeof(float) * (nblk * C + C + rows), st));
  float* part = work.as<float>();
  float* t = part + nblk * C;
  float* s = t + C;
  KernelTimer timer("spectral_norm_forward", st);
  TFC_HIP(hipMemsetAsync(t, 0, sizeof(float) * C, st));
  hipLaunchKernelGGL(sn_wtu_kernel, dim3(static_cast<unsigned>(nblk)), dim3(256), 0, st, w, u, static_cast<long long>(rows), C, part);
  launch_sum_rows(part, nblk, C, C, t, st);
  hipLaunchKernelGGL(sn_rowdot_kernel, dim3(hg_blocks(rows, 4)), dim3(256), 0, st, w, t, static_cast<long long>(rows), C, v_out, s);
  hipLaunchKernelGGL(sn_scale_kernel, dim3(hg_blocks(rows * cols, 1024)), dim3(256), 0, st, w, s, static_cast<long long>(rows), C, w_sn,
                     u_out, sigma);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_spectral_norm_backward(const float* g, const float* w, const float* u, const float* v,
                                          const float* sigma, int64_t rows, int64_t cols, float* dw, void* stream) {
  using namespace tfc;
  if (rows < 1 || rows > (1ll << 24)) return fail("tfc_spectral_norm_backward: rows must be in [1, 2^24], got %lld", static_cast<long long>(rows));
  if (cols < 1 || cols > (1 << 16)) return fail("tfc_spectral_norm_backward: cols must be in [1, 65536], got %lld", static_cast<long long>(cols));
  if (!g || !w || !u || !v || !sigma || !dw) return fail("tfc_spectral_norm_backward: null tensor");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned blocks = hg_blocks(rows * cols, 1024);
  DevBuf part;
  TFC_HIP(part.alloc(sizeof(float) * blocks, st));
  KernelTimer timer("spectral_norm_backward", st);
  hipLaunchKernelGGL(sn_inner_kernel, dim3(blocks), dim3(256), 0, st, g, w, static_cast<long long>(rows * cols), part.as<float>());
  hipLaunchKernelGGL(sn_backward_kernel, dim3(blocks), dim3(256), 0, st, g, part.as<float>(), static_cast<int>(blocks), u, v, sigma,
                     static_cast<long long>(rows), static_cast<int>(cols), dw);
  TFC_HIP(hipGetLastError());
  return 0;
}

namespace tfc {
namespace {
int front_validate(const char* name, int dtype, int64_t n, int64_t H, int64_t W, int64_t h, int64_t w, int cx, int cl,
                   int P) {
  if (int rc = check_dtype(name, dtype)) return rc;
  if (n < 0 || H < 1 || W < 1 || h < 1 || w < 1 || H > (1 << 15) || W > (1 << 15) || h > (1 << 15) || w > (1 << 15))
    return fail("%s: sizes must be positive and at most 2^15 per axis", name);
  if (cx < 1 || cl < 1 || cx + cl > 16)
    return fail("%s: image and latent channels must be positive and at most 16 together, got %d + %d", name, cx, cl);
  if (P < cx + cl || P % 4 != 0 || P > 1024)
    return fail("%s: padded_channels must be a multiple of 4, at least %d and at most 1024, got %d", name, cx + cl, P);
  return 0;
}
}  // namespace
}  // namespace tfc

extern "C" int tfc_disc_front_forward(const void* x, const void* latent, void* out, int dtype, int64_t n, int64_t height,
                                      int64_t width, int64_t latent_height, int64_t latent_width, int image_channels,
                                      int latent_channels, int padded_channels, void* stream) {
  using namespace tfc;
  if (int rc = front_validate("tfc_disc_front_forward", dtype, n, height, width, latent_height, latent_width,
                              image_channels, latent_channels, padded_channels)) return rc;
  if (n == 0) return 0;
  if (!x || !latent || !out) return fail("tfc_disc_front_forward: null tensor");
  FrontParams p = {};
  p.x = x; p.lat = latent; p.out = out; p.N = n;
  p.H = static_cast<int>(height); p.W = static_cast<int>(width);
  p.h = static_cast<int>(latent_height); p.w = static_cast<int>(latent_width);
  p.cx = image_channels; p.cl = latent_channels; p.P = padded_channels;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(ceil_div(width * (padded_channels / 4), 256)),
                  static_cast<unsigned>(std::min<long long>(n * height, 65535)));
  KernelTimer timer("disc_front_forward", st);
  if (dtype == 1) hipLaunchKernelGGL(front_forward_kernel<true>, grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(front_forward_kernel<false>, grid, dim3(256), 0, st, p);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_disc_front_backward(const void* g, const void* latent, void* dx, void* dlatent, int dtype, int64_t n,
                                       int64_t height, int64_t width, int64_t latent_height, int64_t latent_width,
                                       int image_channels, int latent_channels, int padded_channels, void* stream) {
  using namespace tfc;
  if (int rc = front_validate("tfc_disc_front_backward", dtype, n, height, width, latent_height, latent_width,
                              image_channels, latent_channels, padded_channels)) return rc;
  if (n == 0) return 0;
  if (!g || !latent || !dx || !dlatent) return fail("tfc_disc_front_backward: null tensor");
  FrontParams p = {};
  p.g = g; p.lat = latent; p.dx = dx; p.dlat = dlatent; p.N = n;
  p.H = static_cast<int>(height); p.W = static_cast<int>(width);
  p.h = static_cast<int>(latent_height); p.w = static_cast<int>(latent_width);
  p.cx = image_channels; p.cl = latent_channels; p.P = padded_channels;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned blocks = hg_blocks(n * latent_height * latent_width, 4);
  KernelTimer timer("disc_front_backward", st);
  if (dtype == 1) hipLaunchKernelGGL(front_backward_kernel<true>, dim3(blocks), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(front_backward_kernel<false>, dim3(blocks), dim3(256), 0, st, p);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_lrelu_forward(void* y, int dtype, int64_t count, void* stream) {
  using namespace tfc;
  if (int rc = check_dtype("tfc_lrelu_forward", dtype)) return rc;
  if (count < 0) return fail("tfc_lrelu_forward: count must be non-negative, got %lld", static_cast<long long>(count));
  if (count == 0) return 0;
  if (!y) return fail("tfc_lrelu_forward: null tensor");
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer("lrelu_forward", st);
  const int per = dtype == 1 ? 8 : 4;
  long long done = 0;
  if (reinterpret_cast<uintptr_t>(y) % 16 == 0 && count >= per) {
    const long long groups = count / per;
    const unsigned blocks = hg_blocks(groups, 1024);
    if (dtype == 1) hipLaunchKernelGGL(lrelu_forward_vec_kernel<true>, dim3(blocks), dim3(256), 0, st, static_cast<uint4*>(y), groups);
    else hipLaunchKernelGGL(lrelu_forward_vec_kernel<false>, dim3(blocks), dim3(256), 0, st, static_cast<uint4*>(y), groups);
    done = groups * per;
  }
  if (done < count) {
    void* const rest = static_cast<char*>(y) + done * dtype_bytes(dtype);
    const unsigned blocks = hg_blocks(count - done, 1024);
    if (dtype == 1) hipLaunchKernelGGL(lrelu_forward_kernel<true>, dim3(blocks), dim3(256), 0, st, rest, static_cast<long long>(count - done));
    else hipLaunchKernelGGL(lrelu_forward_kernel<false>, dim3(blocks), dim3(256), 0, st, rest, static_cast<long long>(count - done));
  }
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_lrelu_bias_backward(const void* gy, const void* y, void* gm, float* dbias, int dtype, int64_t pixels,
                                       int64_t channels, int masked, void* stream) {
  using namespace tfc;
  if (int rc = check_dtype("tfc_lrelu_bias_backward", dtype)) return rc;
  if (pixels < 0) return fail("tfc_lrelu_bias_backward: pixels must be non-negative, got %lld", static_cast<long long>(pixels));
  if (channels < 1 || channels > (1 << 24))
    return fail("tfc_lrelu_bias_backward: channels must be in [1, 2^24], got %lld", static_cast<long long>(channels));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dbias) TFC_HIP(hipMemsetAsync(dbias, 0, sizeof(float) * channels, st));
  if (pixels == 0) return 0;
  if (!gy || (masked && (!y || !gm))) return fail("tfc_lrelu_bias_backward: null tensor");
  if (!masked && !dbias) return 0;
  const int C = static_cast<int>(channels);
  const int vec = dtype == 1 ? 8 : 4;
  const int groups = C % vec == 0 ? C / vec : 0;
  bool aligned = reinterpret_cast<uintptr_t>(gy) % 16 == 0;
  if (masked) aligned = aligned && reinterpret_cast<uintptr_t>(y) % 16 == 0 && reinterpret_cast<uintptr_t>(gm) % 16 == 0;
  const bool vector = aligned && groups >= 1 && groups <= 256 && (groups & (groups - 1)) == 0;
  // at most 1024 workgroups, at least 16 pixels each (vector kernel: 256 / groups rows are in flight at once)
  const int rows = static_cast<int>(std::max<long long>(vector ? std::max(16, 4 * (256 / groups)) : 16, ceil_div(pixels, 1024)));
  const long long nblk = ceil_div(pixels, rows);
  DevBuf part;
  if (dbias) TFC_HIP(part.alloc(sizeof(float) * nblk * C, st));
  KernelTimer timer("lrelu_bias_backward", st);
  void* const out = masked ? gm : nullptr;
  const dim3 grid(static_cast<unsigned>(nblk));
  if (vector) {
    const uint4* const g4 = static_cast<const uint4*>(gy);
    const uint4* const y4 = static_cast<const uint4*>(y);
    if (dtype == 1)
      hipLaunchKernelGGL(lrelu_backward_vec_kernel<true>, grid, dim3(256), 0, st, g4, y4, static_cast<uint4*>(out),
                         part.as<float>(), static_cast<long long>(pixels), C, rows, masked ? 1 : 0);
    else
      hipLaunchKernelGGL(lrelu_backward_vec_kernel<false>, grid, dim3(256), 0, st, g4, y4, static_cast<uint4*>(out),
                         part.as<float>(), static_cast<long long>(pixels), C, rows, masked ? 1 : 0);
  } else if (dtype == 1) {
    hipLaunchKernelGGL(lrelu_backward_kernel<true>, grid, dim3(256), 0, st, gy, y, out, part.as<float>(),
                       static_cast<long long>(pixels), C, rows, masked ? 1 : 0);
  } else {
    hipLaunchKernelGGL(lrelu_backward_kernel<false>, grid, dim3(256), 0, st, gy, y, out, part.as<float>(),
                       static_cast<long long>(pixels), C, rows, masked ? 1 : 0);
  }
  if (dbias) launch_sum_rows(part.as<float>(), nblk, C, C, dbias, st);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_gan_loss_forward(const void* logits, int dtype, int64_t half, float* out, void* stream) {
  using namespace tfc;
  if (int rc = check_dtype("tfc_gan_loss_forward", dtype)) return rc;
  if (half < 1) return fail("tfc_gan_loss_forward: at least one real and one fake logit, got half = %lld", static_cast<long long>(half));
  if (!logits || !out) return fail("tfc_gan_loss_forward: null tensor");
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer("gan_loss_forward", st);
  if (dtype == 1) hipLaunchKernelGGL(gan_loss_forward_kernel<true>, dim3(1), dim3(1024), 0, st, logits, static_cast<long long>(half), out);
  else hipLaunchKernelGGL(gan_loss_forward_kernel<false>, dim3(1), dim3(1024), 0, st, logits, static_cast<long long>(half), out);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_gan_loss_backward(const void* logits, const float* scale, int dtype, int64_t half, int mode,
                                     void* grad, void* stream) {
  using namespace tfc;
  if (int rc = check_dtype("tfc_gan_loss_backward", dtype)) return rc;
  if (half < 1) return fail("tfc_gan_loss_backward: at least one real and one fake logit, got half = %lld", static_cast<long long>(half));
  if (mode != 0 && mode != 1) return fail("tfc_gan_loss_backward: mode must be 0 (d_loss) or 1 (g_loss), got %d", mode);
  if (!logits || !scale || !grad) return fail("tfc_gan_loss_backward: null tensor");
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer("gan_loss_backward", st);
  const unsigned blocks = hg_blocks(2 * half, 1024);
  if (dtype == 1) hipLaunchKernelGGL(gan_loss_backward_kernel<true>, dim3(blocks), dim3(256), 0, st, logits, scale, static_cast<long long>(half), mode, grad);
  else hipLaunchKernelGGL(gan_loss_backward_kernel<false>, dim3(blocks), dim3(256), 0, st, logits, scale, static_cast<long long>(half), mode, grad);
  TFC_HIP(hipGetLastError());
  return 0;
}
