// One scale of SSIM / multiscale SSIM (tf.image.ssim, tf.image.ssim_multiscale) for gfx950, forward and backward.
//
// Images x, y: [batch, H, W, C], channels last; a PLANE is one image's one channel.  With F the separable window
// (taps g[0..n), applied VALID: (H - n + 1) x (W - n + 1) positions), C1 = (k1 max_val)^2, C2 = (k2 max_val)^2:
//   mu1 = F(x), mu2 = F(y), S = F(x^2 + y^2), P = F(x y)
//   l  = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)
//   cs = (2 P - 2 mu1 mu2 + C2) / (S - mu1^2 - mu2^2 + C2)
//   means[plane] = (mean(l cs), mean(cs)) over the valid positions
// and, between scales, both images halved: mean of each 2x2 block, the last row / column repeated where H / W is odd.
//
// Forward, one launch per scale (ssim_fwd_kernel): a workgroup of 256 threads owns a T x T tile of positions of one
// plane.  It stages the (T + n - 1)^2 pixels of x and y the tile needs in LDS, runs the horizontal pass of the four
// moment images into LDS and the vertical pass into registers, forms l cs and cs per position and reduces them to
// one pair per workgroup, scaled by 1 / positions.  launch_sum_rows (reduce_rows.h) adds the pairs of a plane in a
// fixed order: no float atomics, the same bits on every call.  None of the moment images reaches HBM.  The same
// workgroup writes the 2x2 means of the pixels its tile starts at (the last tile of a row / column: up to the
// border, with the repeated row / column of an odd size) to the next scale's pair, from the staged tile: every scale
// reads its two images once.  The pooled pair is float32 [planes, H2, W2, 1] — channels last with one channel, so
// that the coarser scales read and write whole lines whatever C is.
//
// Numerics: the staged values are x - c, y - c with c the tile's first pixel of x.  Variances and the covariance do
// not change with c, so S - mu1^2 - mu2^2 no longer cancels two numbers near 65 025 against a C2 of 58.5; c goes back
// on the means for l only.  The gradient is taken in the same variables (c is a constant of the tile: the value does
// not depend on it).
//
// Backward, one launch per scale (ssim_bwd_kernel): given g = d loss / d means[plane], a workgroup owns a T x T tile
// of PIXELS.  It stages the (T + 2(n - 1))^2 pixels around it, recomputes the moments at the (T + n - 1)^2 positions
// whose window touches the tile, forms there a1 = dV/dmu1, a2 = dV/dmu2, b = dV/dS, c = dV/dP of
// V = (g[0] l cs + g[1] cs) / positions, applies the window as a FULL correlation (horizontal, then vertical pass,
// through LDS) and writes
//   dx = F'(a1) + 2 x F'(b) + y F'(c),   dy = F'(a2) + 2 y F'(b) + x F'(c)
// plus the adjoint of the pool: a quarter of the coarser scale's gradient at [i / 2, j / 2], twice that on the last
// row / column of an odd size (the repeated one folds back onto it).
//
// A channels-last plane of C = 3 is read with a stride of 3 elements.  The C workgroups of one tile are neighbours in
// the grid (channel is the fastest block index), so the lines one of them brings in serve the other C - 1 from L2.
//
// The taps arrive at run time (n <= 31), in the kernel arguments: a wave-uniform index into them is a scalar load.
// T = 32 for n <= 11 (forward 36 KB, backward 63 KB of LDS), 16 above (backward up to 103 KB).  n = 11, the window of
// every model, also has kernels with the tap count as a compile-time constant (see ssim_fwd_kernel).  These numbers
// are the constants of ssim_params.h, which the tests read to place their shapes on the tile seams.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/tfc_hip.h"
#include "bf16_io.h"
#include "launch.h"
#include "reduce_rows.h"
#include "ssim_params.h"

namespace tfc {
namespace {

constexpr int kSsimMaxTaps = SSIM_MAX_TAPS;

struct SsimParams {
  const void* x;
  const void* y;
  float* part;             // forward: [tiles][planes][2]
  float* px;               // forward: pooled x, y [planes, H2, W2] or null
  float* py;
  const float* gmeans;     // backward: [planes][2]
  const float* gpx;        // backward: gradient of the pooled pair [planes, H2, W2] or null
  const float* gpy;
  float* dx;               // backward: [batch, H, W, C] float32 or null
  float* dy;
  int C, H, W, OH, OW, H2, W2, n;
  int batch, tiles_x, tiles_y;   // the grid is one-dimensional: channel fastest, then tile column, tile row, image
  float c1, c2, inv_count;
  float taps[kSsimMaxTaps + 1];
};

// Which channel, tile and image a workgroup has.
struct SsimBlock {
  int ch, tx, ty, img;
  __device__ explicit SsimBlock(const SsimParams& p) {
    unsigned int t = blockIdx.x;
    ch = t % p.C; t /= p.C;
    tx = t % p.tiles_x; t /= p.tiles_x;
    ty = t % p.tiles_y;
    img = t / p.tiles_y;
  }
};

// Sum over the 256 threads of a workgroup in a fixed order; the result in thread 0.  `red`: 4 floats of LDS.
__device__ inline float ssim_block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// Stages rows x cols pixels of x and y from (y0, x0), minus `cen`, into LDS images with `stride` floats per row; zero
// outside the image and in the padding columns.  NIT > 0: rows * stride <= NIT * 256 is known at compile time, and all
// 2 NIT loads of a thread are issued (at clamped, always valid addresses) before the first value is used; the plain loop
// of NIT = 0 waits for each pair of loads in turn.
template <typename T, int NIT>
__device__ inline void ssim_stage(const T* gx, const T* gy, long long base, long long rowstride, const SsimParams& p,
                                  int y0, int x0, int rows, int cols, int stride, const float& cen, float* sx, float* sy) {
  const int tid = threadIdx.x, total = rows * stride;
  if constexpr (NIT > 0) {
    float a[NIT], b[NIT];
    bool ok[NIT];
#pragma unroll
    for (int q = 0; q < NIT; ++q) {
      const int idx = tid + q * 256;
      const int r = idx / stride, c = idx - r * stride;
      const int iy = y0 + r, ix = x0 + c;
      ok[q] = c < cols && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      const long long at = base + min(max(iy, 0), p.H - 1) * rowstride + static_cast<long long>(min(max(ix, 0), p.W - 1)) * p.C;
      a[q] = load_as_float(gx, at);
      b[q] = load_as_float(gy, at);
    }
#pragma unroll
    for (int q = 0; q < NIT; ++q) {
      const int idx = tid + q * 256;
      if (idx < total) {
        sx[idx] = ok[q] ? a[q] - cen : 0.f;
        sy[idx] = ok[q] ? b[q] - cen : 0.f;
      }
    }
  } else {
    for (int idx = tid; idx < total; idx += 256) {
      const int r = idx / stride, c = idx - r * stride;
      const int iy = y0 + r, ix = x0 + c;
      float a = 0.f, b = 0.f;
      if (c < cols && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
        const long long at = base + iy * rowstride + static_cast<long long>(ix) * p.C;
        a = load_as_float(gx, at) - cen;
        b = load_as_float(gy, at) - cen;
      }
      sx[idx] = a;
      sy[idx] = b;
    }
  }
}

// The row stride of the staged tile.  NT (taps known at compile time): a thread of the horizontal pass takes four
// neighbouring positions from NV 16-byte reads of each image, so rows are padded to whole 16-byte slots.
template <int TILE, int NT>
__host__ __device__ constexpr int ssim_fwd_stride(int n) {
  return NT ? TILE - 4 + 4 * ((NT + 6) / 4) : TILE + n - 1;
}

// NT = 0: n = p.n taps read from the arguments inside the loops, one position per thread and step.
// NT > 0: n = NT, the loops unrolled (taps in scalar registers, LDS reads batched), four positions per thread in both
// passes: 14 + 14 values of a row give 4 x 4 horizontal sums, 4 x 14 values of a column give 4 x 4 moments.
template <typename T, int TILE, int NT>
__global__ void __launch_bounds__(256) ssim_fwd_kernel(SsimParams p) {
  extern __shared__ __attribute__((aligned(16))) float ssim_lds[];
  static_assert(NT == 0 || (TILE == SSIM_TILE_SMALL_N && TILE * TILE == 4 * 256),
                "the blocked passes map 256 threads onto a 32 x 32 tile");
  static_assert(SSIM_FIXED_TAPS <= SSIM_TILE_SMALL_N_MAX, "the unrolled kernels run on the tile of the small windows");
  const int n = NT ? NT : p.n, IW = TILE + n - 1; // the staged tile is IW x IW, its rows IWP apart
  const int IWP = ssim_fwd_stride<TILE, NT>(n);
  float* sx = ssim_lds;
  float* sy = sx + IW * IWP;
  float* hm = sy + IW * IWP;                      // [4][IW][TILE]: the horizontal pass
  float* red = hm + 4 * IW * TILE;                // [4]
  const int tid = threadIdx.x;
  const SsimBlock blk(p);
  const int ch = blk.ch, tx = blk.tx, ty = blk.ty;
  const int oy0 = ty * TILE, ox0 = tx * TILE;
  const long long rowstride = static_cast<long long>(p.W) * p.C;
  const long long base = static_cast<long long>(blk.img) * p.H * rowstride + ch;
  const T* gx = static_cast<const T*>(p.x);
  const T* gy = static_cast<const T*>(p.y);
  const float cen = load_as_float(gx, base + oy0 * rowstride + static_cast<long long>(ox0) * p.C);

  constexpr int NIT = NT ? ((TILE + NT - 1) * ssim_fwd_stride<TILE, NT>(NT) + 255) / 256 : 0;
  ssim_stage<T, NIT>(gx, gy, base, rowstride, p, oy0, ox0, IW, IW, IWP, cen, sx, sy);
  __syncthreads();

  const int plane_h = IW * TILE;
  float sum_lcs = 0.f, sum_cs = 0.f;
  auto position = [&](int r, int c, float u1, float u2, float s, float pr) {
    if (oy0 + r < p.OH && ox0 + c < p.OW) {
      const float m1 = u1 + cen, m2 = u2 + cen;
      const float l = (2.f * m1 * m2 + p.c1) / (m1 * m1 + m2 * m2 + p.c1);
      const float cs = (2.f * (pr - u1 * u2) + p.c2) / ((s - u1 * u1 - u2 * u2) + p.c2);
      sum_lcs += l * cs;
      sum_cs += cs;
    }
  };
  if constexpr (NT > 0) {
    constexpr int NV = (NT + 6) / 4, NE = NT + 3;
    float g[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) g[k] = p.taps[k];
    for (int item = tid; item < IW * (TILE / 4); item += 256) {
      const int r = item / (TILE / 4), c = 4 * (item % (TILE / 4));
      const float4* qx = reinterpret_cast<const float4*>(sx + r * IWP + c);
      const float4* qy = reinterpret_cast<const float4*>(sy + r * IWP + c);
      float a[4 * NV], b[4 * NV], sq[NE], pr[NE];
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const float4 va = qx[j], vb = qy[j];
        a[4 * j] = va.x; a[4 * j + 1] = va.y; a[4 * j + 2] = va.z; a[4 * j + 3] = va.w;
        b[4 * j] = vb.x; b[4 * j + 1] = vb.y; b[4 * j + 2] = vb.z; b[4 * j + 3] = vb.w;
      }
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        sq[j] = fmaf(a[j], a[j], b[j] * b[j]);
        pr[j] = a[j] * b[j];
      }
      float h[4][4] = {};
#pragma unroll
      for (int k = 0; k < NT; ++k) {
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          h[0][o] = fmaf(g[k], a[k + o], h[0][o]);
          h[1][o] = fmaf(g[k], b[k + o], h[1][o]);
          h[2][o] = fmaf(g[k], sq[k + o], h[2][o]);
          h[3][o] = fmaf(g[k], pr[k + o], h[3][o]);
        }
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
        *reinterpret_cast<float4*>(hm + m * plane_h + r * TILE + c) = make_float4(h[m][0], h[m][1], h[m][2], h[m][3]);
    }
    __syncthreads();
    {
      const int c = tid % TILE, r0 = 4 * (tid / TILE);
      const float* col = hm + r0 * TILE + c;
      float m[4][4] = {};
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        const float v0 = col[j * TILE], v1 = col[plane_h + j * TILE], v2 = col[2 * plane_h + j * TILE],
                    v3 = col[3 * plane_h + j * TILE];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          if (j - o >= 0 && j - o < NT) {
            m[0][o] = fmaf(g[j - o], v0, m[0][o]);
            m[1][o] = fmaf(g[j - o], v1, m[1][o]);
            m[2][o] = fmaf(g[j - o], v2, m[2][o]);
            m[3][o] = fmaf(g[j - o], v3, m[3][o]);
          }
        }
      }
#pragma unroll
      for (int o = 0; o < 4; ++o) position(r0 + o, c, m[0][o], m[1][o], m[2][o], m[3][o]);
    }
  } else {
    for (int idx = tid; idx < IW * TILE; idx += 256) {
      const int r = idx / TILE, c = idx % TILE;
      const float* rx = sx + r * IWP + c;
      const float* ry = sy + r * IWP + c;
      float h1 = 0.f, h2 = 0.f, hs = 0.f, hp = 0.f;
      for (int k = 0; k < n; ++k) {
        const float g = p.taps[k], a = rx[k], b = ry[k];
        h1 = fmaf(g, a, h1);
        h2 = fmaf(g, b, h2);
        hs = fmaf(g, fmaf(a, a, b * b), hs);
        hp = fmaf(g, a * b, hp);
      }
      hm[idx] = h1;
      hm[plane_h + idx] = h2;
      hm[2 * plane_h + idx] = hs;
      hm[3 * plane_h + idx] = hp;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TILE * TILE / 256; ++q) {
      const int idx = tid + q * 256;
      const int r = idx / TILE, c = idx % TILE;
      const float* col = hm + r * TILE + c;
      float u1 = 0.f, u2 = 0.f, s = 0.f, pr = 0.f;
      for (int k = 0; k < n; ++k) {
        const float g = p.taps[k];
        const float* at = col + k * TILE;
        u1 = fmaf(g, at[0], u1);
        u2 = fmaf(g, at[plane_h], u2);
        s = fmaf(g, at[2 * plane_h], s);
        pr = fmaf(g, at[3 * plane_h], pr);
      }
      position(r, c, u1, u2, s, pr);
    }
  }
  const float t0 = ssim_block_sum(sum_lcs, red);
  const float t1 = ssim_block_sum(sum_cs, red);
  if (tid == 0) {
    const long long planes = static_cast<long long>(p.batch) * p.C;
    const long long tile = static_cast<long long>(ty) * p.tiles_x + tx;
    float* out = p.part + (tile * planes + static_cast<long long>(blk.img) * p.C + ch) * 2;
    out[0] = t0 * p.inv_count;
    out[1] = t1 * p.inv_count;
  }

  if (p.px) {
    // the pixels this tile owns: TILE x TILE from its origin, or up to the border for the last tile of a row / column
    const int rows = (ty == p.tiles_y - 1 ? p.H : oy0 + TILE) - oy0;
    const int cols = (tx == p.tiles_x - 1 ? p.W : ox0 + TILE) - ox0;
    const int prn = (rows + 1) / 2, pcn = (cols + 1) / 2;
    const long long plane = static_cast<long long>(blk.img) * p.C + ch;
    float* ox = p.px + plane * p.H2 * p.W2;
    float* oy = p.py + plane * p.H2 * p.W2;
    for (int idx = tid; idx < prn * pcn; idx += 256) {
      const int r = idx / pcn, c = idx - r * pcn;
      const int r0 = 2 * r, r1 = min(2 * r + 1, rows - 1), c0 = 2 * c, c1 = min(2 * c + 1, cols - 1);
      const long long at = static_cast<long long>(oy0 / 2 + r) * p.W2 + ox0 / 2 + c;
      ox[at] = 0.25f * ((sx[r0 * IWP + c0] + sx[r0 * IWP + c1]) + (sx[r1 * IWP + c0] + sx[r1 * IWP + c1])) + cen;
      oy[at] = 0.25f * ((sy[r0 * IWP + c0] + sy[r0 * IWP + c1]) + (sy[r1 * IWP + c0] + sy[r1 * IWP + c1])) + cen;
    }
  }
}

// NT as in the forward kernel: 0 reads p.n taps inside the loops, NT > 0 unrolls them.
template <typename T, int TILE, int NT>
__global__ void __launch_bounds__(256) ssim_bwd_kernel(SsimParams p) {
  extern __shared__ float ssim_lds[];
  constexpr int PER = TILE * TILE / 256;
  const int n = NT ? NT : p.n, R = n - 1;
  const int MW = TILE + R;                        // positions whose window touches the tile: MW x MW
  const int IW = TILE + 2 * R;                    // pixels those positions read: IW x IW
  const int a_floats = max(2 * IW * IW, 4 * MW * MW);
  float* sx = ssim_lds;                           // region A: the staged pixels, then the four derivative maps
  float* sy = sx + IW * IW;
  float* maps = ssim_lds;                         // [4][MW][MW]
  float* hm = ssim_lds + a_floats;                // region B: [4][IW][MW] horizontal pass, then [4][MW][TILE] adjoint
  const int tid = threadIdx.x;
  const SsimBlock blk(p);
  const int ch = blk.ch, tx = blk.tx, ty = blk.ty;
  const int i0 = ty * TILE, j0 = tx * TILE;
  const long long rowstride = static_cast<long long>(p.W) * p.C;
  const long long base = static_cast<long long>(blk.img) * p.H * rowstride + ch;
  const long long plane = static_cast<long long>(blk.img) * p.C + ch;
  const T* gx = static_cast<const T*>(p.x);
  const T* gy = static_cast<const T*>(p.y);
  const float cen = load_as_float(gx, base + i0 * rowstride + static_cast<long long>(j0) * p.C);
  const float wa = p.gmeans[2 * plane] * p.inv_count, wb = p.gmeans[2 * plane + 1] * p.inv_count;

  constexpr int NIT = NT ? ((TILE + 2 * NT - 2) * (TILE + 2 * NT - 2) + 255) / 256 : 0;
  ssim_stage<T, NIT>(gx, gy, base, rowstride, p, i0 - R, j0 - R, IW, IW, IW, cen, sx, sy);
  __syncthreads();

  // this thread's pixels, for the last step
  float xs[PER], ys[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int idx = tid + q * 256;
    const int at = (idx / TILE + R) * IW + idx % TILE + R;
    xs[q] = sx[at];
    ys[q] = sy[at];
  }

  const int plane_b = IW * MW;
  for (int idx = tid; idx < IW * MW; idx += 256) {
    const int r = idx / MW, c = idx - r * MW;
    const float* rx = sx + r * IW + c;
    const float* ry = sy + r * IW + c;
    float h1 = 0.f, h2 = 0.f, hs = 0.f, hp = 0.f;
#pragma unroll
    for (int k = 0; k < n; ++k) {
      const float g = p.taps[k], a = rx[k], b = ry[k];
      h1 = fmaf(g, a, h1);
      h2 = fmaf(g, b, h2);
      hs = fmaf(g, fmaf(a, a, b * b), hs);
      hp = fmaf(g, a * b, hp);
    }
    hm[idx] = h1;
    hm[plane_b + idx] = h2;
    hm[2 * plane_b + idx] = hs;
    hm[3 * plane_b + idx] = hp;
  }
  __syncthreads();

  // moments and the derivatives of V at the positions (i0 - R + r, j0 - R + c); zero outside the valid ones
  const int plane_m = MW * MW;
  for (int idx = tid; idx < MW * MW; idx += 256) {
    const int r = idx / MW, c = idx - r * MW;
    const int pi = i0 - R + r, pj = j0 - R + c;
    float a1 = 0.f, a2 = 0.f, db = 0.f, dc = 0.f;
    if (pi >= 0 && pi < p.OH && pj >= 0 && pj < p.OW) {
      const float* col = hm + r * MW + c;
      float u1 = 0.f, u2 = 0.f, s = 0.f, pr = 0.f;
#pragma unroll
      for (int k = 0; k < n; ++k) {
        const float g = p.taps[k];
        const float* at = col + k * MW;
        u1 = fmaf(g, at[0], u1);
        u2 = fmaf(g, at[plane_b], u2);
        s = fmaf(g, at[2 * plane_b], s);
        pr = fmaf(g, at[3 * plane_b], pr);
      }
      const float m1 = u1 + cen, m2 = u2 + cen;
      const float ld = m1 * m1 + m2 * m2 + p.c1;
      const float l = (2.f * m1 * m2 + p.c1) / ld;
      const float cd = (s - u1 * u1 - u2 * u2) + p.c2;
      const float cs = (2.f * (pr - u1 * u2) + p.c2) / cd;
      const float q = (wa * l + wb) / cd;          // dV/dcs / cd
      const float dl = wa * cs / ld;               // dV/dl / ld
      a1 = dl * 2.f * (m2 - m1 * l) + q * 2.f * (u1 * cs - u2);
      a2 = dl * 2.f * (m1 - m2 * l) + q * 2.f * (u2 * cs - u1);
      db = -q * cs;
      dc = 2.f * q;
    }
    maps[idx] = a1;
    maps[plane_m + idx] = a2;
    maps[2 * plane_m + idx] = db;
    maps[3 * plane_m + idx] = dc;
  }
  __syncthreads();

  // FULL correlation, horizontal: pixel column j takes the positions j - k
  const int plane_t = MW * TILE;
  for (int idx = tid; idx < MW * TILE; idx += 256) {
    const int r = idx / TILE, c = idx % TILE;
    const float* row = maps + r * MW + c + R;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll
    for (int k = 0; k < n; ++k) {
      const float g = p.taps[k];
      const float* at = row - k;
      t0 = fmaf(g, at[0], t0);
      t1 = fmaf(g, at[plane_m], t1);
      t2 = fmaf(g, at[2 * plane_m], t2);
      t3 = fmaf(g, at[3 * plane_m], t3);
    }
    hm[idx] = t0;
    hm[plane_t + idx] = t1;
    hm[2 * plane_t + idx] = t2;
    hm[3 * plane_t + idx] = t3;
  }
  __syncthreads();

  const int odd_h = p.H & 1, odd_w = p.W & 1;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int idx = tid + q * 256;
    const int r = idx / TILE, c = idx % TILE;
    const int iy = i0 + r, ix = j0 + c;
    if (iy >= p.H || ix >= p.W) continue;
    const float* col = hm + (r + R) * TILE + c;
    float f1 = 0.f, f2 = 0.f, fb = 0.f, fc = 0.f;
#pragma unroll
    for (int k = 0; k < n; ++k) {
      const float g = p.taps[k];
      const float* at = col - k * TILE;
      f1 = fmaf(g, at[0], f1);
      f2 = fmaf(g, at[plane_t], f2);
      fb = fmaf(g, at[2 * plane_t], fb);
      fc = fmaf(g, at[3 * plane_t], fc);
    }
    float vx = f1 + 2.f * xs[q] * fb + ys[q] * fc;
    float vy = f2 + 2.f * ys[q] * fb + xs[q] * fc;
    if (p.gpx || p.gpy) {
      const float w = 0.25f * ((odd_h && iy == p.H - 1) ? 2.f : 1.f) * ((odd_w && ix == p.W - 1) ? 2.f : 1.f);
      const long long at = (plane * p.H2 + (iy >> 1)) * p.W2 + (ix >> 1);
      if (p.gpx) vx += w * p.gpx[at];
      if (p.gpy) vy += w * p.gpy[at];
    }
    const long long at = base + iy * rowstride + static_cast<long long>(ix) * p.C;
    if (p.dx) p.dx[at] = vx;
    if (p.dy) p.dy[at] = vy;
  }
}

int ssim_tile(int n) { return n <= SSIM_TILE_SMALL_N_MAX ? SSIM_TILE_SMALL_N : SSIM_TILE_LARGE_N; }

size_t ssim_fwd_lds(int n, int tile, bool fixed) {
  const size_t iw = tile + n - 1, iwp = fixed ? ssim_fwd_stride<SSIM_TILE_SMALL_N, SSIM_FIXED_TAPS>(n) : iw;
  return sizeof(float) * (2 * iw * iwp + 4 * iw * tile + 4);
}

size_t ssim_bwd_lds(int n, int tile) {
  const size_t mw = tile + n - 1, iw = tile + 2 * (n - 1);
  return sizeof(float) * (std::max(2 * iw * iw, 4 * mw * mw) + 4 * iw * mw);
}

int ssim_validate(const char* name, const void* x, const void* y, int dtype, int64_t batch, int64_t height,
                  int64_t width, int64_t channels, const float* taps, int filter_size, float c1, float c2) {
  if (dtype < 0 || dtype > 3) return fail("%s: dtype must be 0 (float32), 1 (bfloat16), 2 (float16) or 3 (uint8)", name);
  if (filter_size < 1 || filter_size > kSsimMaxTaps)
    return fail("%s: filter_size must be between 1 and %d, got %d", name, kSsimMaxTaps, filter_size);
  if (!taps) return fail("%s: taps must not be null", name);
  if (batch < 1 || batch > (1 << 24)) return fail("%s: batch must be between 1 and 2^24, got %lld", name, static_cast<long long>(batch));
  if (channels < 1 || channels > 4096)
    return fail("%s: channels must be between 1 and 4096, got %lld", name, static_cast<long long>(channels));
  if (height < filter_size || width < filter_size)
    return fail("%s: the image (%lld x %lld) is smaller than the window (%d)", name, static_cast<long long>(height),
                static_cast<long long>(width), filter_size);
  if (height > (1 << 20) || width > (1 << 20)) return fail("%s: height and width must be at most 2^20", name);
  if (!std::isfinite(c1) || !std::isfinite(c2) || c1 < 0.f || c2 <= 0.f)
    return fail("%s: c1 must be finite and non-negative, c2 finite and positive", name);
  // (the smaller tile bounds the count)
  if (ceil_div(height, SSIM_TILE_LARGE_N) * ceil_div(width, SSIM_TILE_LARGE_N) * channels * batch > 0x7fffffffll)
    return fail("%s: batch x channels x tiles exceeds the 2^31 - 1 workgroups of a launch", name);
  if (!x || !y) return fail("%s: x and y must not be null", name);
  return 0;
}

void ssim_fill(SsimParams& p, const void* x, const void* y, int64_t height, int64_t width, int64_t channels,
               const float* taps, int n, float c1, float c2) {
  p.x = x; p.y = y;
  p.C = static_cast<int>(channels); p.H = static_cast<int>(height); p.W = static_cast<int>(width);
  p.OH = p.H - n + 1; p.OW = p.W - n + 1;
  p.H2 = (p.H + 1) / 2; p.W2 = (p.W + 1) / 2;
  p.n = n; p.c1 = c1; p.c2 = c2;
  p.inv_count = static_cast<float>(1.0 / (static_cast<double>(p.OH) * p.OW));
  for (int k = 0; k < n; ++k) p.taps[k] = taps[k];
}

template <typename T, int TILE, int NT>
int ssim_launch_fwd(const SsimParams& p, dim3 grid, size_t lds, hipStream_t st) {
  return launch(&ssim_fwd_kernel<T, TILE, NT>, grid, dim3(256), lds, st, p);
}

template <typename T, int TILE, int NT>
int ssim_launch_bwd(const SsimParams& p, dim3 grid, size_t lds, hipStream_t st) {
  return launch(&ssim_bwd_kernel<T, TILE, NT>, grid, dim3(256), lds, st, p);
}

// The window of the models (11 taps) has kernels of its own with the tap count a compile-time constant; every other
// filter_size, or TFC_SSIM_RUNTIME_TAPS=1 in the environment (for a same-process comparison), takes the general ones.
bool ssim_fixed_taps(int n) {
  const char* e = env_str("TFC_SSIM_RUNTIME_TAPS");
  return n == SSIM_FIXED_TAPS && !(e && e[0] == '1');
}

#define TFC_SSIM_DISPATCH_T(LAUNCH, TILE, NT, ...)                                          \
  (dtype == 0   ? LAUNCH<float, TILE, NT>(__VA_ARGS__)                                      \
   : dtype == 1 ? LAUNCH<unsigned short, TILE, NT>(__VA_ARGS__)                             \
   : dtype == 2 ? LAUNCH<_Float16, TILE, NT>(__VA_ARGS__)                                   \
                : LAUNCH<unsigned char, TILE, NT>(__VA_ARGS__))
#define TFC_SSIM_DISPATCH(LAUNCH, ...)                                                                \
  do {                                                                                                \
    const int rc__ =                                                                                  \
        fixed                       ? TFC_SSIM_DISPATCH_T(LAUNCH, SSIM_TILE_SMALL_N, SSIM_FIXED_TAPS, __VA_ARGS__) \
        : tile == SSIM_TILE_SMALL_N ? TFC_SSIM_DISPATCH_T(LAUNCH, SSIM_TILE_SMALL_N, 0, __VA_ARGS__)  \
                                    : TFC_SSIM_DISPATCH_T(LAUNCH, SSIM_TILE_LARGE_N, 0, __VA_ARGS__); \
    if (rc__) return rc__;                                                                            \
  } while (0)

}  // namespace
}  // namespace tfc

extern "C" int tfc_ssim_scale_forward(const void* x, const void* y, int dtype, int64_t batch, int64_t height,
                                      int64_t width, int64_t channels, const float* taps, int filter_size, float c1,
                                      float c2, float* means, float* pooled_x, float* pooled_y, void* stream) {
  using namespace tfc;
  if (int rc = ssim_validate("tfc_ssim_scale_forward", x, y, dtype, batch, height, width, channels, taps, filter_size,
                             c1, c2))
    return rc;
  if (!means) return fail("tfc_ssim_scale_forward: means must not be null");
  if ((pooled_x == nullptr) != (pooled_y == nullptr))
    return fail("tfc_ssim_scale_forward: pooled_x and pooled_y must both be given or both be null");
  hipStream_t st = static_cast<hipStream_t>(stream);
  SsimParams p = {};
  ssim_fill(p, x, y, height, width, channels, taps, filter_size, c1, c2);
  p.px = pooled_x; p.py = pooled_y;
  const int tile = ssim_tile(filter_size);
  const long long tiles_x = ceil_div(p.OW, tile), tiles_y = ceil_div(p.OH, tile);
  const long long planes = batch * channels;
  DevBuf part;
  TFC_HIP(part.alloc(sizeof(float) * 2 * planes * tiles_x * tiles_y, st));
  p.part = part.as<float>();
  p.batch = static_cast<int>(batch); p.tiles_x = static_cast<int>(tiles_x); p.tiles_y = static_cast<int>(tiles_y);
  const dim3 grid(static_cast<unsigned>(tiles_x * tiles_y * channels * batch));
  const bool fixed = ssim_fixed_taps(filter_size);
  const size_t lds = ssim_fwd_lds(filter_size, tile, fixed);
  TFC_HIP(hipMemsetAsync(means, 0, sizeof(float) * 2 * planes, st));
  KernelTimer timer("ssim_scale_forward", st);
  TFC_SSIM_DISPATCH(ssim_launch_fwd, p, grid, lds, st);
  launch_sum_rows(p.part, tiles_x * tiles_y, 2 * planes, static_cast<int>(2 * planes), means, st);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_ssim_scale_backward(const void* x, const void* y, int dtype, int64_t batch, int64_t height,
                                       int64_t width, int64_t channels, const float* taps, int filter_size, float c1,
                                       float c2, const float* grad_means, const float* grad_pooled_x,
                                       const float* grad_pooled_y, float* grad_x, float* grad_y, void* stream) {
  using namespace tfc;
  if (int rc = ssim_validate("tfc_ssim_scale_backward", x, y, dtype, batch, height, width, channels, taps, filter_size,
                             c1, c2))
    return rc;
  if (!grad_means) return fail("tfc_ssim_scale_backward: grad_means must not be null");
  if (!grad_x && !grad_y) return fail("tfc_ssim_scale_backward: grad_x and grad_y must not both be null");
  hipStream_t st = static_cast<hipStream_t>(stream);
  SsimParams p = {};
  ssim_fill(p, x, y, height, width, channels, taps, filter_size, c1, c2);
  p.gmeans = grad_means; p.gpx = grad_pooled_x; p.gpy = grad_pooled_y;
  p.dx = grad_x; p.dy = grad_y;
  const int tile = ssim_tile(filter_size);
  p.batch = static_cast<int>(batch); p.tiles_x = static_cast<int>(ceil_div(p.W, tile)); p.tiles_y = static_cast<int>(ceil_div(p.H, tile));
  const dim3 grid(static_cast<unsigned>(static_cast<long long>(p.tiles_x) * p.tiles_y * channels * batch));
  const bool fixed = ssim_fixed_taps(filter_size);
  const size_t lds = ssim_bwd_lds(filter_size, tile);
  KernelTimer timer("ssim_scale_backward", st);
  TFC_SSIM_DISPATCH(ssim_launch_bwd, p, grid, lds, st);
  TFC_HIP(hipGetLastError());
  return 0;
}
