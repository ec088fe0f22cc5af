// YUV4MPEG2 frames on the device: splitting the planes of raw frame bytes into the (y, cbcr) tensors of Y4MDataset
// (cc/kernels/y4m_dataset_kernels.cc:165-178, which de-interleaves one byte at a time on the host), the inverse for
// writing, and the fused YCbCr <-> RGB conversions in front of and behind the models (no counterpart in the reference).
//
// All four kernels move bytes and nothing else, so they are laid out for 16-byte accesses:
//   * unpack / pack: every plane of every frame is a segment.  A plane starts on any byte (a 6-byte FRAME marker in
//     front of the frame, an odd W H / 4 in front of V), so a segment aligns on its DESTINATION: up to 15 head bytes
//     and up to 15 tail bytes go one narrow access per lane, the body is one aligned 16-byte store per lane fed by
//     loads from whatever address the source has (gfx950 serves unaligned global loads; nothing is read outside the
//     plane).
//   * the conversions: a lane owns 8 neighbouring pixels of one row (of two rows for 4:2:0 subsampling), a wave 512
//     neighbouring pixels.  Rows whose width is a multiple of 8 take 8/16-byte loads and stores; any other width, or an
//     output that is not aligned, takes the same arithmetic with one access per value.
// Byte offsets are 64-bit throughout.  No atomics, no LDS, no scratch.
#include "bf16_io.h"
#include "common.h"

#include <cmath>

namespace tfc {
namespace {

typedef unsigned char u8;

constexpr int Y4M_THREADS = 256;
constexpr int Y4M_EDGE = 32;        // lanes of a segment that own its head (the first 16) and tail (the last 16) units
constexpr int CSC_LANES = 64;       // pixel groups of one row per workgroup
constexpr int CSC_ROWS = 4;         // rows (row pairs) per workgroup
constexpr int CSC_PX = 8;           // pixels of a row per lane

__device__ __forceinline__ uint4 load16(const u8* p) {       // any alignment
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}
__device__ __forceinline__ uint2 load8(const u8* p) {
  uint2 v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
__device__ __forceinline__ void store16(void* p, uint4 v) { *reinterpret_cast<uint4*>(p) = v; }     // 16-byte aligned
__device__ __forceinline__ void store8(void* p, uint2 v) { *reinterpret_cast<uint2*>(p) = v; }      // 8-byte aligned

__device__ __forceinline__ long long head_bytes(const void* dst) {
  return static_cast<long long>((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15);
}

// ---------------------------------------------------------------------------------------------------------------
// Plane segments.  `j` is the lane's index within the segment; a segment of L units has at most L / chunk body lanes
// and Y4M_EDGE edge lanes behind them.

// dst[0, len) = src[0, len)
__device__ __forceinline__ void seg_copy(u8* dst, const u8* src, long long len, long long j) {
  const long long h = min(len, head_bytes(dst));
  const long long nb = (len - h) >> 4;
  if (j < nb) {
    const long long at = h + (j << 4);
    store16(dst + at, load16(src + at));
    return;
  }
  const long long e = j - nb;
  if (e < 16) {
    if (e < h) dst[e] = src[e];
  } else if (e < Y4M_EDGE) {
    const long long at = h + (nb << 4) + (e - 16);
    if (at < len) dst[at] = src[at];
  }
}

// dst[2 i] = u[i], dst[2 i + 1] = v[i] for i in [0, pairs); dst is 2-byte aligned
__device__ __forceinline__ void seg_interleave(u8* dst, const u8* u, const u8* v, long long pairs, long long j) {
  const long long h = min(pairs, head_bytes(dst) >> 1);
  const long long nb = (pairs - h) >> 3;
  if (j < nb) {
    const long long at = h + (j << 3);
    const uint2 a = load8(u + at), b = load8(v + at);
    uint4 o;
    o.x = (a.x & 0xffu) | ((b.x & 0xffu) << 8) | ((a.x & 0xff00u) << 8) | ((b.x & 0xff00u) << 16);
    o.y = ((a.x >> 16) & 0xffu) | ((b.x >> 8) & 0xff00u) | ((a.x >> 8) & 0xff0000u) | (b.x & 0xff000000u);
    o.z = (a.y & 0xffu) | ((b.y & 0xffu) << 8) | ((a.y & 0xff00u) << 8) | ((b.y & 0xff00u) << 16);
    o.w = ((a.y >> 16) & 0xffu) | ((b.y >> 8) & 0xff00u) | ((a.y >> 8) & 0xff0000u) | (b.y & 0xff000000u);
    store16(dst + 2 * at, o);
    return;
  }
  const long long e = j - nb;
  long long at = -1;
  if (e < 16) {
    if (e < h) at = e;
  } else if (e < Y4M_EDGE) {
    at = h + (nb << 3) + (e - 16);
  }
  if (at >= 0 && at < pairs)
    *reinterpret_cast<unsigned short*>(dst + 2 * at) =
        static_cast<unsigned short>(u[at] | (static_cast<unsigned>(v[at]) << 8));
}

// dst[i] = src[2 i + which] for i in [0, len)
__device__ __forceinline__ unsigned even_bytes(unsigned lo, unsigned hi) {
  return (lo & 0xffu) | ((lo >> 8) & 0xff00u) | ((hi & 0xffu) << 16) | ((hi << 8) & 0xff000000u);
}
__device__ __forceinline__ void seg_extract(u8* dst, const u8* src, int which, long long len, long long j) {
  const long long h = min(len, head_bytes(dst));
  const long long nb = (len - h) >> 4;
  if (j < nb) {
    const long long at = h + (j << 4);
    const uint4 a = load16(src + 2 * at), b = load16(src + 2 * at + 16);
    const int s = 8 * which;
    uint4 o;
    o.x = even_bytes(a.x >> s, a.y >> s);
    o.y = even_bytes(a.z >> s, a.w >> s);
    o.z = even_bytes(b.x >> s, b.y >> s);
    o.w = even_bytes(b.z >> s, b.w >> s);
    store16(dst + at, o);
    return;
  }
  const long long e = j - nb;
  if (e < 16) {
    if (e < h) dst[e] = src[2 * e + which];
  } else if (e < Y4M_EDGE) {
    const long long at = h + (nb << 4) + (e - 16);
    if (at < len) dst[at] = src[2 * at + which];
  }
}

struct PlaneParams {
  u8* raw;                 // the frame bytes: read by unpack, written by pack
  u8* y;                   // [N, H, W, 1]
  u8* c;                   // [N, h, w, 2]
  long long ys, cs;        // bytes of the luma plane and of one chroma plane
  long long stride, first;
  long long N;
  long long ty, tc;        // lanes of the luma segment and of one chroma segment
};

__global__ void __launch_bounds__(Y4M_THREADS) y4m_unpack_kernel(PlaneParams p) {
  const long long j = static_cast<long long>(blockIdx.x) * Y4M_THREADS + threadIdx.x;
  for (long long n = blockIdx.y; n < p.N; n += gridDim.y) {
    const u8* src = p.raw + p.first + n * p.stride;
    if (j < p.ty)
      seg_copy(p.y + n * p.ys, src, p.ys, j);
    else if (j < p.ty + p.tc)
      seg_interleave(p.c + 2 * n * p.cs, src + p.ys, src + p.ys + p.cs, p.cs, j - p.ty);
  }
}

__global__ void __launch_bounds__(Y4M_THREADS) y4m_pack_kernel(PlaneParams p) {
  const long long j = static_cast<long long>(blockIdx.x) * Y4M_THREADS + threadIdx.x;
  for (long long n = blockIdx.y; n < p.N; n += gridDim.y) {
    u8* dst = p.raw + p.first + n * p.stride;
    const u8* cn = p.c + 2 * n * p.cs;
    if (j < p.ty)
      seg_copy(dst, p.y + n * p.ys, p.ys, j);
    else if (j < p.ty + p.tc)
      seg_extract(dst + p.ys, cn, 0, p.cs, j - p.ty);
    else if (j < p.ty + 2 * p.tc)
      seg_extract(dst + p.ys + p.cs, cn, 1, p.cs, j - p.ty - p.tc);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Colour conversion

enum { CSC_U8 = 0, CSC_F32 = 1, CSC_BF16 = 2 };
enum { CSC_444 = 0, CSC_420_NEAREST = 1, CSC_420_BILINEAR = 2 };

struct CscParams {
  const u8* y;             // to RGB: the inputs
  const u8* c;
  void* rgb;               // to RGB: the output; from RGB: the input
  u8* yo;                  // from RGB: the outputs
  u8* co;
  long long rows;          // N H, or N H / 2 where a lane owns two rows
  int W, H, cw, ch;
  int gpr;                 // lanes per row
  int vec, clip;
  // to RGB: Y' = y y_scale + y_off (y_off = -16 y_scale for the limited range) and the four coefficients in k0..k3
  // times the chroma scale (1 or 255 / 224), applied to c - 128.  From RGB: Kr, Kg, Kb in k0..k2, y = Y' y_scale +
  // y_off, c = C' c_scale + 128.
  float y_off, y_scale, c_scale;
  float k0, k1, k2, k3;
  float icb, icr;                      // from RGB: 1 / (2(1-Kb)), 1 / (2(1-Kr))
};

__device__ __forceinline__ float byte_of(unsigned v, int k) { return static_cast<float>((v >> (8 * k)) & 0xffu); }
__device__ __forceinline__ float clamp255(float v) { return __builtin_amdgcn_fmed3f(v, 0.f, 255.f); }
// Clamp, then round half to even: adding 2^23 leaves the integer in the low mantissa bits, rounded by the addition itself.
__device__ __forceinline__ unsigned to_u8(float v) { return __float_as_uint(clamp255(v) + 8388608.f) & 0xffu; }

template <int MODE>
__device__ __forceinline__ void load_chroma(const CscParams& p, unsigned n, unsigned i, int x0, float cb[CSC_PX],
                                            float cr[CSC_PX]) {
  if (MODE == CSC_444) {
    const u8* cp = p.c + ((static_cast<long long>(n) * p.H + i) * p.W + x0) * 2;
    if (p.vec) {
      const uint4 v = load16(cp);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < CSC_PX; ++k) {
        cb[k] = byte_of(w[k >> 1], 2 * (k & 1));
        cr[k] = byte_of(w[k >> 1], 2 * (k & 1) + 1);
      }
    } else {
#pragma unroll
      for (int k = 0; k < CSC_PX; ++k) {
        const int kk = min(x0 + k, p.W - 1) - x0;
        cb[k] = cp[2 * kk];
        cr[k] = cp[2 * kk + 1];
      }
    }
    return;
  }
  const int m = static_cast<int>(i >> 1), q0 = x0 >> 1;
  const u8* ra = p.c + (static_cast<long long>(n) * p.ch + m) * p.cw * 2;
  if (MODE == CSC_420_NEAREST) {
    float ub[4], vb[4];
    if (p.vec) {
      const uint2 v = load8(ra + 2 * q0);
      const unsigned w[2] = {v.x, v.y};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ub[q] = byte_of(w[q >> 1], 2 * (q & 1));
        vb[q] = byte_of(w[q >> 1], 2 * (q & 1) + 1);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = min(q0 + q, p.cw - 1);
        ub[q] = ra[2 * col];
        vb[q] = ra[2 * col + 1];
      }
    }
#pragma unroll
    for (int k = 0; k < CSC_PX; ++k) {
      cb[k] = ub[k >> 1];
      cr[k] = vb[k >> 1];
    }
    return;
  }
  // bilinear, centre siting: the row above an even luma row, below an odd one, clamped; columns alike
  const int m2 = (i & 1) ? min(m + 1, p.ch - 1) : max(m - 1, 0);
  const u8* rb = p.c + (static_cast<long long>(n) * p.ch + m2) * p.cw * 2;
  float ub[6], vb[6];      // columns q0 - 1 .. q0 + 4 after the vertical step
  if (p.vec) {
    const uint2 a = load8(ra + 2 * q0), b = load8(rb + 2 * q0);
    const unsigned wa[2] = {a.x, a.y}, wb[2] = {b.x, b.y};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ub[q + 1] = 0.75f * byte_of(wa[q >> 1], 2 * (q & 1)) + 0.25f * byte_of(wb[q >> 1], 2 * (q & 1));
      vb[q + 1] = 0.75f * byte_of(wa[q >> 1], 2 * (q & 1) + 1) + 0.25f * byte_of(wb[q >> 1], 2 * (q & 1) + 1);
    }
    const int lo = max(q0 - 1, 0), hi = min(q0 + 4, p.cw - 1);
    ub[0] = 0.75f * ra[2 * lo] + 0.25f * rb[2 * lo];
    vb[0] = 0.75f * ra[2 * lo + 1] + 0.25f * rb[2 * lo + 1];
    ub[5] = 0.75f * ra[2 * hi] + 0.25f * rb[2 * hi];
    vb[5] = 0.75f * ra[2 * hi + 1] + 0.25f * rb[2 * hi + 1];
  } else {
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const int col = min(max(q0 + q - 1, 0), p.cw - 1);
      ub[q] = 0.75f * ra[2 * col] + 0.25f * rb[2 * col];
      vb[q] = 0.75f * ra[2 * col + 1] + 0.25f * rb[2 * col + 1];
    }
  }
#pragma unroll
  for (int k = 0; k < CSC_PX; ++k) {
    const int q = (k >> 1) + 1, side = (k & 1) ? q + 1 : q - 1;
    cb[k] = 0.75f * ub[q] + 0.25f * ub[side];
    cr[k] = 0.75f * vb[q] + 0.25f * vb[side];
  }
}

template <int OUT, int MODE>
__global__ void __launch_bounds__(CSC_LANES * CSC_ROWS) ycbcr_to_rgb_kernel(CscParams p) {
  const int g = blockIdx.x * CSC_LANES + threadIdx.x;
  if (g >= p.gpr) return;
  const int x0 = g * CSC_PX;
  const int npx = min(CSC_PX, p.W - x0);
  for (long long r = static_cast<long long>(blockIdx.y) * CSC_ROWS + threadIdx.y; r < p.rows;
       r += static_cast<long long>(gridDim.y) * CSC_ROWS) {
    const unsigned n = static_cast<unsigned>(r) / static_cast<unsigned>(p.H);
    const unsigned i = static_cast<unsigned>(r) - n * static_cast<unsigned>(p.H);
    const long long px = r * p.W + x0;
    float yy[CSC_PX], cb[CSC_PX], cr[CSC_PX];
    if (p.vec) {
      const uint2 v = load8(p.y + px);
      const unsigned w[2] = {v.x, v.y};
#pragma unroll
      for (int k = 0; k < CSC_PX; ++k) yy[k] = byte_of(w[k >> 2], k & 3);
    } else {
#pragma unroll
      for (int k = 0; k < CSC_PX; ++k) yy[k] = p.y[px + min(k, npx - 1)];
    }
    load_chroma<MODE>(p, n, i, x0, cb, cr);
    float o[3 * CSC_PX];
#pragma unroll
    for (int k = 0; k < CSC_PX; ++k) {
      const float yl = fmaf(yy[k], p.y_scale, p.y_off);
      const float b = cb[k] - 128.f, rr = cr[k] - 128.f;
      float vr = fmaf(p.k0, rr, yl);
      float vg = fmaf(-p.k2, b, fmaf(-p.k1, rr, yl));
      float vb = fmaf(p.k3, b, yl);
      if (OUT != CSC_U8 && p.clip) {       // uint8 clamps where it rounds
        vr = clamp255(vr);
        vg = clamp255(vg);
        vb = clamp255(vb);
      }
      o[3 * k] = vr;
      o[3 * k + 1] = vg;
      o[3 * k + 2] = vb;
    }
    if (OUT == CSC_U8) {
      u8* op = static_cast<u8*>(p.rgb) + 3 * px;
      if (p.vec) {
        unsigned w[6];
#pragma unroll
        for (int d = 0; d < 6; ++d)
          w[d] = to_u8(o[4 * d]) | (to_u8(o[4 * d + 1]) << 8) | (to_u8(o[4 * d + 2]) << 16) | (to_u8(o[4 * d + 3]) << 24);
        store8(op, make_uint2(w[0], w[1]));
        store8(op + 8, make_uint2(w[2], w[3]));
        store8(op + 16, make_uint2(w[4], w[5]));
      } else {
#pragma unroll
        for (int e = 0; e < 3 * CSC_PX; ++e)
          if (e < 3 * npx) op[e] = static_cast<u8>(to_u8(o[e]));
      }
    } else if (OUT == CSC_F32) {
      float* op = static_cast<float*>(p.rgb) + 3 * px;
      if (p.vec) {
#pragma unroll
        for (int d = 0; d < 6; ++d)
          *reinterpret_cast<float4*>(op + 4 * d) = make_float4(o[4 * d], o[4 * d + 1], o[4 * d + 2], o[4 * d + 3]);
      } else {
#pragma unroll
        for (int e = 0; e < 3 * CSC_PX; ++e)
          if (e < 3 * npx) op[e] = o[e];
      }
    } else {
      unsigned short* op = static_cast<unsigned short*>(p.rgb) + 3 * px;
      if (p.vec) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          uint4 w;
          w.x = pack_bf16(o[8 * d], o[8 * d + 1]);
          w.y = pack_bf16(o[8 * d + 2], o[8 * d + 3]);
          w.z = pack_bf16(o[8 * d + 4], o[8 * d + 5]);
          w.w = pack_bf16(o[8 * d + 6], o[8 * d + 7]);
          store16(op + 8 * d, w);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 3 * CSC_PX; ++e)
          if (e < 3 * npx) op[e] = float_to_bf16_bits(o[e]);
      }
    }
  }
}

// 8 pixels of one row as float, from any of the three input types
template <int IN>
__device__ __forceinline__ void load_rgb(const CscParams& p, long long px, int npx, float v[3 * CSC_PX]) {
  if (IN == CSC_U8) {
    const u8* ip = static_cast<const u8*>(p.rgb) + 3 * px;
    if (p.vec) {
      const uint2 a = load8(ip), b = load8(ip + 8), c = load8(ip + 16);
      const unsigned w[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
#pragma unroll
      for (int e = 0; e < 3 * CSC_PX; ++e) v[e] = byte_of(w[e >> 2], e & 3);
    } else {
#pragma unroll
      for (int e = 0; e < 3 * CSC_PX; ++e) v[e] = e < 3 * npx ? static_cast<float>(ip[e]) : 0.f;
    }
  } else if (IN == CSC_F32) {
    const float* ip = static_cast<const float*>(p.rgb) + 3 * px;
    if (p.vec) {
#pragma unroll
      for (int d = 0; d < 6; ++d) {
        const uint4 w = load16(reinterpret_cast<const u8*>(ip + 4 * d));
        v[4 * d] = __uint_as_float(w.x);
        v[4 * d + 1] = __uint_as_float(w.y);
        v[4 * d + 2] = __uint_as_float(w.z);
        v[4 * d + 3] = __uint_as_float(w.w);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 3 * CSC_PX; ++e) v[e] = e < 3 * npx ? ip[e] : 0.f;
    }
  } else {
    const unsigned short* ip = static_cast<const unsigned short*>(p.rgb) + 3 * px;
    if (p.vec) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const uint4 w = load16(reinterpret_cast<const u8*>(ip + 8 * d));
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int t = 0; t < 8; ++t) v[8 * d + t] = bf16_bits_to_float((ww[t >> 1] >> (16 * (t & 1))) & 0xffffu);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 3 * CSC_PX; ++e) v[e] = e < 3 * npx ? bf16_bits_to_float(ip[e]) : 0.f;
    }
  }
}

__device__ __forceinline__ void luma_chroma(const CscParams& p, const float v[3 * CSC_PX], float yl[CSC_PX],
                                            float cb[CSC_PX], float cr[CSC_PX]) {
#pragma unroll
  for (int k = 0; k < CSC_PX; ++k) {
    const float r = v[3 * k], g = v[3 * k + 1], b = v[3 * k + 2];
    yl[k] = fmaf(p.k2, b, fmaf(p.k1, g, p.k0 * r));
    cb[k] = (b - yl[k]) * p.icb;
    cr[k] = (r - yl[k]) * p.icr;
  }
}

__device__ __forceinline__ void store_luma(const CscParams& p, long long px, int npx, const float yl[CSC_PX]) {
  unsigned q[CSC_PX];
#pragma unroll
  for (int k = 0; k < CSC_PX; ++k) q[k] = to_u8(fmaf(yl[k], p.y_scale, p.y_off));
  if (p.vec) {
    store8(p.yo + px, make_uint2(q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24),
                                 q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24)));
  } else {
#pragma unroll
    for (int k = 0; k < CSC_PX; ++k)
      if (k < npx) p.yo[px + k] = static_cast<u8>(q[k]);
  }
}

template <int IN, bool SUB>
__global__ void __launch_bounds__(CSC_LANES * CSC_ROWS) rgb_to_ycbcr_kernel(CscParams p) {
  const int g = blockIdx.x * CSC_LANES + threadIdx.x;
  if (g >= p.gpr) return;
  const int x0 = g * CSC_PX;
  const int npx = min(CSC_PX, p.W - x0);
  for (long long r = static_cast<long long>(blockIdx.y) * CSC_ROWS + threadIdx.y; r < p.rows;
       r += static_cast<long long>(gridDim.y) * CSC_ROWS) {
    float v[3 * CSC_PX], yl[CSC_PX], cb[CSC_PX], cr[CSC_PX];
    if (!SUB) {
      const long long px = r * p.W + x0;
      load_rgb<IN>(p, px, npx, v);
      luma_chroma(p, v, yl, cb, cr);
      store_luma(p, px, npx, yl);
      unsigned q[2 * CSC_PX];
#pragma unroll
      for (int k = 0; k < CSC_PX; ++k) {
        q[2 * k] = to_u8(fmaf(cb[k], p.c_scale, 128.f));
        q[2 * k + 1] = to_u8(fmaf(cr[k], p.c_scale, 128.f));
      }
      u8* cp = p.co + 2 * px;
      if (p.vec) {
        uint4 w;
        w.x = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
        w.y = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
        w.z = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
        w.w = q[12] | (q[13] << 8) | (q[14] << 16) | (q[15] << 24);
        store16(cp, w);
      } else {
#pragma unroll
        for (int e = 0; e < 2 * CSC_PX; ++e)
          if (e < 2 * npx) cp[e] = static_cast<u8>(q[e]);
      }
    } else {
      // r counts row pairs: luma rows 2 r and 2 r + 1, chroma row r (p.rows = N H / 2, so frames do not mix)
      const long long px = 2 * r * p.W + x0;
      float sb[CSC_PX / 2], sr[CSC_PX / 2];
      load_rgb<IN>(p, px, npx, v);
      luma_chroma(p, v, yl, cb, cr);
      store_luma(p, px, npx, yl);
#pragma unroll
      for (int q = 0; q < CSC_PX / 2; ++q) {
        sb[q] = cb[2 * q] + cb[2 * q + 1];
        sr[q] = cr[2 * q] + cr[2 * q + 1];
      }
      load_rgb<IN>(p, px + p.W, npx, v);
      luma_chroma(p, v, yl, cb, cr);
      store_luma(p, px + p.W, npx, yl);
      unsigned q8[CSC_PX];
#pragma unroll
      for (int q = 0; q < CSC_PX / 2; ++q) {
        const float mb = 0.25f * (sb[q] + (cb[2 * q] + cb[2 * q + 1]));
        const float mr = 0.25f * (sr[q] + (cr[2 * q] + cr[2 * q + 1]));
        q8[2 * q] = to_u8(fmaf(mb, p.c_scale, 128.f));
        q8[2 * q + 1] = to_u8(fmaf(mr, p.c_scale, 128.f));
      }
      u8* cp = p.co + (r * p.cw + (x0 >> 1)) * 2;
      if (p.vec) {
        store8(cp, make_uint2(q8[0] | (q8[1] << 8) | (q8[2] << 16) | (q8[3] << 24),
                              q8[4] | (q8[5] << 8) | (q8[6] << 16) | (q8[7] << 24)));
      } else {
#pragma unroll
        for (int e = 0; e < CSC_PX; ++e)
          if (e < npx) cp[e] = static_cast<u8>(q8[e]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Host side

struct FrameShape {
  long long ys, cs, frame_bytes;
  int cw, ch;
};

// chroma is 420 or 444, as the header's C parameter reads
int frame_shape(const char* name, int64_t n, int64_t w, int64_t h, int chroma, FrameShape* s) {
  if (n < 0) return fail("%s: num_frames must not be negative, got %lld", name, static_cast<long long>(n));
  if (w < 1 || h < 1 || w > (1 << 20) || h > (1 << 20))
    return fail("%s: width and height must be in [1, 2^20], got %lld x %lld", name, static_cast<long long>(w),
                static_cast<long long>(h));
  if (chroma != 420 && chroma != 444) return fail("%s: chroma must be 420 or 444, got %d", name, chroma);
  if (chroma == 420 && ((w | h) & 1))
    return fail("%s: 4:2:0 chroma format, but odd width or height (%lld x %lld)", name, static_cast<long long>(w),
                static_cast<long long>(h));
  if (n * h >= (1ll << 31)) return fail("%s: num_frames * height must be below 2^31", name);
  s->cw = static_cast<int>(chroma == 420 ? w / 2 : w);
  s->ch = static_cast<int>(chroma == 420 ? h / 2 : h);
  s->ys = w * h;
  s->cs = static_cast<long long>(s->cw) * s->ch;
  s->frame_bytes = s->ys + 2 * s->cs;
  return 0;
}

int plane_params(const char* name, const void* raw, int64_t raw_bytes, int64_t n, int64_t w, int64_t h, int chroma,
                 int64_t stride, int64_t first, const void* y, const void* c, PlaneParams* p) {
  FrameShape s;
  if (int rc = frame_shape(name, n, w, h, chroma, &s)) return rc;
  if (stride < s.frame_bytes)
    return fail("%s: frame_stride %lld is less than the %lld bytes of a frame", name, static_cast<long long>(stride),
                s.frame_bytes);
  if (first < 0) return fail("%s: first_offset must not be negative, got %lld", name, static_cast<long long>(first));
  if (n > 0 && raw_bytes < first + (n - 1) * stride + s.frame_bytes)
    return fail("%s: %lld frames of stride %lld from byte %lld need %lld bytes, the buffer has %lld", name,
                static_cast<long long>(n), static_cast<long long>(stride), static_cast<long long>(first),
                static_cast<long long>(first + (n - 1) * stride + s.frame_bytes), static_cast<long long>(raw_bytes));
  if (n > 0 && (!raw || !y || !c)) return fail("%s: raw, y and cbcr must not be null", name);
  if (reinterpret_cast<uintptr_t>(c) & 1) return fail("%s: cbcr must be 2-byte aligned", name);
  p->raw = static_cast<u8*>(const_cast<void*>(raw));
  p->y = static_cast<u8*>(const_cast<void*>(y));
  p->c = static_cast<u8*>(const_cast<void*>(c));
  p->ys = s.ys; p->cs = s.cs;
  p->stride = stride; p->first = first;
  p->N = n;
  return 0;
}

dim3 plane_grid(long long lanes, long long n) {
  return dim3(static_cast<unsigned>(ceil_div(lanes, Y4M_THREADS)), static_cast<unsigned>(std::min<long long>(n, 65535)));
}

struct Matrix { double kr, kb; };

int csc_params(const char* name, int64_t n, int64_t w, int64_t h, int chroma, int matrix, int full_range, int dtype,
               FrameShape* s, Matrix* m, CscParams* p) {
  if (int rc = frame_shape(name, n, w, h, chroma, s)) return rc;
  if (matrix != 0 && matrix != 1) return fail("%s: matrix must be 0 (bt601) or 1 (bt709), got %d", name, matrix);
  if (full_range != 0 && full_range != 1) return fail("%s: full_range must be 0 or 1, got %d", name, full_range);
  if (dtype != CSC_U8 && dtype != CSC_F32 && dtype != CSC_BF16)
    return fail("%s: dtype must be 0 (uint8), 1 (float32) or 2 (bfloat16), got %d", name, dtype);
  *m = matrix == 0 ? Matrix{0.299, 0.114} : Matrix{0.2126, 0.0722};
  p->W = static_cast<int>(w); p->H = static_cast<int>(h);
  p->cw = s->cw; p->ch = s->ch;
  p->gpr = static_cast<int>(ceil_div(w, CSC_PX));
  return 0;
}

dim3 csc_grid(const CscParams& p) {
  return dim3(static_cast<unsigned>(ceil_div(p.gpr, CSC_LANES)),
              static_cast<unsigned>(std::min<long long>(ceil_div(p.rows, CSC_ROWS), 65535)));
}

bool aligned(const void* ptr, int to) { return reinterpret_cast<uintptr_t>(ptr) % to == 0; }

}  // namespace
}  // namespace tfc

extern "C" int tfc_y4m_unpack(const void* raw, int64_t raw_bytes, int64_t num_frames, int64_t width, int64_t height,
                              int chroma, int64_t frame_stride, int64_t first_offset, void* y, void* cbcr,
                              void* stream) {
  using namespace tfc;
  PlaneParams p = {};
  if (int rc = plane_params("tfc_y4m_unpack", raw, raw_bytes, num_frames, width, height, chroma, frame_stride,
                            first_offset, y, cbcr, &p))
    return rc;
  if (num_frames == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  p.ty = p.ys / 16 + Y4M_EDGE;
  p.tc = p.cs / 8 + Y4M_EDGE;
  KernelTimer timer("y4m_unpack", st);
  hipLaunchKernelGGL(y4m_unpack_kernel, plane_grid(p.ty + p.tc, p.N), dim3(Y4M_THREADS), 0, st, p);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_y4m_pack(const void* y, const void* cbcr, void* raw, int64_t raw_bytes, int64_t num_frames,
                            int64_t width, int64_t height, int chroma, int64_t frame_stride, int64_t first_offset,
                            void* stream) {
  using namespace tfc;
  PlaneParams p = {};
  if (int rc = plane_params("tfc_y4m_pack", raw, raw_bytes, num_frames, width, height, chroma, frame_stride,
                            first_offset, y, cbcr, &p))
    return rc;
  if (num_frames == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  p.ty = p.ys / 16 + Y4M_EDGE;
  p.tc = p.cs / 16 + Y4M_EDGE;
  KernelTimer timer("y4m_pack", st);
  hipLaunchKernelGGL(y4m_pack_kernel, plane_grid(p.ty + 2 * p.tc, p.N), dim3(Y4M_THREADS), 0, st, p);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_ycbcr_to_rgb(const void* y, const void* cbcr, void* rgb, int64_t num_frames, int64_t width,
                                int64_t height, int chroma, int matrix, int full_range, int upsample, int dtype,
                                int clip, void* stream) {
  using namespace tfc;
  FrameShape s;
  Matrix m;
  CscParams p = {};
  if (int rc = csc_params("tfc_ycbcr_to_rgb", num_frames, width, height, chroma, matrix, full_range, dtype, &s, &m, &p))
    return rc;
  if (upsample != 0 && upsample != 1)
    return fail("tfc_ycbcr_to_rgb: upsample must be 0 (nearest) or 1 (bilinear), got %d", upsample);
  if (num_frames == 0) return 0;
  if (!y || !cbcr || !rgb) return fail("tfc_ycbcr_to_rgb: y, cbcr and rgb must not be null");
  const int elem = dtype == CSC_U8 ? 1 : dtype == CSC_F32 ? 4 : 2;
  if (!aligned(rgb, elem)) return fail("tfc_ycbcr_to_rgb: rgb is not aligned to its element size");
  const double kr = m.kr, kb = m.kb, kg = 1.0 - kr - kb;
  p.y = static_cast<const u8*>(y); p.c = static_cast<const u8*>(cbcr); p.rgb = rgb;
  p.rows = num_frames * height;
  p.vec = width % CSC_PX == 0 && aligned(rgb, dtype == CSC_U8 ? 8 : 16);
  p.clip = clip != 0;
  const double ys = full_range ? 1.0 : 255.0 / 219.0, cs = full_range ? 1.0 : 255.0 / 224.0;
  p.y_scale = static_cast<float>(ys);
  p.y_off = static_cast<float>(full_range ? 0.0 : -16.0 * ys);
  p.k0 = static_cast<float>(cs * 2.0 * (1.0 - kr));
  p.k1 = static_cast<float>(cs * 2.0 * kr * (1.0 - kr) / kg);
  p.k2 = static_cast<float>(cs * 2.0 * kb * (1.0 - kb) / kg);
  p.k3 = static_cast<float>(cs * 2.0 * (1.0 - kb));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int mode = chroma == 444 ? CSC_444 : upsample ? CSC_420_BILINEAR : CSC_420_NEAREST;
  KernelTimer timer("ycbcr_to_rgb", st);
  const dim3 grid = csc_grid(p), block(CSC_LANES, CSC_ROWS);
#define TFC_CSC_TO_RGB(OUT, MODE)                                                            \
  if (dtype == OUT && mode == MODE) hipLaunchKernelGGL((ycbcr_to_rgb_kernel<OUT, MODE>), grid, block, 0, st, p);
  TFC_CSC_TO_RGB(CSC_U8, CSC_444) TFC_CSC_TO_RGB(CSC_U8, CSC_420_NEAREST) TFC_CSC_TO_RGB(CSC_U8, CSC_420_BILINEAR)
  TFC_CSC_TO_RGB(CSC_F32, CSC_444) TFC_CSC_TO_RGB(CSC_F32, CSC_420_NEAREST) TFC_CSC_TO_RGB(CSC_F32, CSC_420_BILINEAR)
  TFC_CSC_TO_RGB(CSC_BF16, CSC_444) TFC_CSC_TO_RGB(CSC_BF16, CSC_420_NEAREST) TFC_CSC_TO_RGB(CSC_BF16, CSC_420_BILINEAR)
#undef TFC_CSC_TO_RGB
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_rgb_to_ycbcr(const void* rgb, int dtype, void* y, void* cbcr, int64_t num_frames, int64_t width,
                                int64_t height, int chroma, int matrix, int full_range, void* stream) {
  using namespace tfc;
  FrameShape s;
  Matrix m;
  CscParams p = {};
  if (int rc = csc_params("tfc_rgb_to_ycbcr", num_frames, width, height, chroma, matrix, full_range, dtype, &s, &m, &p))
    return rc;
  if (num_frames == 0) return 0;
  if (!y || !cbcr || !rgb) return fail("tfc_rgb_to_ycbcr: rgb, y and cbcr must not be null");
  const int elem = dtype == CSC_U8 ? 1 : dtype == CSC_F32 ? 4 : 2;
  if (!aligned(rgb, elem)) return fail("tfc_rgb_to_ycbcr: rgb is not aligned to its element size");
  const double kr = m.kr, kb = m.kb, kg = 1.0 - kr - kb;
  const bool sub = chroma == 420;
  p.rgb = const_cast<void*>(rgb); p.yo = static_cast<u8*>(y); p.co = static_cast<u8*>(cbcr);
  p.rows = sub ? num_frames * height / 2 : num_frames * height;
  p.vec = width % CSC_PX == 0 && aligned(y, 8) && aligned(cbcr, 16);
  p.y_off = full_range ? 0.f : 16.f;
  p.y_scale = full_range ? 1.f : static_cast<float>(219.0 / 255.0);
  p.c_scale = full_range ? 1.f : static_cast<float>(224.0 / 255.0);
  p.k0 = static_cast<float>(kr); p.k1 = static_cast<float>(kg); p.k2 = static_cast<float>(kb);
  p.icb = static_cast<float>(1.0 / (2.0 * (1.0 - kb)));
  p.icr = static_cast<float>(1.0 / (2.0 * (1.0 - kr)));
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer("rgb_to_ycbcr", st);
  const dim3 grid = csc_grid(p), block(CSC_LANES, CSC_ROWS);
#define TFC_CSC_FROM_RGB(IN)                                                                              \
  if (dtype == IN) {                                                                                      \
    if (sub) hipLaunchKernelGGL((rgb_to_ycbcr_kernel<IN, true>), grid, block, 0, st, p);                   \
    else hipLaunchKernelGGL((rgb_to_ycbcr_kernel<IN, false>), grid, block, 0, st, p);                      \
  }
  TFC_CSC_FROM_RGB(CSC_U8) TFC_CSC_FROM_RGB(CSC_F32) TFC_CSC_FROM_RGB(CSC_BF16)
#undef TFC_CSC_FROM_RGB
  TFC_HIP(hipGetLastError());
  return 0;
}
