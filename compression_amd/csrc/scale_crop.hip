// HiFiC's training input (models/hific/model.py:316-351): every image is resized by a random factor with
// tf.image.resize_images (TF1 bilinear, align_corners=False, half_pixel_centers=False) on a host thread and ONE
// crop_size x crop_size patch of the result is kept.  Here the resize is folded into the crop:
//
//   * scale_crop_kernel<OUT>: B patches [P, P, 3] of the RESIZED images, computed straight from the decoded images in
//     the byte pool of csrc/train.hip.  Only the P x P output pixels are ever computed; the resized image never
//     exists.  As in crop_patches_kernel the output [B, P, P, 3] is one contiguous array and a lane owns one aligned
//     16-byte piece of it (4 float32 or 8 bfloat16 values), which spans at most 2 or 4 output pixels.  A pixel's
//     source coordinates, weights and four source pixels are computed once and serve its three channels; the walk
//     from one pixel of the piece to the next is an increment, the table row is read again only where the patch
//     changes.  Source reads are byte loads: neighbouring lanes read neighbouring pixels of the same two image rows,
//     which the vector cache serves.  Every float operation is rounded on its own (contraction is off for this
//     code), so the kernel is bit-identical to the tensor-op twin in ops/train_ops.py.  A table row that fails the
//     host-side conditions is not read from and yields zeros.
// No LDS, no atomics, no scratch.
#include "common.h"
#include "../../include/tfc_hip.h"

namespace tfc {
namespace {

typedef unsigned char u8;

constexpr int SCALE_CROP_THREADS = 256;
constexpr int SCALE_CROP_MAX_BLOCKS = 2048;       // 8 workgroups per CU; the grid-stride loop takes the rest
enum { SC_F32 = 1, SC_BF16 = 2 };                 // the dtype codes of tfc_crop_patches

struct ScaleCropParams {
  const u8* pool;
  long long pool_bytes;
  const long long* table;      // [B, 7]: byte offset of the image, W, H, resized OW, OH, top and left in the resized image
  void* out;
  unsigned total;              // B P P 3 values
  unsigned pixels;             // B P P
  unsigned P;
};

// One table row, ready for use: the image, the two scale factors and the patch's corner.
struct ScaleCropRow {
  const u8* image;             // null where the row does not fit
  int W, H, top, left;
  float sy, sx;
};

__device__ __forceinline__ ScaleCropRow scale_crop_row(const ScaleCropParams& p, unsigned b) {
  const long long* t = p.table + 7ll * b;
  const long long off = t[0], W = t[1], H = t[2], OW = t[3], OH = t[4], top = t[5], left = t[6];
  ScaleCropRow r;
  r.image = nullptr;
  r.W = r.H = 1;
  r.top = r.left = 0;
  r.sy = r.sx = 0.f;
  constexpr long long LIM = 1ll << 24;
  // the host-side conditions (ops/train_ops.py), in an order that cannot overflow
  if ((off | W | H | OW | OH | top | left) < 0) return r;
  if (W < 1 || H < 1 || OW < 1 || OH < 1 || W > LIM || H > LIM || OW > LIM || OH > LIM) return r;
  if (top + p.P > OH || left + p.P > OW) return r;
  if (off > p.pool_bytes || off + 3 * W * H > p.pool_bytes) return r;
  r.image = p.pool + off;
  r.W = static_cast<int>(W);
  r.H = static_cast<int>(H);
  r.top = static_cast<int>(top);
  r.left = static_cast<int>(left);
  r.sy = __fdiv_rn(static_cast<float>(H), static_cast<float>(OH));
  r.sx = __fdiv_rn(static_cast<float>(W), static_cast<float>(OW));
  return r;
}

// The three channels of output pixel (i, j) of the patch of row r: include/tfc_hip.h, every operation rounded alone.
__device__ __forceinline__ void scale_crop_pixel(const ScaleCropRow& r, unsigned i, unsigned j, float* v) {
#pragma clang fp contract(off)
  if (!r.image) {
    v[0] = v[1] = v[2] = 0.f;
    return;
  }
  const float py = static_cast<float>(r.top + static_cast<int>(i)) * r.sy;
  const float px = static_cast<float>(r.left + static_cast<int>(j)) * r.sx;
  // the minimum is taken on the floats: both sides are whole numbers, and a product past the int range cannot pass
  const float y0f = fminf(floorf(py), static_cast<float>(r.H - 1));
  const float x0f = fminf(floorf(px), static_cast<float>(r.W - 1));
  const float wy = py - y0f, wx = px - x0f;
  const int y0 = static_cast<int>(y0f), x0 = static_cast<int>(x0f);
  const int y1 = min(y0 + 1, r.H - 1), x1 = min(x0 + 1, r.W - 1);
  const long long W3 = 3ll * r.W;
  const u8* top_row = r.image + y0 * W3;
  const u8* bottom_row = r.image + y1 * W3;
  const u8* tl = top_row + 3 * x0;
  const u8* tr = top_row + 3 * x1;
  const u8* bl = bottom_row + 3 * x0;
  const u8* br = bottom_row + 3 * x1;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = static_cast<float>(tl[c]), b = static_cast<float>(tr[c]);
    const float d = static_cast<float>(bl[c]), e = static_cast<float>(br[c]);
    const float dt = b - a;
    const float mt = dt * wx;
    const float t = a + mt;
    const float db = e - d;
    const float mb = db * wx;
    const float bo = d + mb;
    const float dv = bo - t;
    const float mv = dv * wy;
    v[c] = t + mv;
  }
}

// float32 -> bfloat16, round to nearest even; the values here are finite.  Deliberately not bf16_io.h's hardware convert:
// integer arithmetic, three instructions, another answer on NaN — the bits the tests pin come from this.
__device__ __forceinline__ unsigned bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

template <int OUT> struct ScaleCropGroup;
template <> struct ScaleCropGroup<SC_F32> { static constexpr int n = 4; };
template <> struct ScaleCropGroup<SC_BF16> { static constexpr int n = 8; };

template <int OUT>
__global__ void __launch_bounds__(SCALE_CROP_THREADS) scale_crop_kernel(ScaleCropParams p) {
  constexpr int G = ScaleCropGroup<OUT>::n;
  constexpr int NP = (G + 1) / 3 + 1;      // a piece of G values that starts at channel 2 touches this many pixels
  const unsigned groups = (p.total + G - 1) / G;
  const unsigned PP = p.P * p.P;
  for (unsigned g = blockIdx.x * SCALE_CROP_THREADS + threadIdx.x; g < groups; g += gridDim.x * SCALE_CROP_THREADS) {
    const unsigned e0 = g * G;
    const unsigned q0 = e0 / 3u, ch0 = e0 - 3u * q0;      // the first pixel of the piece and the channel it starts at
    unsigned b = q0 / PP;
    const unsigned rest = q0 - b * PP;
    unsigned i = rest / p.P, j = rest - i * p.P;
    ScaleCropRow row = scale_crop_row(p, b);
    float f[3 * NP];
#pragma unroll
    for (int n = 0; n < NP; ++n) {
      if (n > 0) {
        if (++j == p.P) {
          j = 0;
          if (++i == p.P) {
            i = 0;
            ++b;
            if (q0 + n < p.pixels) row = scale_crop_row(p, b);
          }
        }
      }
      // pixel n is wanted if the piece reaches it and it exists
      if (3u * n < ch0 + G && q0 + n < p.pixels) {
        scale_crop_pixel(row, i, j, f + 3 * n);
      } else {
        f[3 * n] = f[3 * n + 1] = f[3 * n + 2] = 0.f;
      }
    }
    // value k of the piece is f[ch0 + k]: a choice of three, no indexed register array
    float v[G];
#pragma unroll
    for (int k = 0; k < G; ++k) v[k] = ch0 == 0 ? f[k] : ch0 == 1 ? f[k + 1] : f[k + 2];
    const bool full = p.total - e0 >= static_cast<unsigned>(G);
    if constexpr (OUT == SC_F32) {
      float* o = static_cast<float*>(p.out) + e0;
      if (full) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int k = 0; k < G; ++k)
          if (e0 + k < p.total) o[k] = v[k];
      }
    } else {
      unsigned h[G];
#pragma unroll
      for (int k = 0; k < G; ++k) h[k] = bf16_bits(v[k]);
      unsigned short* o = static_cast<unsigned short*>(p.out) + e0;
      if (full) {
        *reinterpret_cast<uint4*>(o) = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16),
                                                  h[6] | (h[7] << 16));
      } else {
#pragma unroll
        for (int k = 0; k < G; ++k)
          if (e0 + k < p.total) o[k] = static_cast<unsigned short>(h[k]);
      }
    }
  }
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_scale_crop_patches(const void* pool, int64_t pool_bytes, const int64_t* table, int64_t num_patches,
                                      int64_t patchsize, int dtype, void* out, void* stream) {
  using namespace tfc;
  if (num_patches < 0) return fail("tfc_scale_crop_patches: num_patches must not be negative, got %lld",
                                   static_cast<long long>(num_patches));
  if (patchsize < 1 || patchsize > (1 << 15))
    return fail("tfc_scale_crop_patches: patchsize must be in [1, 2^15], got %lld", static_cast<long long>(patchsize));
  if (pool_bytes < 0) return fail("tfc_scale_crop_patches: pool_bytes must not be negative");
  if (dtype != SC_F32 && dtype != SC_BF16)
    return fail("tfc_scale_crop_patches: dtype must be 1 (float32) or 2 (bfloat16), got %d", dtype);
  const long long total = num_patches * patchsize * patchsize * 3;
  if (num_patches > (1ll << 31) || total >= (1ll << 31))
    return fail("tfc_scale_crop_patches: num_patches * patchsize^2 * 3 must be below 2^31, got %lld patches of %lld",
                static_cast<long long>(num_patches), static_cast<long long>(patchsize));
  if (num_patches == 0) return 0;
  if (!pool || !table || !out) return fail("tfc_scale_crop_patches: pool, table and out must not be null");
  if (reinterpret_cast<uintptr_t>(table) & 7) return fail("tfc_scale_crop_patches: table must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(out) & 15) return fail("tfc_scale_crop_patches: out must be 16-byte aligned");
  ScaleCropParams p = {};
  p.pool = static_cast<const u8*>(pool);
  p.pool_bytes = pool_bytes;
  p.table = reinterpret_cast<const long long*>(table);
  p.out = out;
  p.total = static_cast<unsigned>(total);
  p.pixels = static_cast<unsigned>(total / 3);
  p.P = static_cast<unsigned>(patchsize);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int group = dtype == SC_BF16 ? 8 : 4;
  const dim3 grid(static_cast<unsigned>(
      std::min<int64_t>(ceil_div(ceil_div(total, group), SCALE_CROP_THREADS), SCALE_CROP_MAX_BLOCKS)));
  KernelTimer timer("scale_crop_patches", st);
  if (dtype == SC_F32) hipLaunchKernelGGL(scale_crop_kernel<SC_F32>, grid, dim3(SCALE_CROP_THREADS), 0, st, p);
  if (dtype == SC_BF16) hipLaunchKernelGGL(scale_crop_kernel<SC_BF16>, grid, dim3(SCALE_CROP_THREADS), 0, st, p);
  TFC_HIP(hipGetLastError());
  return 0;
}
