// The training loop's two streaming kernels: the random crops of the input pipeline (models/bls2017.py:198-232, where
// tf.image.random_crop runs per image on host threads) and the optimiser step (tf.keras.optimizers.Adam; the reference
// leaves both to TensorFlow).
//
//   * crop_patches_kernel<OUT>: B patches [P, P, 3] out of decoded images that lie back to back in one byte pool.  The
//     output [B, P, P, 3] is one contiguous array, so a lane owns one aligned 16-byte piece of it (16 uint8, 8 bfloat16
//     or 4 float32 values) and finds the source byte of its first value from the patch's table row.  A piece that lies
//     within one patch row takes ONE load of its 16, 8 or 4 source bytes from whatever address they have (gfx950
//     serves unaligned global loads); a piece that runs over the end of a row, and the last partial piece, take one
//     byte load per value.  Only bytes of patch rows are ever read, so nothing outside [0, pool bytes) is touched; a
//     table row that does not fit the pool yields zeros instead of a read (the Python op rejects it before the launch).
//   * keras_adam_kernel: one Adam step over up to TFC_KERAS_ADAM_CAPACITY tensors.  The tensor table and the chunk list
//     (the first chunk of every tensor) travel in the kernel arguments, so a launch needs no upload; a workgroup looks
//     its chunk up and streams p, g, m, v in 16-byte accesses: 16 bytes read and 12 written per parameter.
// No LDS, no atomics, no scratch.
#include "launch.h"
#include "../../include/tfc_hip.h"

namespace tfc {
namespace {

typedef unsigned char u8;

constexpr int CROP_THREADS = 256;
enum { CROP_U8 = 0, CROP_F32 = 1, CROP_BF16 = 2 };

struct CropParams {
  const u8* pool;
  long long pool_bytes;
  const long long* table;      // [B, 4]: byte offset of the image, its width, top, left
  void* out;
  unsigned total;              // B P P 3 values
  unsigned row;                // 3 P values of one patch row
  unsigned P;
};

// The source byte of output value e, or null where the table row does not fit the pool.
__device__ __forceinline__ const u8* crop_source(const CropParams& p, unsigned e, unsigned* col) {
  const unsigned R = e / p.row, c = e - R * p.row;
  const unsigned b = R / p.P, r = R - b * p.P;
  const long long* t = p.table + 4ll * b;
  const long long off = t[0], W = t[1], top = t[2], left = t[3];
  *col = c;
  if ((off | W | top | left) < 0) return nullptr;
  // the last byte the patch uses; the same expression as the host-side check, here against overflow as well
  if (W > (1ll << 24) || top > (1ll << 24) || left > (1ll << 24) || off > p.pool_bytes) return nullptr;
  const long long end = off + ((top + p.P - 1) * W + left + p.P) * 3;
  if (end > p.pool_bytes) return nullptr;
  return p.pool + off + ((top + r) * W + left) * 3 + c;
}

template <int OUT> struct CropGroup;
template <> struct CropGroup<CROP_U8> { static constexpr int n = 16; };
template <> struct CropGroup<CROP_BF16> { static constexpr int n = 8; };
template <> struct CropGroup<CROP_F32> { static constexpr int n = 4; };

template <int OUT>
__global__ void __launch_bounds__(CROP_THREADS) crop_patches_kernel(CropParams p) {
  constexpr int G = CropGroup<OUT>::n;
  const unsigned groups = (p.total + G - 1) / G;
  for (unsigned j = blockIdx.x * CROP_THREADS + threadIdx.x; j < groups; j += gridDim.x * CROP_THREADS) {
    const unsigned e0 = j * G;
    const bool full = p.total - e0 >= static_cast<unsigned>(G);
    unsigned c;
    const u8* src = crop_source(p, e0, &c);
    unsigned w[4] = {0u, 0u, 0u, 0u};      // the G source bytes, little endian
    if (full && c + G <= p.row) {
      if (src) __builtin_memcpy(w, src, G);
    } else {
#pragma unroll
      for (int k = 0; k < G; ++k) {
        if (e0 + k < p.total) {
          unsigned ck;
          const u8* s = crop_source(p, e0 + k, &ck);
          if (s) w[k >> 2] |= static_cast<unsigned>(*s) << (8 * (k & 3));
        }
      }
    }
    if (OUT == CROP_U8) {
      u8* o = static_cast<u8*>(p.out) + e0;
      if (full) {
        *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
#pragma unroll
        for (int k = 0; k < G; ++k)
          if (e0 + k < p.total) o[k] = static_cast<u8>(w[k >> 2] >> (8 * (k & 3)));
      }
    } else if (OUT == CROP_BF16) {
      // an integer below 256 has at most 8 significant bits: the upper half of its float32 form is its bfloat16 form
      unsigned short h[G];
#pragma unroll
      for (int k = 0; k < G; ++k)
        h[k] = static_cast<unsigned short>(__float_as_uint(static_cast<float>((w[k >> 2] >> (8 * (k & 3))) & 0xffu)) >> 16);
      unsigned short* o = static_cast<unsigned short*>(p.out) + e0;
      if (full) {
        *reinterpret_cast<uint4*>(o) = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16),
                                                  h[6] | (h[7] << 16));
      } else {
#pragma unroll
        for (int k = 0; k < G; ++k)
          if (e0 + k < p.total) o[k] = h[k];
      }
    } else {
      float f[G];
#pragma unroll
      for (int k = 0; k < G; ++k) f[k] = static_cast<float>((w[0] >> (8 * k)) & 0xffu);
      float* o = static_cast<float*>(p.out) + e0;
      if (full) {
        *reinterpret_cast<float4*>(o) = make_float4(f[0], f[1], f[2], f[3]);
      } else {
#pragma unroll
        for (int k = 0; k < G; ++k)
          if (e0 + k < p.total) o[k] = f[k];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Keras Adam

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_CAP = TFC_KERAS_ADAM_CAPACITY;
constexpr int ADAM_CHUNK = TFC_KERAS_ADAM_CHUNK;
static_assert(ADAM_CHUNK % (4 * ADAM_THREADS) == 0, "a chunk is a whole number of float4 per lane");

struct AdamTensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  long long numel;
};

struct AdamParams {
  AdamTensor t[ADAM_CAP];
  unsigned first[ADAM_CAP + 1];        // the chunk list: tensor k owns the chunks [first[k], first[k + 1])
  int count;
  float alpha, c1, c2, eps;
  const int* skip;
};
static_assert(sizeof(AdamParams) <= 4096, "the table travels in the kernel arguments");

// The rule of include/tfc_hip.h, every operation rounded on its own (no fused multiply-add).
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float alpha, float c1, float c2,
                                            float eps) {
#pragma clang fp contract(off)
  const float dm = g - m;
  const float sm = dm * c1;
  m = m + sm;
  const float gg = g * g;
  const float dv = gg - v;
  const float sv = dv * c2;
  v = v + sv;
  const float num = m * alpha;
  const float den = sqrtf(v) + eps;
  const float u = num / den;
  p = p - u;
}

__global__ void __launch_bounds__(ADAM_THREADS) keras_adam_kernel(AdamParams a) {
  if (a.skip && *a.skip != 0) return;
  // the tensor of this chunk: first[] ascends, zero-element tensors own no chunk
  const unsigned chunk = blockIdx.x;
  int lo = 0, hi = a.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.first[mid] <= chunk) lo = mid; else hi = mid;
  }
  const AdamTensor t = a.t[lo];
  const long long begin = static_cast<long long>(chunk - a.first[lo]) * ADAM_CHUNK;
  const long long len = min(static_cast<long long>(ADAM_CHUNK), t.numel - begin);
  float* p = t.p + begin;
  const float* g = t.g + begin;
  float* m = t.m + begin;
  float* v = t.v + begin;
  const bool wide = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                      reinterpret_cast<uintptr_t>(v)) & 15) == 0;
  const int quads = wide ? static_cast<int>(len >> 2) : 0;
  for (int q = threadIdx.x; q < quads; q += ADAM_THREADS) {
    float4 pp = reinterpret_cast<float4*>(p)[q];
    const float4 gg = reinterpret_cast<const float4*>(g)[q];
    float4 mm = reinterpret_cast<float4*>(m)[q];
    float4 vv = reinterpret_cast<float4*>(v)[q];
    adam_update(pp.x, gg.x, mm.x, vv.x, a.alpha, a.c1, a.c2, a.eps);
    adam_update(pp.y, gg.y, mm.y, vv.y, a.alpha, a.c1, a.c2, a.eps);
    adam_update(pp.z, gg.z, mm.z, vv.z, a.alpha, a.c1, a.c2, a.eps);
    adam_update(pp.w, gg.w, mm.w, vv.w, a.alpha, a.c1, a.c2, a.eps);
    reinterpret_cast<float4*>(p)[q] = pp;
    reinterpret_cast<float4*>(m)[q] = mm;
    reinterpret_cast<float4*>(v)[q] = vv;
  }
  // what is left of the chunk (all of it where a tensor is not 16-byte aligned), one value per lane
  for (int i = 4 * quads + threadIdx.x; i < len; i += ADAM_THREADS) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam_update(pp, g[i], mm, vv, a.alpha, a.c1, a.c2, a.eps);
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
  }
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_crop_patches(const void* pool, int64_t pool_bytes, const int64_t* table, int64_t num_patches,
                                int64_t patchsize, int dtype, void* out, void* stream) {
  using namespace tfc;
  if (num_patches < 0) return fail("tfc_crop_patches: num_patches must not be negative, got %lld",
                                   static_cast<long long>(num_patches));
  if (patchsize < 1 || patchsize > (1 << 15))
    return fail("tfc_crop_patches: patchsize must be in [1, 2^15], got %lld", static_cast<long long>(patchsize));
  if (pool_bytes < 0) return fail("tfc_crop_patches: pool_bytes must not be negative");
  if (dtype != CROP_U8 && dtype != CROP_F32 && dtype != CROP_BF16)
    return fail("tfc_crop_patches: dtype must be 0 (uint8), 1 (float32) or 2 (bfloat16), got %d", dtype);
  const long long total = num_patches * patchsize * patchsize * 3;
  if (num_patches > (1ll << 31) || total >= (1ll << 31))
    return fail("tfc_crop_patches: num_patches * patchsize^2 * 3 must be below 2^31, got %lld patches of %lld",
                static_cast<long long>(num_patches), static_cast<long long>(patchsize));
  if (num_patches == 0) return 0;
  if (!pool || !table || !out) return fail("tfc_crop_patches: pool, table and out must not be null");
  if (reinterpret_cast<uintptr_t>(table) & 7) return fail("tfc_crop_patches: table must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(out) & 15) return fail("tfc_crop_patches: out must be 16-byte aligned");
  CropParams p = {};
  p.pool = static_cast<const u8*>(pool);
  p.pool_bytes = pool_bytes;
  p.table = reinterpret_cast<const long long*>(table);
  p.out = out;
  p.total = static_cast<unsigned>(total);
  p.row = static_cast<unsigned>(3 * patchsize);
  p.P = static_cast<unsigned>(patchsize);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int group = dtype == CROP_U8 ? 16 : dtype == CROP_BF16 ? 8 : 4;
  const dim3 grid(static_cast<unsigned>(std::min<int64_t>(ceil_div(ceil_div(total, group), CROP_THREADS), 1 << 20)));
  KernelTimer timer("crop_patches", st);
  if (dtype == CROP_U8) hipLaunchKernelGGL(crop_patches_kernel<CROP_U8>, grid, dim3(CROP_THREADS), 0, st, p);
  if (dtype == CROP_F32) hipLaunchKernelGGL(crop_patches_kernel<CROP_F32>, grid, dim3(CROP_THREADS), 0, st, p);
  if (dtype == CROP_BF16) hipLaunchKernelGGL(crop_patches_kernel<CROP_BF16>, grid, dim3(CROP_THREADS), 0, st, p);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_keras_adam(void* const* params, const void* const* grads, void* const* ms, void* const* vs,
                              const int64_t* numels, int count, float alpha, float c1, float c2, float eps,
                              const int32_t* skip, void* stream) {
  using namespace tfc;
  if (count < 0 || count > ADAM_CAP)
    return fail("tfc_keras_adam: count must be in [0, %d], got %d", ADAM_CAP, count);
  if (count == 0) return 0;
  if (!params || !grads || !ms || !vs || !numels) return fail("tfc_keras_adam: the tensor lists must not be null");
  if (reinterpret_cast<uintptr_t>(skip) & 3) return fail("tfc_keras_adam: skip must be 4-byte aligned");
  AdamParams a = {};
  long long chunks = 0;
  for (int k = 0; k < count; ++k) {
    if (numels[k] < 0) return fail("tfc_keras_adam: tensor %d has a negative element count", k);
    if (numels[k] > 0 && (!params[k] || !grads[k] || !ms[k] || !vs[k]))
      return fail("tfc_keras_adam: tensor %d has a null pointer", k);
    if ((reinterpret_cast<uintptr_t>(params[k]) | reinterpret_cast<uintptr_t>(grads[k]) |
         reinterpret_cast<uintptr_t>(ms[k]) | reinterpret_cast<uintptr_t>(vs[k])) & 3)
      return fail("tfc_keras_adam: tensor %d is not 4-byte aligned", k);
    a.t[k].p = static_cast<float*>(params[k]);
    a.t[k].g = static_cast<const float*>(grads[k]);
    a.t[k].m = static_cast<float*>(ms[k]);
    a.t[k].v = static_cast<float*>(vs[k]);
    a.t[k].numel = numels[k];
    a.first[k] = static_cast<unsigned>(chunks);
    chunks += ceil_div(numels[k], ADAM_CHUNK);
    if (chunks > kMaxGridX) return fail("tfc_keras_adam: more than 2^31 chunks in one launch");
  }
  for (int k = count; k <= ADAM_CAP; ++k) a.first[k] = static_cast<unsigned>(chunks);
  if (chunks == 0) return 0;
  a.count = count;
  a.alpha = alpha; a.c1 = c1; a.c2 = c2; a.eps = eps;
  a.skip = skip;
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer("keras_adam", st);
  hipLaunchKernelGGL(keras_adam_kernel, dim3(static_cast<unsigned>(chunks)), dim3(ADAM_THREADS), 0, st, a);
  TFC_HIP(hipGetLastError());
  return 0;
}
