// SignalConv2D for gfx950: 2-D, non-separable, `same_zeros`, NHWC
// (python/layers/signal_conv.py:663-690 `_correlate_down_explicit` and
//  :778-847 `_up_convolve_transpose_explicit`, extra_pad_end=True).
//
// ONE implicit-GEMM kernel serves both directions:
//   down (analysis):  y[q] = sum_u x[q*sd + u - k/2] * w[u]            (cross-correlation)
//   up (synthesis):   y[q*s + phi] = sum_i x[i] * w[phi + (q-i)*s + k/2]  (transposed conv)
// The upsampled convolution is decomposed into its s*s output phases; each phase
// is a small stride-1 correlation over the LOW-resolution input, and the phases
// become extra output columns (N' = s*s*Cout) that the epilogue scatters back
// (depth-to-space).  No zero-insertion, no wasted multiplies on inserted zeros.
//
// GEMM orientation is the same as in gdn.hip: D^T = W'^T * patches^T, i.e. the
// MFMA A operand is the packed weight tile (rows = output columns) staged in
// LDS, the B operand is 8 consecutive input channels of ONE pixel per lane —
// a plain 16-byte load from the NHWC tensor, zero-filled outside the image.
// A lane therefore ends up with groups of 4 consecutive output channels of one
// pixel, which leave as 8/16-byte stores after bias (+ ReLU).
//
// bf16: v_mfma_f32_32x32x16_bf16, fp32 accumulate.  f32: v_mfma_f32_32x32x2_f32
// (exact fp32 FMA chains; 1/16 of the bf16 rate) for the parity path.
// Cin must be a multiple of 16, or <= 4 (image input: the host packs it to a
// zero-bordered 4-channel buffer and whole kernel rows become contiguous K runs).
// Roofline: MFMA-bound, 2*M*K*N FLOP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "conv_shared.h"
#include "gdn_params.h"

namespace tfc {

WeightsCache& WeightsCache::get() {
  static WeightsCache* c = new WeightsCache;               // leaked: entries may outlive static destruction order
  return *c;
}
// set by tfc_conv2d_weights_key, taken (and cleared) by the thread's next tfc_conv2d_* call
static thread_local unsigned long long t_next_weights_key = 0;

constexpr int kConvWaves = 4;          // pixel tiles (32 px) per workgroup
#ifndef TFC_CONV_MAX_TILES
#define TFC_CONV_MAX_TILES 6
#endif
constexpr int kMaxTiles = TFC_CONV_MAX_TILES;   // 32-column tiles per column group (6: 192 columns)

template <typename T> struct ConvTraits;
template <> struct ConvTraits<__bf16> {
  static constexpr int kFragBytes = 16;        // A fragment bytes per lane per K step per tile
};
template <> struct ConvTraits<float> {
  static constexpr int kFragBytes = 32;
};

// ---------------------------------------------------------------------------
// Weight packing: A fragments in the order the main kernel reads them:
//   packed[((group * ksteps + ks) * tiles + t) * 64 + lane]  (16 B bf16 / 32 B f32)
// lane (i = lane & 31, h = lane >> 5), element e (0..7): K offset 8h + e of step ks,
// output column group*tiles*32 + 32 t + i.
// ---------------------------------------------------------------------------
// (TFC_CONV_XCD=0 in the environment: workgroup id = work item, for same-box comparisons)
inline int xcd_blocks() {
  static const int on = env_switch("TFC_CONV_XCD") != 0;
  return on;
}

__device__ inline float packed_weight(const float* w, const PackGeom& g, const ConvGeom& c, int ks,
                                      int koff, int col) {
  if (col >= c.cols) return 0.f;
  int uy, ux, ci;
  if (c.small_cin) {
    uy = ks / c.kw4;
    const int o = (ks % c.kw4) * 16 + koff;
    ux = o >> 2;
    ci = o & 3;
    if (ux >= c.Ux || ci >= g.Cin_real) return 0.f;
  } else if (c.cbmajor) {
    const int grp = col / (c.tiles * 32);
    const int wx = c.tx1[grp] - c.tx0[grp];
    const int nt = (c.ty1[grp] - c.ty0[grp]) * wx;
    const int cbi = ks / nt, tap = ks % nt;
    if (cbi >= c.Cin / 16) return 0.f;
    uy = c.ty0[grp] + tap / wx;
    ux = c.tx0[grp] + tap % wx;
    ci = cbi * 16 + koff;
  } else if (c.compact) {
    const int grp = col / (c.tiles * 32);
    const int cb = c.Cin / 16;
    const int tap = ks / cb;
    const int wx = c.tx1[grp] - c.tx0[grp];
    uy = c.ty0[grp] + tap / wx;
    ux = c.tx0[grp] + tap % wx;
    if (uy >= c.ty1[grp]) return 0.f;
    ci = (ks % cb) * 16 + koff;
  } else {
    const int cb = c.Cin / 16;
    const int tap = ks / cb;
    uy = tap / c.Ux;
    ux = tap % c.Ux;
    ci = (ks % cb) * 16 + koff;
  }
  const int co = col % g.Cout;
  int ty, tx;
  if (g.up) {
    const int phase = col / g.Cout;
    const int phy = phase / g.su, phx = phase % g.su;
    // tap u reads input i = q + u - dmax, i.e. d = q - i = dmax - u; kernel index t = phi + d*s + k/2
    ty = phy + (g.dmax_y - uy) * g.su + g.kh / 2;
    tx = phx + (g.dmax_x - ux) * g.su + g.kw / 2;
    if (ty < 0 || ty >= g.kh || tx < 0 || tx >= g.kw) return 0.f;
  } else {
    ty = uy;
    tx = ux;
  }
  return w[((static_cast<long long>(ty) * g.kw + tx) * g.Cin_real + ci) * g.Cout + co];
}

template <typename T>
__global__ void conv_pack_kernel(const float* w, PackGeom g, ConvGeom c, void* packed) {
  const long long idx = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
  const long long total = static_cast<long long>(c.groups) * c.ksteps * c.tiles * 64;
  if (idx >= total) return;
  const int lane = idx & 63;
  long long rest = idx >> 6;
  const int t = rest % c.tiles; rest /= c.tiles;
  const int ks = rest % c.ksteps;
  const int group = static_cast<int>(rest / c.ksteps);
  const int i = lane & 31, h = lane >> 5;
  const int col = (group * c.tiles + t) * 32 + i;
  if constexpr (std::is_same<T, __bf16>::value) {
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = static_cast<__bf16>(packed_weight(w, g, c, ks, 8 * h + e, col));
    static_cast<bf16x8*>(packed)[idx] = v;
  } else {
    // f32: K offset of MFMA step u (0..7), half h is 8h + u -> store u-major
    float* dst = static_cast<float*>(packed) + idx * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[e] = packed_weight(w, g, c, ks, 8 * h + e, col);
  }
}

// Image input (Cin <= 4): zero-bordered 4-channel copy so that a kernel row is one
// contiguous K run.  xp[n][y + py0][x + px0][c] = x[n][y][x][c].
template <typename T>
__global__ void conv_pad_image_kernel(const T* x, ConvGeom c, int cin_real, T* xp) {
  const long long idx = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
  const long long total = c.N * c.Hp * c.Wp;
  if (idx >= total) return;
  const int xw = idx % c.Wp;
  const int yh = (idx / c.Wp) % c.Hp;
  const long long n = idx / (static_cast<long long>(c.Wp) * c.Hp);
  const int sy = yh - c.py0, sx = xw - c.px0;
  T v[4] = {T(0.f), T(0.f), T(0.f), T(0.f)};
  if (sy >= 0 && sy < c.H && sx >= 0 && sx < c.W)
    for (int ch = 0; ch < cin_real; ++ch) v[ch] = x[((n * c.H + sy) * c.W + sx) * cin_real + ch];
  for (int ch = 0; ch < 4; ++ch) xp[idx * 4 + ch] = v[ch];
}

void launch_conv_pack(bool bf16, const float* w, const PackGeom& g, const ConvGeom& c, long long frags, void* dst,
                      hipStream_t st) {
  SlowCall slow("conv_pack_kernel launch", __FILE__, __LINE__);
  const dim3 grid(static_cast<unsigned>(ceil_div(frags, 256)));
  if (bf16) hipLaunchKernelGGL((conv_pack_kernel<__bf16>), grid, dim3(256), 0, st, w, g, c, dst);
  else hipLaunchKernelGGL((conv_pack_kernel<float>), grid, dim3(256), 0, st, w, g, c, dst);
}

// ---------------------------------------------------------------------------
// Main kernel
// ---------------------------------------------------------------------------
template <typename T, int TILES>
__global__ void __launch_bounds__(64 * kConvWaves) conv_kernel(const T* x, const void* packed,
                                                               const float* bias, T* y, ConvGeom c) {
  constexpr bool BF = std::is_same<T, __bf16>::value;
  constexpr int FB = ConvTraits<T>::kFragBytes;
  extern __shared__ unsigned char smem[];          // kchunk * TILES * 64 fragments

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int h = lane >> 5;
  const int group = blockIdx.x % c.groups;         // column groups innermost: neighbours share inputs
  const long long pblock = blockIdx.x / c.groups;
  const long long M = c.N * c.OHq * c.OWq;
  const long long m = (pblock * kConvWaves + wid) * 32 + (lane & 31);
  const bool live = m < M;
  const long long mm = live ? m : M - 1;
  int qx, qy;
  long long n;
  if (c.pix32) {          // (a 64-bit division is ~150 instructions in front of the first request)
    const unsigned int m32 = static_cast<unsigned int>(mm);
    const unsigned int r1 = fast_div(m32, c.owq_mul, c.owq_sh);
    qx = static_cast<int>(m32 - r1 * static_cast<unsigned int>(c.OWq));
    const unsigned int n1 = fast_div(r1, c.ohq_mul, c.ohq_sh);
    qy = static_cast<int>(r1 - n1 * static_cast<unsigned int>(c.OHq));
    n = n1;
  } else {
    qx = mm % c.OWq;
    qy = (mm / c.OWq) % c.OHq;
    n = mm / (static_cast<long long>(c.OWq) * c.OHq);
  }

  f32x16 acc[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const unsigned char* wsrc = static_cast<const unsigned char*>(packed) +
                              static_cast<size_t>(group) * c.ksteps * TILES * 64 * FB;
  const int cb = c.small_cin ? 1 : c.Cin / 16;

  for (int k0 = 0; k0 < c.ksteps; k0 += c.kchunk) {
    const int kn = min(c.kchunk, c.ksteps - k0);
    __syncthreads();
    {  // stage the chunk's weight fragments: contiguous 16-byte copies
      const u32x4* src = reinterpret_cast<const u32x4*>(wsrc + static_cast<size_t>(k0) * TILES * 64 * FB);
      u32x4* dst = reinterpret_cast<u32x4*>(smem);
      const int n16 = kn * TILES * 64 * FB / 16;
      for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();
    for (int kk = 0; kk < kn; ++kk) {
      const int ks = k0 + kk;
      // ---- B fragment: 8 input values of this lane's pixel at K offset 8h ----
      const T* src;
      bool ok = live;
      if (c.small_cin) {
        const int uy = ks / c.kw4;
        const int seg = ks % c.kw4;
        // zero-bordered image: always in bounds (the buffer carries a right margin)
        src = x + ((n * c.Hp + (qy * c.sd + uy)) * c.Wp + qx * c.sd) * 4 + seg * 16 + 8 * h;
      } else {
        const int tap = ks / cb;
        const int uy = tap / c.Ux, ux = tap % c.Ux;
        const int iy = qy * c.sd + uy - c.py0, ix = qx * c.sd + ux - c.px0;
        ok = ok && iy >= 0 && iy < c.H && ix >= 0 && ix < c.W;
        src = x + ((n * c.H + (ok ? iy : 0)) * c.W + (ok ? ix : 0)) * c.Cin + (ks % cb) * 16 + 8 * h;
      }
      if constexpr (BF) {
        u32x4 v = ok ? *reinterpret_cast<const u32x4*>(src) : u32x4{0u, 0u, 0u, 0u};
        const bf16x8 bfrag = __builtin_bit_cast(bf16x8, v);
        const bf16x8* a = reinterpret_cast<const bf16x8*>(smem) + (kk * TILES) * 64 + lane;
#pragma unroll
        for (int t = 0; t < TILES; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[t * 64], bfrag, acc[t], 0, 0, 0);
      } else {
        f32x4 v0 = ok ? *reinterpret_cast<const f32x4*>(src) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 v1 = ok ? *reinterpret_cast<const f32x4*>(src + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4* a = reinterpret_cast<const f32x4*>(smem) + ((kk * TILES) * 64 + lane) * 2;
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
          const f32x4 a0 = a[t * 128], a1 = a[t * 128 + 1];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], v0[e], acc[t], 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], v1[e], acc[t], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- epilogue: acc[t][4q + r] = column group_base + 32t + 8q + 4h + r of pixel m ----
#ifdef TFC_CONV_NOSTORE
  if (!live || !bias || bias[0] != 12345.f) return;
#else
  if (!live) return;
#endif
  const int colbase = group * TILES * 32;
  if constexpr (BF) {
    if (c.su == 1 && (c.Cout & 7) == 0) {
      // 16-byte stores: lanes l and l + 32 (one pixel) trade halves of a pair of column groups, see the
      // second-generation kernel's epilogue
#pragma unroll
      for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int qp = 0; qp < 2; ++qp) {
          const int col0 = colbase + 32 * t + 16 * qp;
          if (col0 >= c.cols) continue;
          u32x4 o;
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const int colq = col0 + 8 * half + 4 * h;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float b = (bias && colq + r < c.cols) ? bias[colq + r] : 0.f;
              v[r] = acc[t][4 * (2 * qp + half) + r] + b;
              if (c.activation == 1) v[r] = fmaxf(v[r], 0.f);
            }
            o[2 * half] = pack_bf16(v[0], v[1]);
            o[2 * half + 1] = pack_bf16(v[2], v[3]);
          }
          const auto s0 = __builtin_amdgcn_permlane32_swap(o.x, o.z, false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(o.y, o.w, false, false);
          const int colh = col0 + 8 * h;
          if (colh < c.cols)
            *reinterpret_cast<u32x4*>(y + mm * c.Cout + colh) = u32x4{s0[0], s1[0], s0[1], s1[1]};
        }
      return;
    }
  }
#pragma unroll
  for (int t = 0; t < TILES; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col0 = colbase + 32 * t + 8 * q + 4 * h;
      if (col0 >= c.cols) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = col0 + r;
        float b = 0.f;
        if (bias && col < c.cols) b = bias[col % c.Cout];
        v[r] = acc[t][4 * q + r] + b;
        if (c.activation == 1) v[r] = fmaxf(v[r], 0.f);
      }
      if (c.su == 1 && (c.Cout & 3) == 0) {
        T* dst = y + mm * c.Cout + col0;
        if constexpr (BF) {
          u32x2 o;
          o.x = pack_bf16(v[0], v[1]);
          o.y = pack_bf16(v[2], v[3]);
          *reinterpret_cast<u32x2*>(dst) = o;
        } else {
          *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int col = col0 + r;
          if (col >= c.cols) continue;
          const int co = col % c.Cout, phase = col / c.Cout;
          const int oy = qy * c.su + phase / c.su, ox = qx * c.su + phase % c.su;
          y[((n * c.OH + oy) * c.OW + ox) * c.Cout + co] = static_cast<T>(v[r]);
        }
      }
    }
}

// ---------------------------------------------------------------------------
// bf16 main kernel, second generation.  The first kernel above (still used for f32) reads its
// six A fragments from LDS for every 6 MFMAs, which saturates LDS (4 waves x 6 KB per K step),
// and waits for each K step's B load.  Here
//   * a wave owns MT pixel tiles (MT * 32 pixels) x TILES column tiles, so an A fragment read
//     feeds MT MFMAs (MT = 2: 12 accumulators = 192 AGPRs, one wave per SIMD);
//   * A fragments are double-buffered in registers (the next K step's reads fly under this
//     step's MFMAs) and B fragments are fetched PF K steps ahead into a register ring;
//   * weight chunks are double-buffered in LDS: the next chunk travels global -> registers while
//     the current one is consumed, registers -> LDS at the chunk boundary (one barrier).
// ---------------------------------------------------------------------------
#ifndef TFC_CONV_PF
#define TFC_CONV_PF 4
#endif
#ifndef TFC_CONV_CHUNK
#define TFC_CONV_CHUNK 4
#endif
#ifndef TFC_CONV_INTERLEAVE
#define TFC_CONV_INTERLEAVE 1
#endif
#ifndef TFC_CONV_NO_FASTK
#define TFC_CONV_NO_FASTK 0
#endif
constexpr int kPF = TFC_CONV_PF;         // B fragments in flight per pixel tile
constexpr int kChunk2 = TFC_CONV_CHUNK;  // K steps per LDS weight buffer (multiple of kPF)

#ifndef TFC_CONV_WGS
#define TFC_CONV_WGS 1
#endif
// FASTK (the host sets it when the channel blocks of a tap are a whole number of weight chunks, Cin % 64 == 0,
// and B fragments are requested exactly one chunk ahead): all K steps of a chunk then belong to ONE tap, so
// the tap's coordinates, the bounds test and the per-lane pointer (the zero page for lanes outside the image)
// are set up once per chunk and the K steps' loads are that pointer plus an immediate offset — no address
// arithmetic, no tap walk and no selects inside the K step.
template <int TILES, int MT, bool FASTK, bool OUTF32 = false>
__global__ void __launch_bounds__(256, TFC_CONV_WGS) conv_bf16_kernel(const __bf16* x, const void* packed,
                                                        const float* bias, __bf16* y, ConvGeom c) {
  static_assert(!FASTK || kPF == kChunk2, "FASTK requests the B fragments of the next chunk during this one");
  extern __shared__ unsigned char smem[];          // 2 x kChunk2 * TILES * 64 fragments of 16 B
  constexpr int CHUNK_FRAGS = kChunk2 * TILES * 64;
  constexpr int STAGE = (CHUNK_FRAGS + 255) / 256;  // 16-byte pieces each thread moves per chunk
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int h = lane >> 5;
  // (workgroups in XCD order, xcd_order, were measured on this kernel: 6.79 -> 6.96 ms for the 384x256 stride-2 layer)
  const int group = blockIdx.x % c.groups;
  const long long pblock = blockIdx.x / c.groups;
  const long long M = c.N * c.OHq * c.OWq;

  long long nn[MT];
  int qy[MT], qx[MT];
  bool live[MT];
  long long mm[MT];
  // per lane, fixed for the whole K loop: element offset of (n, qy*sd - py0, qx*sd - px0, 8h) and
  // the two coordinates the taps are added to (kept as int: the bounds test is two unsigned compares)
  long long base_off[MT];
  int iy0[MT], ix0[MT];
#pragma unroll
  for (int p = 0; p < MT; ++p) {
    const long long m = ((pblock * 4 + wid) * MT + p) * 32 + (lane & 31);
    live[p] = m < M;
    mm[p] = live[p] ? m : M - 1;
    if (c.pix32) {          // (a 64-bit division is ~150 instructions in front of the first request)
      const unsigned int m32 = static_cast<unsigned int>(mm[p]);
      const unsigned int r1 = fast_div(m32, c.owq_mul, c.owq_sh);
      qx[p] = static_cast<int>(m32 - r1 * static_cast<unsigned int>(c.OWq));
      const unsigned int n1 = fast_div(r1, c.ohq_mul, c.ohq_sh);
      qy[p] = static_cast<int>(r1 - n1 * static_cast<unsigned int>(c.OHq));
      nn[p] = n1;
    } else {
      qx[p] = static_cast<int>(mm[p] % c.OWq);
      qy[p] = static_cast<int>((mm[p] / c.OWq) % c.OHq);
      nn[p] = mm[p] / (static_cast<long long>(c.OWq) * c.OHq);
    }
    iy0[p] = qy[p] * c.sd - c.py0;
    ix0[p] = qx[p] * c.sd - c.px0;
    base_off[p] = ((nn[p] * c.H + iy0[p]) * c.W + ix0[p]) * c.Cin + 8 * h;
  }
  const int cb = c.Cin / 16;
  // 16 zero bytes behind the packed weights: where lanes outside the image (or the tensor) read
  const __bf16* zeros = reinterpret_cast<const __bf16*>(
      static_cast<const unsigned char*>(packed) + static_cast<size_t>(c.groups) * c.ksteps * TILES * 64 * 16);

  // Position of a K step inside the (tap row, tap column, 16-channel block) order, advanced
  // incrementally: the per-step divisions by runtime Cin / kernel width were the single largest
  // block of non-MFMA instructions in the loop.
  struct KPos { int uy, ux, cbi; long long off; };      // off = (uy * W + ux) * Cin + 16 * cbi
  // taps of this column group: all of them, or the sub-rectangle of its output phase
  const int uy0 = c.compact ? c.ty0[group] : 0, uy1 = c.compact ? c.ty1[group] : c.Uy;
  const int ux0 = c.compact ? c.tx0[group] : 0, ux1 = c.compact ? c.tx1[group] : c.Ux;
  const int ksteps = (uy1 - uy0) * (ux1 - ux0) * cb;
  const long long row_step = static_cast<long long>(c.W - (ux1 - ux0)) * c.Cin + 16;   // last tap of a row -> next row
  // (selects, not branches: the unrolled K steps of a chunk stay ONE basic block, which is what lets the
  // scheduler put their address arithmetic, LDS reads and loads between the MFMAs)
  auto advance = [&](KPos& k) {
    const int cbi1 = k.cbi + 1;
    const bool wc = cbi1 == cb;                      // next channel block, or the next pixel of the row: contiguous
    const int uxn = k.ux + (wc ? 1 : 0);
    const bool wx = uxn == ux1;                      // last tap of a row -> next row
    k.cbi = wc ? 0 : cbi1;
    k.ux = wx ? ux0 : uxn;
    k.uy += wx ? 1 : 0;
    k.off += wx ? row_step : 16;
  };
  // B fragment of pixel tile p at K position k: 8 input values at K offset 8h, zero outside the image
  auto bload = [&](const KPos& k, int p) -> u32x4 {
    // (& on purpose: && is control flow, an EXEC-masked block per term)
    const bool ok = live[p] & (static_cast<unsigned int>(iy0[p] + k.uy) < static_cast<unsigned int>(c.H)) &
                    (static_cast<unsigned int>(ix0[p] + k.ux) < static_cast<unsigned int>(c.W)) & (k.uy < uy1);
    // address as an integer select (a pointer select became an EXEC-masked block per load)
    unsigned long long a_in = reinterpret_cast<unsigned long long>(x) +
                              2ull * static_cast<unsigned long long>(base_off[p] + k.off);
    asm volatile("" : "+v"(a_in));     // computed for every lane: the select below stays two v_cndmask
#ifdef TFC_CONV_NOBLOAD     // experiment: the K loop without its input traffic
    const unsigned long long a = ok && k.uy > 1000 ? a_in : reinterpret_cast<unsigned long long>(zeros);
#else
    const unsigned long long a = ok ? a_in : reinterpret_cast<unsigned long long>(zeros);
#endif
    return *reinterpret_cast<__attribute__((address_space(1))) const u32x4*>(a);     // a global, not a flat, load
  };

  f32x16 acc[MT][TILES];
#pragma unroll
  for (int p = 0; p < MT; ++p)
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[p][t][r] = 0.f;

  const u32x4* wsrc = reinterpret_cast<const u32x4*>(
      static_cast<const unsigned char*>(packed) + static_cast<size_t>(group) * c.ksteps * TILES * 64 * 16);
  const int nchunks = (ksteps + kChunk2 - 1) / kChunk2;
  const long long wtotal = static_cast<long long>(ksteps) * TILES * 64;     // fragments of this group in use

  u32x4 stage[STAGE];
  // Unconditional loads from a clamped index (fragments past the chunk / the group's K steps are never
  // read by an MFMA that counts: their B operand is zero).  A load under a condition is a path WITHOUT
  // the load for the compiler's s_waitcnt bookkeeping: it then allows fewer loads in flight at the first
  // MFMA of a chunk than really are, and the wave waits there for the weights it has just requested
  // (SQ_WAIT_ANY was 30 % of the wave cycles of the 192 -> 192 layers).
  auto wfetch = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < STAGE; ++i) {
      const long long f = static_cast<long long>(chunk) * CHUNK_FRAGS + i * 256 + threadIdx.x;
      stage[i] = wsrc[f < wtotal ? f : wtotal - 1];
    }
  };
  auto wstore = [&](int buf) {
    u32x4* dst = reinterpret_cast<u32x4*>(smem) + buf * CHUNK_FRAGS;
#pragma unroll
    for (int i = 0; i < STAGE; ++i)
      if (i * 256 + static_cast<int>(threadIdx.x) < CHUNK_FRAGS) dst[i * 256 + threadIdx.x] = stage[i];
  };

  // prologue: chunk 0 into buffer 0, first PF B fragments
  wfetch(0);
  wstore(0);
  u32x4 bq[kPF][MT];
  KPos kpre{uy0, ux0, 0, (static_cast<long long>(uy0) * c.W + ux0) * c.Cin};   // the next B fragment to request
  // FASTK: per-lane source of the chunk being requested (K step kk of it at + 32 kk bytes), and its tap
  unsigned long long bsrc[MT];
  int fuy = uy0, fux = ux0, fcbi = 0;
  auto chunk_sources = [&]() __attribute__((always_inline)) {
    const long long off = (static_cast<long long>(fuy) * c.W + fux) * c.Cin + 16 * fcbi;
#pragma unroll
    for (int p = 0; p < MT; ++p) {
      const bool ok = live[p] & (static_cast<unsigned int>(iy0[p] + fuy) < static_cast<unsigned int>(c.H)) &
                      (static_cast<unsigned int>(ix0[p] + fux) < static_cast<unsigned int>(c.W)) & (fuy < uy1);
      unsigned long long a_in = reinterpret_cast<unsigned long long>(x) +
                                2ull * static_cast<unsigned long long>(base_off[p] + off);
      asm volatile("" : "+v"(a_in));
      bsrc[p] = ok ? a_in : reinterpret_cast<unsigned long long>(zeros);
    }
    // on to the next chunk's position: kChunk2 channel blocks further, by selects
    const int cbn = fcbi + kChunk2;
    const bool wc = cbn == cb;
    const int uxn = fux + (wc ? 1 : 0);
    const bool wx = uxn == ux1;
    fcbi = wc ? 0 : cbn;
    fux = wx ? ux0 : uxn;
    fuy += wx ? 1 : 0;
  };
  auto fast_load = [&](int kk, int p) __attribute__((always_inline)) -> u32x4 {
    return *reinterpret_cast<__attribute__((address_space(1))) const u32x4*>(bsrc[p] + 32ull * kk);
  };
  if constexpr (FASTK) {
    chunk_sources();
#pragma unroll
    for (int k = 0; k < kPF; ++k)
#pragma unroll
      for (int p = 0; p < MT; ++p) bq[k][p] = fast_load(k, p);
  } else {
#pragma unroll
    for (int k = 0; k < kPF; ++k) {
#pragma unroll
      for (int p = 0; p < MT; ++p) bq[k][p] = bload(kpre, p);
      advance(kpre);
    }
  }
  __syncthreads();

  for (int chunk = 0; chunk < nchunks; ++chunk) {
    const int buf = chunk & 1;
#ifndef TFC_CONV_BARE       // (experiment: MFMAs only -- no weight staging, no barrier, with NOAREAD / NOBLOAD)
    wfetch(chunk + 1);          // past the last chunk: the clamped fragment, not used
#endif
    if constexpr (FASTK) chunk_sources();     // of chunk + 1, whose fragments this chunk's K steps request
    const bf16x8* abase = reinterpret_cast<const bf16x8*>(smem) + buf * CHUNK_FRAGS + lane;
    bf16x8 af[2][TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) af[0][t] = abase[t * 64];
#pragma unroll
    for (int kk = 0; kk < kChunk2; ++kk) {
#ifndef TFC_CONV_NOAREAD    // (experiment: without the A fragment reads of the steps after a chunk's first)
      if (kk + 1 < kChunk2) {
#pragma unroll
        for (int t = 0; t < TILES; ++t) af[(kk + 1) & 1][t] = abase[((kk + 1) * TILES + t) * 64];
      }
#else
#pragma unroll
      for (int t = 0; t < TILES; ++t) af[(kk + 1) & 1][t] = af[kk & 1][t];
#endif
#pragma unroll
      for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int p = 0; p < MT; ++p)
          acc[p][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              af[kk & 1][t], __builtin_bit_cast(bf16x8, bq[kk % kPF][p]), acc[p][t], 0, 0, 0);
      // refill the ring slot with K step ks + PF (past the last tap row: zeros); after the MFMAs
      // that read it so that no copy of the slot is needed
#ifndef TFC_CONV_BARE
      if constexpr (FASTK) {
#pragma unroll
        for (int p = 0; p < MT; ++p) bq[kk % kPF][p] = fast_load(kk, p);
      } else {
#pragma unroll
        for (int p = 0; p < MT; ++p) bq[kk % kPF][p] = bload(kpre, p);
        advance(kpre);
      }
#endif
#if TFC_CONV_INTERLEAVE
      // One wave per SIMD: an MFMA occupies the matrix pipe for 32 cycles = 8 issue slots, about five other
      // instructions fit in its shadow, and this K step has ~4.5 of them per MFMA (address arithmetic of
      // the two B loads, the six A reads of the next step) -- but only if they sit BETWEEN the MFMAs;
      // left to itself the scheduler issues the 12 MFMAs in a row and everything else behind them.
#pragma unroll
      for (int i = 0; i < TILES * MT; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                    // one MFMA
        if (i < TILES) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // one A fragment read
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                    // two VALU
        __builtin_amdgcn_sched_group_barrier(0x004, 3, 0);                    // three SALU
      }
#endif
      __builtin_amdgcn_sched_barrier(0);
    }
#ifndef TFC_CONV_BARE
    if (chunk + 1 < nchunks) wstore(buf ^ 1);
    __syncthreads();
#endif
  }

  // ---- epilogue: acc[p][t][4q + r] = column group_base + 32t + 8q + 4h + r of pixel mm[p] ----
  const int colbase = group * TILES * 32;
  const bool vec4 = (c.Cout & 3) == 0;       // 4 consecutive columns = 4 channels of one phase
  if ((c.Cout & 7) == 0 && !OUTF32) {
    // 8 consecutive columns = 8 channels of one pixel: lanes l and l + 32 (the same pixel, h = 0 / 1) trade
    // halves of a pair of column groups (v_permlane32_swap, as in gdn_common.h) and each stores 16 bytes,
    // 32 contiguous bytes per pixel and instruction.  With 8-byte stores the output traffic of the layers
    // that write the most (the image-side analysis layer, the last 192 -> 192 synthesis layer) took 2.6 and
    // 3.3 ms of their 4.4 and 14.8 ms at the C4 shapes.
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
#pragma unroll
      for (int qp = 0; qp < 2; ++qp) {
        const int col0 = colbase + 32 * t + 16 * qp;          // the pair covers columns col0 .. col0 + 15
        if (col0 >= c.cols) continue;                          // wave-uniform
        const int co = col0 % c.Cout, phase = col0 / c.Cout;
        f32x4 be = f32x4{0.f, 0.f, 0.f, 0.f}, bo = be;
        if (bias) {
          be = *reinterpret_cast<const f32x4*>(bias + co + 4 * h);
          if (col0 + 8 < c.cols) bo = *reinterpret_cast<const f32x4*>(bias + (col0 + 8) % c.Cout + 4 * h);
        }
#pragma unroll
        for (int p = 0; p < MT; ++p) {
          u32x4 o;
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const f32x4& b4 = half ? bo : be;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              v[r] = acc[p][t][4 * (2 * qp + half) + r] + b4[r];
              if (c.activation == 1) v[r] = fmaxf(v[r], 0.f);
            }
            o[2 * half] = pack_bf16(v[0], v[1]);
            o[2 * half + 1] = pack_bf16(v[2], v[3]);
          }
          const auto s0 = __builtin_amdgcn_permlane32_swap(o.x, o.z, false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(o.y, o.w, false, false);
          // lane h stores columns col0 + 8h .. + 7 (h = 1: the odd group, possibly another phase / past the end)
          const int colh = col0 + 8 * h;
          if (!live[p] || colh >= c.cols) continue;
          const int coh = colh % c.Cout, ph = colh / c.Cout;
          const int oy = qy[p] * c.su + ph / c.su, ox = qx[p] * c.su + ph % c.su;
          *reinterpret_cast<u32x4*>(y + ((nn[p] * c.OH + oy) * c.OW + ox) * c.Cout + coh) =
              u32x4{s0[0], s1[0], s0[1], s1[1]};
          (void)phase;
        }
      }
      __builtin_amdgcn_sched_barrier(0);     // one column tile at a time (register pressure)
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col0 = colbase + 32 * t + 8 * q + 4 * h;
      const int co = col0 % c.Cout, phase = col0 / c.Cout;
      f32x4 b4 = f32x4{0.f, 0.f, 0.f, 0.f};
      if (bias && col0 < c.cols) {
        if (vec4) {
          b4 = *reinterpret_cast<const f32x4*>(bias + co);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) b4[r] = col0 + r < c.cols ? bias[(col0 + r) % c.Cout] : 0.f;
        }
      }
#pragma unroll
      for (int p = 0; p < MT; ++p) {
#ifdef TFC_CONV_NOSTORE      // experiment: the kernel without its output traffic (stores only for an impossible bias)
        if (!live[p] || col0 >= c.cols || b4[0] != 12345.f) continue;
#else
        if (!live[p] || col0 >= c.cols) continue;
#endif
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = acc[p][t][4 * q + r] + b4[r];
          if (c.activation == 1) v[r] = fmaxf(v[r], 0.f);
        }
        if (OUTF32 && vec4) {
          const int oy = qy[p] * c.su + phase / c.su, ox = qx[p] * c.su + phase % c.su;
          *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(y) + ((nn[p] * c.OH + oy) * c.OW + ox) * c.Cout + co) =
              f32x4{v[0], v[1], v[2], v[3]};
        } else if (vec4) {
          // su == 1: phase 0, (oy, ox) = (qy, qx); else depth-to-space of the column's phase
          const int oy = qy[p] * c.su + phase / c.su, ox = qx[p] * c.su + phase % c.su;
          u32x2 o;
          o.x = pack_bf16(v[0], v[1]);
          o.y = pack_bf16(v[2], v[3]);
          *reinterpret_cast<u32x2*>(y + ((nn[p] * c.OH + oy) * c.OW + ox) * c.Cout + co) = o;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int col = col0 + r;
            if (col >= c.cols) continue;
            const int co1 = col % c.Cout, ph1 = col / c.Cout;
            const int oy = qy[p] * c.su + ph1 / c.su, ox = qx[p] * c.su + ph1 % c.su;
            y[((nn[p] * c.OH + oy) * c.OW + ox) * c.Cout + co1] = static_cast<__bf16>(v[r]);
          }
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);     // one column tile at a time (register pressure)
  }
}

template <typename T>
int run_conv(const void* x, const float* w, const float* bias, void* y, ConvGeom c, PackGeom g,
             unsigned long long key, hipStream_t st, int* gdn_fused) {
  constexpr int FB = ConvTraits<T>::kFragBytes;
  if constexpr (std::is_same<T, __bf16>::value) {
    const int rc = run_conv3(static_cast<const __bf16*>(x), w, bias, static_cast<__bf16*>(y), c, g, key, st);
    if (rc == 0 && c.gdn && gdn_fused) *gdn_fused = 1;
    if (rc >= 0) return rc;
  }
  c.gdn = 0;                          // (the other kernels leave the activation to the caller)
  const int tiles_total = (c.cols + 31) / 32;
  // image-side layers (first kernel): 3 column tiles per group — half the accumulators, twice the waves per
  // CU; measured 3.39 -> 2.98 ms on the 5x5 3 -> 192 /2 layer of bmshj2018 at 128 x 768x512 (for the 192 -> 192
  // layers of the second kernel the same split costs 45 %: every B gather is then issued twice)
  c.tiles = std::min(tiles_total, (c.small_cin && std::is_same<T, __bf16>::value) ? std::min(3, kMaxTiles) : kMaxTiles);
  c.groups = (tiles_total + c.tiles - 1) / c.tiles;
  // 64 KiB of LDS per workgroup (two workgroups per CU)
  c.kchunk = std::max(1, std::min(c.ksteps, (64 * 1024) / (c.tiles * 64 * FB)));
  const size_t lds = static_cast<size_t>(c.kchunk) * c.tiles * 64 * FB;

  c.compact = 0;
  if (std::is_same<T, __bf16>::value && !c.small_cin && g.up && c.groups <= kMaxGroups &&
      c.Cout % (c.tiles * 32) == 0) {
    // every column group lies inside one output phase: its taps are those with a kernel index in range
    c.compact = 1;
    int most = 0;
    for (int grp = 0; grp < c.groups; ++grp) {
      int taps = phase_taps(c, g, grp, grp * c.tiles * 32 / c.Cout);
      if (!taps) { c.ty0[grp] = 0; c.ty1[grp] = 1; c.tx0[grp] = 0; c.tx1[grp] = 1; taps = 1; }   // a phase without taps: one (zero) block
      most = std::max(most, taps);
    }
    c.ksteps = most * (c.Cin / 16);          // packed K steps per group (the stride of the packed buffer)
  }
  DevBuf packed_local, padded;
  DevView packed;
  const long long frags = static_cast<long long>(c.groups) * c.ksteps * c.tiles * 64;
  // + a zero page behind the fragments: what lanes outside the image read (16 bytes; the per-chunk pointers of
  // the FASTK kernel read it at + 32 (kChunk2 - 1))
  {
    const int rc = packed_weights(key, 2, {g.kh, g.kw, g.Cin_real, g.Cout, g.su, g.up, g.Uy, g.Ux, g.dmax_y, g.dmax_x, c.groups,
                                      c.ksteps, c.tiles, c.compact * 4 + c.cbmajor * 2 + c.small_cin + 8 * static_cast<int>(sizeof(T)),
                                      c.kw4},
                                  static_cast<size_t>(frags) * FB + 32 * kChunk2, st, packed_local, &packed.p, [&](void* dst) {
      TFC_HIP(hipMemsetAsync(static_cast<unsigned char*>(dst) + static_cast<size_t>(frags) * FB, 0, 32 * kChunk2, st));
      launch_conv_pack(std::is_same<T, __bf16>::value, w, g, c, frags, dst, st);
      return 0;
    });
    if (rc) return rc;
  }
  const T* xin = static_cast<const T*>(x);
  if (c.small_cin) {
    // right margin: a K run may read up to kw4*16 values past the last window start
    const size_t elems = (static_cast<size_t>(c.N) * c.Hp * c.Wp + c.kw4 * 16 + 16) * 4;
    TFC_HIP(padded.alloc(elems * sizeof(T), st));
    TFC_HIP(hipMemsetAsync(padded.p, 0, elems * sizeof(T), st));
    const long long total = c.N * c.Hp * c.Wp;
    hipLaunchKernelGGL((conv_pad_image_kernel<T>), dim3(static_cast<unsigned>(ceil_div(total, 256))),
                       dim3(256), 0, st, xin, c, g.Cin_real, padded.as<T>());
    xin = padded.as<T>();
  }
  const long long M = c.N * c.OHq * c.OWq;
  if constexpr (std::is_same<T, __bf16>::value) if (!c.small_cin) {
    // second-generation kernel (not for the image layer: its K is only a few dozen steps and the
    // first kernel, which stages all of them at once, is faster there); 2 pixel tiles per wave
    // when that still fills the chip
    const int mt = ceil_div(M, 256) * c.groups >= 2 * device_cus() ? 2 : 1;
    const long long blocks2 = ceil_div(M, 128 * mt) * c.groups;
    if (blocks2 > kMaxGridX) return fail("tfc_conv2d: problem too large for one launch");
    const size_t lds2 = static_cast<size_t>(2) * kChunk2 * c.tiles * 64 * 16;
    KernelTimer timer("conv2d", st);
    // (F32: the kernel writes its float32 accumulators)
#define TFC_CONV2_LAUNCH(NT, MTV, FK, F32)                                                         \
    return launch(&conv_bf16_kernel<NT, MTV, FK, F32>, dim3(static_cast<unsigned>(blocks2)), dim3(256), lds2, st,         \
                  static_cast<const __bf16*>(static_cast<const void*>(xin)), packed.p, bias, static_cast<__bf16*>(y), c)
    // one tap per weight chunk (see the kernel): channel blocks per tap a multiple of the chunk
    const bool fastk = kPF == kChunk2 && (c.Cin / 16) % kChunk2 == 0 && !TFC_CONV_NO_FASTK;
    // (the fp32-output variant is a compile-time property: as a run-time flag in the epilogue it cost the
    // 6-tile kernel 832 bytes of scratch per lane, accumulators spilled inside the K loop)
    // (round 6: with the one-tap-per-chunk K loop too, for the float32 layers that run as six bfloat16 planes — built for
    // the 128- and 192-column groups, the widths of the models' layers)
#define TFC_CONV2_LAUNCH_F32(NT, MTV)                                                              \
    do {                                                                                           \
      if constexpr (NT == 6 || NT == 4) {                                                          \
        if (fastk) TFC_CONV2_LAUNCH(NT, MTV, true, true);                                          \
      }                                                                                            \
      TFC_CONV2_LAUNCH(NT, MTV, false, true);                                                      \
    } while (0)
#define TFC_CONV2_CASE(NT)                                                                         \
    case NT:                                                                                       \
      if (c.out_f32) { if (mt == 2) TFC_CONV2_LAUNCH_F32(NT, 2); else TFC_CONV2_LAUNCH_F32(NT, 1); } \
      else if (mt == 2) { if (fastk) TFC_CONV2_LAUNCH(NT, 2, true, false); else TFC_CONV2_LAUNCH(NT, 2, false, false); } \
      else { if (fastk) TFC_CONV2_LAUNCH(NT, 1, true, false); else TFC_CONV2_LAUNCH(NT, 1, false, false); }
    switch (c.tiles) {
      TFC_CONV2_CASE(1);
      TFC_CONV2_CASE(2);
      TFC_CONV2_CASE(3);
      TFC_CONV2_CASE(4);
      TFC_CONV2_CASE(5);
      default:
        TFC_CONV2_CASE(6);
    }
#undef TFC_CONV2_CASE
#undef TFC_CONV2_LAUNCH
#undef TFC_CONV2_LAUNCH_F32
  }
  const long long blocks = ceil_div(M, 32 * kConvWaves) * c.groups;
  if (blocks > kMaxGridX) return fail("tfc_conv2d: problem too large for one launch");
  KernelTimer timer("conv2d", st);
#define TFC_CONV_CASE(NT) \
  case NT: return launch(&conv_kernel<T, NT>, dim3(static_cast<unsigned>(blocks)), dim3(64 * kConvWaves), lds, st, xin, packed.p, bias, static_cast<T*>(y), c)
  switch (c.tiles) {
    TFC_CONV_CASE(1);
    TFC_CONV_CASE(2);
    TFC_CONV_CASE(3);
    TFC_CONV_CASE(4);
    TFC_CONV_CASE(5);
    default:
      TFC_CONV_CASE(6);
  }
#undef TFC_CONV_CASE
}

// ---------------------------------------------------------------------------
// Transposed convolution into a few channels (the last synthesis layer, C -> 3), bf16: as an implicit
// GEMM over output pixels it gathers every input pixel once per low-resolution tap (9 times for a 5x5
// stride-2 kernel) for 12 useful of 32 MFMA columns, and those gathers are all its time (6.8 ms at the
// C4 shape, 1.9 ms without them).  Instead: ONE 1x1 product per INPUT pixel with all kh*kw taps as output
// columns, z[i][(ty, tx, c)] = sum_ci x[i][ci] w[ty][tx][ci][c] (the same kernel, 12 K steps per pixel
// tile instead of 108), then every output pixel sums the <= ceil(k/s)^2 entries that land on it:
// o = i*s + t - k/2 (signal_conv.py:778-847; the alignment test_identity_kernel_alignment pins).
// z holds the products' fp32 accumulators (a bf16 z would round once per tap: with cancelling taps the error
// is relative to the taps, not to the output), 4 columns per tap so that a tap's channels are one aligned
// 16-byte read; the output is rounded once, like the implicit GEMM's.
// ---------------------------------------------------------------------------
__global__ void conv_up_weights_kernel(const float* w, int kh, int kw, int cin, int cout, float* w1) {
  const long long idx = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
  const long long total = static_cast<long long>(cin) * kh * kw * 4;
  if (idx >= total) return;
  const int c = idx & 3;
  const int tap = static_cast<int>((idx >> 2) % (kh * kw));
  const int ci = static_cast<int>(idx / (4ll * kh * kw));
  w1[idx] = c < cout ? w[(static_cast<long long>(tap) * cin + ci) * cout + c] : 0.f;     // [ci][tap][4]
}

__global__ void __launch_bounds__(256) conv_up_gather_kernel(const float* z, const float* bias, __bf16* y,
                                                             long long N, int H, int W, int kh, int kw, int s,
                                                             int cout, int activation) {
  const int OH = H * s, OW = W * s;
  const long long o = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
  if (o >= N * OH * OW) return;
  const int ox = static_cast<int>(o % OW);
  const int oy = static_cast<int>((o / OW) % OH);
  const long long n = o / (static_cast<long long>(OW) * OH);
  const int zc = kh * kw * 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  // o = i*s + t - k/2  =>  t = (o + k/2) mod s, + s, ... ;  i = (o + k/2 - t) / s
  for (int ty = (oy + kh / 2) % s; ty < kh; ty += s) {
    const int iy = (oy + kh / 2 - ty) / s;
    if (iy < 0 || iy >= H) continue;
    for (int tx = (ox + kw / 2) % s; tx < kw; tx += s) {
      const int ix = (ox + kw / 2 - tx) / s;
      if (ix < 0 || ix >= W) continue;
      const f32x4 v = *reinterpret_cast<const f32x4*>(z + ((n * H + iy) * W + ix) * zc + (ty * kw + tx) * 4);
      acc[0] += v[0];
      acc[1] += v[1];
      acc[2] += v[2];
      acc[3] += v[3];
    }
  }
  for (int c = 0; c < cout; ++c) {
    float v = acc[c] + (bias ? bias[c] : 0.f);
    if (activation == 1) v = fmaxf(v, 0.f);
    y[o * cout + c] = static_cast<__bf16>(v);
  }
}

// ---------------------------------------------------------------------------
// Image-side analysis layer (Cin <= 4 -> 128 / 192 channels, stride 2 or 4, bf16): all of its time is the output
// (4.8 GB at the C4 shape) — K is a few dozen steps.  A workgroup takes an 8 x 32 block of output pixels, stages the
// image patch under it in LDS as rows of interleaved (x, c) values (19 x 67 pixels x 3 channels = 8 KB for 5x5 / 2),
// and runs K kernel row by kernel row: the kw * Cin values of a row are CONTIGUOUS in the patch, so a row is
// ceil(kw * Cin / 16) K steps (one for 5x5 x 3, against two with the 4-channel padding of the first kernel), and a
// B fragment is 16 bytes at (row, 2-byte-aligned column): four ds_read_b32.  Two workgroups per CU (LDS 40 KB, 256
// registers per wave): one's output stores drain under the other's MFMAs.
// ---------------------------------------------------------------------------
struct ImageConvGeom {
  long long N;
  int H, W, Cin, Cout;
  int kh, kw, sd;
  int py0, px0;
  int OH, OW;
  int BXn, BYn;
  int PH, RL, RS;           // patch rows; values per row in use; row stride (values)
  int ksr;                  // K steps per kernel row
  int activation;
  int pairs;                // 1: patch loaded two values at a time
  int items;                // blocks per workgroup
};

__global__ void conv_image_weights_kernel(const float* w, ImageConvGeom g, int tiles, bf16x8* packed) {
  // packed[((ty * ksr + ks) * tiles + t) * 64 + lane], lane (i, h): row values 16 ks + 8h .. + 7, output column 32t + i
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = g.kh * g.ksr * tiles * 64;
  if (idx >= total) return;
  const int lane = idx & 63;
  int r = idx >> 6;
  const int t = r % tiles; r /= tiles;
  const int ks = r % g.ksr, ty = r / g.ksr;
  const int co = 32 * t + (lane & 31), h = lane >> 5;
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = 16 * ks + 8 * h + e;
    const int tx = k / g.Cin, c = k % g.Cin;
    v[e] = static_cast<__bf16>(tx < g.kw && co < g.Cout
                                   ? w[((static_cast<long long>(ty) * g.kw + tx) * g.Cin + c) * g.Cout + co] : 0.f);
  }
  packed[idx] = v;
}

template <int TILES>
__global__ void __launch_bounds__(256, 2) conv_image_kernel(const __bf16* x, const bf16x8* wpk, const float* bias,
                                                            __bf16* y, ImageConvGeom g) {
  extern __shared__ unsigned char smem[];            // patch: PH rows of RS values | weight fragments
  constexpr int MT = 2;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, l = lane & 31;
  unsigned short* patch = reinterpret_cast<unsigned short*>(smem);
  bf16x8* wl = reinterpret_cast<bf16x8*>(smem + static_cast<size_t>(g.PH) * g.RS * 2);
  const int nfr = g.kh * g.ksr * TILES * 64;
  for (int i = tid; i < nfr; i += 256) wl[i] = wpk[i];
  // the epilogue's staging area, one per wave, behind the fragments
  constexpr int ROW = 144;                             // bytes of a pixel's 64 channels in the staging area (+ 16: banks)
  unsigned char* const stg = reinterpret_cast<unsigned char*>(wl + nfr) + wid * (32 * ROW);
  // A workgroup takes g.items consecutive blocks: the weight fragments (30 KB at 5x5 x 3 -> 192, as much as a third of
  // a block's output) are staged once for all of them
  const long long nblk = g.N * g.BYn * g.BXn;
  const long long item_end = std::min(nblk, (static_cast<long long>(blockIdx.x) + 1) * g.items);
  // (requesting the next item's patch in front of this item's epilogue was measured: 1.83 -> 2.12 ms — the wait for
  // those loads is a wait for every store issued behind them)
  for (long long item = static_cast<long long>(blockIdx.x) * g.items; item < item_end; ++item) {
  long long b = item;
  const int bx = static_cast<int>(b % g.BXn); b /= g.BXn;
  const int by = static_cast<int>(b % g.BYn);
  const long long n = b / g.BYn;
  const int qx0 = bx * 32, qy0 = by * 8;
  // patch: value j of row py = x[n][iy][ix0 + j / Cin][j % Cin]: contiguous in the image row
  const unsigned short* xn = reinterpret_cast<const unsigned short*>(x) + n * g.H * g.W * g.Cin;
  const int ix0 = qx0 * g.sd - g.px0;
  constexpr int PB = 8;                                // loads in flight per thread
  if (g.pairs) {
    // two values per load: every image row and every patch row start on a 4-byte boundary (host check).  A pair that
    // straddles the image's edge is split by value, not by address: both halves are tested
    const int pvals = g.PH * g.RS / 2;
    unsigned int* patch2 = reinterpret_cast<unsigned int*>(patch);
    const int rs2 = g.RS / 2;
    for (int i0 = tid; i0 < pvals; i0 += 256 * PB) {
      unsigned int v[PB];
#pragma unroll
      for (int k = 0; k < PB; ++k) {
        const int i = i0 + 256 * k;
        const int py = i / rs2, j = 2 * (i - py * rs2);
        const int iy = qy0 * g.sd - g.py0 + py;
        const int ixa = ix0 + j / g.Cin, ixb = ix0 + (j + 1) / g.Cin;
        const bool row = (i < pvals) & (static_cast<unsigned int>(iy) < static_cast<unsigned int>(g.H));
        const bool oka = row & (j < g.RL) & (static_cast<unsigned int>(ixa) < static_cast<unsigned int>(g.W));
        const bool okb = row & (j + 1 < g.RL) & (static_cast<unsigned int>(ixb) < static_cast<unsigned int>(g.W));
        // the pair lies inside the image's allocation whenever one half is inside the image, except at the very first
        // and last value of the tensor: those pairs are read half by half
        const long long a = (static_cast<long long>(iy) * g.W + ix0) * g.Cin + j;
        const long long last = static_cast<long long>(g.H) * g.W * g.Cin - 2;
        unsigned int t = 0;
        if (oka | okb) {
          if (a >= 0 && a <= last) t = *reinterpret_cast<const unsigned int*>(xn + a);
          else t = (oka ? xn[a] : 0u) | (okb ? static_cast<unsigned int>(xn[a + 1]) << 16 : 0u);
        }
        v[k] = (oka ? t & 0xFFFFu : 0u) | (okb ? t & 0xFFFF0000u : 0u);
      }
#pragma unroll
      for (int k = 0; k < PB; ++k)
        if (i0 + 256 * k < pvals) patch2[i0 + 256 * k] = v[k];
    }
  } else {
    const int pvals = g.PH * g.RS;
    for (int i0 = tid; i0 < pvals; i0 += 256 * PB) {
      unsigned short v[PB];
#pragma unroll
      for (int k = 0; k < PB; ++k) {
        const int i = i0 + 256 * k;
        const int py = i / g.RS, j = i - py * g.RS;
        const int iy = qy0 * g.sd - g.py0 + py;
        const int ix = ix0 + j / g.Cin;                  // (j >= RL: pixels nobody multiplies with a weight)
        const bool ok = (i < pvals) & (j < g.RL) & (static_cast<unsigned int>(iy) < static_cast<unsigned int>(g.H)) &
                        (static_cast<unsigned int>(ix) < static_cast<unsigned int>(g.W));
        // clamped address, value selected afterwards: the loads of a batch are issued together
        const long long a = ok ? (static_cast<long long>(iy) * g.W + ix0) * g.Cin + j : 0;
        const unsigned short t = xn[a];
        v[k] = ok ? t : static_cast<unsigned short>(0);
      }
#pragma unroll
      for (int k = 0; k < PB; ++k)
        if (i0 + 256 * k < pvals) patch[i0 + 256 * k] = v[k];
    }
  }
  __syncthreads();
  f32x16 acc[MT][TILES];
#pragma unroll
  for (int p = 0; p < MT; ++p)
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[p][t][r] = 0.f;
  // per-lane patch position of (tile p, kernel row 0, K step 0), in values
  int lb[MT];
#pragma unroll
  for (int p = 0; p < MT; ++p) lb[p] = ((2 * wid + p) * g.sd) * g.RS + l * g.sd * g.Cin + 8 * h;
  const int steps = g.kh * g.ksr;
  for (int st = 0; st < steps; ++st) {
    const int ty = st / g.ksr, ks = st - ty * g.ksr;
    const int o = ty * g.RS + 16 * ks;
    u32x4 bq[MT];
#pragma unroll
    for (int p = 0; p < MT; ++p) {
      const unsigned int* src = reinterpret_cast<const unsigned int*>(patch + lb[p] + o);     // 4-byte aligned
      bq[p] = u32x4{src[0], src[1], src[2], src[3]};
    }
    const bf16x8* abase = wl + st * TILES * 64 + lane;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      const bf16x8 a = abase[t * 64];
#pragma unroll
      for (int p = 0; p < MT; ++p)
        acc[p][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, bq[p]), acc[p][t], 0, 0, 0);
    }
  }
  // ---- epilogue: acc[p][t][4q + r] = column 32t + 8q + 4h + r of pixel (qy0 + 2 wid + p, qx0 + l).  The layer's time
  // is its output, so the stores are laid out for the memory system: a wave parks 64 channels of its 32 pixels in LDS
  // and takes them back eight lanes to a pixel, so that a
  // store instruction writes eight whole 128-byte lines — straight from the accumulators a lane holds 8 channels of a
  // pixel and an instruction touches 32 lines, 32 bytes of each ----
  __syncthreads();                                     // every wave is through with the patch: the next item may stage its own
#pragma unroll
  for (int p = 0; p < MT; ++p) {
    const int qy = qy0 + 2 * wid + p;
#pragma unroll
    for (int cnk = 0; cnk < TILES / 2; ++cnk) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = 2 * cnk + tt;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 b4 = f32x4{0.f, 0.f, 0.f, 0.f};
          if (bias) b4 = *reinterpret_cast<const f32x4*>(bias + 32 * t + 8 * q + 4 * h);
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            v[r] = acc[p][t][4 * q + r] + b4[r];
            if (g.activation == 1) v[r] = fmaxf(v[r], 0.f);
          }
          uint2 o;
          o.x = pack_bf16(v[0], v[1]);
          o.y = pack_bf16(v[2], v[3]);
          *reinterpret_cast<uint2*>(stg + l * ROW + (32 * tt + 8 * q + 4 * h) * 2) = o;
        }
      }
      // (a wave's own staging area: its LDS accesses execute in order, no barrier)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int px = 8 * j + (lane >> 3), piece = lane & 7;
        const u32x4 o = *reinterpret_cast<const u32x4*>(stg + px * ROW + piece * 16);
        const int qx = qx0 + px;
        const int col = 64 * cnk + 8 * piece;
        if (qy < g.OH && qx < g.OW && col < g.Cout)
          *reinterpret_cast<u32x4*>(y + ((n * g.OH + qy) * g.OW + qx) * g.Cout + col) = o;
      }
    }
  }
  }       // items
}

// What the two image-side routes have in common: the layers they take, the geometry, the packed weights.
static bool image_side(const ConvCall& k) { return !k.up && k.dtype == 1 && k.cin <= 4 && !k.out_f32; }
static ImageConvGeom image_geom(const ConvCall& k) {
  ImageConvGeom g{};
  g.N = k.n; g.H = static_cast<int>(k.h); g.W = static_cast<int>(k.wd); g.Cin = static_cast<int>(k.cin); g.Cout = static_cast<int>(k.cout);
  g.kh = k.kh; g.kw = k.kw; g.sd = k.stride; g.py0 = k.kh / 2; g.px0 = k.kw / 2; g.activation = k.activation;
  g.OH = static_cast<int>((k.h + k.stride - 1) / k.stride); g.OW = static_cast<int>((k.wd + k.stride - 1) / k.stride);
  g.ksr = (k.kw * g.Cin + 15) / 16;
  return g;
}
static int image_weights(const ConvCall& k, const ImageConvGeom& g, int tiles, int frags, DevBuf& local, DevView* wpk) {
  return packed_weights(k.weights_key, 3, {k.kh, k.kw, k.cin, k.cout, tiles, g.ksr}, static_cast<size_t>(frags) * 16, k.stream,
                        local, &wpk->p, [&](void* dst) {
    hipLaunchKernelGGL(conv_image_weights_kernel, dim3((frags + 255) / 256), dim3(256), 0, k.stream, k.w, g, tiles,
                       static_cast<bf16x8*>(dst));
    return 0;
  });
}

int route_image(const ConvCall& k) {
  if (!image_side(k) || (k.cout != 128 && k.cout != 192) || (k.stride != 2 && k.stride != 4) || (k.stride * k.cin) % 2) return -1;
  hipStream_t st = k.stream;
  ImageConvGeom g = image_geom(k);
  g.BXn = (g.OW + 31) / 32; g.BYn = (g.OH + 7) / 8;
  g.PH = 7 * k.stride + k.kh;
  g.RL = (31 * k.stride + k.kw) * g.Cin;
  g.RS = ((31 * k.stride * g.Cin + 16 * g.ksr + 8) + 7) & ~7;       // the last lane's last K step stays inside its row
  const int tiles = static_cast<int>(k.cout / 32);
  // (patch | weight fragments | the epilogue's staging area: 4 waves x 32 pixels x 144 bytes)
  const size_t lds = static_cast<size_t>(g.PH) * g.RS * 2 + static_cast<size_t>(k.kh) * g.ksr * tiles * 64 * 16 + 4 * 32 * 144;
  g.items = 8;
  if (lds > kLdsBytesPerCu || k.n * g.BXn * g.BYn > kMaxGridX) return -1;
  // image rows and patch rows on 4-byte boundaries (x itself is: torch allocations are 256-byte aligned, and a slice
  // of a batch starts at a whole image)
  g.pairs = (g.W * g.Cin) % 2 == 0 && (g.px0 * g.Cin) % 2 == 0 && (g.H * g.W * g.Cin) % 2 == 0 &&
            reinterpret_cast<uintptr_t>(k.x) % 4 == 0;
  if (g.OW < 24) return -1;
  DevBuf wpk_local;
  DevView wpk;
  const int frags = k.kh * g.ksr * tiles * 64;
  if (const int rc = image_weights(k, g, tiles, frags, wpk_local, &wpk)) return rc;
  KernelTimer timer("conv2d", st);
  const dim3 grid(static_cast<unsigned>(ceil_div(k.n * g.BXn * g.BYn, g.items)));
  auto* kernel = tiles == 6 ? conv_image_kernel<6> : conv_image_kernel<4>;
  return launch(kernel, grid, dim3(256), lds, st, static_cast<const __bf16*>(k.x), wpk.as<bf16x8>(), k.bias,
                static_cast<__bf16*>(k.y), g);
}

// ---------------------------------------------------------------------------
// Image-side analysis layer, B fragments straight from the image, optionally WITH its GDN (bmshj2018's / ms2020's first
// layer: SignalConv2D(192, 5x5, /2, activation=GDN); bls2017's: 9x9, /4, its GDN as a kernel of its own — the 108 KB of
// 9x9 weight fragments and gamma's 74 KB do not share the LDS).  Cin = 3, Cout = 192, output rows of whole 32-pixel
// tiles.
// conv_image_kernel stages an image patch in LDS with 4-byte loads (0.79 ms for the 0.8 GB of bls2017's first layer at
// 512 x 256x256), and writes 4.8 GB at the C4 shape that the GDN kernel reads and writes again.  Here a wave takes 32
// consecutive pixels of an output row at a time and computes their 32 x Cout convolution outputs with KH * KSR K steps
// of MFMAs whose B fragments are 16 bytes of an image row each (the KW * Cin values of a kernel row are contiguous
// there; KSR = ceil(KW * Cin / 16) K steps per row) — which leaves them in the accumulators in exactly the layout the
// GDN contraction wants as ITS B fragments (gdn_common.h): contract |y| with gamma (fragments in LDS, as in the GDN
// kernel), divide, and store the result eight lanes to a pixel (whole 128-byte lines) through a wave-private staging
// area.  HBM traffic: the image in, the activations out, once.
// Same values as conv_image_kernel followed by the GDN kernel: the bias and beta are added to the finished float32 sums
// as there, the convolution's output is rounded to bfloat16 before the GDN as there.  (Carrying the bias in the spare
// sixteenth value of a kernel row's K step and beta as the contraction's initial accumulator was measured: 1.43 against
// 1.53 ms for the 5x5 layer, and two float32 additions that move inside the sums — 32 of 590 000 values differ, some by
// two bfloat16 units.  Interleaving a channel pair's epilogue with the next pair's MFMAs inside the wave: no change.)
// Persistent: a workgroup (8 waves) stages gamma's image and the convolution's fragments once and its waves walk the
// tiles (scalar arithmetic); image fragments live in a ring of PF registers sets, refilled — with this tile's later K
// steps, then the next tile's first ones — as soon as their MFMAs have read them.
// alpha = epsilon = 1, no rectification, not inverse.
// ---------------------------------------------------------------------------
template <int TILES, int KH, int KW, int SD, bool GDN>
__global__ void __launch_bounds__(512, 1) conv_image_direct_kernel(const __bf16* x, const bf16x8* wpk, const float* bias,
                                                                   const void* gimage, __bf16* y, ImageConvGeom g) {
  extern __shared__ unsigned char smem[];            // [gamma fragments | beta] | bias | conv fragments | staging (per wave)
  constexpr int KT = TILES, KS = 2 * TILES, C = 32 * TILES;
  constexpr int GFR = GDN ? KT * KS * 64 : 0, GBYTES = GDN ? GFR * 16 + C * 4 : 0;
  constexpr int ROW = 144;
  constexpr int CIN = 3, KSR = (KW * CIN + 15) / 16, NK = KH * KSR, PX0 = KW / 2, PY0 = KH / 2, PF = NK < 6 ? NK : 6;
  // zero padding left and right of an image row touches one lane each: (l, h) = (0, *) of a row's first tile, whose
  // fragment starts PX0 pixels left of the image, and (31, *) of its last tile
  static_assert(PX0 % 2 == 0 && (SD + PX0) % 2 == 0, "edge fix-ups move whole dwords");
  static_assert(SD >= PX0 && 16 * KSR <= CIN * (2 * SD + PX0), "only lanes 0 and 31 reach over the row's ends");
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l = lane & 31;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bf16x8* const ga = reinterpret_cast<const bf16x8*>(smem) + lane;
  const float* const beta_s = reinterpret_cast<const float*>(smem + GFR * 16);
  float* const bias_s = reinterpret_cast<float*>(smem + GBYTES);
  bf16x8* const wl = reinterpret_cast<bf16x8*>(smem + GBYTES + C * 4);
  constexpr int NFR = NK * TILES * 64;
  unsigned char* const stg = reinterpret_cast<unsigned char*>(wl + NFR) + wid * (32 * ROW);
  {
    if constexpr (GDN) {
      const u32x4* src = static_cast<const u32x4*>(gimage);
      u32x4* dst = reinterpret_cast<u32x4*>(smem);
      for (int i = tid; i < GFR + C / 4; i += 512) dst[i] = src[i];
    }
    for (int i = tid; i < NFR; i += 512) wl[i] = wpk[i];
    if (tid < C) bias_s[tid] = bias ? bias[tid] : 0.f;
  }
  __syncthreads();
  // (host: the tile count and the image's row count fit 32 bits)
  const unsigned int tpr = static_cast<unsigned int>(g.OW) / 32u;                  // tiles per output row
  const unsigned int ntiles = static_cast<unsigned int>(g.N) * g.OH * tpr;
  const unsigned int nwaves = gridDim.x * 8u, wave = blockIdx.x * 8u + wid;
  if (wave >= ntiles) return;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<__bf16*>(x), 0, static_cast<unsigned int>(g.N * g.H * g.W * CIN * 2), 0x00020000);
  // Fragment (K step ks = kernel row ks / KSR, part kk = ks % KSR) of lane (l, h): values 16 kk + 8 h ... + 7 of the
  // image row, counted from PX0 pixels left of pixel SD * (32 tx + l).  A row outside the image is read at an offset
  // outside the buffer (zeros).  Left of the image lie the first values of lane (0, h) in a row's first tile: that lane
  // reads DL dwords further right and the fix-up at the MFMA moves the fragment up by as much; right of it the last
  // values of lane (31, h) in the row's last tile: DT dwords further left (no load leaves the tensor), moved down.
  constexpr unsigned int kOutside = 0xFFFFFFF0u;
  auto clamp4 = [](int v) constexpr { return v < 0 ? 0 : v > 4 ? 4 : v; };
  struct Pos {
    unsigned int tx, n, oy;
    bool valid;
  };
  auto pos_of = [&](unsigned int tile) __attribute__((always_inline)) {
    Pos p;
    p.valid = tile < ntiles;
    p.tx = tile % tpr;
    const unsigned int r = tile / tpr;
    p.n = r / static_cast<unsigned int>(g.OH);
    p.oy = r - p.n * g.OH;
    return p;
  };
  auto columns = [&](const Pos& p, unsigned int (&cb)[KSR]) __attribute__((always_inline)) {
    const bool first = p.tx == 0 && l == 0, last = p.tx == tpr - 1 && l == 31;
#pragma unroll
    for (int kk = 0; kk < KSR; ++kk) {
      const int dla = clamp4((PX0 * CIN - 16 * kk + 1) / 2), dlb = clamp4((PX0 * CIN - 16 * kk - 8 + 1) / 2);
      const int dta = clamp4((16 * kk + 8 - CIN * (SD + PX0) + 1) / 2), dtb = clamp4((16 * kk + 16 - CIN * (SD + PX0) + 1) / 2);
      const int dl = h ? dlb : dla, dt = h ? dtb : dta;
      const int col = ((static_cast<int>(p.tx) * 32 + l) * SD - PX0) * CIN + 16 * kk + 8 * h;
      const bool none = (first && dl == 4) || (last && dt == 4);
      cb[kk] = none ? kOutside : static_cast<unsigned int>((col + (first ? 2 * dl : 0) - (last ? 2 * dt : 0)) * 2);
    }
  };
  auto fragment = [&](const Pos& p, const unsigned int (&cb)[KSR], int ks) __attribute__((always_inline)) {
    const int iy = static_cast<int>(p.oy) * SD - PY0 + ks / KSR;
    const bool rowok = p.valid && static_cast<unsigned int>(iy) < static_cast<unsigned int>(g.H);
    const unsigned int rowbytes = (p.n * g.H + iy) * static_cast<unsigned int>(g.W) * (CIN * 2u);   // < 2^32 (host)
    return __builtin_amdgcn_raw_buffer_load_b128(xr, rowok ? cb[ks % KSR] : kOutside, rowok ? rowbytes : 0u, 0);
  };
  auto up = [](u32x4 v, int d) __attribute__((always_inline)) {
    return d == 0 ? v : d == 1 ? u32x4{0u, v[0], v[1], v[2]} : d == 2 ? u32x4{0u, 0u, v[0], v[1]}
         : d == 3 ? u32x4{0u, 0u, 0u, v[0]} : u32x4{0u, 0u, 0u, 0u};
  };
  auto down = [](u32x4 v, int d) __attribute__((always_inline)) {
    return d == 0 ? v : d == 1 ? u32x4{v[1], v[2], v[3], 0u} : d == 2 ? u32x4{v[2], v[3], 0u, 0u}
         : d == 3 ? u32x4{v[3], 0u, 0u, 0u} : u32x4{0u, 0u, 0u, 0u};
  };
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  Pos cur = pos_of(wave);
  unsigned int cb[KSR];
  columns(cur, cb);
  u32x4 bq[PF];
#pragma unroll
  for (int k = 0; k < PF; ++k) bq[k] = fragment(cur, cb, k);
  for (unsigned int tile = wave;; tile += nwaves) {
    const Pos nxt = pos_of(tile + nwaves);
    unsigned int ncb[KSR];
    columns(nxt, ncb);
    const bool first = cur.tx == 0 && l == 0, last = cur.tx == tpr - 1 && l == 31;
    __bf16* const yrow = y + ((static_cast<long long>(cur.n) * g.OH + cur.oy) * g.OW + cur.tx * 32) * C;
    // ---- convolution: the weights' fragments one K step ahead of their MFMAs ----
    f32x16 acc[KT];
    bf16x8 aw[2][KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) aw[0][t] = wl[t * 64 + lane];
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      const int kk = ks % KSR, slot = ks % PF;
      if (ks + 1 < NK) {
#pragma unroll
        for (int t = 0; t < KT; ++t) aw[(ks + 1) & 1][t] = wl[((ks + 1) * TILES + t) * 64 + lane];
      }
      u32x4 v = bq[slot];
      {
        const int dla = clamp4((PX0 * CIN - 16 * kk + 1) / 2), dlb = clamp4((PX0 * CIN - 16 * kk - 8 + 1) / 2);
        const int dta = clamp4((16 * kk + 8 - CIN * (SD + PX0) + 1) / 2), dtb = clamp4((16 * kk + 16 - CIN * (SD + PX0) + 1) / 2);
        if (dla || dlb) v = first ? (h ? up(v, dlb) : up(v, dla)) : v;
        if (dta || dtb) v = last ? (h ? down(v, dtb) : down(v, dta)) : v;
      }
      const bf16x8 bfrag = __builtin_bit_cast(bf16x8, v);
#pragma unroll
      for (int t = 0; t < KT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aw[ks & 1][t], bfrag, ks ? acc[t] : zero, 0, 0, 0);
      // the slot's next fragment: a later K step of this tile, then the next tile's first ones
      const int kn = ks + PF;
      bq[slot] = kn < NK ? fragment(cur, cb, kn) : fragment(nxt, ncb, kn - NK);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (GDN) {
      // y = convolution + bias as the bfloat16 tensor would hold it: acc[t][4q + r] = channel 32 t + 8 q + 4 h + r of
      // pixel l, and K step s of the contraction = channels 16 s + 4 h + {0..3} and + 8
      u32x4 xb[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int t0 = s >> 1, q0 = 2 * (s & 1);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias_s + 32 * t0 + 8 * (q0 + half) + 4 * h);
          const int e = 4 * (q0 + half);
          xb[s][2 * half] = pack_bf16(f32x2{acc[t0][e], acc[t0][e + 1]} + f32x2{b4[0], b4[1]});
          xb[s][2 * half + 1] = pack_bf16(f32x2{acc[t0][e + 2], acc[t0][e + 3]} + f32x2{b4[2], b4[3]});
        }
      }
      // gamma's fragments one K step ahead, each register set refilled as soon as its MFMA has read it (a second
      // set does not fit: 96 accumulators + 48 of y + the image fragments in flight)
      bf16x8 af[KT];
#pragma unroll
      for (int t = 0; t < KT; ++t) af[t] = ga[(t * KS) * 64];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const bf16x8 bfrag = __builtin_bit_cast(bf16x8, xb[s] & 0x7FFF7FFFu);
#pragma unroll
        for (int t = 0; t < KT; ++t) {
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t], bfrag, s ? acc[t] : zero, 0, 0, 0);
          if (s + 1 < KS) af[t] = ga[(t * KS + s + 1) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // y / (beta + gamma^T |y|), 64 channels at a time through the staging area, then eight lanes to a pixel
#pragma unroll
      for (int cnk = 0; cnk < TILES / 2; ++cnk) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const int t = 2 * cnk + tt;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int s = 2 * t + (q >> 1), half = q & 1;
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(beta_s + 32 * t + 8 * q + 4 * h);
            f32x2 v[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              const unsigned int word = xb[s][2 * half + k];
              const f32x2 yv = {__uint_as_float(word << 16), __uint_as_float(word & 0xFFFF0000u)};
              const f32x2 nn = f32x2{acc[t][4 * q + 2 * k], acc[t][4 * q + 2 * k + 1]} + f32x2{b4[2 * k], b4[2 * k + 1]};
              const f32x2 rn = {__builtin_amdgcn_rcpf(nn[0]), __builtin_amdgcn_rcpf(nn[1])};
              v[k] = yv * rn;
            }
            uint2 o;
            o.x = pack_bf16(v[0]);
            o.y = pack_bf16(v[1]);
            *reinterpret_cast<uint2*>(stg + l * ROW + (32 * tt + 8 * q + 4 * h) * 2) = o;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int px = 8 * j + (lane >> 3), piece = lane & 7;
          const u32x4 o = *reinterpret_cast<const u32x4*>(stg + px * ROW + piece * 16);
          // (non-temporal stores measured level here: 1.56 ms either way at 128 x 768x512 — the layer writes at 3.1 TB/s where a
          // fill of its output runs at 6.9: it is bound by instruction issue, profiles/r04_notes.md)
          *reinterpret_cast<u32x4*>(yrow + px * C + 64 * cnk + 8 * piece) = o;
        }
      }
    } else {
      // bias, activation, round; 64 channels at a time through the staging area, then eight lanes to a pixel
#pragma unroll
      for (int cnk = 0; cnk < TILES / 2; ++cnk) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const int t = 2 * cnk + tt;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias_s + 32 * t + 8 * q + 4 * h);
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              v[k] = acc[t][4 * q + k] + b4[k];
              if (g.activation == 1) v[k] = fmaxf(v[k], 0.f);
            }
            uint2 o;
            o.x = pack_bf16(v[0], v[1]);
            o.y = pack_bf16(v[2], v[3]);
            *reinterpret_cast<uint2*>(stg + l * ROW + (32 * tt + 8 * q + 4 * h) * 2) = o;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int px = 8 * j + (lane >> 3), piece = lane & 7;
          const u32x4 o = *reinterpret_cast<const u32x4*>(stg + px * ROW + piece * 16);
          // (non-temporal stores measured level here: 1.56 ms either way at 128 x 768x512 — the layer writes at 3.1 TB/s where a
          // fill of its output runs at 6.9: it is bound by instruction issue, profiles/r04_notes.md)
          *reinterpret_cast<u32x4*>(yrow + px * C + 64 * cnk + 8 * piece) = o;
        }
      }
    }
    if (!nxt.valid) break;
    cur = nxt;
#pragma unroll
    for (int kk = 0; kk < KSR; ++kk) cb[kk] = ncb[kk];
  }
}

// With the layer's GDN where the caller asks for it and it is the 5x5 / 2 one.
int route_image_direct(const ConvCall& k) {
  if (!image_side(k) || k.cin != 3 || k.cout != 192 || k.kh != k.kw) return -1;
  hipStream_t st = k.stream;
  const tfc_gdn_params* gdn = k.gdn && k.gdn_fused && !k.gdn_inverse && k.activation == 0 && k.kh == 5 ? k.gdn : nullptr;
  const bool k5 = k.kh == 5 && k.stride == 2, k9 = k.kh == 9 && k.stride == 4;
  if (!k5 && !k9) return -1;
  if (gdn && (!k5 || gdn->channels != k.cout || gdn->dtype != 1 || k.activation != 0)) return -1;
  const ImageConvGeom g = image_geom(k);
  const int nk = k.kh * g.ksr;
  // whole tiles, the row's last pixel a whole stride from its end, dword-aligned rows
  if (g.OW % 32 != 0 || g.W % k.stride != 0 || reinterpret_cast<uintptr_t>(k.x) % 4 != 0) return -1;
  // one buffer resource over the tensor, 32-bit tile and row arithmetic in the kernel
  if (static_cast<double>(k.n) * k.h * k.wd * k.cin * 2 >= 4294967280.0 || static_cast<double>(k.n) * g.OH * (g.OW / 32) >= 2147483648.0)
    return -1;
  constexpr int tiles = 6;
  const size_t lds = (gdn ? static_cast<size_t>(tiles) * 2 * tiles * 64 * 16 + tiles * 32 * 4 : 0) + tiles * 32 * 4 +
                     static_cast<size_t>(nk) * tiles * 64 * 16 + 8 * 32 * 144;
  if (lds > kLdsBytesPerCu) return -1;
  DevBuf wpk_local;
  DevView wpk;
  const int frags = nk * tiles * 64;
  if (const int rc = image_weights(k, g, tiles, frags, wpk_local, &wpk)) return rc;
  const long long ntiles = k.n * g.OH * (g.OW / 32);
  const unsigned grid = static_cast<unsigned>(std::min<long long>(device_cus(), ceil_div(ntiles, 8)));
  KernelTimer timer("conv2d", st);
  auto* kernel = k5 && gdn ? conv_image_direct_kernel<6, 5, 5, 2, true>
                 : k5      ? conv_image_direct_kernel<6, 5, 5, 2, false>
                           : conv_image_direct_kernel<6, 9, 9, 4, false>;
  if (int rc = launch(kernel, dim3(grid), dim3(512), lds, st, static_cast<const __bf16*>(k.x), wpk.as<bf16x8>(), k.bias,
                      gdn ? gdn->image.p : nullptr, static_cast<__bf16*>(k.y), g))
    return rc;
  if (gdn) {
    const_cast<tfc_gdn_params*>(gdn)->image.touch(st);
    *k.gdn_fused = 1;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// The same, fused: the tap products of a block never leave the CU.  A workgroup takes an 8 x 32 block of INPUT pixels
// plus the halo the block's output pixels reach into ((8 + Uy - 1) x (32 + Ux - 1) patch pixels, 340 for a 5x5
// stride-2 kernel), computes z[patch pixel][(tap, c)] for them with the MFMA (fp32, into LDS: <= 80 columns, row
// stride 84 floats so that the 16-byte accumulator writes of 8 lanes cover all banks), and then every thread sums, for
// 4 consecutive output pixels of the block's (8s) x (32s) output tile, the <= ceil(k/s)^2 products that land on each.
// HBM traffic: the input once (+ 33 % halo, mostly L2 hits) and the output, instead of + 2 x 400 bytes of z per input
// pixel (5 GB each way at the C4 shape).  K and tap order as in the unfused pair.
// ---------------------------------------------------------------------------
struct UpFusedGeom {
  long long N;
  int H, W, Cin, Cout;
  int kh, kw, s;
  int dmax_y, dmax_x;       // halo before: patch origin = block origin - dmax
  int PH, PW;               // patch rows, columns
  int BXn, BYn;
  int NC;                   // kh * kw * Cout product columns
  int activation;
};
constexpr int kUpZStride = 84;      // floats per patch pixel in LDS
constexpr int kUpColTiles = 3;      // 96 >= NC columns

__global__ void conv_up_fused_weights_kernel(const float* w, int kh, int kw, int cin, int cout, bf16x8* packed) {
  // A fragments: packed[(ks * kUpColTiles + t) * 64 + lane], lane (i, h): K offsets 8h .. 8h + 7 of step ks,
  // column 32t + i = ((ty * kw + tx) * cout + c)
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int cb = cin / 16;
  const int total = cb * kUpColTiles * 64;
  if (idx >= total) return;
  const int lane = idx & 63;
  int r = idx >> 6;
  const int t = r % kUpColTiles; r /= kUpColTiles;
  const int ks = r % cb;
  const int col = 32 * t + (lane & 31), h = lane >> 5;
  const int jy = col / (kw * cout), rem = col % (kw * cout);
  const int tx = rem / cout, c = rem % cout;
  const int ty = jy;
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ci = ks * 16 + 8 * h + e;
    v[e] = static_cast<__bf16>(ty < kh ? w[((static_cast<long long>(ty) * kw + tx) * cin + ci) * cout + c] : 0.f);
  }
  packed[idx] = v;
}

constexpr int kUpThreads = 512;     // 8 waves: the block's 11 pixel tiles and 1024 output pixels over more waves
// KH, KW, S, COUT > 0: the gather is unrolled for that kernel (5, 5, 2, 3: bmshj2018's last layer); 0: any.
template <int KH, int KW, int S, int COUT>
__global__ void __launch_bounds__(kUpThreads) conv_up_fused_kernel(const __bf16* x, const bf16x8* wpk,
                                                                    const float* bias, __bf16* y, UpFusedGeom g) {
  extern __shared__ unsigned char smem[];            // z: tiles * 32 rows of kUpZStride floats | weight fragments
  constexpr int WAVES = kUpThreads / 64;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, l = lane & 31;
  long long b = blockIdx.x;
  const int bx = static_cast<int>(b % g.BXn); b /= g.BXn;
  const int by = static_cast<int>(b % g.BYn);
  const long long n = b / g.BYn;
  const int npix = g.PH * g.PW;
  const int tiles = (npix + 31) / 32;
  float* z = reinterpret_cast<float*>(smem);
  bf16x8* wl = reinterpret_cast<bf16x8*>(smem + static_cast<size_t>(tiles) * 32 * kUpZStride * 4);
  const int cb = g.Cin / 16;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<__bf16*>(x + n * g.H * g.W * g.Cin), 0, g.H * g.W * g.Cin * 2, 0x00020000);
  // this wave's first pixel tile: its first four K steps are requested before the weights are staged
  auto tile_offset = [&](int tile) -> unsigned int {
    const int pi = tile * 32 + l;
    const int py = pi / g.PW, px = pi - py * g.PW;
    const int iy = by * 8 - g.dmax_y + py, ix = bx * 32 - g.dmax_x + px;
    const bool ok = (pi < npix) & (static_cast<unsigned int>(iy) < static_cast<unsigned int>(g.H)) &
                    (static_cast<unsigned int>(ix) < static_cast<unsigned int>(g.W));
    return ok ? static_cast<unsigned int>(((iy * g.W + ix) * g.Cin + 8 * h) * 2) : 0x80000000u;
  };
  constexpr int PF = 4;                              // K steps in flight per pixel tile
  const int kh = KH ? KH : g.kh, kw = KW ? KW : g.kw, s = S ? S : g.s, cout = COUT ? COUT : g.Cout;
  const int OH = g.H * s, OW = g.W * s;
  const int tw = 32 * s, th = 8 * s;
  float bc[4] = {0.f, 0.f, 0.f, 0.f};
  if (bias)
    for (int c = 0; c < cout; ++c) bc[c] = bias[c];
  u32x4 bq[PF];
  unsigned int off = tile_offset(wid);
#pragma unroll
  for (int k = 0; k < PF; ++k) bq[k] = __builtin_amdgcn_raw_buffer_load_b128(xr, off, (k < cb ? k : cb - 1) * 32, 0);
  {
    const bf16x8* src = wpk;
    for (int i = tid; i < cb * kUpColTiles * 64; i += kUpThreads) wl[i] = src[i];
  }
  __syncthreads();
  // ---- z of the patch, a pixel tile (32 patch pixels) per wave at a time ----
  for (int tile = wid; tile < tiles; tile += WAVES) {
    const int pi = tile * 32 + l;
    f32x16 acc[kUpColTiles];
#pragma unroll
    for (int t = 0; t < kUpColTiles; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const unsigned int offn = tile_offset(tile + WAVES < tiles ? tile + WAVES : tile);
    for (int ks = 0; ks < cb; ks += PF) {            // (Cin % 64 == 0: PF K steps per turn, a ring of PF fragments)
#pragma unroll
      for (int k = 0; k < PF; ++k) {
#pragma unroll
        for (int t = 0; t < kUpColTiles; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[((ks + k) * kUpColTiles + t) * 64 + lane],
                                                          __builtin_bit_cast(bf16x8, bq[k]), acc[t], 0, 0, 0);
        // refill the slot: K step ks + k + PF of this tile, or the next tile's first ones
        const int kn = ks + k + PF;
        bq[k] = kn < cb ? __builtin_amdgcn_raw_buffer_load_b128(xr, off, kn * 32, 0)
                        : __builtin_amdgcn_raw_buffer_load_b128(xr, offn, (kn - cb) * 32, 0);
      }
    }
    off = offn;
    // acc[t][4q + r] = column 32t + 8q + 4h + r of patch pixel pi; columns < 80 go to LDS
    float* zrow = z + static_cast<size_t>(pi) * kUpZStride;
#pragma unroll
    for (int t = 0; t < kUpColTiles; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (32 * t + 8 * q >= kUpZStride) continue;
        if (32 * t + 8 * q + 4 * h + 4 > kUpZStride) continue;      // (columns 84 .. 87 of the h = 1 lanes: no room)
        *reinterpret_cast<f32x4*>(zrow + 32 * t + 8 * q + 4 * h) =
            f32x4{acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]};
      }
  }
  __syncthreads();
  // ---- gather: thread -> 4 consecutive output pixels of the (8 s) x (32 s) output tile ----
  for (int grp = tid; grp < th * (tw / 4); grp += kUpThreads) {
    const int ry = grp / (tw / 4), rx = (grp % (tw / 4)) * 4;
    const int oy = by * th + ry;
    if (oy >= OH) continue;
    // o = i*s + t - k/2  =>  t = (o + k/2) mod s, + s, ... ;  i = (o + k/2 - t) / s
    const int ty0 = (oy + kh / 2) % s;
    const int py0 = (oy + kh / 2 - ty0) / s - (by * 8 - g.dmax_y);       // patch row of tap ty0; ty0 + s: one row up
    unsigned short outv[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ox = bx * tw + rx + k;
      const int tx0 = (ox + kw / 2) % s;
      const int px0 = (ox + kw / 2 - tx0) / s - (bx * 32 - g.dmax_x);
      float a[4] = {bc[0], bc[1], bc[2], bc[3]};
#pragma unroll
      for (int jy = 0; jy < (KH ? (KH + S - 1) / S : 8); ++jy) {
        const int ty = ty0 + jy * s;
        if (ty >= kh) break;
#pragma unroll
        for (int jx = 0; jx < (KW ? (KW + S - 1) / S : 8); ++jx) {
          const int tx = tx0 + jx * s;
          if (tx >= kw) break;
          const float* zp = z + static_cast<size_t>((py0 - jy) * g.PW + (px0 - jx)) * kUpZStride +
                            (ty * kw + tx) * cout;
#pragma unroll
          for (int c = 0; c < (COUT ? COUT : 4); ++c)
            if (c < cout) a[c] += zp[c];
        }
      }
#pragma unroll
      for (int c = 0; c < (COUT ? COUT : 4); ++c) {
        float v = a[c];
        if (g.activation == 1) v = fmaxf(v, 0.f);
        outv[k * 4 + c] = float_to_bf16_bits(v);
      }
    }
    __bf16* dst = y + ((n * OH + oy) * OW + bx * tw + rx) * cout;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (bx * tw + rx + k >= OW) continue;
#pragma unroll
      for (int c = 0; c < (COUT ? COUT : 4); ++c)
        if (c < cout) dst[k * cout + c] = __builtin_bit_cast(__bf16, outv[k * 4 + c]);
    }
  }
}

// ---------------------------------------------------------------------------
// Transposed convolution into three channels (the synthesis transforms' last layer: bls2017's 9x9 x4, bmshj2018's 5x5
// x2, 192 -> 3) as a 3x3 convolution over the INPUT grid with S * S * 3 output columns, one per (output phase, channel):
//   y[S I + ry, S J + rx, c] = sum over dy, dx in {-1, 0, 1}, ci of x[I + dy, J + dx, ci] * w[t(ry, dy), t(rx, dx), ci, c]
// with t(r, d) = (r + K/2) mod S + S ((r + K/2) div S - d), taps outside [0, K) contributing nothing (from
// o = S i + t - K/2, the transposed convolution behind signal_conv.py:778-847's same_zeros padding).  The sums run in
// the MFMA's K dimension (v_mfma_f32_16x16x32_bf16: 16 columns x 16 pixels x 32 channels), so no tap products pass
// through memory or LDS (conv_up_fused_kernel parks 80 float32 products per input pixel in LDS and gathers; a 9x9
// kernel's 243 do not fit and that layer ran as an implicit GEMM over output pixels: 1.12 ms at 512 x 64x64).
// Columns: 16 per MFMA — S = 4: the twelve (rx, c) of one output row phase ry (+ 4 unused), four groups; S = 2: eight
// per ry (six used), one group.  Lane (n, g) of an accumulator then holds four consecutive values of output pixel
// row S I + ry at byte 2 (3 S (J0 + n) + 4 g): a wave's stores cover whole contiguous runs of the output row.
// A workgroup (8 waves) takes 8 input rows x 32 pixels, a wave one row (two 16-pixel halves); per 32-channel chunk the
// block's input tile (10 x 34 pixels, 96-byte pixel stride: conflict-free ds_read_b128 for the b128 lane groups) and
// the chunk's weight fragments are staged in LDS, the next chunk's global loads in flight under the MFMAs.  Two
// workgroups per CU.  For S = 4 the row phases ry >= 1 have no tap at dy = -1: those MFMAs are not issued.
// ---------------------------------------------------------------------------
struct UpPhaseGeom {
  long long N;
  int H, W, Cin;
  int activation;
  int nchunk;               // Cin / 32
};
constexpr int kPhaseRows = 8;                          // input rows per workgroup
constexpr int kPhaseTilePix = (kPhaseRows + 2) * 34;

template <int K, int S>
struct UpPhase {
  static constexpr int GROUPS = S == 4 ? 4 : 1;        // MFMA column groups
  // fragments per chunk, in the order the kernel walks them: dy, dx, group (skipping the groups without a tap)
  static constexpr int FRAGS = S == 4 ? 3 * 1 + 2 * 3 * 4 : 9;
  // 32-channel chunks staged at a time, and the tile's pixel stride in LDS (bytes; 64 of data per chunk): S = 2 takes two
  // chunks = one whole 128-byte line of a pixel per stage (a half line per stage was measured: 1.22 against 1.18 ms at
  // 128 x 256x384 — the other half has left the L2 by the next stage); S = 4 has 27 KB of fragments per chunk and
  // stays with one.  Both strides keep ds_read_b128 conflict-free for the b128 lane groups (16 n + g -> n PXS + 16 g).
  static constexpr int CPS = S == 4 ? 1 : 2;
  static constexpr int PXS = CPS == 1 ? 96 : 160;
  __host__ __device__ static constexpr int tap(int r, int d) { return (r + K / 2) % S + S * ((r + K / 2) / S - d); }
  __host__ __device__ static constexpr bool group_has(int grp, int dy) {
    return S != 4 || (tap(grp, dy) >= 0 && tap(grp, dy) < K);
  }
};

template <int K, int S>
__global__ void conv_up_phase_weights_kernel(const float* w, int cin, int cout, bf16x8* packed) {
  // packed[(chunk * FRAGS + slot) * 64 + lane], lane (m, g): column m of the slot's group, channels 32 chunk + 8 g ... + 7
  using P = UpPhase<K, S>;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = (cin / 32) * P::FRAGS * 64;
  if (idx >= total) return;
  const int lane = idx & 63, m = lane & 15, gq = lane >> 4;
  int slot = (idx >> 6) % P::FRAGS;
  const int chunk = (idx >> 6) / P::FRAGS;
  int dy = -1, dx = -1, grp = 0;
  {
    int s = 0;
    bool found = false;
    for (int a = -1; a <= 1 && !found; ++a)
      for (int b = -1; b <= 1 && !found; ++b)
        for (int gr = 0; gr < P::GROUPS && !found; ++gr) {
          if (!P::group_has(gr, a)) continue;
          if (s == slot) { dy = a; dx = b; grp = gr; found = true; }
          ++s;
        }
  }
  // column m of the group -> (ry, rx, c)
  int ry, rest;
  if (S == 4) { ry = grp; rest = m; } else { ry = m >> 3; rest = m & 7; }
  const int rx = rest / 3, c = rest % 3;
  const bool col_ok = rest < 3 * S && c < cout;
  const int ty = P::tap(ry, dy), tx = col_ok ? P::tap(rx, dx) : -1;
  const bool ok = col_ok && ty >= 0 && ty < K && tx >= 0 && tx < K;
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ci = 32 * chunk + 8 * gq + e;
    v[e] = static_cast<__bf16>(ok ? w[((static_cast<long long>(ty) * K + tx) * cin + ci) * cout + c] : 0.f);
  }
  packed[idx] = v;
}

template <int K, int S>
__global__ void __launch_bounds__(512, 2) conv_up_phase_kernel(const __bf16* x, const bf16x8* wpk, const float* bias,
                                                               __bf16* y, UpPhaseGeom g) {
  using P = UpPhase<K, S>;
  constexpr int GROUPS = P::GROUPS, FRAGS = P::FRAGS, HALVES = 2, CPS = P::CPS, PXS = P::PXS;
  extern __shared__ unsigned char smem[];            // input tile (CPS chunks) | weight fragments (CPS chunks)
  unsigned char* const xt = smem;
  bf16x8* const wt = reinterpret_cast<bf16x8*>(smem + kPhaseTilePix * PXS);
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, gq = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bxn = (g.W + 31) / 32, byn = (g.H + kPhaseRows - 1) / kPhaseRows;
  long long b = blockIdx.x;                          // (blocks in XCD order, xcd_order: measured level, 1.17-1.22 ms)
  const int bx = static_cast<int>(b % bxn); b /= bxn;
  const int by = static_cast<int>(b % byn);
  const long long img = b / byn;
  const int I0 = by * kPhaseRows, J0 = bx * 32;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<__bf16*>(x + img * g.H * g.W * g.Cin), 0, static_cast<unsigned int>(g.H * g.W * g.Cin * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16x8*>(wpk), 0, static_cast<unsigned int>(g.nchunk * FRAGS * 1024), 0x00020000);
  // staging: 16-byte pieces, 4 CPS to a tile pixel t (row t / 34, column t % 34 of the tile, origin (I0 - 1, J0 - 1))
  constexpr int PPP = 4 * CPS;                         // pieces per pixel
  constexpr int XP = (kPhaseTilePix * PPP + 511) / 512, WP = (CPS * FRAGS * 64 + 511) / 512;
  unsigned int xoff[XP];
#pragma unroll
  for (int r = 0; r < XP; ++r) {
    const int piece = tid + 512 * r, t = piece / PPP, q = piece % PPP;
    const int iy = I0 - 1 + t / 34, ix = J0 - 1 + t % 34;
    const bool ok = t < kPhaseTilePix && static_cast<unsigned int>(iy) < static_cast<unsigned int>(g.H) &&
                    static_cast<unsigned int>(ix) < static_cast<unsigned int>(g.W);
    xoff[r] = ok ? static_cast<unsigned int>(((iy * g.W + ix) * g.Cin) * 2 + q * 16) : 0x80000000u;
  }
  u32x4 xs[XP], ws[WP];
  auto request = [&](int stage) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < XP; ++r) xs[r] = __builtin_amdgcn_raw_buffer_load_b128(xr, xoff[r], stage * (64 * CPS), 0);
#pragma unroll
    for (int r = 0; r < WP; ++r) {
      const int i = tid + 512 * r;
      ws[r] = __builtin_amdgcn_raw_buffer_load_b128(wr, i < CPS * FRAGS * 64 ? i * 16u : 0x80000000u,
                                                    stage * (CPS * FRAGS * 1024), 0);
    }
  };
  auto park = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < XP; ++r) {
      const int piece = tid + 512 * r;
      if (piece < kPhaseTilePix * PPP)
        *reinterpret_cast<u32x4*>(xt + (piece / PPP) * PXS + (piece % PPP) * 16) = xs[r];
    }
#pragma unroll
    for (int r = 0; r < WP; ++r) {
      const int i = tid + 512 * r;
      if (i < CPS * FRAGS * 64) reinterpret_cast<u32x4*>(wt)[i] = ws[r];
    }
  };
  f32x4 acc[GROUPS][HALVES];
#pragma unroll
  for (int gr = 0; gr < GROUPS; ++gr)
#pragma unroll
    for (int p = 0; p < HALVES; ++p) acc[gr][p] = f32x4{0.f, 0.f, 0.f, 0.f};
  // this lane's B fragment of tap (0, 0), half 0: tile pixel (wid + 1, n + 1), channels 8 gq ... + 7 of the chunk
  const unsigned char* const bbase = xt + ((wid + 1) * 34 + n + 1) * PXS + 16 * gq;
  const int stages = g.nchunk / CPS;
  request(0);
  for (int stage = 0; stage < stages; ++stage) {
    __syncthreads();                                 // every wave is through with the previous stage
    park();
    __syncthreads();
    if (stage + 1 < stages) request(stage + 1);
#pragma unroll
    for (int sub = 0; sub < CPS; ++sub) {
      int slot = sub * FRAGS;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          bf16x8 bf[HALVES];
#pragma unroll
          for (int p = 0; p < HALVES; ++p)
            bf[p] = *reinterpret_cast<const bf16x8*>(bbase + (dy * 34 + dx + 16 * p) * PXS + 64 * sub);
#pragma unroll
          for (int gr = 0; gr < GROUPS; ++gr) {
            if (!P::group_has(gr, dy)) continue;
            const bf16x8 a = wt[slot * 64 + lane];
            ++slot;
#pragma unroll
            for (int p = 0; p < HALVES; ++p)
              acc[gr][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf[p], acc[gr][p], 0, 0, 0);
          }
        }
    }
  }
  // ---- epilogue: acc[gr][p][i] = column 4 gq + i of the group, input pixel (I0 + wid, J0 + 16 p + n) ----
  const int I = I0 + wid;
  if (I >= g.H) return;
  const int OW = g.W * S;
  // the values of this lane: S = 4: (rx, c) = 4 gq + i of 12 (gq = 3: none); S = 2: ry = gq >> 1, 4 (gq & 1) + i of 6
  const int first = S == 4 ? 4 * gq : 4 * (gq & 1);
  const int count = S == 4 ? (gq < 3 ? 4 : 0) : ((gq & 1) ? 2 : 4);
  float bc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) bc[i] = bias ? bias[(first + i) % 3] : 0.f;
#pragma unroll
  for (int gr = 0; gr < GROUPS; ++gr) {
    const int ry = S == 4 ? gr : (gq >> 1);
    __bf16* const yrow = y + ((img * g.H * S + static_cast<long long>(I) * S + ry) * OW) * 3;
#pragma unroll
    for (int p = 0; p < HALVES; ++p) {
      const int J = J0 + 16 * p + n;
      if (J >= g.W || count == 0) continue;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = acc[gr][p][i] + bc[i];
        if (g.activation == 1) v[i] = fmaxf(v[i], 0.f);
      }
      unsigned int* dst = reinterpret_cast<unsigned int*>(yrow + static_cast<long long>(J) * (3 * S) + first);
      dst[0] = pack_bf16(v[0], v[1]);
      if (count == 4) dst[1] = pack_bf16(v[2], v[3]);
    }
  }
}

// The synthesis transforms' last layer as a 3x3 convolution over the input grid.
int route_up_phase(const ConvCall& k) {
  if (!k.up || k.dtype != 1 || k.cout != 3 || k.out_f32) return -1;
  hipStream_t st = k.stream;
  static const bool off = env_switch("TFC_CONV_UP_PHASE") == 0;
  if (off || k.cin % 32 || k.kh != k.kw) return -1;
  const bool k5 = k.kh == 5 && k.stride == 2, k9 = k.kh == 9 && k.stride == 4;
  if (!k5 && !k9) return -1;
  if (static_cast<double>(k.h) * k.wd * k.cin * 2 >= 2147483648.0) return -1;          // one buffer resource per image
  // (rows of 3 S bfloat16 per input pixel: 4-byte stores need S even — both are — and a 4-byte aligned y)
  if (reinterpret_cast<uintptr_t>(k.y) % 4 != 0 || reinterpret_cast<uintptr_t>(k.x) % 16 != 0) return -1;
  UpPhaseGeom g{};
  g.N = k.n; g.H = static_cast<int>(k.h); g.W = static_cast<int>(k.wd); g.Cin = static_cast<int>(k.cin);
  g.activation = k.activation; g.nchunk = static_cast<int>(k.cin / 32);
  const long long blocks = k.n * ((g.H + kPhaseRows - 1) / kPhaseRows) * ((g.W + 31) / 32);
  if (blocks > kMaxGridX) return -1;
  const int frags_per_chunk = k9 ? UpPhase<9, 4>::FRAGS : UpPhase<5, 2>::FRAGS;
  const int frags = g.nchunk * frags_per_chunk * 64;
  const int cps = k9 ? UpPhase<9, 4>::CPS : UpPhase<5, 2>::CPS, pxs = k9 ? UpPhase<9, 4>::PXS : UpPhase<5, 2>::PXS;
  if (g.nchunk % cps) return -1;
  const size_t lds = static_cast<size_t>(kPhaseTilePix) * pxs + static_cast<size_t>(cps) * frags_per_chunk * 1024;
  auto run = [&](auto weights_kernel, auto kernel) -> int {
    DevBuf wpk_local;
    DevView wpk;
    const int rc = packed_weights(k.weights_key, 5, {k.kh, k.kw, k.cin, k.cout, k.stride}, static_cast<size_t>(frags) * 16, st,
                                  wpk_local, &wpk.p, [&](void* dst) {
      hipLaunchKernelGGL(weights_kernel, dim3((frags + 255) / 256), dim3(256), 0, st, k.w, static_cast<int>(k.cin),
                         static_cast<int>(k.cout), static_cast<bf16x8*>(dst));
      return 0;
    });
    if (rc) return rc;
    KernelTimer timer("conv2d", st);
    return launch(kernel, dim3(static_cast<unsigned>(blocks)), dim3(512), lds, st, static_cast<const __bf16*>(k.x),
                  wpk.as<bf16x8>(), k.bias, static_cast<__bf16*>(k.y), g);
  };
  return k9 ? run(conv_up_phase_weights_kernel<9, 4>, conv_up_phase_kernel<9, 4>)
            : run(conv_up_phase_weights_kernel<5, 2>, conv_up_phase_kernel<5, 2>);
}

}  // namespace tfc
extern "C" int tfc_conv2d_drop_weights(uint64_t key);
namespace tfc {
// ---------------------------------------------------------------------------
// float32 layers on the bfloat16 matrix cores (round 6).  v_mfma_f32_32x32x2_f32 runs at 1/16 of the bfloat16 rate, and
// the float32 model steps are 90 % convolutions.  A float32 value is the sum of three bfloat16 values to its last bit
// (a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2): 3 x 8 significant bits), and the product of two such sums is
//     a b = a1 b1 + a1 b2 + a2 b1 + a1 b3 + a2 b2 + a3 b1 + (terms below 2^-25 |a b|),
// every retained product exact in float32 and accumulated in float32 by the MFMA: the convolution of float32 tensors is
// ONE bfloat16 convolution with six times the input channels, [x1 | x1 | x1 | x2 | x2 | x3] against the kernel planes
// [w1 | w2 | w3 | w1 | w2 | w1], with float32 output — 6/16 of the float32 MFMA time on kernels that are also further
// along (second generation: 16-byte gathers 4 K steps ahead, packed weights through LDS).  The result differs from a
// float32 FMA chain by float32 rounding noise (a few 1e-7 relative; tests/test_signal_conv_gpu.py holds both to the float32
// definition).  TFC_CONV_F32=native keeps the float32 MFMA kernel; layers with <= 4 channels on one side keep it anyway.
// ---------------------------------------------------------------------------
// x float32 [pixels, C] -> xs bfloat16 [pixels, 6 C]; a thread takes 8 channels of a pixel (C % 8 == 0)
__global__ void __launch_bounds__(256) conv_split_x_kernel(const float* x, long long pixels, int C, __bf16* xs) {
  const int per = C / 8;
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= pixels * per) return;
  const long long pix = i / per;
  const int c0 = static_cast<int>(i - pix * per) * 8;
  const f32x4 lo = *reinterpret_cast<const f32x4*>(x + pix * C + c0), hi = *reinterpret_cast<const f32x4*>(x + pix * C + c0 + 4);
  bf16x8 p1, p2, p3;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    __bf16 a, b, c;
    split3(e < 4 ? lo[e] : hi[e - 4], &a, &b, &c);
    p1[e] = a; p2[e] = b; p3[e] = c;
  }
  __bf16* row = xs + pix * 6 * C + c0;
  *reinterpret_cast<bf16x8*>(row) = p1;
  *reinterpret_cast<bf16x8*>(row + C) = p1;
  *reinterpret_cast<bf16x8*>(row + 2 * C) = p1;
  *reinterpret_cast<bf16x8*>(row + 3 * C) = p2;
  *reinterpret_cast<bf16x8*>(row + 4 * C) = p2;
  *reinterpret_cast<bf16x8*>(row + 5 * C) = p3;
}
void launch_conv_split_x(const float* x, long long pixels, int C, __bf16* xs, hipStream_t st) {
  hipLaunchKernelGGL(conv_split_x_kernel, dim3(static_cast<unsigned>(ceil_div(pixels * (C / 8), 256))), dim3(256), 0, st, x,
                     pixels, C, xs);
}
// w float32 [taps, C, Cout] -> w6 float32 [taps, 6 C, Cout] holding the planes [w1 | w2 | w3 | w1 | w2 | w1] as float32
// values (each exactly a bfloat16: the packing kernels' rounding leaves them as they are)
__global__ void __launch_bounds__(256) conv_split_w_kernel(const float* w, long long taps, int C, int Cout, float* w6) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= taps * C * Cout) return;
  const int co = static_cast<int>(i % Cout);
  const long long tc = i / Cout;
  const int c = static_cast<int>(tc % C);
  const long long t = tc / C;
  __bf16 a, b, d;
  split3(w[i], &a, &b, &d);
  const float p[3] = {static_cast<float>(a), static_cast<float>(b), static_cast<float>(d)};
  const int plane[6] = {0, 1, 2, 0, 1, 0};
  float* base = w6 + (t * 6 * C + c) * Cout + co;
#pragma unroll
  for (int q = 0; q < 6; ++q) base[static_cast<long long>(q) * C * Cout] = p[plane[q]];
}

// (read per call: the tests compare the two in one process)
static bool conv_f32_split_enabled() {
  const char* e = env_str("TFC_CONV_F32");
  return !(e && std::strcmp(e, "native") == 0);
}

// The input's planes go through in chunks of images (conv_f32_chunks), each chunk split and convolved before the next —
// the kernel's six planes are made and packed once, under the key derived from the caller's or a key of this call's own.
int route_f32_planes(const ConvCall& k) {
  if (k.dtype != 0 || !conv_f32_split_enabled() || k.cin % 16 || k.cout % 4 || k.gdn ||
      6 * k.cin * static_cast<int64_t>(k.kh) * k.kw >= (int64_t{1} << 24))
    return -1;
  hipStream_t st = k.stream;
  const int64_t cin = k.cin, cout = k.cout;
  const long long taps = static_cast<long long>(k.kh) * k.kw;
  DevBuf w6;
  TFC_HIP(w6.alloc(static_cast<size_t>(taps) * 6 * cin * cout * sizeof(float), st));
  const long long wthreads = taps * cin * cout;
  hipLaunchKernelGGL(conv_split_w_kernel, dim3(static_cast<unsigned>(ceil_div(wthreads, 256))), dim3(256), 0, st,
                     k.w, taps, static_cast<int>(cin), static_cast<int>(cout), w6.as<float>());
  static std::atomic<unsigned long long> own_keys{0};
  // one bfloat16 convolution per chunk: six times the channels, float32 out, the planes' key
  ConvCall planes = k;
  planes.w = w6.as<float>(); planes.dtype = 1; planes.cin = 6 * cin; planes.out_f32 = true;
  planes.weights_key = k.weights_key ? (k.weights_key ^ kPlanesKey)
                                     : (0xf32c000000000000ull | own_keys.fetch_add(1, std::memory_order_relaxed));
  const long long out_image = (k.up ? static_cast<long long>(k.h) * k.stride * k.wd * k.stride
                                    : static_cast<long long>((k.h + k.stride - 1) / k.stride) * ((k.wd + k.stride - 1) / k.stride)) * cout;
  const int rc = conv_f32_chunks("tfc_conv2d", "conv2d", static_cast<const float*>(k.x), k.n, static_cast<long long>(k.h) * k.wd,
                                 cin, st, [&](int64_t n0, int64_t images, const __bf16* xs) {
    planes.x = xs; planes.n = images;
    planes.y = static_cast<float*>(k.y) + n0 * out_image;
    return conv_entry(planes);
  });
  if (!k.weights_key) (void)tfc_conv2d_drop_weights(planes.weights_key);
  return rc;
}

// Fused variant of the transposed convolution into few channels.
int route_up_fused(const ConvCall& k) {
  if (!k.up || k.dtype != 1 || k.cout > 4 || k.cin % 64 || k.stride < 2 || k.out_f32) return -1;
  hipStream_t st = k.stream;
  UpFusedGeom g{};
  g.N = k.n; g.H = static_cast<int>(k.h); g.W = static_cast<int>(k.wd); g.Cin = static_cast<int>(k.cin);
  g.Cout = static_cast<int>(k.cout); g.kh = k.kh; g.kw = k.kw; g.s = k.stride; g.activation = k.activation;
  const UpTaps ty = up_taps(k.kh, k.stride), tx = up_taps(k.kw, k.stride);
  g.dmax_y = ty.dmax; g.dmax_x = tx.dmax;
  g.PH = 8 + ty.dmax - ty.dmin; g.PW = 32 + tx.dmax - tx.dmin;
  g.BXn = (g.W + 31) / 32; g.BYn = (g.H + 7) / 8;
  g.NC = k.kh * k.kw * g.Cout;
  // all kh * kw * Cout tap products of a patch pixel in one LDS row; kernels with more of them (bls2017's 9 x 9 x 3)
  // keep the implicit GEMM over output pixels (a pass per kernel-row residue was built and measured level with it)
  if (g.NC > kUpZStride) return -1;
  const int tiles = (g.PH * g.PW + 31) / 32;
  const size_t lds = static_cast<size_t>(tiles) * 32 * kUpZStride * 4 + static_cast<size_t>(k.cin / 16) * kUpColTiles * 64 * 16;
  if (lds > kLdsBytesPerCu || k.n * g.BXn * g.BYn > kMaxGridX) return -1;
  DevBuf wpk;
  const int frags = static_cast<int>(k.cin / 16) * kUpColTiles * 64;
  TFC_HIP(wpk.alloc(static_cast<size_t>(frags) * 16, st));
  hipLaunchKernelGGL(conv_up_fused_weights_kernel, dim3((frags + 255) / 256), dim3(256), 0, st, k.w, k.kh, k.kw,
                     static_cast<int>(k.cin), static_cast<int>(k.cout), wpk.as<bf16x8>());
  KernelTimer timer("conv2d", st);
  auto* kernel = k.kh == 5 && k.kw == 5 && k.stride == 2 && k.cout == 3   ? conv_up_fused_kernel<5, 5, 2, 3>      // bmshj2018
                 : k.kh == 9 && k.kw == 9 && k.stride == 4 && k.cout == 3 ? conv_up_fused_kernel<9, 9, 4, 3>      // bls2017
                                                                          : conv_up_fused_kernel<0, 0, 0, 0>;
  return launch(kernel, dim3(static_cast<unsigned>(k.n * g.BXn * g.BYn)), dim3(kUpThreads), lds, st,
                static_cast<const __bf16*>(k.x), wpk.as<bf16x8>(), k.bias, static_cast<__bf16*>(k.y), g);
}

// The 1x1 product and the gather as two kernels: what route_up_fused has left.
// (up to 128 product columns, i.e. one column group: a 9x9 stride-4 kernel has 324 and measured the same
// or slower this way — 0.19 against 0.16 ms at batch 64 — so it keeps the implicit GEMM over output pixels)
int route_up_gather(const ConvCall& k) {
  if (!k.up || k.dtype != 1 || k.cout > 4 || k.cin % 16 || k.stride < 2 || k.kh * k.kw * 4 > 128 || k.out_f32) return -1;
  hipStream_t st = k.stream;
  const int zc = k.kh * k.kw * 4;
  DevBuf w1, z;
  TFC_HIP(w1.alloc(sizeof(float) * k.cin * zc, st));
  TFC_HIP(z.alloc(sizeof(float) * static_cast<size_t>(k.n) * k.h * k.wd * zc, st));
  const long long wtotal = static_cast<long long>(k.cin) * zc;
  hipLaunchKernelGGL(conv_up_weights_kernel, dim3(static_cast<unsigned>(ceil_div(wtotal, 256))), dim3(256), 0, st, k.w,
                     k.kh, k.kw, static_cast<int>(k.cin), static_cast<int>(k.cout), w1.as<float>());
  // the 1x1 product: a "down" convolution with a 1x1 kernel, stride 1, no bias, no activation, float32 out; its
  // weights are made above for this call: no key
  ConvCall prod{};
  prod.x = k.x; prod.w = w1.as<float>(); prod.y = z.p; prod.dtype = 1;
  prod.n = k.n; prod.h = k.h; prod.wd = k.wd; prod.cin = k.cin; prod.cout = zc;
  prod.kh = prod.kw = prod.stride = 1;
  prod.out_f32 = true; prod.stream = st; prod.weights_key = 0;
  if (int rc = conv_entry(prod)) return rc;
  const long long outs = k.n * k.h * k.stride * k.wd * k.stride;
  if (ceil_div(outs, 256) > kMaxGridX) return fail("tfc_conv2d_up: problem too large for one launch");
  KernelTimer timer("conv2d", st);
  hipLaunchKernelGGL(conv_up_gather_kernel, dim3(static_cast<unsigned>(ceil_div(outs, 256))), dim3(256), 0, st,
                     z.as<float>(), k.bias, static_cast<__bf16*>(k.y), static_cast<long long>(k.n), static_cast<int>(k.h),
                     static_cast<int>(k.wd), k.kh, k.kw, k.stride, static_cast<int>(k.cout), k.activation);
  TFC_HIP(hipGetLastError());
  return 0;
}

// The implicit GEMM over low-resolution output pixels: every shape the routes before it have left.
int route_gemm(const ConvCall& k) {
  ConvGeom c{};
  c.xcd = xcd_blocks();
  PackGeom g{};
  g.kh = k.kh; g.kw = k.kw; g.Cin_real = static_cast<int>(k.cin); g.Cout = static_cast<int>(k.cout);
  g.up = k.up; g.su = k.up ? k.stride : 1;
  c.N = k.n; c.H = static_cast<int>(k.h); c.W = static_cast<int>(k.wd);
  c.Cout = static_cast<int>(k.cout);
  c.activation = k.activation;
  c.out_f32 = k.out_f32 ? 1 : 0;      // only reached with the second-generation bf16 kernel (Cin % 16 == 0, Cout % 4 == 0)
  if (!k.up) {
    c.sd = k.stride; c.su = 1;
    c.Uy = k.kh; c.Ux = k.kw;
    c.py0 = k.kh / 2; c.px0 = k.kw / 2;
    c.OHq = static_cast<int>((k.h + k.stride - 1) / k.stride);
    c.OWq = static_cast<int>((k.wd + k.stride - 1) / k.stride);
  } else {
    const UpTaps ty = up_taps(k.kh, k.stride), tx = up_taps(k.kw, k.stride);
    g.dmax_y = ty.dmax; g.dmax_x = tx.dmax;
    c.sd = 1; c.su = k.stride;
    c.Uy = ty.dmax - ty.dmin + 1; c.Ux = tx.dmax - tx.dmin + 1;
    c.py0 = g.dmax_y; c.px0 = g.dmax_x;
    c.OHq = c.H; c.OWq = c.W;
  }
  g.Uy = c.Uy; g.Ux = c.Ux;
  fast_div_setup(static_cast<unsigned int>(c.OWq), &c.owq_mul, &c.owq_sh);
  fast_div_setup(static_cast<unsigned int>(c.OHq), &c.ohq_mul, &c.ohq_sh);
  c.pix32 = static_cast<long long>(k.n) * c.OHq * c.OWq + 512 < (1ll << 31) ? 1 : 0;    // (+ the last workgroup's overhang)
  c.cols = c.su * c.su * c.Cout;
  c.OH = c.OHq * c.su; c.OW = c.OWq * c.su;
  if (k.cin <= 4) {
    c.small_cin = 1;
    c.Cin = 4;
    c.kw4 = (c.Ux * 4 + 15) / 16;
    c.ksteps = c.Uy * c.kw4;
    c.Hp = (c.OHq - 1) * c.sd + c.Uy;
    c.Wp = std::max((c.OWq - 1) * c.sd + c.Ux, c.px0 + c.W);
    c.Hp = std::max(c.Hp, c.py0 + c.H);
  } else {
    c.small_cin = 0;
    c.Cin = static_cast<int>(k.cin);
    c.Hp = c.H; c.Wp = c.W;
    c.ksteps = c.Uy * c.Ux * (c.Cin / 16);
  }
  if (k.gdn && k.gdn_fused && k.dtype == 1 && k.gdn->dtype == 1 && k.gdn->channels == k.cout && k.activation == 0 &&
      !k.out_f32) {
    // GDN / IGDN as the activation: where the third-generation kernel takes the layer (it says so through *gdn_fused)
    c.gdn = k.gdn_inverse ? 2 : 1;
    c.gdn_image = k.gdn->image.p;
    const_cast<tfc_gdn_params*>(k.gdn)->image.touch(k.stream);
  }
  return k.dtype == 1 ? run_conv<__bf16>(k.x, k.w, k.bias, k.y, c, g, k.weights_key, k.stream, k.gdn_fused)
                      : run_conv<float>(k.x, k.w, k.bias, k.y, c, g, k.weights_key, k.stream, k.gdn_fused);
}

int conv_entry(const ConvCall& k) {
  if (k.gdn_fused) *k.gdn_fused = 0;
  if (int rc = check_dtype("tfc_conv2d", k.dtype)) return rc;
  if (k.kh < 1 || k.kw < 1 || k.stride < 1 || k.cin < 1 || k.cout < 1) return fail("tfc_conv2d: bad geometry");
  if (!(k.cin % 16 == 0 || k.cin <= 4))
    return fail("tfc_conv2d: input channels must be a multiple of 16 or <= 4 (got %lld)", static_cast<long long>(k.cin));
  if (k.activation != 0 && k.activation != 1) return fail("tfc_conv2d: activation must be 0 (none) or 1 (relu)");
  if (k.n == 0 || k.h == 0 || k.wd == 0) return 0;
  // the first route that takes the shape runs it; route_gemm takes every shape the others leave
  static int (*const routes[])(const ConvCall&) = {
      route_f32_planes,
#ifndef TFC_CONV_NO_UP_GATHER
      route_up_phase, route_up_fused, route_up_gather,
#endif
      route_image_direct, route_image, route_gemm,
  };
  int rc = -1;
  for (auto route : routes)
    if ((rc = route(k)) >= 0) break;
  return rc;
}

static ConvCall conv_call(const void* x, const void* w, const float* bias, void* y, int dtype, int64_t n, int64_t h,
                          int64_t wd, int64_t cin, int64_t cout, int kh, int kw, int stride, int activation, int up,
                          void* stream) {
  ConvCall k{};
  k.x = x; k.w = static_cast<const float*>(w); k.bias = bias; k.y = y; k.dtype = dtype;
  k.n = n; k.h = h; k.wd = wd; k.cin = cin; k.cout = cout; k.kh = kh; k.kw = kw; k.stride = stride;
  k.activation = activation; k.up = up;
  k.stream = static_cast<hipStream_t>(stream);
  k.weights_key = t_next_weights_key;
  t_next_weights_key = 0;
  return k;
}

}  // namespace tfc

extern "C" void tfc_conv2d_weights_key(uint64_t key) { tfc::t_next_weights_key = key; }

extern "C" int tfc_conv2d_drop_weights(uint64_t key) {
  tfc::WeightsCache& c = tfc::WeightsCache::get();
  std::lock_guard<std::mutex> lock(c.mu);
  // A kernel on any stream that used an entry may still read its fragments.  The memory goes back in STREAM order: the
  // stream the entry was made on waits for an event on every other stream that read it, and the block returns to the
  // library's cache behind that (DevBuf::release: reusable on that stream at once, on another once its event has
  // completed).  Nothing here holds the host — model.eval() drops one key per layer.  Only when a reader's stream no
  // longer takes an event (destroyed by its owner) is that entry's device drained instead.
  int home = 0;
  (void)hipGetDevice(&home);
  for (auto it = c.entries.begin(); it != c.entries.end();) {
    // (and the six-plane kernel a float32 layer packed under the key derived from it: route_f32_planes)
    if (it->first.key != key && it->first.key != (key ^ tfc::kPlanesKey)) { ++it; continue; }
    tfc::WeightsCache::Entry& e = it->second;
    if (it->first.dev != home) (void)hipSetDevice(it->first.dev);
    bool ordered = true;
    for (hipStream_t s : e.users) {
      hipEvent_t ev = nullptr;
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { ordered = false; break; }
      if (hipEventRecord(ev, s) != hipSuccess || hipStreamWaitEvent(e.made_on, ev, 0) != hipSuccess) ordered = false;
      (void)hipEventDestroy(ev);
      if (!ordered) break;
    }
    if (!ordered) {
      (void)hipGetLastError();
      (void)hipDeviceSynchronize();
    }
    e.buf.touch(e.made_on);
    (void)hipEventDestroy(e.ready);
    it = c.entries.erase(it);          // ~DevBuf: release() in the order of made_on
    if (it == c.entries.end() || it->first.dev != home) (void)hipSetDevice(home);
  }
  (void)hipSetDevice(home);
  return 0;
}

extern "C" int tfc_conv2d_down(const void* x, const void* w, const float* bias, void* y, int dtype,
                               int64_t n, int64_t h, int64_t wd, int64_t cin, int64_t cout, int kh,
                               int kw, int stride, int activation, void* stream) {
  return tfc::conv_entry(tfc::conv_call(x, w, bias, y, dtype, n, h, wd, cin, cout, kh, kw, stride, activation, 0, stream));
}

extern "C" int tfc_conv2d_gdn(const void* x, const void* w, const float* bias, void* y, int dtype,
                              int64_t n, int64_t h, int64_t wd, int64_t cin, int64_t cout, int kh,
                              int kw, int stride, int up, const tfc_gdn_params* gdn, int inverse, int* fused,
                              void* stream) {
  // (the key named for THIS call is taken before the checks: it must not reach another layer's)
  tfc::ConvCall k = tfc::conv_call(x, w, bias, y, dtype, n, h, wd, cin, cout, kh, kw, stride, 0, up, stream);
  if (!gdn || !fused) return tfc::fail("tfc_conv2d_gdn: gdn and fused must not be null");
  k.gdn = gdn; k.gdn_inverse = inverse; k.gdn_fused = fused;
  return tfc::conv_entry(k);
}

extern "C" int tfc_conv2d_up(const void* x, const void* w, const float* bias, void* y, int dtype,
                             int64_t n, int64_t h, int64_t wd, int64_t cin, int64_t cout, int kh,
                             int kw, int stride, int activation, void* stream) {
  return tfc::conv_entry(tfc::conv_call(x, w, bias, y, dtype, n, h, wd, cin, cout, kh, kw, stride, activation, 1, stream));
}
