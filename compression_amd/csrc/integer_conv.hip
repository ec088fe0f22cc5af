// The integer convolution layer (include/tfc_hip.h, tfc_integer_conv2d): an implicit GEMM on v_mfma_i32_16x16x64_i8 with
// int32 accumulators in registers; bias, rounding division, clamp and the uint8 store in the same kernel.
//
// Roles.  A tile is 16 output channels (the MFMA's A side: its rows) by 16 pixels (the B side: its columns), so that the
// result has the pixel on the lane (lane & 15) and four CONSECUTIVE output channels in a lane's four registers
// (row = 4 (lane >> 4) + reg): one dword store per tile and lane.  The reduction runs over (tap, input channel) in
// chunks of 16 channels: lane group g = lane >> 4 of step s takes chunk 4 s + g, for A (16 bytes of the weights
// [kh, kw, Cout, Cin]) and for B (16 bytes of x at the tap's source pixel) alike.  Both operands put the same (tap,
// channel) into the same (lane group, byte), which is all an integer sum needs of the instruction's k order.
//
// A wave takes 64 pixels x 64 output channels (16 accumulator tiles), a workgroup four such waves side by side in the
// pixel direction; the weights and the activations come straight from global memory (they are L2 resident: a layer's
// weights are under 1 MB), the next step's fragments loaded in front of this step's MFMAs.  No LDS.
//
// The transposed direction is phase-split: blockIdx.z is the output phase (oy mod s, ox mod s), whose pixels see only
// the taps t = t0 + s m with t0 = (phase + k / 2) mod s; the inserted zeros are never multiplied.
//
// uint8 activations travel as a - 128 (one XOR per packed dword).  A source outside the image, and a chunk past the
// end of the reduction, is loaded as 0 and XORed like every other, i.e. it IS the value 0 in that representation, so
// the correction is 128 times the sum of ALL the weights the lane multiplied, whichever pixel: summed beside the MFMAs
// (v_dot4 with ones) and added in the epilogue.
#include <cstdint>

#include "common.h"
#include "integer_conv_params.h"
#include "launch.h"
#include "../../include/tfc_hip.h"

namespace tfc {
namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;

static_assert(IC_WAVE_PIXELS % IC_TILE_PIXELS == 0 && IC_WAVE_COUTS % IC_TILE_COUTS == 0, "whole tiles");
static_assert(IC_BLOCK_PIXELS % IC_WAVE_PIXELS == 0, "whole waves");
static_assert(IC_TILE_PIXELS == 16 && IC_TILE_COUTS == 16 && IC_CHUNK_CHANNELS == 16, "the 16x16x64 i8 MFMA");

constexpr int PT = IC_WAVE_PIXELS / IC_TILE_PIXELS;      // pixel tiles of a wave
constexpr int CT = IC_WAVE_COUTS / IC_TILE_COUTS;        // output-channel tiles of a wave

struct IcParams {
  const int8_t* x;
  const int8_t* w;
  const int* bias;
  const int* divisor;
  uint8_t* y;
  int H, W, Cin, Cout, kh, kw, stride, up, out_max;
  int gh, gw;            // the pixels of one phase of one image: the output grid (down), the input grid (up)
  int OH, OW;
  unsigned pixels;       // n gh gw
};

// One axis of a phase: `cnt` taps m = 0 .. cnt - 1 with weight index t0 + tstep m and source g scale + off + dm m.
struct IcAxis {
  int cnt, t0, tstep, scale, off, dm;
};

__device__ inline IcAxis ic_axis(int k, int stride, int up, int phase) {
  IcAxis a;
  if (!up) {
    a.cnt = k; a.t0 = 0; a.tstep = 1; a.scale = stride; a.off = -(k / 2); a.dm = 1;
  } else {
    // y[q s + phase] = sum_i x[i] w[phase + (q - i) s + k / 2]: t = t0 + s m, i = q + (phase + k / 2) / s - m
    a.t0 = (phase + k / 2) % stride;
    a.cnt = a.t0 < k ? (k - a.t0 + stride - 1) / stride : 0;
    a.tstep = stride; a.scale = 1; a.off = (phase + k / 2) / stride; a.dm = -1;
  }
  return a;
}

template <bool UNSIGNED>
__global__ __launch_bounds__(IC_BLOCK_PIXELS / IC_WAVE_PIXELS * 64) void integer_conv_kernel(IcParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int phase_y = p.up ? static_cast<int>(blockIdx.z) / p.stride : 0;
  const int phase_x = p.up ? static_cast<int>(blockIdx.z) % p.stride : 0;
  const IcAxis ay = ic_axis(p.kh, p.stride, p.up, phase_y), ax = ic_axis(p.kw, p.stride, p.up, phase_x);
  const int c16s = p.Cin / IC_CHUNK_CHANNELS;
  const int chunks = ay.cnt * ax.cnt * c16s;
  const int steps = (chunks + 3) / 4;
  const int co_base = static_cast<int>(blockIdx.y) * IC_WAVE_COUTS;
  const unsigned px_base = blockIdx.x * static_cast<unsigned>(IC_BLOCK_PIXELS) + wave * IC_WAVE_PIXELS;
  if (px_base >= p.pixels) return;               // wave-uniform; nothing below synchronises the workgroup

  // this lane's pixel of every pixel tile
  bool valid[PT];
  int img_row[PT], by[PT], bx[PT], gy_[PT], gx_[PT];
#pragma unroll
  for (int t = 0; t < PT; ++t) {
    const unsigned px = px_base + t * IC_TILE_PIXELS + col;
    valid[t] = px < p.pixels;
    const unsigned q = valid[t] ? px : 0u;
    const unsigned rowi = q / static_cast<unsigned>(p.gw);
    const int gx = static_cast<int>(q - rowi * p.gw);
    const unsigned n = rowi / static_cast<unsigned>(p.gh);
    const int gy = static_cast<int>(rowi - n * p.gh);
    gy_[t] = gy; gx_[t] = gx;
    img_row[t] = static_cast<int>(n);
    by[t] = gy * ay.scale + ay.off;
    bx[t] = gx * ax.scale + ax.off;
  }

  // this lane's chunk of the reduction: (my, mx, c16), advanced by four chunks a step
  int c16 = 0, mx = 0, my = 0;
  {
    const int tap = grp / c16s;
    c16 = grp - tap * c16s;
    if (ax.cnt > 0) { my = tap / ax.cnt; mx = tap - my * ax.cnt; }
  }
  int chunk = grp;

  i32x4 acc[CT][PT];
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int t = 0; t < PT; ++t) acc[c][t] = i32x4{0, 0, 0, 0};
  int wsum[CT] = {};

  const i32x4 zero = {0, 0, 0, 0};
  auto load_step = [&](i32x4 (&a)[CT], i32x4 (&b)[PT]) {
    const bool active = chunk < chunks;
    const int ty = ay.t0 + ay.tstep * my, tx = ax.t0 + ax.tstep * mx;
    const long long wtap = static_cast<long long>(ty * p.kw + tx) * p.Cout;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int co = co_base + c * IC_TILE_COUTS + col;
      a[c] = zero;
      if (active && co < p.Cout)
        a[c] = *reinterpret_cast<const i32x4*>(p.w + (wtap + co) * p.Cin + c16 * IC_CHUNK_CHANNELS);
    }
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      const int iy = by[t] + ay.dm * my, ix = bx[t] + ax.dm * mx;
      b[t] = zero;
      if (active && valid[t] && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
        b[t] = *reinterpret_cast<const i32x4*>(
            p.x + ((static_cast<long long>(img_row[t]) * p.H + iy) * p.W + ix) * p.Cin + c16 * IC_CHUNK_CHANNELS);
      if (UNSIGNED) b[t] ^= i32x4{INT32_MIN | 0x00808080, INT32_MIN | 0x00808080, INT32_MIN | 0x00808080,
                                  INT32_MIN | 0x00808080};
    }
    // the next chunk of this lane
    chunk += 4;
    c16 += 4;
    while (c16 >= c16s) {
      c16 -= c16s;
      if (++mx >= ax.cnt) { mx = 0; ++my; }
    }
  };

  i32x4 a_cur[CT] = {}, b_cur[PT] = {}, a_next[CT] = {}, b_next[PT] = {};
  if (steps > 0) load_step(a_cur, b_cur);
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) load_step(a_next, b_next);
    if (UNSIGNED) {
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) wsum[c] = __builtin_amdgcn_sdot4(a_cur[c][j], 0x01010101, wsum[c], false);
    }
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int t = 0; t < PT; ++t)
        acc[c][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_cur[c], b_cur[t], acc[c][t], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < CT; ++c) a_cur[c] = a_next[c];
#pragma unroll
    for (int t = 0; t < PT; ++t) b_cur[t] = b_next[t];
  }

  // epilogue: this lane holds output channels co_base + 16 c + 4 grp + r of its pixel of tile t
  const bool packed = p.Cout % 4 == 0;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    int corr[4] = {0, 0, 0, 0};
    if (UNSIGNED) {
      int s = wsum[c];
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);                    // the whole sum of channel co_base + 16 c + col, in every lane group
#pragma unroll
      for (int r = 0; r < 4; ++r) corr[r] = 128 * __shfl(s, 4 * grp + r);
    }
    const int co0 = co_base + c * IC_TILE_COUTS + 4 * grp;
    int bias[4];
    unsigned div[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool in = co0 + r < p.Cout;
      bias[r] = in ? p.bias[co0 + r] : 0;
      div[r] = in ? static_cast<unsigned>(p.divisor[co0 + r]) : 1u;
    }
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      if (!valid[t] || co0 >= p.Cout) continue;
      unsigned out[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int v = acc[c][t][r] + corr[r] + bias[r];      // the exact sum first, then the bias: inside int32
        const unsigned u = (static_cast<unsigned>(v) + (div[r] >> 1)) / div[r];
        out[r] = v < 0 ? 0u : min(u, static_cast<unsigned>(p.out_max));
      }
      const int oy = p.up ? gy_[t] * p.stride + phase_y : gy_[t];
      const int ox = p.up ? gx_[t] * p.stride + phase_x : gx_[t];
      uint8_t* dst = p.y + ((static_cast<long long>(img_row[t]) * p.OH + oy) * p.OW + ox) * p.Cout + co0;
      if (packed) {
        *reinterpret_cast<unsigned*>(dst) = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (co0 + r < p.Cout) dst[r] = static_cast<uint8_t>(out[r]);
      }
    }
  }
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_integer_conv2d(const void* x, int x_unsigned, const int8_t* w, const int32_t* bias,
                                  const int32_t* divisor, uint8_t* y, int64_t n, int64_t h, int64_t wd, int64_t cin,
                                  int64_t cout, int kh, int kw, int stride, int up, int out_max, void* stream) {
  using namespace tfc;
  const char* name = "tfc_integer_conv2d";
  if (x_unsigned != 0 && x_unsigned != 1) return fail("%s: x_unsigned must be 0 (int8) or 1 (uint8), got %d", name, x_unsigned);
  if (up != 0 && up != 1) return fail("%s: up must be 0 or 1, got %d", name, up);
  if (stride != 1 && stride != 2) return fail("%s: stride must be 1 or 2, got %d", name, stride);
  if (kh < 1 || kh > IC_MAX_SUPPORT || kw < 1 || kw > IC_MAX_SUPPORT)
    return fail("%s: the kernel support must be 1 ... %d per axis, got %d x %d", name, IC_MAX_SUPPORT, kh, kw);
  if (out_max < 1 || out_max > 255) return fail("%s: out_max must be 1 ... 255, got %d", name, out_max);
  if (cin < 1 || cin % IC_CIN_MULTIPLE != 0)
    return fail("%s: cin must be a positive multiple of %d, got %lld", name, IC_CIN_MULTIPLE, static_cast<long long>(cin));
  if (static_cast<long long>(kh) * kw * cin > IC_MAX_REDUCTION)
    return fail("%s: kh * kw * cin must be at most %d, got %lld", name, IC_MAX_REDUCTION,
                static_cast<long long>(kh) * kw * cin);
  if (n < 1 || h < 1 || wd < 1 || cout < 1)
    return fail("%s: batch, height, width and cout must be at least 1, got %lld, %lld, %lld, %lld", name,
                static_cast<long long>(n), static_cast<long long>(h), static_cast<long long>(wd),
                static_cast<long long>(cout));
  if (h > (1 << 24) || wd > (1 << 24) || cout > (1 << 24))
    return fail("%s: height, width and cout must be at most 2^24", name);
  const int64_t oh = up ? h * stride : ceil_div(h, stride), ow = up ? wd * stride : ceil_div(wd, stride);
  const int64_t gh = up ? h : oh, gw = up ? wd : ow;
  if (n * h * wd > kMaxGridX || n * oh * ow > kMaxGridX)
    return fail("%s: batch * height * width must be below 2^31, input and output", name);
  if (ceil_div(cout, IC_WAVE_COUTS) > kMaxGridYZ) return fail("%s: cout is too large for one launch", name);
  if (!x || !w || !bias || !divisor || !y) return fail("%s: x, w, bias, divisor and y must not be null", name);
  if (reinterpret_cast<uintptr_t>(x) % 16 != 0 || reinterpret_cast<uintptr_t>(w) % 16 != 0)
    return fail("%s: x and w must be 16-byte aligned", name);
  if (cout % 4 == 0 && reinterpret_cast<uintptr_t>(y) % 4 != 0) return fail("%s: y must be 4-byte aligned", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  IcParams p = {};
  p.x = static_cast<const int8_t*>(x); p.w = w; p.bias = bias; p.divisor = divisor; p.y = y;
  p.H = static_cast<int>(h); p.W = static_cast<int>(wd); p.Cin = static_cast<int>(cin); p.Cout = static_cast<int>(cout);
  p.kh = kh; p.kw = kw; p.stride = stride; p.up = up; p.out_max = out_max;
  p.gh = static_cast<int>(gh); p.gw = static_cast<int>(gw); p.OH = static_cast<int>(oh); p.OW = static_cast<int>(ow);
  p.pixels = static_cast<unsigned>(n * gh * gw);
  const dim3 grid(static_cast<unsigned>(ceil_div(n * gh * gw, IC_BLOCK_PIXELS)),
                  static_cast<unsigned>(ceil_div(cout, IC_WAVE_COUTS)), up ? stride * stride : 1);
  const dim3 block(IC_BLOCK_PIXELS / IC_WAVE_PIXELS * 64);
  KernelTimer timer("integer_conv2d", st);
  if (x_unsigned) return launch(integer_conv_kernel<true>, grid, block, 0, st, p);
  return launch(integer_conv_kernel<false>, grid, block, 0, st, p);
}
