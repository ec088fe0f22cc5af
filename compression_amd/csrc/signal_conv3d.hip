// SignalConv1D / SignalConv3D on the bfloat16 matrix cores: tfc_conv3d_down, tfc_conv3d_up and
// tfc_conv3d_wgrad, and the host-only queries tfc_conv3d_plan / tfc_conv3d_wgrad_plan.  Activations NDHWC, kernels the
// layer's float32 DHWIO, one stride per axis; rank 1 is the case d = h = 1, kd = kh = 1.
//
// Forward: an implicit GEMM per output phase.  A phase is the set of outputs o * OS + PH0 (per axis) that one
// stride-S correlation with T taps produces:
//   down  y[i] = sum_t x[i s + t - k/2] w[t]                    one phase: S = s, T = k, J0 = -k/2, OS = 1
//   up    y[q s + phi] = sum_d x[q - d] w[d s + phi + k/2]      s phases: S = 1, T = the taps d the phase has
// so that the transposed direction spends no MFMA on inserted zeros.  A workgroup computes 128 output samples of one
// (image, depth) slice, laid out along W (TH x TW, TW = 128 / 64 / 32 by the row's length) for 32 NT output channels.
// K runs over 16-channel blocks and depth taps: each (block, depth tap) stages the input patch of the tile and the
// packed weight fragments of its H x W taps in LDS, and a tap is an LDS offset into the patch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "conv_shared.h"

namespace tfc {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 128;                     // output samples per workgroup (4 waves x 32)
constexpr size_t kHalfLds = kLdsBytesPerCu / 2;     // two workgroups per CU where the stage fits in half

struct C3Geom {
  long long N;
  int D, H, W, Cin;          // input extents; Cin as the kernel sees it (% 16 == 0)
  int OD, OH, OW;            // the phase's output grid
  int YD, YH, YW;            // the output tensor's extents
  int Cout;
  int S[3];                  // input step per output sample (d, h, w)
  int J0[3];                 // input offset of tap 0
  int T[3];                  // taps per axis (a phase may have none: bias only)
  int OS[3], PH0[3];         // output position = o * OS + PH0
  int TH, TW, lgTW;          // the tile: TH x TW output samples
  int PR, PC, PCh;           // patch rows, columns, columns per W-residue plane (ceil(PC / S[2]))
  int tiles_w, tiles_h;
  long long wofs;            // the phase's packed weights, in 16-byte pieces
  int patch_pieces;          // 16-byte pieces of the patch image in LDS
  int activation;
};

// The weights of one phase as B fragments of mfma_f32_32x32x16_bf16, in the order the kernel stages them:
// [column block][channel block][td][th][tw][nt][lane], lane l holding w[tap][cb 16 + 8 (l >> 5) + j][col (l & 31)].
// planes = 6: the kernel's channel c' = q Cin + c carries plane w_plane(q) of w[.., c, ..].
struct PackArgs {
  int kd, kh, kw, Cin, Cout;  // the layer's kernel
  int planes, cblocks, NT, nblk;
  int T[3];
  int A[3], B[3];             // kernel index of phase tap t: A + B t
};

__global__ void __launch_bounds__(256) conv3d_pack_kernel(const float* w, PackArgs p, bf16x8* out) {
  const long long pieces = static_cast<long long>(p.nblk) * p.cblocks * p.T[0] * p.T[1] * p.T[2] * p.NT * 64;
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= pieces) return;
  long long r = i;
  const int lane = static_cast<int>(r % 64); r /= 64;
  const int nt = static_cast<int>(r % p.NT); r /= p.NT;
  const int tw = static_cast<int>(r % p.T[2]); r /= p.T[2];
  const int th = static_cast<int>(r % p.T[1]); r /= p.T[1];
  const int td = static_cast<int>(r % p.T[0]); r /= p.T[0];
  const int cb = static_cast<int>(r % p.cblocks); r /= p.cblocks;
  const int blk = static_cast<int>(r);
  const int co = (blk * p.NT + nt) * 32 + (lane & 31);
  const int wd = p.A[0] + p.B[0] * td, wh = p.A[1] + p.B[1] * th, ww = p.A[2] + p.B[2] * tw;
  const long long tap = (static_cast<long long>(wd) * p.kh + wh) * p.kw + ww;
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ck = cb * 16 + 8 * (lane >> 5) + j;
    const int q = ck / p.Cin, c = ck - q * p.Cin;
    float f = co < p.Cout ? w[(tap * p.Cin + c) * p.Cout + co] : 0.f;
    if (p.planes == 6) f = split_plane(f, w_plane(q));
    v[j] = static_cast<__bf16>(f);
  }
  out[i] = v;
}

template <int NT, bool OUTF32>
__global__ void __launch_bounds__(kThreads, 2) conv3d_fwd_kernel(const __bf16* __restrict__ x, const bf16x8* __restrict__ wpk,
                                                                 const float* __restrict__ bias, void* __restrict__ y,
                                                                 C3Geom g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16x8* patch = reinterpret_cast<bf16x8*>(smem);          // [row][w residue][column / S[2]][channel half]
  bf16x8* wl = patch + g.patch_pieces;                       // [th][tw][nt][lane]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l = lane & 31;
  long long t = blockIdx.x;
  const int tw_i = static_cast<int>(t % g.tiles_w); t /= g.tiles_w;
  const int th_i = static_cast<int>(t % g.tiles_h); t /= g.tiles_h;
  const int od = static_cast<int>(t % g.OD);
  const long long n = t / g.OD;
  const int blk = blockIdx.y;
  const int oh0 = th_i * g.TH, ow0 = tw_i * g.TW;
  const int wr = (wave * 32) >> g.lgTW, wc = (wave * 32) & (g.TW - 1);     // this wave's 32 samples: row wr, columns wc ..
  const int Sw = g.S[2];
  const int taps_hw = g.T[1] * g.T[2];
  const int cblocks = g.Cin / 16;
  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x16{};
  const int pieces = g.PR * g.PC * 2;
  const long long row_px = g.W;
  for (int cb = 0; cb < cblocks && taps_hw > 0; ++cb) {
    for (int td = 0; td < g.T[0]; ++td) {
      const int id = od * g.S[0] + g.J0[0] + td;
      __syncthreads();                                       // the previous stage's reads are done
      if (id >= 0 && id < g.D) {
        const __bf16* xs = x + ((n * g.D + id) * g.H) * row_px * g.Cin + cb * 16;
        for (int i = tid; i < pieces; i += kThreads) {
          const int half = i & 1, p = i >> 1;
          const int r = p / g.PC, c = p - r * g.PC;
          const int ih = oh0 * g.S[1] + g.J0[1] + r, iw = ow0 * Sw + g.J0[2] + c;
          bf16x8 v = {};
          if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
            v = *reinterpret_cast<const bf16x8*>(xs + (ih * row_px + iw) * g.Cin + half * 8);
          const int cq = c / Sw;
          patch[((r * Sw + (c - cq * Sw)) * g.PCh + cq) * 2 + half] = v;
        }
      } else {
        for (int i = tid; i < pieces; i += kThreads) {
          const int half = i & 1, p = i >> 1;
          const int r = p / g.PC, c = p - r * g.PC, cq = c / Sw;
          patch[((r * Sw + (c - cq * Sw)) * g.PCh + cq) * 2 + half] = bf16x8{};
        }
      }
      const int wpieces = taps_hw * NT * 64;
      const bf16x8* src = wpk + g.wofs + ((static_cast<long long>(blk) * cblocks + cb) * g.T[0] + td) * wpieces;
      for (int i = tid; i < wpieces; i += kThreads) wl[i] = src[i];
      __syncthreads();
      for (int th = 0; th < g.T[1]; ++th) {
        const int rbase = (wr * g.S[1] + th) * Sw;
        for (int tw = 0; tw < g.T[2]; ++tw) {
          const int twq = tw / Sw;
          const bf16x8 a = patch[((rbase + (tw - twq * Sw)) * g.PCh + wc + l + twq) * 2 + h];
          const bf16x8* b = wl + (th * g.T[2] + tw) * NT * 64 + lane;
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[j * 64], acc[j], 0, 0, 0);
        }
      }
    }
  }
  // epilogue: lane (l, h) holds column l of rows (r & 3) + 8 (r >> 2) + 4 h of each 32 x 32 tile
  const int oh = oh0 + wr;
  if (oh >= g.OH) return;
  const long long ybase = ((n * g.YD + static_cast<long long>(od) * g.OS[0] + g.PH0[0]) * g.YH +
                           static_cast<long long>(oh) * g.OS[1] + g.PH0[1]) * g.YW;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int co = (blk * NT + j) * 32 + l;
    if (co >= g.Cout) continue;
    const float bv = bias ? bias[co] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ow = ow0 + wc + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (ow >= g.OW) continue;
      float v = acc[j][r] + bv;
      if (g.activation == 1) v = fmaxf(v, 0.f);
      const long long at = (ybase + static_cast<long long>(ow) * g.OS[2] + g.PH0[2]) * g.Cout + co;
      if (OUTF32) static_cast<float*>(y)[at] = v;
      else static_cast<__bf16*>(y)[at] = static_cast<__bf16>(v);
    }
  }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------
// G[t][ca][cb] = sum_{n,q} A[n, q o s + t - k/2, ca] B[n, q, cb]: per tap a GEMM whose K is B's pixels.  A workgroup
// computes a 64 x 64 (ca, cb) block of one tap over one chunk of B's pixels, 64 pixels per LDS stage with both operands
// stored transposed ([channel][pixel]); the partials [chunk][tap][ca][cb] are summed in chunk order by a second kernel:
// no float atomics, the same bits on every call.  bfloat16 on mfma_f32_32x32x16_bf16, float32 on the float32-input
// mfma_f32_32x32x2f32 (fmaf numerics).
struct WGeom {
  long long N, P;            // images; B pixels = N DB HB WB
  int DA, HA, WA, CA, DB, HB, WB, CB;
  int k[3], s[3];
  int cbt;                   // cb tiles
  long long chunk_px;        // B pixels per chunk (a multiple of 64)
};

// 8 consecutive channels (16- / 32-byte aligned: channel counts are multiples of 16)
__device__ inline void load8(const __bf16* p, __bf16* v) {
  const bf16x8 r = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = r[e];
}
__device__ inline void load8(const float* p, float* v) {
  const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[e + 4] = hi[e]; }
}

template <typename T> struct WPad;
template <> struct WPad<__bf16> { static constexpr int kRow = 64 + 8; };
template <> struct WPad<float> { static constexpr int kRow = 64 + 4; };

template <typename T>
__global__ void __launch_bounds__(256) conv3d_wgrad_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                           float* __restrict__ part, WGeom g) {
  constexpr int R = WPad<T>::kRow;
  __shared__ __attribute__((aligned(16))) T la[64 * R];      // [ca][pixel]
  __shared__ __attribute__((aligned(16))) T lb[64 * R];      // [cb][pixel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l = lane & 31;
  const int tap = blockIdx.x;
  const int tw = tap % g.k[2], th = (tap / g.k[2]) % g.k[1], td = tap / (g.k[2] * g.k[1]);
  const int ca0 = (blockIdx.y / g.cbt) * 64, cb0 = (blockIdx.y % g.cbt) * 64;
  const long long p0 = static_cast<long long>(blockIdx.z) * g.chunk_px;
  const long long p1 = std::min(g.P, p0 + g.chunk_px);
  const int wa = (wave >> 1) * 32, wb = (wave & 1) * 32;       // this wave's 32 x 32 block
  f32x16 acc = {};
  for (long long q0 = p0; q0 < p1; q0 += 64) {
    __syncthreads();
    // stage: item i = (channel group of 8, pixel); consecutive threads take consecutive pixels
    for (int i = tid; i < 2 * 64 * 8; i += 256) {
      const int which = i >> 9, cg = (i >> 6) & 7, px = i & 63;
      const long long q = q0 + px;
      T v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = static_cast<T>(0.f);
      if (q < p1) {
        long long r = q;
        const int qw = static_cast<int>(r % g.WB); r /= g.WB;
        const int qh = static_cast<int>(r % g.HB); r /= g.HB;
        const int qd = static_cast<int>(r % g.DB);
        const long long n = r / g.DB;
        if (which == 0) {
          const int c = ca0 + cg * 8;
          const int id = qd * g.s[0] + td - g.k[0] / 2, ih = qh * g.s[1] + th - g.k[1] / 2, iw = qw * g.s[2] + tw - g.k[2] / 2;
          if (c < g.CA && id >= 0 && id < g.DA && ih >= 0 && ih < g.HA && iw >= 0 && iw < g.WA)
            load8(a + (((n * g.DA + id) * g.HA + ih) * g.WA + iw) * g.CA + c, v);
        } else {
          const int c = cb0 + cg * 8;
          if (c < g.CB) load8(b + q * g.CB + c, v);
        }
      }
      T* dst = (which == 0 ? la : lb) + cg * 8 * R + px;
#pragma unroll
      for (int e = 0; e < 8; ++e) dst[e * R] = v[e];
    }
    __syncthreads();
    if constexpr (std::is_same<T, __bf16>::value) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 fa = *reinterpret_cast<const bf16x8*>(la + (wa + l) * R + ks * 16 + 8 * h);
        const bf16x8 fb = *reinterpret_cast<const bf16x8*>(lb + (wb + l) * R + ks * 16 + 8 * h);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < 32; ++ks)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(la[(wa + l) * R + 2 * ks + h], lb[(wb + l) * R + 2 * ks + h], acc, 0, 0, 0);
    }
  }
  float* out = part + ((static_cast<long long>(blockIdx.z) * gridDim.x + tap) * g.CA) * g.CB;
  const int cb = cb0 + wb + l;
  if (cb >= g.CB) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int ca = ca0 + wa + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (ca < g.CA) out[static_cast<long long>(ca) * g.CB + cb] = acc[r];
  }
}

// dw[t][ca][cb] (or [t][cb][ca]) = sum over chunks, in chunk order
__global__ void __launch_bounds__(256) conv3d_wgrad_sum_kernel(const float* part, long long per_chunk, int chunks, int CA,
                                                               int CB, int transpose, float* dw) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= per_chunk) return;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += part[c * per_chunk + i];
  if (!transpose) {
    dw[i] = s;
    return;
  }
  const long long plane = static_cast<long long>(CA) * CB;
  const long long t = i / plane, r = i - t * plane;
  const int ca = static_cast<int>(r / CB), cb = static_cast<int>(r - static_cast<long long>(ca) * CB);
  dw[t * plane + static_cast<long long>(cb) * CA + ca] = s;
}

// ---- host --------------------------------------------------------------------------------------------------------
// NT (32-column tiles per workgroup) for Cout: the fewest padded columns, then the widest tile
int pick_nt(int64_t cout) {
  int best = 1;
  long long best_cols = -1;
  for (int nt = 1; nt <= 4; ++nt) {
    const long long cols = ceil_div(cout, 32 * nt) * 32 * nt;
    if (best_cols < 0 || cols <= best_cols) { best = nt; best_cols = cols; }
  }
  return best;
}

struct Phase {
  int S[3], J0[3], T[3], OS[3], PH0[3], OD[3];
  int A[3], B[3];
};

// What the host chooses for one forward call: the phases, the tile, the column blocks and the LDS stage.  conv3d_bf16
// launches from it and tfc_conv3d_plan reports it, so the two cannot drift.
struct FwdPlan {
  std::vector<Phase> phases;
  int64_t yd[3];             // the output tensor's extents
  int TW, TH, NT, nblk, tiles_w, tiles_h;
  size_t patch_pieces, lds;
};

int conv3d_plan(const char* name, int up, const int64_t in[3], int64_t cout, const int k[3], const int s[3], FwdPlan* plan) {
  // phases
  int nph = 1;
  for (int a = 0; a < 3; ++a) nph *= up ? s[a] : 1;
  int64_t* yd = plan->yd;
  for (int a = 0; a < 3; ++a) yd[a] = up ? in[a] * s[a] : ceil_div(in[a], s[a]);
  for (int a = 0; a < 3; ++a)
    if (yd[a] >= (1ll << 31) || in[a] >= (1ll << 31)) return fail("%s: extent too large (%lld)", name, static_cast<long long>(yd[a]));
  std::vector<Phase>& phases = plan->phases;
  phases.assign(nph, Phase{});
  for (int p = 0; p < nph; ++p) {
    Phase& f = phases[p];
    int rest = p;
    for (int a = 2; a >= 0; --a) {
      const int su = up ? s[a] : 1;
      const int phi = rest % su;
      rest /= su;
      if (!up) {
        f.S[a] = s[a]; f.J0[a] = -(k[a] / 2); f.T[a] = k[a]; f.OS[a] = 1; f.PH0[a] = 0;
        f.OD[a] = static_cast<int>(yd[a]); f.A[a] = 0; f.B[a] = 1;
      } else {
        auto fdiv = [](int v, int d) { return v >= 0 ? v / d : -((-v + d - 1) / d); };
        const int dmin = -fdiv(phi + k[a] / 2, s[a]);                  // ceil((-phi - k/2) / s)
        const int dmax = fdiv(k[a] - 1 - phi - k[a] / 2, s[a]);
        f.S[a] = 1; f.J0[a] = -dmax; f.T[a] = std::max(0, dmax - dmin + 1); f.OS[a] = s[a]; f.PH0[a] = phi;
        f.OD[a] = static_cast<int>(in[a]); f.A[a] = dmax * s[a] + phi + k[a] / 2; f.B[a] = -s[a];
      }
    }
  }
  // tile and column blocks
  const int ow = phases[0].OD[2];
  int TW = ow > 64 ? 128 : ow > 32 ? 64 : 32;
  int NT = pick_nt(cout);
  // LDS: the largest patch of any phase, then the largest weight stage
  auto lds_of = [&](int tw, int nt, size_t* patch_pieces) {
    size_t pp = 0, wp = 0;
    for (const Phase& f : phases) {
      const int th = kTile / tw;
      const int pr = (th - 1) * f.S[1] + f.T[1], pc = (tw - 1) * f.S[2] + f.T[2];
      const int pch = (pc + f.S[2] - 1) / f.S[2];
      pp = std::max(pp, static_cast<size_t>(pr) * f.S[2] * pch * 2);
      wp = std::max(wp, static_cast<size_t>(f.T[1]) * f.T[2] * nt * 64);
    }
    if (patch_pieces) *patch_pieces = pp;
    return (pp + wp) * 16;
  };
  // two workgroups per CU where possible: narrower column blocks first, then narrower tiles
  while (NT > 1 && lds_of(TW, NT, nullptr) > kHalfLds) --NT;
  while (TW > 32 && lds_of(TW, NT, nullptr) > kHalfLds) TW /= 2;
  plan->lds = lds_of(TW, NT, &plan->patch_pieces);
  if (plan->lds > kLdsBytesPerCu) return fail("%s: kernel support too large for one workgroup's LDS (%zu bytes)", name, plan->lds);
  plan->nblk = static_cast<int>(ceil_div(cout, 32 * NT));
  if (plan->nblk > kMaxGridYZ) return fail("%s: too many output channels for one launch", name);
  plan->TW = TW; plan->TH = kTile / TW; plan->NT = NT;
  plan->tiles_w = static_cast<int>(ceil_div(phases[0].OD[2], TW));          // every phase has the same output grid
  plan->tiles_h = static_cast<int>(ceil_div(phases[0].OD[1], plan->TH));
  return 0;
}

int conv3d_bf16(const char* name, const __bf16* x, const float* w, int planes, const float* bias, void* y, bool out_f32,
                int64_t n, const int64_t in[3], int64_t cin_k, int64_t cin_w, int64_t cout, const int k[3], const int s[3],
                int activation, int up, hipStream_t st) {
  FwdPlan plan;
  if (int rc = conv3d_plan(name, up, in, cout, k, s, &plan)) return rc;
  const std::vector<Phase>& phases = plan.phases;
  const int nph = static_cast<int>(phases.size());
  const int64_t* yd = plan.yd;
  const int TW = plan.TW, NT = plan.NT, nblk = plan.nblk;
  const size_t patch_pieces = plan.patch_pieces, lds = plan.lds;
  const int cblocks = static_cast<int>(cin_k / 16);
  // packed weights of every phase
  std::vector<long long> wofs(nph);
  long long wtotal = 0;
  for (int p = 0; p < nph; ++p) {
    wofs[p] = wtotal;
    wtotal += static_cast<long long>(nblk) * cblocks * phases[p].T[0] * phases[p].T[1] * phases[p].T[2] * NT * 64;
  }
  DevBuf wpk;
  if (wtotal > 0) {
    TFC_HIP(wpk.alloc(static_cast<size_t>(wtotal) * 16, st));
    for (int p = 0; p < nph; ++p) {
      const Phase& f = phases[p];
      PackArgs pa{};
      pa.kd = k[0]; pa.kh = k[1]; pa.kw = k[2]; pa.Cin = static_cast<int>(cin_w); pa.Cout = static_cast<int>(cout);
      pa.planes = planes; pa.cblocks = cblocks; pa.NT = NT; pa.nblk = nblk;
      for (int a = 0; a < 3; ++a) { pa.T[a] = f.T[a]; pa.A[a] = f.A[a]; pa.B[a] = f.B[a]; }
      const long long pieces = (p + 1 < nph ? wofs[p + 1] : wtotal) - wofs[p];
      if (pieces == 0) continue;
      if (ceil_div(pieces, 256) > kMaxGridX) return fail("%s: kernel too large for one launch", name);
      hipLaunchKernelGGL(conv3d_pack_kernel, dim3(static_cast<unsigned>(ceil_div(pieces, 256))), dim3(256), 0, st, w, pa,
                         wpk.as<bf16x8>() + wofs[p]);
    }
    TFC_HIP(hipGetLastError());
  }
  KernelTimer timer("conv3d", st);
  for (int p = 0; p < nph; ++p) {
    const Phase& f = phases[p];
    C3Geom g{};
    g.N = n; g.D = static_cast<int>(in[0]); g.H = static_cast<int>(in[1]); g.W = static_cast<int>(in[2]);
    g.Cin = static_cast<int>(cin_k);
    g.OD = f.OD[0]; g.OH = f.OD[1]; g.OW = f.OD[2];
    g.YD = static_cast<int>(yd[0]); g.YH = static_cast<int>(yd[1]); g.YW = static_cast<int>(yd[2]);
    g.Cout = static_cast<int>(cout);
    for (int a = 0; a < 3; ++a) { g.S[a] = f.S[a]; g.J0[a] = f.J0[a]; g.T[a] = f.T[a]; g.OS[a] = f.OS[a]; g.PH0[a] = f.PH0[a]; }
    g.TW = TW; g.TH = plan.TH; g.lgTW = TW == 128 ? 7 : TW == 64 ? 6 : 5;
    g.PR = (g.TH - 1) * f.S[1] + f.T[1];
    g.PC = (TW - 1) * f.S[2] + f.T[2];
    g.PCh = (g.PC + f.S[2] - 1) / f.S[2];
    g.tiles_w = plan.tiles_w;
    g.tiles_h = plan.tiles_h;
    g.wofs = wofs[p];
    g.patch_pieces = static_cast<int>(patch_pieces);
    g.activation = activation;
    const long long blocks = n * g.OD * g.tiles_h * static_cast<long long>(g.tiles_w);
    if (blocks > kMaxGridX) return fail("%s: problem too large for one launch (%lld tiles)", name, blocks);
    if (blocks == 0) continue;
#define TFC_C3_KERNEL(NTV) (out_f32 ? conv3d_fwd_kernel<NTV, true> : conv3d_fwd_kernel<NTV, false>)
    auto* kern = NT == 1 ? TFC_C3_KERNEL(1) : NT == 2 ? TFC_C3_KERNEL(2) : NT == 3 ? TFC_C3_KERNEL(3) : TFC_C3_KERNEL(4);
#undef TFC_C3_KERNEL
    if (int rc = launch(kern, dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(nblk)), dim3(kThreads), lds, st, x,
                        wpk.as<bf16x8>(), bias, y, g))
      return rc;
  }
  return 0;
}

// the scalar arguments of a forward call, as conv3d_entry and tfc_conv3d_plan both demand them
int conv3d_check(const char* name, int64_t n, const int64_t in[3], int64_t cin, int64_t cout, const int k[3], const int s[3]) {
  if (k[0] < 1 || k[1] < 1 || k[2] < 1) return fail("%s: kernel support must be >= 1 (got %d, %d, %d)", name, k[0], k[1], k[2]);
  if (s[0] < 1 || s[1] < 1 || s[2] < 1) return fail("%s: strides must be >= 1 (got %d, %d, %d)", name, s[0], s[1], s[2]);
  if (n < 0 || in[0] < 0 || in[1] < 0 || in[2] < 0) return fail("%s: negative extent", name);
  if (cin < 1 || cout < 1) return fail("%s: channel counts must be >= 1", name);
  if (cin % 16) return fail("%s: input channels must be a multiple of 16 (got %lld)", name, static_cast<long long>(cin));
  if (cin >= (1 << 24) || cout >= (1 << 24)) return fail("%s: too many channels", name);
  return 0;
}
int conv3d_check_extents(const char* name, const int64_t in[3], const int s[3]) {
  for (int a = 0; a < 3; ++a)
    if (in[a] >= (1ll << 31) / std::max(1, s[a])) return fail("%s: extent too large", name);
  return 0;
}

int conv3d_entry(const char* name, const void* x, const void* w, const float* bias, void* y, int dtype, int64_t n,
                 int64_t d, int64_t h, int64_t wd, int64_t cin, int64_t cout, int kd, int kh, int kw, int sd, int sh,
                 int sw, int activation, int up, void* stream) {
  if (int rc = check_dtype(name, dtype)) return rc;
  const int64_t in[3] = {d, h, wd};
  const int k[3] = {kd, kh, kw}, s[3] = {sd, sh, sw};
  if (int rc = conv3d_check(name, n, in, cin, cout, k, s)) return rc;
  if (activation != 0 && activation != 1) return fail("%s: activation must be 0 (none) or 1 (relu)", name);
  if (n == 0 || d == 0 || h == 0 || wd == 0) return 0;
  if (!x || !w || !y) return fail("%s: x, w and y must not be null", name);
  if (int rc = conv3d_check_extents(name, in, s)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == 1)
    return conv3d_bf16(name, static_cast<const __bf16*>(x), static_cast<const float*>(w), 1, bias, y, false, n, in, cin,
                       cin, cout, k, s, activation, up, st);
  // float32: six bfloat16 planes (split3) through the same kernel, float32 out, a chunk of images at a time
  long long out_image = cout;
  for (int a = 0; a < 3; ++a) out_image *= up ? in[a] * s[a] : ceil_div(in[a], s[a]);
  return conv_f32_chunks(name, "conv3d", static_cast<const float*>(x), n, d * h * wd, cin, st,
                         [&](int64_t n0, int64_t images, const __bf16* xs) {
    return conv3d_bf16(name, xs, static_cast<const float*>(w), 6, bias, static_cast<float*>(y) + n0 * out_image, true,
                       images, in, 6 * cin, cin, cout, k, s, activation, up, st);
  });
}

// the scalar arguments of a weight gradient call, as tfc_conv3d_wgrad and tfc_conv3d_wgrad_plan both demand them
int conv3d_wgrad_check(const char* name, int64_t n, std::initializer_list<int64_t> extents, int64_t ca, int64_t cb, int kd,
                       int kh, int kw) {
  if (kd < 1 || kh < 1 || kw < 1) return fail("%s: kernel support must be >= 1 (got %d, %d, %d)", name, kd, kh, kw);
  if (n < 0) return fail("%s: negative extent", name);
  for (int64_t e : extents)
    if (e < 0) return fail("%s: negative extent", name);
  if (ca < 16 || cb < 16 || ca % 16 || cb % 16)
    return fail("%s: channel counts must be multiples of 16 (got %lld, %lld)", name, static_cast<long long>(ca),
                static_cast<long long>(cb));
  if (static_cast<long long>(kd) * kh * kw >= (1ll << 20)) return fail("%s: kernel support too large", name);
  if (ca >= (1 << 24) || cb >= (1 << 24)) return fail("%s: too many channels", name);
  for (int64_t e : extents)
    if (e >= (1ll << 31)) return fail("%s: extent too large", name);
  return 0;
}

// What the host chooses for one weight gradient call over P > 0 pixels of B: the 64 x 64 channel tiles and the chunks of
// pixels.  tfc_conv3d_wgrad launches from it and tfc_conv3d_wgrad_plan reports it.
struct WgradPlan {
  long long tiles_ca, tiles_cb, chunks, chunk_steps;      // chunk_steps: LDS stages of 64 pixels per chunk
};

int conv3d_wgrad_plan(const char* name, long long P, long long taps, int64_t ca, int64_t cb, WgradPlan* plan) {
  plan->tiles_ca = ceil_div(ca, 64);
  plan->tiles_cb = ceil_div(cb, 64);
  const long long tiles = plan->tiles_ca * plan->tiles_cb;
  if (tiles > kMaxGridYZ || taps > kMaxGridX) return fail("%s: problem too large for one launch", name);
  // chunks of B's pixels: about 4096 workgroups in all, and at most 256 MB of partials
  const long long per_chunk = taps * ca * cb;
  const long long steps = ceil_div(P, 64);
  long long chunks = std::min<long long>(steps, std::max<long long>(1, ceil_div(4096, taps * tiles)));
  chunks = std::max<long long>(1, std::min<long long>(chunks, static_cast<long long>((size_t{256} << 20) / (static_cast<size_t>(per_chunk) * 4))));
  chunks = std::min<long long>(chunks, kMaxGridYZ);
  plan->chunk_steps = ceil_div(steps, chunks);
  plan->chunks = ceil_div(steps, plan->chunk_steps);
  return 0;
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_conv3d_down(const void* x, const void* w, const float* bias, void* y, int dtype, int64_t n, int64_t d,
                               int64_t h, int64_t wd, int64_t cin, int64_t cout, int kd, int kh, int kw, int sd, int sh,
                               int sw, int activation, void* stream) {
  return tfc::conv3d_entry("tfc_conv3d_down", x, w, bias, y, dtype, n, d, h, wd, cin, cout, kd, kh, kw, sd, sh, sw,
                           activation, 0, stream);
}

extern "C" int tfc_conv3d_up(const void* x, const void* w, const float* bias, void* y, int dtype, int64_t n, int64_t d,
                             int64_t h, int64_t wd, int64_t cin, int64_t cout, int kd, int kh, int kw, int sd, int sh,
                             int sw, int activation, void* stream) {
  return tfc::conv3d_entry("tfc_conv3d_up", x, w, bias, y, dtype, n, d, h, wd, cin, cout, kd, kh, kw, sd, sh, sw,
                           activation, 1, stream);
}

extern "C" int tfc_conv3d_wgrad(const void* a, const void* b, float* dw, int dtype, int64_t n, int64_t da, int64_t ha,
                                int64_t wa, int64_t ca, int64_t db, int64_t hb, int64_t wb, int64_t cb, int kd, int kh,
                                int kw, int sd, int sh, int sw, int transpose, void* stream) {
  using namespace tfc;
  const char* name = "tfc_conv3d_wgrad";
  if (int rc = check_dtype(name, dtype)) return rc;
  if (sd < 1 || sh < 1 || sw < 1) return fail("%s: strides must be >= 1 (got %d, %d, %d)", name, sd, sh, sw);
  if (transpose != 0 && transpose != 1) return fail("%s: transpose must be 0 or 1", name);
  if (int rc = conv3d_wgrad_check(name, n, {da, ha, wa, db, hb, wb}, ca, cb, kd, kh, kw)) return rc;
  const long long taps = static_cast<long long>(kd) * kh * kw;
  if (!dw) return fail("%s: dw must not be null", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long per_chunk = taps * ca * cb;
  const long long P = n * db * hb * wb;
  if (P == 0) {
    TFC_HIP(hipMemsetAsync(dw, 0, static_cast<size_t>(per_chunk) * sizeof(float), st));
    return 0;
  }
  if (!a || !b) return fail("%s: a and b must not be null", name);
  WGeom g{};
  g.N = n; g.P = P;
  g.DA = static_cast<int>(da); g.HA = static_cast<int>(ha); g.WA = static_cast<int>(wa); g.CA = static_cast<int>(ca);
  g.DB = static_cast<int>(db); g.HB = static_cast<int>(hb); g.WB = static_cast<int>(wb); g.CB = static_cast<int>(cb);
  g.k[0] = kd; g.k[1] = kh; g.k[2] = kw; g.s[0] = sd; g.s[1] = sh; g.s[2] = sw;
  WgradPlan plan;
  if (int rc = conv3d_wgrad_plan(name, P, taps, ca, cb, &plan)) return rc;
  g.cbt = static_cast<int>(plan.tiles_cb);
  const long long tiles = plan.tiles_ca * plan.tiles_cb, chunks = plan.chunks;
  g.chunk_px = plan.chunk_steps * 64;
  DevBuf part;
  TFC_HIP(part.alloc(static_cast<size_t>(chunks * per_chunk) * sizeof(float), st));
  KernelTimer timer("conv3d", st);
  const dim3 grid(static_cast<unsigned>(taps), static_cast<unsigned>(tiles), static_cast<unsigned>(chunks));
  if (dtype == 1)
    hipLaunchKernelGGL(conv3d_wgrad_kernel<__bf16>, grid, dim3(256), 0, st, static_cast<const __bf16*>(a),
                       static_cast<const __bf16*>(b), part.as<float>(), g);
  else
    hipLaunchKernelGGL(conv3d_wgrad_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(a),
                       static_cast<const float*>(b), part.as<float>(), g);
  TFC_HIP(hipGetLastError());
  if (ceil_div(per_chunk, 256) > kMaxGridX) return fail("%s: problem too large for one launch", name);
  hipLaunchKernelGGL(conv3d_wgrad_sum_kernel, dim3(static_cast<unsigned>(ceil_div(per_chunk, 256))), dim3(256), 0, st,
                     part.as<float>(), per_chunk, static_cast<int>(chunks), static_cast<int>(ca), static_cast<int>(cb),
                     transpose, dw);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_conv3d_plan(int up, int64_t d, int64_t h, int64_t wd, int64_t cin_k, int64_t cout, int kd, int kh,
                               int kw, int sd, int sh, int sw, int32_t* out) {
  using namespace tfc;
  const char* name = "tfc_conv3d_plan";
  const int64_t in[3] = {d, h, wd};
  const int k[3] = {kd, kh, kw}, s[3] = {sd, sh, sw};
  if (up != 0 && up != 1) return fail("%s: up must be 0 or 1", name);
  if (int rc = conv3d_check(name, 1, in, cin_k, cout, k, s)) return rc;
  if (d == 0 || h == 0 || wd == 0) return fail("%s: an empty input launches nothing", name);
  if (int rc = conv3d_check_extents(name, in, s)) return rc;
  if (!out) return fail("%s: out must not be null", name);
  FwdPlan plan;
  if (int rc = conv3d_plan(name, up, in, cout, k, s, &plan)) return rc;
  const int32_t v[8] = {plan.TW, plan.TH, plan.NT, plan.nblk, plan.tiles_w, plan.tiles_h,
                        static_cast<int32_t>(plan.phases.size()), static_cast<int32_t>(plan.lds)};
  std::copy(v, v + 8, out);
  return 0;
}

extern "C" int tfc_conv3d_wgrad_plan(int64_t n, int64_t db, int64_t hb, int64_t wb, int64_t ca, int64_t cb, int kd, int kh,
                                     int kw, int32_t* out) {
  using namespace tfc;
  const char* name = "tfc_conv3d_wgrad_plan";
  if (int rc = conv3d_wgrad_check(name, n, {db, hb, wb}, ca, cb, kd, kh, kw)) return rc;
  const long long P = n * db * hb * wb;
  if (P == 0) return fail("%s: an empty cotangent launches nothing", name);
  if (!out) return fail("%s: out must not be null", name);
  WgradPlan plan;
  if (int rc = conv3d_wgrad_plan(name, P, static_cast<long long>(kd) * kh * kw, ca, cb, &plan)) return rc;
  const int32_t v[5] = {static_cast<int32_t>(plan.tiles_ca), static_cast<int32_t>(plan.tiles_cb),
                        static_cast<int32_t>(plan.chunks), static_cast<int32_t>(plan.chunk_steps),
                        static_cast<int32_t>(P - (plan.chunks - 1) * plan.chunk_steps * 64)};
  std::copy(v, v + 5, out);
  return 0;
}
