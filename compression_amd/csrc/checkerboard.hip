// The checkerboard context model of He, Zheng, Sun, Wang and Qin, "Checkerboard context model for efficient learned
// image compression" (CVPR 2021) on gfx950: for all positions of one pass, the masked 5x5 correlation over the decoded
// anchors, the pointwise entropy-parameter network and the quantisation, in ONE launch per pass
// (checkerboard_params_kernel), and the decoder's store of a decoded pass (checkerboard_place_kernel).
// include/tfc_hip.h states the definition.  The MFMA walk and the layer driver described below live in ckb_engine.h,
// which space_channel.hip shares.
//
// A workgroup of CKB_THREADS threads owns CKB_TILE = 32 consecutive compact positions of one image and runs the four
// dense layers on v_mfma_f32_32x32x2_f32: the 32 positions are the rows of the A operand, 32 output columns the
// columns of B, and a wave accumulates up to CKB_BLOCKS column blocks side by side (16 accumulator registers each)
// while it walks K.  That instruction is bit for bit D = fmaf(a[k+1], b[k+1], fmaf(a[k], b[k], C)), so every output
// element is ONE chain: its bias, then one fmaf per input row in ascending k (for the correlation: taps in row-major
// order, the channels of a tap ascending, a neighbour outside the latent contributing fmaf(0, w, acc); for the first
// layer: the 2M context features, then the P hyperprior features).  Rows and columns of an MFMA do not interact,
// so the chain depends on (M, P, H1, H2) alone: not on the batch, the tile, the slot in the tile or the neighbours
// that exist.  Encoder and decoder run this kernel.
//
// Activations stay in LDS between the layers, k-major: row k holds the 32 positions' values of feature k, so the A
// operand of k-step s is the 64 consecutive floats at row 2 s, one ds_read_b32 without a bank conflict, and an
// accumulator column goes back as four 16-byte stores.  Buffer A holds ctx, then h2; buffer B holds h1, then the
// output; a third region stages the gathered inputs (a tap's y_hat rows, psi) CKB_STAGE_K rows at a time, the next
// chunk's global loads in flight while the current one is multiplied.  [ctx, psi] are two K ranges of the first layer.
// With the model's widths A is 64 KiB and B 80 KiB: the kernel declares gfx950's whole 160 KiB of LDS, on purpose
// (one workgroup of four waves per CU, one wave per SIMD, which is what the f32 MFMA needs to reach its rate).
//
// Weights: no two waves of a workgroup use the same weight element (a wave owns its columns for all 32 positions),
// so a trip through LDS would add traffic and save none; each lane loads its B operand, one float of the packed
// buffer, straight into a register, 128 contiguous bytes per half wave, eight k-steps ahead.  The whole packed buffer
// is read once per tile of 32 positions.
//
// Nothing waits on another workgroup; every loop bound comes from the shapes.  In pass 1 the kernel reads y_hat at
// anchors only and writes it at the other positions only, so concurrent workgroups never touch the same element.
#include "ckb_engine.h"

#include "../../include/tfc_hip.h"

namespace tfc {
namespace {

struct CkbArgs {
  ContextLayout L;
  int pass, hl, wl, num_scales;
  int64_t positions;        // of this pass, per image
  int64_t tiles;            // per image
  const float* packed;
  const float* psi;         // [B, Hl, Wl, P]
  const float* y;           // [B, Hl, Wl, M] or null
  float* y_hat;             // [B, Hl, Wl, M]
  float* mu;                // [B, positions, M]
  float* index_float;
  int32_t* idx;
  int32_t* sym;
};

template <int PASS>
__global__ void __launch_bounds__(CKB_THREADS) checkerboard_params_kernel(const CkbArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[CKB_LDS_FLOATS];
  const ContextLayout& L = a.L;
  const int M = L.m;
  const int b = static_cast<int>(blockIdx.x / a.tiles);
  const int64_t slot0 = (blockIdx.x - static_cast<int64_t>(b) * a.tiles) * CKB_TILE;
  float* bufA = lds;
  float* bufB = bufA + static_cast<size_t>(L.a_floats) * CKB_TILE;
  float* stage = bufB + static_cast<size_t>(L.b_floats) * CKB_TILE;

  CkbTile t;
  t.b = b;
  t.hl = a.hl;
  t.wl = a.wl;
  t.np = static_cast<int>(min<int64_t>(CKB_TILE, a.positions - slot0));
  {
    const int sp = threadIdx.x & (CKB_TILE - 1);
    t.pi = -1;
    t.pj = 0;
    if (sp < t.np) ckb_position(slot0 + sp, PASS, a.wl, &t.pi, &t.pj);
  }

  // ctx -> A: the bias alone for the anchors, the bias and the 12 taps' chain for the rest
  if (PASS == 0) {
    const float* bc = a.packed + L.bc;
    for (int e = threadIdx.x; e < L.c2p * CKB_TILE; e += CKB_THREADS) {
      const int k = e / CKB_TILE;
      bufA[e] = k < L.c2 ? bc[k] : 0.f;
    }
  } else {
    const CkbSeg none = {};
    const CkbSeg anchors = {a.y_hat, a.packed + L.wc, M, M, L.mp, CTX_TAPS, 1, 2};
    ckb_layer_n(t, stage, nullptr, 0, a.packed, 1, anchors, none, a.packed + L.bc, L.c2, L.c2p, ckb_store_to(bufA, false));
  }
  __syncthreads();
  ckb_network(t, L, a.packed, a.psi, bufA, bufB, stage);

  // the outputs of the tile, channels innermost
  const float hi = static_cast<float>(a.num_scales - 1);
  for (int e = threadIdx.x; e < t.np * M; e += CKB_THREADS) {
    const int p = e / M, m = e - p * M;
    const float mu = bufB[static_cast<size_t>(m) * CKB_TILE + p];
    const float fi = bufB[static_cast<size_t>(M + m) * CKB_TILE + p];
    const int64_t at = (static_cast<int64_t>(b) * a.positions + slot0 + p) * M + m;
    a.mu[at] = mu;
    a.index_float[at] = fi;
    a.idx[at] = ctx_index(fi, hi);
    if (a.y) {
      int i, j;
      ckb_position(slot0 + p, PASS, a.wl, &i, &j);
      const int64_t full = ((static_cast<int64_t>(b) * a.hl + i) * a.wl + j) * M + m;
      const int32_t s = static_cast<int32_t>(rintf(a.y[full] - mu));
      a.sym[at] = s;
      a.y_hat[full] = static_cast<float>(s) + mu;
    }
  }
}

struct CkbPlace {
  int pass, hl, wl, m;
  int64_t positions, total;     // per image; batch * positions * M
  const float* sym;
  const float* mu;
  float* y_hat;
};

__global__ void __launch_bounds__(256) checkerboard_place_kernel(const CkbPlace a) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < a.total; e += stride) {
    const int64_t s = e / a.m;
    const int m = static_cast<int>(e - s * a.m);
    const int64_t b = s / a.positions;
    int i, j;
    ckb_position(s - b * a.positions, a.pass, a.wl, &i, &j);
    a.y_hat[((b * a.hl + i) * a.wl + j) * a.m + m] = a.sym[e] + a.mu[e];
  }
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_checkerboard_params(int pass, const float* y, float* y_hat, const float* psi, const float* packed,
                                       int64_t packed_floats, int64_t batch, int64_t hl, int64_t wl, int m, int p,
                                       int h1, int h2, int num_scales, float* mu, float* index_float, int32_t* idx,
                                       int32_t* sym, void* stream) {
  using namespace tfc;
  const char* name = "tfc_checkerboard_params";
  CkbArgs a = {};
  if (int rc = ctx_check_args(name, m, p, h1, h2, batch, hl, wl, true, num_scales, packed_floats, &a.L)) return rc;
  if (const char* e = ckb_check(pass, batch, hl, wl, a.L))
    return fail("%s: %s (pass %d, batch %lld, Hl %lld, Wl %lld, M %d, P %d, H1 %d, H2 %d)", name, e, pass,
                static_cast<long long>(batch), static_cast<long long>(hl), static_cast<long long>(wl), m, p, h1, h2);
  a.positions = ckb_positions(hl, wl, pass);
  if (batch == 0 || a.positions == 0) return 0;
  if (!y_hat || !psi || !packed || !mu || !index_float || !idx)
    return fail("%s: y_hat, psi, packed, mu, index_float and idx must not be null", name);
  if (y && !sym) return fail("%s: sym must not be null when y is given", name);
  a.pass = pass;
  a.hl = static_cast<int>(hl);
  a.wl = static_cast<int>(wl);
  a.num_scales = num_scales;
  a.tiles = (a.positions + CKB_TILE - 1) / CKB_TILE;
  a.packed = packed;
  a.psi = psi;
  a.y = y;
  a.y_hat = y_hat;
  a.mu = mu;
  a.index_float = index_float;
  a.idx = idx;
  a.sym = sym;
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer("checkerboard_params", st);
  const dim3 grid(static_cast<unsigned>(a.tiles * batch));
  if (pass == 0)
    hipLaunchKernelGGL(checkerboard_params_kernel<0>, grid, dim3(CKB_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL(checkerboard_params_kernel<1>, grid, dim3(CKB_THREADS), 0, st, a);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_checkerboard_place(int pass, const float* sym, const float* mu, float* y_hat, int64_t batch,
                                      int64_t hl, int64_t wl, int m, void* stream) {
  using namespace tfc;
  const char* name = "tfc_checkerboard_place";
  if (pass != 0 && pass != 1) return fail("%s: pass must be 0 or 1, got %d", name, pass);
  if (m < 1 || m > CTX_MAX_DIM) return fail("%s: M must be in [1, 65536], got %d", name, m);
  if (batch < 0) return fail("%s: the batch size must not be negative", name);
  if (hl < 1 || wl < 1 || hl > (1 << 24) || wl > (1 << 24))
    return fail("%s: Hl and Wl must be in [1, 2^24] (Hl %lld, Wl %lld)", name, static_cast<long long>(hl),
                static_cast<long long>(wl));
  if (batch > 0 && hl * wl > (1ll << 40) / batch) return fail("%s: batch * Hl * Wl must be at most 2^40", name);
  CkbPlace a = {};
  a.positions = ckb_positions(hl, wl, pass);
  a.total = batch * a.positions * m;
  if (a.total == 0) return 0;
  if (!sym || !mu || !y_hat) return fail("%s: sym, mu and y_hat must not be null", name);
  a.pass = pass;
  a.hl = static_cast<int>(hl);
  a.wl = static_cast<int>(wl);
  a.m = m;
  a.sym = sym;
  a.mu = mu;
  a.y_hat = y_hat;
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimer timer("checkerboard_place", st);
  const int64_t blocks = (a.total + 255) / 256;
  hipLaunchKernelGGL(checkerboard_place_kernel, dim3(static_cast<unsigned>(blocks < 65536 ? blocks : 65536)), dim3(256),
                     0, st, a);
  TFC_HIP(hipGetLastError());
  return 0;
}
