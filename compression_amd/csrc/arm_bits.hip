// The autoregressive-MLP entropy model of the overfitted codecs (the ARM of Cool-chic / C3) as one fused rate kernel.
//
//   context h0[k] = y[i + ARM_DI[k], j + ARM_DJ[k]], k < C (zero outside the grid)
//   h <- relu(h W_l + b_l) + h,  l < L;   (mu, s) = h W_out + b_out;   scale = exp(clamp(s, ARM_S_MIN, ARM_S_MAX))
//   p = Laplace(mu, scale) mass of [y - 1/2, y + 1/2];   bits = -log2(max(p, 2^-16)), summed per grid
//
// Forward.  A workgroup owns ARM_ROWS x ARM_COLS pixels, one per thread (a wave is a row of 64 columns).  The tile and
// its halo (4 rows above, 4 columns to either side) are staged in LDS, the parameters once per workgroup beside them;
// a thread gathers its context from the tile, keeps the activations in registers and reads every weight as a 16-byte
// LDS broadcast (all lanes of a wave ask for the same address).  Every output is ONE fmaf chain in ascending k with
// the bias added last, so a pixel's result depends on nothing but its inputs.  The tile's bits are added in a fixed
// butterfly; a one-workgroup-per-grid kernel adds the tiles' partials in a fixed order, so a grid's sum depends on
// neither B nor the launch.  No [N, C] tensor exists.
//
// Backward.  The same tile pass recomputes the forward (inputs of layers 1.. stay in registers, the ReLU signs in one
// bit mask per layer; layer 0's input is gathered again) and runs the chain backwards per pixel.
//  * Parameter gradients are sums over pixels, that is over lanes: per layer the tile's layer inputs H [256, C] and
//    deltas D [256, C] are staged in LDS and thread (k, o..o+3) adds H[p, k] D[p, o..o+3] over the pixels p in
//    ascending order.  Where C*C/4 < 256 the spare threads split the pixels (p = g mod G) and are merged in ascending g
//    at the end.  A workgroup walks tiles blockIdx.x, + gridDim.x, ... and keeps its sums in registers across them; it
//    writes ONE partial, and a merge kernel adds the at most ARM_GROUPS partials in ascending order.  No atomics.
//  * dy is a gather: the pass writes d context as C planes [B, C, H, W] (lanes along W: coalesced) and d centre as plane
//    C; a second kernel adds, per pixel, the centre and the C planes read at the pixels that use it, in ascending k.
#include "arm_params.h"
#include "common.h"
#include "launch.h"

#include <cmath>

namespace tfc {
namespace {

constexpr int kArmTile = (ARM_ROWS + ARM_HALO) * ARM_TILE_W;      // floats of the staged tile

// parameters in LDS, in floats: W [L, C, C] | b [L, C] | W_out [C, 2] | b_out [2], padded to 16 bytes
__host__ __device__ constexpr int arm_param_count(int C, int L) { return L * C * C + L * C + 2 * C + 2; }
__host__ __device__ constexpr int arm_param_lds(int C, int L) { return (arm_param_count(C, L) + 3) & ~3; }

struct ArmArgs {
  const float* y;          // [B, H, W]
  const float* w;          // [L, C, C]
  const float* b;          // [L, C]
  const float* w_out;      // [C, 2]
  const float* b_out;      // [2]
  int B, H, W, L;
  int tiles_x, tiles;      // tiles of a row of tiles, of a grid
  float* partial;          // forward: [B, tiles] bits of a tile
  float* mu;               // forward: [B, H, W] or null
  float* scale;
  const float* g;          // backward: [B] d loss / d bits
  float* planes;           // backward: [B, C + 1, H, W] or null
  float* ppart;            // backward: [gridDim.x, arm_param_count] or null
};

template <int C>
__device__ __forceinline__ void arm_load_params(float* sp, const ArmArgs& a) {
  const int nw = a.L * C * C, nb = a.L * C;
  for (int i = threadIdx.x; i < nw; i += ARM_THREADS) sp[i] = a.w[i];
  for (int i = threadIdx.x; i < nb; i += ARM_THREADS) sp[nw + i] = a.b[i];
  if (threadIdx.x < 2 * C) sp[nw + nb + threadIdx.x] = a.w_out[threadIdx.x];
  if (threadIdx.x < 2) sp[nw + nb + 2 * C + threadIdx.x] = a.b_out[threadIdx.x];
}

// rows row0 - 4 .. row0 + 3, columns col0 - 4 .. col0 + 67 of one grid; zero outside it
__device__ __forceinline__ void arm_load_tile(float* st, const float* yb, int H, int W, int row0, int col0) {
  for (int e = threadIdx.x; e < kArmTile; e += ARM_THREADS) {
    const int tr = e / ARM_TILE_W, tc = e - tr * ARM_TILE_W;
    const int gi = row0 - ARM_HALO + tr, gj = col0 - ARM_HALO + tc;
    st[e] = (gi >= 0 && gi < H && gj >= 0 && gj < W) ? yb[static_cast<long long>(gi) * W + gj] : 0.f;
  }
}

// px: the thread's pixel in the staged tile, &st[r * ARM_TILE_W + c]; every offset below is a constant >= 0
template <int C>
__device__ __forceinline__ void arm_gather(const float* px, float (&h)[C]) {
#pragma unroll
  for (int k = 0; k < C; ++k) h[k] = px[(ARM_HALO + ARM_DI[k]) * ARM_TILE_W + ARM_HALO + ARM_DJ[k]];
}

// pre[o] = (sum_k h[k] W[k, o]) + b[o]: per output one fmaf chain in ascending k.  The bias comes last: a chain that
// started at it would round every step at the bias's magnitude, not at the (smaller) partial sum's.
template <int C>
__device__ __forceinline__ void arm_layer(const float* wl, const float* bl, const float (&h)[C], float (&pre)[C]) {
#pragma unroll
  for (int o = 0; o < C; o += 4) {
    const float4 bias = *reinterpret_cast<const float4*>(bl + o);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const float4 wv = *reinterpret_cast<const float4*>(wl + k * C + o);
      acc.x = fmaf(h[k], wv.x, acc.x);
      acc.y = fmaf(h[k], wv.y, acc.y);
      acc.z = fmaf(h[k], wv.z, acc.z);
      acc.w = fmaf(h[k], wv.w, acc.w);
    }
    pre[o] = acc.x + bias.x; pre[o + 1] = acc.y + bias.y; pre[o + 2] = acc.z + bias.z; pre[o + 3] = acc.w + bias.w;
  }
}

template <int C>
__device__ __forceinline__ void arm_head(const float* wo, const float* bo, const float (&h)[C], float* mu, float* s) {
  float m = 0.f, t = 0.f;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const float2 wv = *reinterpret_cast<const float2*>(wo + 2 * k);
    m = fmaf(h[k], wv.x, m);
    t = fmaf(h[k], wv.y, t);
  }
  *mu = m + bo[0];
  *s = t + bo[1];
}

// The rate of one pixel and its derivatives.  With x = y - mu, a = |x|, r = 1 / scale, the mass of [y - .5, y + .5] as
// differences of survival values S(t) = exp(-t r) / 2 taken where both ends lie on one side of mu (the idiom of
// laplace_tail.h, for any scale):
//   a >= .5 :  p = S(a - .5) - S(a + .5) = exp(-(a - .5) r) (1 - exp(-r)) / 2
//   a <  .5 :  p = (1 - 2 S(.5 - a)) / 2 + (1 - 2 S(.5 + a)) / 2 = -(expm1(-(.5 - a) r) + expm1(-(.5 + a) r)) / 2
struct ArmRate {
  float bits, scale;
  float d_mu, d_s;         // d bits / d mu (d bits / d y at the centre is its negative), d bits / d s
};

__device__ __forceinline__ ArmRate arm_rate(float yv, float mu, float s) {
  constexpr float kFloor = 1.f / static_cast<float>(1 << ARM_FLOOR_LOG2);
  constexpr float kInvLn2 = 1.44269504088896341f;
  const float sc = fminf(fmaxf(s, ARM_S_MIN), ARM_S_MAX);
  const float r = expf(-sc);
  const float x = yv - mu, a = fabsf(x);
  float p, ga, gs;         // p; d bits / da and d bits / ds where p is above the floor
  if (a >= 0.5f) {
    // ln p = -u + ln(1 - q) - ln 2 with q = exp(-r): the derivatives of the LOG, with no p to divide by and without the
    // difference u exp(-u) - v exp(-v), which loses a digit where the two are close
    const float u = (a - 0.5f) * r, q = expf(-r), omq = -expm1f(-r);
    p = 0.5f * expf(-u) * omq;
    ga = kInvLn2 * r;
    gs = -kInvLn2 * (u - q * r / omq);
  } else {
    const float u = (0.5f - a) * r, v = (0.5f + a) * r;
    const float eu = expf(-u), ev = expf(-v);
    p = -0.5f * (expm1f(-u) + expm1f(-v));
    const float dbits = -kInvLn2 / p;
    ga = dbits * (0.5f * r * (ev - eu));
    gs = dbits * (-0.5f * (u * eu + v * ev));
  }
  ArmRate out;
  out.bits = -log2f(fmaxf(p, kFloor));
  out.scale = expf(sc);
  const bool live = p >= kFloor;                                  // zero under the floor
  const float dx = !live ? 0.f : (x > 0.f ? ga : (x < 0.f ? -ga : 0.f));
  out.d_mu = -dx;
  out.d_s = (live && s >= ARM_S_MIN && s <= ARM_S_MAX) ? gs : 0.f;   // zero outside the clamp
  return out;
}

// ------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------

template <int C>
__global__ void __launch_bounds__(ARM_THREADS) arm_bits_forward_kernel(ArmArgs a) {
  extern __shared__ float4 arm_lds[];
  float* sp = reinterpret_cast<float*>(arm_lds);
  float* st = sp + arm_param_lds(C, a.L);
  float* red = st + kArmTile;
  const int tile = blockIdx.x, bidx = blockIdx.z;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int row0 = ty * ARM_ROWS, col0 = tx * ARM_COLS;
  const long long plane = static_cast<long long>(a.H) * a.W;
  arm_load_params<C>(sp, a);
  arm_load_tile(st, a.y + bidx * plane, a.H, a.W, row0, col0);
  __syncthreads();

  const int r = threadIdx.x / ARM_COLS, c = threadIdx.x % ARM_COLS;
  const int gi = row0 + r, gj = col0 + c;
  const bool valid = gi < a.H && gj < a.W;
  const float* px = st + r * ARM_TILE_W + c;
  float h[C];
  arm_gather<C>(px, h);
  const float* sb = sp + a.L * C * C;
#pragma unroll 1
  for (int l = 0; l < a.L; ++l) {
    float pre[C];
    arm_layer<C>(sp + l * C * C, sb + l * C, h, pre);
#pragma unroll
    for (int o = 0; o < C; ++o) h[o] = fmaxf(pre[o], 0.f) + h[o];
  }
  float mu, s;
  arm_head<C>(sb + a.L * C, sb + a.L * C + 2 * C, h, &mu, &s);
  const ArmRate rate = arm_rate(px[ARM_HALO * ARM_TILE_W + ARM_HALO], mu, s);
  if (valid && a.mu) {
    a.mu[bidx * plane + static_cast<long long>(gi) * a.W + gj] = mu;
    a.scale[bidx * plane + static_cast<long long>(gi) * a.W + gj] = rate.scale;
  }
  float bits = valid ? rate.bits : 0.f;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) bits += __shfl_xor(bits, m, 64);
  if (c == 0) red[r] = bits;
  __syncthreads();
  if (threadIdx.x == 0)
    a.partial[static_cast<long long>(bidx) * a.tiles + tile] = (red[0] + red[1]) + (red[2] + red[3]);
}

// bits[b] = the sum of partial[b, :]: strided sums per thread, then a fixed tree, in float64 (a handful of adds a
// thread: the one rounding to float32 is the last)
__global__ void __launch_bounds__(ARM_SUM_THREADS) arm_bits_sum_kernel(const float* partial, int tiles, float* bits) {
  __shared__ double red[ARM_SUM_THREADS];
  const float* src = partial + static_cast<long long>(blockIdx.x) * tiles;
  double s = 0.0;
  for (int t = threadIdx.x; t < tiles; t += ARM_SUM_THREADS) s += src[t];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int m = ARM_SUM_THREADS / 2; m >= 1; m >>= 1) {
    if (threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x == 0) bits[blockIdx.x] = static_cast<float>(red[0]);
}

// ------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------

// sum += v with the rounding error carried in comp (Kahan): the bias gradients are plain sums of up to thousands of
// like-signed terms per thread, which a bare float32 chain would round at the running sum's size every step
__device__ __forceinline__ void arm_add(float& sum, float& comp, float v) {
  const float t = v - comp;
  const float u = sum + t;
  comp = (u - sum) - t;
  sum = u;
}

// Adds, in ascending g and in float64, the `groups` copies that the threads left in red [groups, n]; writes dst [n].
__device__ __forceinline__ void arm_merge_groups(const float* red, int groups, int n, float* dst) {
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += ARM_THREADS) {
    double s = red[i];
    for (int g = 1; g < groups; ++g) s += red[g * n + i];
    dst[i] = static_cast<float>(s);
  }
  __syncthreads();
}

template <int C, int L>
__global__ void __launch_bounds__(ARM_THREADS) arm_bits_backward_kernel(ArmArgs a) {
  constexpr int S = C + 4;                       // row stride of the staged H and D: 16-byte rows
  constexpr int E = C * C / 4, G = ARM_THREADS / E;          // hidden layers: entries (k, o..o+3), pixel groups
  constexpr int E2 = 2 * C, G2 = ARM_THREADS / E2;           // output layer: entries (k, j)
  constexpr int P = arm_param_count(C, L);
  extern __shared__ float4 arm_lds[];
  float* sp = reinterpret_cast<float*>(arm_lds);
  float* st = sp + arm_param_lds(C, L);
  float* Hs = st + kArmTile;                     // [256, S]
  float* Ds = Hs + ARM_THREADS * S;              // [256, S]
  const float* sb = sp + L * C * C;
  const float* so = sb + L * C;

  const int tid = threadIdx.x;
  const int e = tid % E, g = tid / E, kh = e / (C / 4), o4 = (e % (C / 4)) * 4;
  const bool hid_active = g < G;
  const int e2 = tid % E2, g2 = tid / E2, ko = e2 >> 1, jo = e2 & 1;
  const bool out_active = g2 < G2;
  float aw[L][4], ab[L][4], cb[L][4], ao = 0.f, abo = 0.f, cbo = 0.f;
#pragma unroll
  for (int l = 0; l < L; ++l)
#pragma unroll
    for (int j = 0; j < 4; ++j) aw[l][j] = ab[l][j] = cb[l][j] = 0.f;

  const int r = tid / ARM_COLS, c = tid % ARM_COLS;
  const float* px = st + r * ARM_TILE_W + c;
  float* hrow = Hs + tid * S;
  float* drow = Ds + tid * S;
  const long long plane = static_cast<long long>(a.H) * a.W;
  const long long items = static_cast<long long>(a.B) * a.tiles;
  arm_load_params<C>(sp, a);

  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int bidx = static_cast<int>(item / a.tiles), tile = static_cast<int>(item - bidx * static_cast<long long>(a.tiles));
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int row0 = ty * ARM_ROWS, col0 = tx * ARM_COLS;
    __syncthreads();                             // the last pass's readers of the tile and of H, D are done
    arm_load_tile(st, a.y + bidx * plane, a.H, a.W, row0, col0);
    __syncthreads();
    const int gi = row0 + r, gj = col0 + c;
    const bool valid = gi < a.H && gj < a.W;

    // the forward again: hs[l - 1] is the input of layer l >= 1, mask[l] the signs of layer l
    float h[C], hs[L > 1 ? L - 1 : 1][C];
    unsigned mask[L];
    arm_gather<C>(px, h);
#pragma unroll
    for (int l = 0; l < L; ++l) {
      if (l >= 1) {
#pragma unroll
        for (int k = 0; k < C; ++k) hs[l - 1][k] = h[k];
      }
      float pre[C];
      arm_layer<C>(sp + l * C * C, sb + l * C, h, pre);
      unsigned m = 0;
#pragma unroll
      for (int o = 0; o < C; ++o) {
        m |= pre[o] > 0.f ? 1u << o : 0u;
        h[o] = fmaxf(pre[o], 0.f) + h[o];
      }
      mask[l] = m;
    }
    float mu, s;
    arm_head<C>(so, so + 2 * C, h, &mu, &s);
    const ArmRate rate = arm_rate(px[ARM_HALO * ARM_TILE_W + ARM_HALO], mu, s);
    const float up = valid ? a.g[bidx] : 0.f;    // a pixel outside the grid adds exact zeros everywhere
    const float d_mu = up * rate.d_mu, d_s = up * rate.d_s;

    // the output layer: dW_out[k, j] += h_L[k] d[j], db_out[j] += d[j]
#pragma unroll
    for (int k = 0; k < C; k += 4) *reinterpret_cast<float4*>(hrow + k) = make_float4(h[k], h[k + 1], h[k + 2], h[k + 3]);
    drow[0] = d_mu;
    drow[1] = d_s;
    __syncthreads();
    if (out_active) {
      for (int p = g2; p < ARM_THREADS; p += G2) {
        const float d = Ds[p * S + jo];
        ao = fmaf(Hs[p * S + ko], d, ao);
        if (ko == 0) arm_add(abo, cbo, d);
      }
    }
    float dh[C];
#pragma unroll
    for (int k = 0; k < C; ++k) dh[k] = fmaf(so[2 * k + 1], d_s, so[2 * k] * d_mu);

#pragma unroll
    for (int l = L - 1; l >= 0; --l) {
      float delta[C];
#pragma unroll
      for (int o = 0; o < C; ++o) delta[o] = (mask[l] >> o) & 1u ? dh[o] : 0.f;
      if (l == 0) arm_gather<C>(px, h);
      const float (&hin)[C] = l == 0 ? h : hs[l > 0 ? l - 1 : 0];
      __syncthreads();                           // the readers of the layer above are done
#pragma unroll
      for (int k = 0; k < C; k += 4) {
        *reinterpret_cast<float4*>(hrow + k) = make_float4(hin[k], hin[k + 1], hin[k + 2], hin[k + 3]);
        *reinterpret_cast<float4*>(drow + k) = make_float4(delta[k], delta[k + 1], delta[k + 2], delta[k + 3]);
      }
      __syncthreads();
      if (hid_active) {
        for (int p = g; p < ARM_THREADS; p += G) {
          const float hv = Hs[p * S + kh];
          const float4 d = *reinterpret_cast<const float4*>(Ds + p * S + o4);
          aw[l][0] = fmaf(hv, d.x, aw[l][0]);
          aw[l][1] = fmaf(hv, d.y, aw[l][1]);
          aw[l][2] = fmaf(hv, d.z, aw[l][2]);
          aw[l][3] = fmaf(hv, d.w, aw[l][3]);
          if (kh == 0) {
            arm_add(ab[l][0], cb[l][0], d.x);
            arm_add(ab[l][1], cb[l][1], d.y);
            arm_add(ab[l][2], cb[l][2], d.z);
            arm_add(ab[l][3], cb[l][3], d.w);
          }
        }
      }
      // d input[k] = (sum_o W[k, o] delta[o]) + dh[k], the residual last
      const float* wl = sp + l * C * C;
#pragma unroll
      for (int k = 0; k < C; ++k) {
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < C; o += 4) {
          const float4 wv = *reinterpret_cast<const float4*>(wl + k * C + o);
          acc = fmaf(delta[o], wv.x, acc);
          acc = fmaf(delta[o + 1], wv.y, acc);
          acc = fmaf(delta[o + 2], wv.z, acc);
          acc = fmaf(delta[o + 3], wv.w, acc);
        }
        dh[k] += acc;                            // delta was taken from the old dh above
      }
    }

    if (valid && a.planes) {
      float* pl = a.planes + bidx * (C + 1) * plane + static_cast<long long>(gi) * a.W + gj;
#pragma unroll
      for (int k = 0; k < C; ++k) pl[k * plane] = dh[k];
      pl[C * plane] = -d_mu;
    }
  }

  if (!a.ppart) return;
  float* out = a.ppart + static_cast<long long>(blockIdx.x) * P;
  float* red = Hs;                               // at most 1024 floats of the 256 * S
#pragma unroll
  for (int l = 0; l < L; ++l) {
    __syncthreads();
    if (hid_active)
      *reinterpret_cast<float4*>(red + g * (C * C) + kh * C + o4) = make_float4(aw[l][0], aw[l][1], aw[l][2], aw[l][3]);
    arm_merge_groups(red, G, C * C, out + l * C * C);
    if (hid_active && kh == 0)
      *reinterpret_cast<float4*>(red + g * C + o4) = make_float4(ab[l][0], ab[l][1], ab[l][2], ab[l][3]);
    arm_merge_groups(red, G, C, out + L * C * C + l * C);
  }
  if (out_active) red[g2 * E2 + e2] = ao;
  arm_merge_groups(red, G2, E2, out + L * C * C + L * C);
  if (out_active && ko == 0) red[g2 * 2 + jo] = abo;
  arm_merge_groups(red, G2, 2, out + L * C * C + L * C + E2);
}

// dy[b, i, j] = d centre (added last) + sum_k d context k of the pixel (i - DI[k], j - DJ[k]) that reads (i, j) as its context k
template <int C>
__global__ void __launch_bounds__(ARM_SUM_THREADS) arm_bits_gather_kernel(const float* planes, int H, int W,
                                                                         long long total, float* dy) {
  const long long plane = static_cast<long long>(H) * W;
  for (long long idx = static_cast<long long>(blockIdx.x) * ARM_SUM_THREADS + threadIdx.x; idx < total;
       idx += static_cast<long long>(gridDim.x) * ARM_SUM_THREADS) {
    const long long bidx = idx / plane;
    const int rem = static_cast<int>(idx - bidx * plane);
    const int i = rem / W, j = rem - i * W;
    const float* pl = planes + bidx * (C + 1) * plane;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const int ii = i - ARM_DI[k], jj = j - ARM_DJ[k];
      if (ii < H && jj >= 0 && jj < W) s += pl[k * plane + static_cast<long long>(ii) * W + jj];
    }
    dy[idx] = s + pl[C * plane + rem];
  }
}

// out[i] = sum over rows of partial[row, i] in ascending row order, in float64; four running sums so that the loads
// overlap
__global__ void __launch_bounds__(ARM_SUM_THREADS) arm_bits_merge_kernel(const float* partial, int rows, int n,
                                                                        float* out) {
  const int i = blockIdx.x * ARM_SUM_THREADS + threadIdx.x;
  if (i >= n) return;
  const float* src = partial + i;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int r = 0;
  for (; r + 4 <= rows; r += 4) {
    a0 += src[static_cast<long long>(r) * n];
    a1 += src[static_cast<long long>(r + 1) * n];
    a2 += src[static_cast<long long>(r + 2) * n];
    a3 += src[static_cast<long long>(r + 3) * n];
  }
  for (; r < rows; ++r) a0 += src[static_cast<long long>(r) * n];
  out[i] = static_cast<float>((a0 + a1) + (a2 + a3));
}

int arm_validate(const char* name, int64_t B, int64_t H, int64_t W, int C, int L) {
  if (C != 8 && C != 16 && C != 24 && C != 32) return fail("%s: the context size must be 8, 16, 24 or 32, got %d", name, C);
  if (L < 1 || L > ARM_MAX_L) return fail("%s: hidden layers must be in [1, %d], got %d", name, ARM_MAX_L, L);
  if (B < 1 || B > ARM_MAX_B) return fail("%s: B must be in [1, %d], got %lld", name, ARM_MAX_B, static_cast<long long>(B));
  if (H < 1 || W < 1 || H > (1ll << 31) - 1 || W > (1ll << 31) - 1 || H * W > (1ll << 31) - 1)
    return fail("%s: H and W must be at least 1 with H * W below 2^31, got %lld x %lld", name,
                static_cast<long long>(H), static_cast<long long>(W));
  if (ceil_div(H, ARM_ROWS) * ceil_div(W, ARM_COLS) > kMaxGridX)
    return fail("%s: a %lld x %lld grid has more tiles than one launch takes", name, static_cast<long long>(H),
                static_cast<long long>(W));
  return 0;
}

void arm_fill(ArmArgs* a, const float* y, const float* w, const float* b, const float* w_out, const float* b_out,
              int64_t B, int64_t H, int64_t W, int L) {
  a->y = y; a->w = w; a->b = b; a->w_out = w_out; a->b_out = b_out;
  a->B = static_cast<int>(B); a->H = static_cast<int>(H); a->W = static_cast<int>(W); a->L = L;
  a->tiles_x = static_cast<int>(ceil_div(W, ARM_COLS));
  a->tiles = static_cast<int>(ceil_div(H, ARM_ROWS) * a->tiles_x);
}

template <int C>
int arm_launch_backward(int L, dim3 grid, size_t lds, hipStream_t st, const ArmArgs& a) {
  switch (L) {
    case 1: return launch(arm_bits_backward_kernel<C, 1>, grid, dim3(ARM_THREADS), lds, st, a);
    case 2: return launch(arm_bits_backward_kernel<C, 2>, grid, dim3(ARM_THREADS), lds, st, a);
    default: return launch(arm_bits_backward_kernel<C, 3>, grid, dim3(ARM_THREADS), lds, st, a);
  }
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_arm_bits_forward(const float* y, const float* w, const float* b, const float* w_out,
                                    const float* b_out, int64_t batch, int64_t height, int64_t width, int context,
                                    int layers, float* bits, float* mu, float* scale, void* stream) {
  using namespace tfc;
  if (int rc = arm_validate("tfc_arm_bits_forward", batch, height, width, context, layers)) return rc;
  if (!y || !w || !b || !w_out || !b_out || !bits)
    return fail("tfc_arm_bits_forward: y, the parameters and bits must not be null");
  if ((mu == nullptr) != (scale == nullptr)) return fail("tfc_arm_bits_forward: mu and scale come together or not at all");
  hipStream_t st = static_cast<hipStream_t>(stream);
  ArmArgs a = {};
  arm_fill(&a, y, w, b, w_out, b_out, batch, height, width, layers);
  a.mu = mu; a.scale = scale;
  DevBuf part;
  TFC_HIP(part.alloc(sizeof(float) * static_cast<size_t>(batch) * a.tiles, st));
  a.partial = part.as<float>();
  const size_t lds = sizeof(float) * (arm_param_lds(context, layers) + kArmTile + ARM_ROWS);
  const dim3 grid(static_cast<unsigned>(a.tiles), 1, static_cast<unsigned>(batch));
  KernelTimer timer("arm_bits_forward", st);
  int rc = 0;
  switch (context) {
    case 8: rc = launch(arm_bits_forward_kernel<8>, grid, dim3(ARM_THREADS), lds, st, a); break;
    case 16: rc = launch(arm_bits_forward_kernel<16>, grid, dim3(ARM_THREADS), lds, st, a); break;
    case 24: rc = launch(arm_bits_forward_kernel<24>, grid, dim3(ARM_THREADS), lds, st, a); break;
    default: rc = launch(arm_bits_forward_kernel<32>, grid, dim3(ARM_THREADS), lds, st, a); break;
  }
  if (rc) return rc;
  return launch(arm_bits_sum_kernel, dim3(static_cast<unsigned>(batch)), dim3(ARM_SUM_THREADS), 0, st, a.partial,
                a.tiles, bits);
}

extern "C" int tfc_arm_bits_backward(const float* y, const float* w, const float* b, const float* w_out,
                                     const float* b_out, const float* g_bits, int64_t batch, int64_t height,
                                     int64_t width, int context, int layers, float* d_y, float* d_params,
                                     void* stream) {
  using namespace tfc;
  if (int rc = arm_validate("tfc_arm_bits_backward", batch, height, width, context, layers)) return rc;
  if (!d_y && !d_params) return 0;
  if (!y || !w || !b || !w_out || !b_out || !g_bits)
    return fail("tfc_arm_bits_backward: y, the parameters and g_bits must not be null");
  hipStream_t st = static_cast<hipStream_t>(stream);
  ArmArgs a = {};
  arm_fill(&a, y, w, b, w_out, b_out, batch, height, width, layers);
  a.g = g_bits;
  const long long pixels = static_cast<long long>(batch) * height * width;
  const long long items = static_cast<long long>(batch) * a.tiles;
  const int groups = static_cast<int>(std::min<long long>(items, ARM_GROUPS));
  const int count = arm_param_count(context, layers);
  DevBuf planes, ppart;
  if (d_y) {
    TFC_HIP(planes.alloc(sizeof(float) * static_cast<size_t>(pixels) * (context + 1), st));
    a.planes = planes.as<float>();
  }
  if (d_params) {
    TFC_HIP(ppart.alloc(sizeof(float) * static_cast<size_t>(groups) * count, st));
    a.ppart = ppart.as<float>();
  }
  const size_t lds = sizeof(float) * (arm_param_lds(context, layers) + kArmTile + 2 * ARM_THREADS * (context + 4));
  const dim3 grid(static_cast<unsigned>(groups));
  KernelTimer timer("arm_bits_backward", st);
  int rc = 0;
  switch (context) {
    case 8: rc = arm_launch_backward<8>(layers, grid, lds, st, a); break;
    case 16: rc = arm_launch_backward<16>(layers, grid, lds, st, a); break;
    case 24: rc = arm_launch_backward<24>(layers, grid, lds, st, a); break;
    default: rc = arm_launch_backward<32>(layers, grid, lds, st, a); break;
  }
  if (rc) return rc;
  if (d_y) {
    const unsigned blocks = static_cast<unsigned>(std::min<long long>(ceil_div(pixels, ARM_SUM_THREADS), 1 << 20));
    const int H = static_cast<int>(height), W = static_cast<int>(width);
    switch (context) {
      case 8: rc = launch(arm_bits_gather_kernel<8>, dim3(blocks), dim3(ARM_SUM_THREADS), 0, st, a.planes, H, W, pixels, d_y); break;
      case 16: rc = launch(arm_bits_gather_kernel<16>, dim3(blocks), dim3(ARM_SUM_THREADS), 0, st, a.planes, H, W, pixels, d_y); break;
      case 24: rc = launch(arm_bits_gather_kernel<24>, dim3(blocks), dim3(ARM_SUM_THREADS), 0, st, a.planes, H, W, pixels, d_y); break;
      default: rc = launch(arm_bits_gather_kernel<32>, dim3(blocks), dim3(ARM_SUM_THREADS), 0, st, a.planes, H, W, pixels, d_y); break;
    }
    if (rc) return rc;
  }
  if (d_params)
    rc = launch(arm_bits_merge_kernel, dim3(static_cast<unsigned>(ceil_div(count, ARM_SUM_THREADS))),
                dim3(ARM_SUM_THREADS), 0, st, a.ppart, groups, count, d_params);
  return rc;
}
