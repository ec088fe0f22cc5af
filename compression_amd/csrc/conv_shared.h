// What the convolution units share.  First the device helpers and the float32 path's split and chunk loop, which
// signal_conv3d.hip and signal_conv_backward.hip use too; then the 2-D forward layer's call, its routes, the implicit
// GEMM's geometry and the cache of packed weights, for signal_conv.hip and conv_gemm3.hip.  State and the shared kernels
// live in ONE unit: the cache, the thread's next key, conv_pack_kernel and conv_split_x_kernel in signal_conv.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <type_traits>

#include "../../include/tfc_hip.h"
#include "bf16_io.h"
#include "launch.h"
#include "gdn_params.h"

namespace tfc {

// n / d for 0 <= n < 2^31 as a multiplication: mul = ceil(2^(31 + s) / d), s = ceil(log2 d), n / d = (n * mul) >> (31 + s)
// exactly (mul * d - 2^(31 + s) < d <= 2^s: the error term is below 1 / d); mul = 0: d = 1.
inline void fast_div_setup(unsigned int d, unsigned int* mul, unsigned int* sh) {
  if (d <= 1) { *mul = 0; *sh = 0; return; }
  unsigned int s = 0;
  while ((1ull << s) < d) ++s;
  *mul = static_cast<unsigned int>(((1ull << (31 + s)) + d - 1) / d);
  *sh = s - 1;
}
__device__ inline unsigned int fast_div(unsigned int n, unsigned int mul, unsigned int sh) {
  return mul ? __umulhi(n, mul) >> sh : n;
}

// float32 on the bfloat16 matrix cores (signal_conv.hip, route_f32_planes): a = a1 + a2 + a3 with a_i bfloat16, and
// a b = a1 b1 + a1 b2 + a2 b1 + a1 b3 + a2 b2 + a3 b1 to float32 rounding noise: one bfloat16 convolution over six times
// the input channels, x planes [x1 | x1 | x1 | x2 | x2 | x3] against w planes [w1 | w2 | w3 | w1 | w2 | w1], float32 out.
__device__ inline void split3(float a, __bf16* p1, __bf16* p2, __bf16* p3) {
  const __bf16 a1 = static_cast<__bf16>(a);
  const float r1 = a - static_cast<float>(a1);
  const __bf16 a2 = static_cast<__bf16>(r1);
  const float r2 = r1 - static_cast<float>(a2);
  *p1 = a1; *p2 = a2; *p3 = static_cast<__bf16>(r2);
}
__device__ inline int x_plane(int q) { return q < 3 ? 0 : q < 5 ? 1 : 2; }
__device__ inline int w_plane(int q) { return q == 0 || q == 3 || q == 5 ? 0 : q == 1 || q == 4 ? 1 : 2; }
__device__ inline float split_plane(float a, int plane) {
  __bf16 p[3];
  split3(a, &p[0], &p[1], &p[2]);
  return static_cast<float>(plane == 0 ? p[0] : plane == 1 ? p[1] : p[2]);
}

// bytes of input planes per chunk of images, for the rank-2 and the rank-3 float32 path (TFC_CONV_F32_CHUNK_BYTES: the
// tests run several chunks at a small shape; read per call)
inline size_t conv_f32_chunk_bytes() {
  const char* e = env_str("TFC_CONV_F32_CHUNK_BYTES");
  const long long v = e ? std::atoll(e) : 0;
  return v > 0 ? static_cast<size_t>(v) : size_t{2} << 30;
}

// conv_split_x_kernel (signal_conv.hip): x float32 [pixels, C] -> xs, its six bfloat16 planes [pixels, 6 C]; C % 8 == 0
void launch_conv_split_x(const float* x, long long pixels, int C, __bf16* xs, hipStream_t st);

// The float32 path's walk over a batch x [n, pix_image, cin], for every rank.  The planes are 3x the input's bytes, so the
// images go through in chunks of ~2 GB of planes (bmshj2018's first 192 -> 192 layer at 128 x 768x512 would need 29 GB at
// once): each chunk is split under the timer `label`, then body(n0, images, planes) convolves images n0 .. n0 + images.
template <typename Body>
int conv_f32_chunks(const char* name, const char* label, const float* x, int64_t n, long long pix_image, int64_t cin,
                    hipStream_t st, Body&& body) {
  const size_t plane_bytes = static_cast<size_t>(pix_image) * 6 * cin * sizeof(__bf16);
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, static_cast<int64_t>(conv_f32_chunk_bytes() / std::max<size_t>(plane_bytes, 1))));
  if (ceil_div(pix_image * chunk * (cin / 8), 256) > kMaxGridX) return fail("%s: problem too large for one launch", name);
  DevBuf xs;
  TFC_HIP(xs.alloc(plane_bytes * static_cast<size_t>(chunk), st));
  for (int64_t n0 = 0; n0 < n; n0 += chunk) {
    const int64_t images = std::min<int64_t>(chunk, n - n0);
    {
      KernelTimer timer(label, st);
      launch_conv_split_x(x + n0 * pix_image * cin, pix_image * images, static_cast<int>(cin), xs.as<__bf16>(), st);
      TFC_HIP(hipGetLastError());
    }
    if (int rc = body(n0, images, xs.as<__bf16>())) return rc;
  }
  return 0;
}

// One 2-D forward call, as the C ABI entries state it and as a route states a nested one.
struct ConvCall {
  const void* x;
  const float *w, *bias;             // HWIO; [cout] or null
  void* y;
  int dtype;                         // 0 float32, 1 bfloat16
  int64_t n, h, wd, cin, cout;
  int kh, kw, stride, activation, up;
  bool out_f32;                      // bfloat16 in, the float32 accumulators out (nested calls only)
  const tfc_gdn_params* gdn;         // GDN / IGDN as the activation where a route fuses it; it says so through *gdn_fused
  int gdn_inverse, *gdn_fused;
  hipStream_t stream;
  unsigned long long weights_key;    // names this value of the weights (tfc_conv2d_weights_key); 0: pack per call
};
int conv_entry(const ConvCall& call);

// The routes, in the order conv_entry tries them.  0 = launched, -1 = not this shape, > 0 = error; each holds its whole
// eligibility test.
int route_f32_planes(const ConvCall& k);
int route_up_phase(const ConvCall& k);
int route_up_fused(const ConvCall& k);
int route_up_gather(const ConvCall& k);
int route_image_direct(const ConvCall& k);
int route_image(const ConvCall& k);
int route_gemm(const ConvCall& k);             // third generation (conv_gemm3.hip), second, first

// Transposed convolution, y[q*s + phi] = sum_d x[q - d] w[phi + d*s + k/2]: d in [dmin, dmax] over all phases
struct UpTaps { int dmax, dmin; };
inline UpTaps up_taps(int k, int s) {
  auto fdiv = [](int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
  return {fdiv(k - 1 - k / 2, s), -fdiv((s - 1) + k / 2, s)};
}

// A float32 layer's six-plane weights are cached under its caller's key ^ this (route_f32_planes; dropped with it)
constexpr unsigned long long kPlanesKey = 0x5bf1600000000000ull;

constexpr int kMaxGroups = 16;         // column groups that can carry their own tap sub-rectangle

struct ConvGeom {
  // input
  long long N;
  int H, W, Cin;          // Cin as seen by the kernel (4 for packed image input)
  int Hp, Wp;             // packed image input: padded extents (else H, W)
  // low-resolution output grid the GEMM rows run over
  int OHq, OWq;
  int sd;                 // input step per output row/col
  int Uy, Ux;             // taps of the equivalent correlation
  int py0, px0;           // zero padding before
  // columns
  int Cout, su;           // real output channels, depth-to-space factor
  int cols;               // su*su*Cout
  int groups;             // column groups of `tiles` 32-wide tiles
  int tiles;
  // K
  int ksteps;             // K steps of 16
  int kchunk;             // K steps staged in LDS at a time
  int small_cin;          // 1: packed-image mode (K runs along kernel rows)
  int kw4;                // small_cin: K steps per kernel row
  int activation;         // 0 none, 1 relu
  int out_f32;            // bf16 kernels: write the fp32 accumulators (the tap products of route_up_gather)
  // output
  int OH, OW;
  // Compact K (second-generation bf16 kernel, transposed convolution whose column groups are whole output
  // phases): a phase only has the taps t = phi + d*s + k/2 inside the kernel, e.g. 3x3, 3x2, 2x3, 2x2 of the
  // 3x3 taps of a 5x5 stride-2 kernel, so a group's K loop (and its packed weights) runs over the
  // sub-rectangle [ty0, ty1) x [tx0, tx1) of taps only: 25 instead of 36 tap blocks in that example.
  int compact;
  int ty0[kMaxGroups], ty1[kMaxGroups], tx0[kMaxGroups], tx1[kMaxGroups];
  // Third-generation kernel: K runs channel block by channel block, a group's taps inside each
  // (K step = cbi * taps + tap); with `compact` tap rectangles for every group.
  int cbmajor;
  // GDN / IGDN as the layer's activation (third-generation kernel: a workgroup holds all channels of its pixels):
  // 0 none, 1 y / (beta + gamma^T |y|), 2 y * (beta + gamma^T |y|); the prepared bfloat16 image of tfc_gdn_params
  int gdn;
  const void* gdn_image;
  int xcd;                  // 1: the third-generation kernel's workgroups take their blocks in XCD order (xcd_order)
  int nt_out;               // third generation: the output's whole-line stores non-temporal (an output beyond the caches)
  // first / second generation: pixel -> (image, row, column) with the divisions as multiplications where the launch has
  // fewer than 2^31 low-resolution pixels (pix32; fast_div by OWq, OHq)
  unsigned int owq_mul, owq_sh, ohq_mul, ohq_sh;
  int pix32;
};

struct PackGeom {
  int kh, kw, Cin_real, Cout, su, up;
  int Uy, Ux, dmax_y, dmax_x;
};


// Transposed layer: the sub-rectangle of taps that output phase `phase` has (those with a kernel index in range), as
// column group grp's -> its tap count, 0: the phase has none.
inline int phase_taps(ConvGeom& c, const PackGeom& g, int grp, int phase) {
  const int phy = phase / g.su, phx = phase % g.su;
  int y0 = c.Uy, y1 = 0, x0 = c.Ux, x1 = 0;
  for (int u = 0; u < c.Uy; ++u) {
    const int t = phy + (g.dmax_y - u) * g.su + g.kh / 2;
    if (t >= 0 && t < g.kh) { y0 = std::min(y0, u); y1 = std::max(y1, u + 1); }
  }
  for (int u = 0; u < c.Ux; ++u) {
    const int t = phx + (g.dmax_x - u) * g.su + g.kw / 2;
    if (t >= 0 && t < g.kw) { x0 = std::min(x0, u); x1 = std::max(x1, u + 1); }
  }
  c.ty0[grp] = y0; c.ty1[grp] = y1; c.tx0[grp] = x0; c.tx1[grp] = x1;
  return y1 > y0 && x1 > x0 ? (y1 - y0) * (x1 - x0) : 0;
}

// conv_pack_kernel<__bf16 / float> over `frags` fragments into dst (signal_conv.hip; every generation's packing)
void launch_conv_pack(bool bf16, const float* w, const PackGeom& g, const ConvGeom& c, long long frags, void* dst,
                      hipStream_t st);
// third-generation kernel (conv_gemm3.hip)
int run_conv3(const __bf16* x, const float* w, const float* bias, __bf16* y, ConvGeom c, PackGeom g,
              unsigned long long key, hipStream_t st);

// ---------------------------------------------------------------------------
// Packed weights of an inference layer, kept between calls.  Every kernel here reads the layer's float32 HWIO kernel as
// fragments in its own order, packed by a small kernel in front of it — 60-90 us each, four to nine a model step (0.35 ms
// of bls2017's 7.4 ms, profiles/r04_bls2017_stats.md).  A caller that knows the weights do not change between calls says
// so with tfc_conv2d_weights_key (a number that names this VALUE of the weights; include/tfc_hip.h): the fragments of
// (key, packing site, geometry) are then packed once and kept until tfc_conv2d_drop_weights(key).  Without a key —
// training, or weights that are tensors computed per call — every call packs, as before.
// The entry is made on the first caller's stream; another stream waits for its event (a completed event costs nothing).
// ---------------------------------------------------------------------------
struct WeightsCache {
  struct Key {
    unsigned long long key;
    int site, dev;
    long long dims[16];
    bool operator<(const Key& o) const {
      if (key != o.key) return key < o.key;
      if (site != o.site) return site < o.site;
      if (dev != o.dev) return dev < o.dev;
      return std::lexicographical_compare(dims, dims + 16, o.dims, o.dims + 16);
    }
  };
  struct Entry {
    DevBuf buf;
    hipEvent_t ready = nullptr;
    hipStream_t made_on = nullptr;
    std::vector<hipStream_t> users;          // other streams whose kernels have read the fragments (a handful)
  };
  std::mutex mu;
  std::map<Key, Entry> entries;
  static WeightsCache& get();                // signal_conv.hip: one cache for all units
};

// The packed weights of a call with weights key `key`: *p = `bytes` of fragments, written by pack(p) on `st` — now into
// `local` (key 0), or once into the cache.  site: which packing (the kernels' orders differ); dims: whatever the packing
// depends on.
template <typename Pack>
int packed_weights(unsigned long long key, int site, std::initializer_list<long long> dims, size_t bytes, hipStream_t st,
                   DevBuf& local, void** p, Pack&& pack) {
  if (!key) {
    TFC_HIP(local.alloc(bytes, st));
    *p = local.p;
    return pack(local.p);
  }
  WeightsCache& c = WeightsCache::get();
  WeightsCache::Key k{};
  k.key = key; k.site = site;
  (void)hipGetDevice(&k.dev);
  int i = 0;
  for (long long d : dims) k.dims[i++] = d;
  k.dims[15] = static_cast<long long>(bytes);
  std::lock_guard<std::mutex> lock(c.mu);
  auto it = c.entries.find(k);
  if (it == c.entries.end()) {
    WeightsCache::Entry e;
    TFC_HIP(e.buf.alloc(bytes, st));
    const int rc = pack(e.buf.p);
    if (rc) return rc;
    TFC_HIP(hipEventCreateWithFlags(&e.ready, hipEventDisableTiming));
    TFC_HIP(hipEventRecord(e.ready, st));
    e.made_on = st;
    it = c.entries.emplace(k, std::move(e)).first;
  } else if (it->second.made_on != st) {
    TFC_HIP(hipStreamWaitEvent(st, it->second.ready, 0));
    auto& users = it->second.users;
    if (std::find(users.begin(), users.end(), st) == users.end()) users.push_back(st);
  }
  *p = it->second.buf.p;
  return 0;
}

}  // namespace tfc
