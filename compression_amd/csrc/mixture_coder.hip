// A range coder whose CDFs are evaluated where they are coded: the discretized Gaussian mixture of Cheng, Sun,
// Takeuchi and Katto (CVPR 2020), K weights, means and scales per element (mixture_cdf.h).  Every other
// coder kernel here consumes (table index, symbol); no finite table set spans 3 K free parameters per element.
//
// One wave per code stream, as the wave-per-stream family (range_wave.h): the range-coder state is wave-uniform and
// serial, the CDF is the parallel part.
//   encode: 64 lanes evaluate (c_s, c_{s+1}) of 64 consecutive elements, the chain consumes them in order.
//   decode: a 64-ary search in place of a table coder's binary search: every lane evaluates c at one candidate boundary,
//           a ballot picks the interval: one round for L <= 64, two for L <= 4096.
// The decoder reads zeros behind the end of a string (window_load) and cannot leave the window: the ballot of each
// round is OR-ed with the bit of the round's last candidate before the first set bit is taken.
// The state arithmetic is range_wave.h's (enc_update, finalize_bytes, dec_narrow, dec_finalize_ok); nothing of it is
// restated here.  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "../../include/tfc_hip.h"
#include "common.h"
#include "launch.h"
#include "mixture_cdf.h"
#include "range_wave.h"

namespace tfc {
namespace {

struct MixCoderParams {
  const float* logits;          // planes [K][batch * elems]
  const float* loc;
  const float* scale;
  long long batch, elems, stream_symbols, streams_per_entry, total_streams;
  const int32_t* lo;            // [batch]
  const int32_t* len;           // [batch]
  // encode
  const int32_t* sym;           // [batch, elems]
  uint8_t* slabs;               // [total_streams][cap]
  unsigned int cap;
  unsigned int* lens;           // [total_streams]
  // decode
  const uint8_t* blob;
  const int64_t* offsets;       // [nstrings + 1]
  const int32_t* stream_index;  // [nstrings] or null (string j is stream j)
  long long nstrings;
  int32_t* out;                 // [batch, elems]
  uint8_t* ok;                  // [nstrings]
};

constexpr long long kMaxStreams = 1ll << 23;

__device__ inline int clamp_window(int len) { return min(max(len, 1), MIX_MAX_WINDOW); }

__device__ inline float lane_float(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

template <int K>
__global__ void __launch_bounds__(kBlock) mixture_enc_kernel(MixCoderParams p) {
  const int lane = threadIdx.x & 63;
  const long long s = static_cast<long long>(blockIdx.x) * kWavesPerBlock +
                      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  if (s >= p.total_streams) return;
  const long long b = s / p.streams_per_entry;
  const long long first = (s - b * p.streams_per_entry) * p.stream_symbols;
  const int n = static_cast<int>(min(p.stream_symbols, p.elems - first));
  const long long at0 = b * p.elems + first;
  const long long planes = p.batch * p.elems;
  const int lo = p.lo[b];
  const int len = clamp_window(p.len[b]);

  EncoderState st{0u, 0xFFFFFFFFu, 0u, 0u};
  DigitSink o;
  o.dst = p.slabs + s * p.cap;
  o.cap = p.cap - 4;
  o.nbytes = 0;
  o.n = 0;
  o.reg = 0;
  o.overflow = 0;
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    int clo = 0, chi = 1 << MIX_PRECISION;
    if (k < n) {
      const MixElem<K> e = mix_load<K>(p.logits, p.loc, p.scale, planes, at0 + k);
      // a symbol outside the window is coded as the window's nearest end (the caller clamps y_hat the same way)
      const long long d = static_cast<long long>(p.sym[at0 + k]) - lo;
      const int v = static_cast<int>(min<long long>(max<long long>(d, 0), len - 1));
      clo = mix_boundary<K>(e, lo, len, v);
      chi = mix_boundary<K>(e, lo, len, v + 1);
    }
    const int cnt = min(64, n - k0);
    for (int i = 0; i < cnt; ++i)
      enc_update(st, __builtin_amdgcn_readlane(clo, i), __builtin_amdgcn_readlane(chi, i), o, lane);
  }
  sink_flush(o, lane);
  if (lane == 0) p.lens[s] = o.overflow ? 0xFFFFFFFFu : finalize_bytes(st, o, o.dst);
}

// One symbol: the first v in [0, len) with target <= span * c_{v+1}; on damaged input (no candidate matches) the last.
template <int K>
__device__ inline int mix_dec_symbol(const MixElem<K>& e, int lo, int len, int step, int last_group,
                                     DecoderState& st, DigitWindow& w, int lane) {
  const unsigned long long span = static_cast<unsigned long long>(st.span_m1) + 1;
  const unsigned long long target =
      (static_cast<unsigned long long>(static_cast<unsigned int>(st.window - st.base)) + 1) << MIX_PRECISION;
  int first = 0, cnt = len;
  unsigned int below = 0;                                  // c_first
  if (step > 1) {
    // round 1: lane j holds the upper boundary of group j (step symbols); the groups behind last_group do not exist
    const int c = mix_boundary<K>(e, lo, len, min((lane + 1) * step, len));
    const unsigned long long m =
        __ballot(target <= span * static_cast<unsigned int>(c)) | (1ull << last_group);
    const int g = __builtin_ctzll(m);
    first = g * step;
    cnt = min(step, len - first);
    if (g) below = static_cast<unsigned int>(__builtin_amdgcn_readlane(c, g - 1));
  }
  // round 2 (the only one for len <= 64): lane j holds c_{first + j + 1}
  const int c = mix_boundary<K>(e, lo, len, min(first + lane + 1, len));
  const unsigned long long m =
      (__ballot(lane < cnt && target <= span * static_cast<unsigned int>(c))) | (1ull << (cnt - 1));
  const int kk = __builtin_ctzll(m);
  const unsigned int hi = static_cast<unsigned int>(__builtin_amdgcn_readlane(c, kk));
  const unsigned int lw = kk ? static_cast<unsigned int>(__builtin_amdgcn_readlane(c, kk - 1)) : below;
  dec_narrow(st, lw, hi, MIX_PRECISION, w, lane);
  return first + kk;
}

template <int K>
__global__ void __launch_bounds__(kBlock) mixture_dec_kernel(MixCoderParams p) {
  const int lane = threadIdx.x & 63;
  const long long j = static_cast<long long>(blockIdx.x) * kWavesPerBlock +
                      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  if (j >= p.nstrings) return;
  const long long s = p.stream_index ? static_cast<long long>(p.stream_index[j]) : j;
  if (s < 0 || s >= p.total_streams) {                     // no such stream: nothing is written but the verdict
    if (lane == 0) p.ok[j] = 0;
    return;
  }
  const long long b = s / p.streams_per_entry;
  const long long first = (s - b * p.streams_per_entry) * p.stream_symbols;
  const int n = static_cast<int>(min(p.stream_symbols, p.elems - first));
  const long long at0 = b * p.elems + first;
  const long long planes = p.batch * p.elems;
  const int lo = p.lo[b];
  const int len = clamp_window(p.len[b]);
  const int step = (len + 63) >> 6;                        // symbols per group of round 1; 1: no round 1
  const int last_group = (len + step - 1) / step - 1;

  DecoderState st{0u, 0xFFFFFFFFu, 0u};
  DigitWindow w;
  w.src = p.blob + p.offsets[j];
  w.len = max<long long>(p.offsets[j + 1] - p.offsets[j], 0);
  w.pulls = 0;
  w.base = 0;
  window_load(w, lane);
  st.window = window_pull(w, lane) << 16;
  st.window |= window_pull(w, lane);
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    MixElem<K> mine = {};
    if (k < n) mine = mix_load<K>(p.logits, p.loc, p.scale, planes, at0 + k);
    const int cnt = min(64, n - k0);
    int outv = 0;
    for (int i = 0; i < cnt; ++i) {
      MixElem<K> e;
#pragma unroll
      for (int c = 0; c < K; ++c) {
        e.w[c] = lane_float(mine.w[c], i);
        e.mu[c] = lane_float(mine.mu[c], i);
        e.sigma[c] = lane_float(mine.sigma[c], i);
      }
      const int v = mix_dec_symbol<K>(e, lo, len, step, last_group, st, w, lane);
      outv = tfc_writelane(lo + v, i, outv);
    }
    if (k < n) p.out[at0 + k] = outv;
  }
  if (lane == 0) {
    // Finalize's verdict, and one rule of this coder's own: while no carry is pending (base + span does not wrap) the
    // encoder has written every digit the decoder pulled behind the first two, so a string that ends before them is
    // short.  (An empty string is then good only where the symbols cost less than one digit, as for L = 1.)
    const bool pending = static_cast<unsigned int>(st.base + st.span_m1) < st.base;
    const bool starved = !pending && 2ll * (static_cast<long long>(w.pulls) - 2) > w.len;
    p.ok[j] = (!starved && dec_finalize_ok(st.base, st.span_m1, st.window, w.pulls, w.len)) ? 1 : 0;
  }
}

struct MixDumpParams {
  const float* logits;
  const float* loc;
  const float* scale;
  long long n;
  int lo, len;
  int32_t* out;                 // [n][len + 1]
};

template <int K>
__global__ void __launch_bounds__(256) mixture_cdf_kernel(MixDumpParams p) {
  const long long width = p.len + 1;
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= p.n * width) return;
  const long long at = i / width;
  const int b = static_cast<int>(i - at * width);
  const MixElem<K> e = mix_load<K>(p.logits, p.loc, p.scale, p.n, at);
  p.out[i] = mix_boundary<K>(e, p.lo, p.len, b);
}

// offsets[0 .. n] = exclusive sums of lens (an overflowed stream counts as empty and raises *bad); one block.
__global__ void __launch_bounds__(256) mixture_offsets_kernel(const unsigned int* lens, long long n, int64_t* offsets,
                                                              unsigned int* bad) {
  __shared__ long long part[256];
  const int t = threadIdx.x;
  const long long chunk = (n + 255) / 256;
  const long long a = min(n, t * chunk), z = min(n, a + chunk);
  long long sum = 0;
  bool over = false;
  for (long long i = a; i < z; ++i) {
    over |= lens[i] == 0xFFFFFFFFu;
    sum += lens[i] == 0xFFFFFFFFu ? 0 : lens[i];
  }
  if (over) atomicOr(bad, 1u);
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    long long run = 0;
    for (int i = 0; i < 256; ++i) {
      const long long v = part[i];
      part[i] = run;
      run += v;
    }
    offsets[n] = run;
  }
  __syncthreads();
  long long run = part[t];
  for (long long i = a; i < z; ++i) {
    offsets[i] = run;
    run += lens[i] == 0xFFFFFFFFu ? 0 : lens[i];
  }
}

// string s: slab -> blob + offsets[s]; one block per string
__global__ void __launch_bounds__(256) mixture_gather_kernel(const uint8_t* slabs, unsigned int cap,
                                                             const int64_t* offsets, uint8_t* blob) {
  const long long s = blockIdx.x;
  const long long n = min<long long>(offsets[s + 1] - offsets[s], cap);
  const uint8_t* src = slabs + s * cap;
  uint8_t* dst = blob + offsets[s];
  for (long long i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
}

int check_common(const char* who, const void* logits, const void* loc, const void* scale, int k) {
  if (k < 1 || k > MIX_MAX_COMPONENTS) return fail("%s: k must be in [1, %d] (got %d)", who, MIX_MAX_COMPONENTS, k);
  if (!logits || !loc || !scale) return fail("%s: null parameter pointer", who);
  return 0;
}

int check_streams(const char* who, int64_t batch, int64_t elems, int64_t stream_symbols, const void* lo,
                  const void* len, MixCoderParams* p) {
  if (batch < 0 || elems < 0) return fail("%s: batch and elems must not be negative", who);
  if (stream_symbols < 1 || stream_symbols > (1ll << 28))
    return fail("%s: stream_symbols must be in [1, 2^28] (got %lld)", who, static_cast<long long>(stream_symbols));
  if (!lo || !len) return fail("%s: null window pointer", who);
  p->batch = batch;
  p->elems = elems;
  p->stream_symbols = stream_symbols;
  p->streams_per_entry = ceil_div(elems, stream_symbols);
  p->total_streams = batch * p->streams_per_entry;
  // one wave per stream in blocks of kBlock threads, and one block per string behind the encoder: 2^23 streams keep
  // both launches inside what one launch takes (blocks x threads below 2^32)
  if (p->total_streams > kMaxStreams)
    return fail("%s: %lld streams, one call takes at most %lld", who, p->total_streams, kMaxStreams);
  p->lo = static_cast<const int32_t*>(lo);
  p->len = static_cast<const int32_t*>(len);
  return 0;
}

unsigned int slab_bytes(int64_t stream_symbols) {
  // a call leaves at most one 16-bit digit (a resolved carry moves digits, it adds none), Finalize at most two bytes;
  // DigitSink keeps 4 bytes of the capacity back
  return static_cast<unsigned int>(2 * stream_symbols + 16);
}

#define TFC_MIX_DISPATCH(kernel, k, ...)                                        \
  switch (k) {                                                                  \
    case 1: hipLaunchKernelGGL(kernel<1>, __VA_ARGS__); break;                  \
    case 2: hipLaunchKernelGGL(kernel<2>, __VA_ARGS__); break;                  \
    case 3: hipLaunchKernelGGL(kernel<3>, __VA_ARGS__); break;                  \
    default: hipLaunchKernelGGL(kernel<4>, __VA_ARGS__); break;                 \
  }

}  // namespace
}  // namespace tfc

using namespace tfc;

extern "C" int tfc_mixture_cdf(const float* logits, const float* loc, const float* scale, int k, int64_t n, int lo,
                               int len, int32_t* cdf, void* stream) {
  if (int rc = check_common("tfc_mixture_cdf", logits, loc, scale, k)) return rc;
  if (len < 1 || len > MIX_MAX_WINDOW) return fail("tfc_mixture_cdf: L must be in [1, %d] (got %d)", MIX_MAX_WINDOW, len);
  if (lo < -MIX_MAX_ABS_LO || lo > MIX_MAX_ABS_LO)
    return fail("tfc_mixture_cdf: lo must be in [-%d, %d] (got %d)", MIX_MAX_ABS_LO, MIX_MAX_ABS_LO, lo);
  if (n < 0) return fail("tfc_mixture_cdf: n must not be negative");
  if (n == 0) return 0;
  if (!cdf) return fail("tfc_mixture_cdf: null output pointer");
  const long long blocks = ceil_div(n * (len + 1ll), 256);
  if (blocks > kMaxGridX) return fail("tfc_mixture_cdf: table too large for one launch");
  hipStream_t st = static_cast<hipStream_t>(stream);
  MixDumpParams p{logits, loc, scale, n, lo, len, cdf};
  KernelTimer timer("mixture_cdf", st);
  TFC_MIX_DISPATCH(mixture_cdf_kernel, k, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st, p);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t tfc_mixture_blob_capacity(int64_t batch, int64_t elems, int64_t stream_symbols) {
  if (batch < 0 || elems < 0 || stream_symbols < 1 || stream_symbols > (1ll << 28)) {
    fail("tfc_mixture_blob_capacity: bad sizes");
    return -1;
  }
  return batch * ceil_div(elems, stream_symbols) * static_cast<int64_t>(slab_bytes(stream_symbols));
}

extern "C" int tfc_mixture_encode(const int32_t* sym, const float* logits, const float* loc, const float* scale, int k,
                                  int64_t batch, int64_t elems, int64_t stream_symbols, const int32_t* lo,
                                  const int32_t* len, uint8_t* blob, int64_t* offsets, uint32_t* overflow,
                                  void* stream) {
  const char* who = "tfc_mixture_encode";
  if (int rc = check_common(who, logits, loc, scale, k)) return rc;
  MixCoderParams p{};
  if (int rc = check_streams(who, batch, elems, stream_symbols, lo, len, &p)) return rc;
  if (!offsets || !overflow) return fail("%s: null output pointer", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  TFC_HIP(hipMemsetAsync(overflow, 0, sizeof(uint32_t), st));
  if (p.total_streams == 0) {
    TFC_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t), st));
    return 0;
  }
  if (!sym || !blob) return fail("%s: null pointer", who);
  p.logits = logits; p.loc = loc; p.scale = scale; p.sym = sym;
  p.cap = slab_bytes(stream_symbols);
  DevBuf slabs, lens;
  TFC_HIP(slabs.alloc(static_cast<size_t>(p.total_streams) * p.cap, st));
  TFC_HIP(lens.alloc(sizeof(unsigned int) * p.total_streams, st));
  p.slabs = slabs.as<uint8_t>();
  p.lens = lens.as<unsigned int>();
  {
    KernelTimer timer("mixture_encode", st);
    const dim3 grid(static_cast<unsigned>(ceil_div(p.total_streams, kWavesPerBlock)));
    TFC_MIX_DISPATCH(mixture_enc_kernel, k, grid, dim3(kBlock), 0, st, p);
  }
  hipLaunchKernelGGL(mixture_offsets_kernel, dim3(1), dim3(256), 0, st, p.lens, p.total_streams, offsets, overflow);
  hipLaunchKernelGGL(mixture_gather_kernel, dim3(static_cast<unsigned>(p.total_streams)), dim3(256), 0, st, p.slabs,
                     p.cap, offsets, blob);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_mixture_decode(const uint8_t* blob, const int64_t* offsets, const int32_t* stream_index,
                                  int64_t nstrings, const float* logits, const float* loc, const float* scale, int k,
                                  int64_t batch, int64_t elems, int64_t stream_symbols, const int32_t* lo,
                                  const int32_t* len, int32_t* out, uint8_t* ok, void* stream) {
  const char* who = "tfc_mixture_decode";
  if (int rc = check_common(who, logits, loc, scale, k)) return rc;
  MixCoderParams p{};
  if (int rc = check_streams(who, batch, elems, stream_symbols, lo, len, &p)) return rc;
  if (nstrings < 0) return fail("%s: nstrings must not be negative", who);
  if (!stream_index && nstrings != p.total_streams)
    return fail("%s: %lld strings for %lld streams and no stream_index", who, static_cast<long long>(nstrings),
                p.total_streams);
  if (nstrings == 0) return 0;
  if (nstrings > kMaxStreams)
    return fail("%s: %lld strings, one call takes at most %lld", who, static_cast<long long>(nstrings), kMaxStreams);
  if (!blob || !offsets || !out || !ok) return fail("%s: null pointer", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  p.logits = logits; p.loc = loc; p.scale = scale;
  p.blob = blob; p.offsets = offsets; p.stream_index = stream_index; p.nstrings = nstrings;
  p.out = out; p.ok = ok;
  KernelTimer timer("mixture_decode", st);
  const dim3 grid(static_cast<unsigned>(ceil_div(nstrings, kWavesPerBlock)));
  TFC_MIX_DISPATCH(mixture_dec_kernel, k, grid, dim3(kBlock), 0, st, p);
  TFC_HIP(hipGetLastError());
  return 0;
}
