// Device primitives of the wave-per-stream coder: one 64-lane wavefront per code stream, the chain on wave-uniform
// values.  Shared by the generic kernels of range_coder.hip and the deprecated single-stream ops of
// range_coder_legacy.hip.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "range_coder_device.h"

namespace tfc {

constexpr int kWavesPerBlock = 4;
constexpr int kBlock = kWavesPerBlock * 64;

// Where symbols come from (encode) / go to (decode).
// Loads and stores of the kernels' tensor arguments go through global-address-space pointers: the functors below travel
// inside job arrays indexed at run time, where hipcc cannot tell that their pointers are global and emits FLAT
// instructions — which count on lgkmcnt as well as vmcnt, so that every wait for an LDS read in the same loop becomes a
// wait for the loop's stores too (seen in dec_parse_kernel and enc_expand_kernel, round 6).
#ifndef TFC_AS1
#define TFC_AS1 __attribute__((address_space(1)))
#endif
template <typename T>
__device__ inline T tfc_gload(const T* p) {
  static_assert(sizeof(T) == 2 || sizeof(T) == 4, "16- and 32-bit elements");
  if constexpr (sizeof(T) == 2) {
    return __builtin_bit_cast(T, *reinterpret_cast<const TFC_AS1 unsigned short*>((const TFC_AS1 void*)p));
  } else {
    return __builtin_bit_cast(T, *reinterpret_cast<const TFC_AS1 unsigned int*>((const TFC_AS1 void*)p));
  }
}
template <typename T>
__device__ inline void tfc_gstore(T* p, T v) {
  static_assert(sizeof(T) == 2 || sizeof(T) == 4, "16- and 32-bit elements");
  if constexpr (sizeof(T) == 2) {
    *reinterpret_cast<TFC_AS1 unsigned short*>((TFC_AS1 void*)p) = __builtin_bit_cast(unsigned short, v);
  } else {
    *reinterpret_cast<TFC_AS1 unsigned int*>((TFC_AS1 void*)p) = __builtin_bit_cast(unsigned int, v);
  }
}

struct SymInt32 {          // plain int32 symbols
  const int32_t* value;
  __device__ int32_t load(int64_t pos, int /*table*/) const { return tfc_gload(value + pos); }
  // split form for kernels that request an element before they know its table
  __device__ int32_t raw(int64_t pos) const { return tfc_gload(value + pos); }
  __device__ int32_t quant(int32_t r, int /*table*/) const { return r; }
  __device__ const int32_t* base() const { return value; }
  using raw_type = int32_t;
};


template <typename T>
__device__ inline float to_float(T v);
template <> __device__ inline float to_float<float>(float v) { return v; }
template <> __device__ inline float to_float<__hip_bfloat16>(__hip_bfloat16 v) { return __bfloat162float(v); }
template <> __device__ inline float to_float<__half>(__half v) { return __half2float(v); }
template <typename T>
__device__ inline T from_float(float v);
template <> __device__ inline float from_float<float>(float v) { return v; }
template <> __device__ inline __hip_bfloat16 from_float<__hip_bfloat16>(float v) { return __float2bfloat16(v); }
template <> __device__ inline __half from_float<__half>(float v) { return __float2half(v); }

// Fused quantisation: sym = int32(rint(y - qoff[t])) - cdf_offset[t].  The
// subtraction happens in the bottleneck dtype like the reference's
// `bottleneck -= offset` (continuous_batched.py:375-378); rintf is
// round-half-to-even like tf.round.
template <typename T>
struct SymQuant {
  const T* y;
  const float* qoffset;        // may be null
  const int32_t* cdf_offset;
  __device__ int32_t load(int64_t pos, int table) const { return quant(tfc_gload(y + pos), table); }
  __device__ T raw(int64_t pos) const { return tfc_gload(y + pos); }
  __device__ const T* base() const { return y; }
  using raw_type = T;
  __device__ int32_t quant(T r, int table) const {
    float f = to_float<T>(r);
    if (qoffset) f = to_float<T>(from_float<T>(f - to_float<T>(from_float<T>(tfc_gload(qoffset + table)))));
    return static_cast<int32_t>(rintf(f)) - tfc_gload(cdf_offset + table);
  }
};

// Per-element classification shared by the counting and the coding pass.
struct Call {
  int32_t lo16, hi16;   // interval scaled to 16-bit precision
  int32_t gamma;        // > 0 => escape follows
  int32_t neg;
  int32_t bad;          // 1: index out of range, 2: value out of range
};

template <bool NORMALISED, typename TabFn>
__device__ inline Call classify_impl(const TabFn& T, const int2 row, int32_t v) {
  Call c;
  c.gamma = 0;
  c.neg = 0;
  c.bad = 0;
  const int32_t sp = T(row.x);
  const int32_t prec = sp < 0 ? -sp : sp;
  int32_t sym = v;
  if (sp > 0) {
    if (v < 0 || v >= row.y - 2) {
      c.bad = 2;
      sym = 0;
    }
  } else {
    const int32_t vmax = row.y - 3;
    if (v < 0) {
      c.neg = 1;
      c.gamma = -v;
      sym = vmax;
    } else if (v >= vmax) {
      c.gamma = v - vmax + 1;
      sym = vmax;
    }
  }
  const int sh = NORMALISED ? 0 : 16 - prec;
  c.lo16 = T(row.x + 1 + sym) << sh;
  c.hi16 = T(row.x + 2 + sym) << sh;
  return c;
}

template <typename TabFn>
__device__ inline Call classify(const TabFn& T, const int2 row, int32_t v) {
  return classify_impl<false>(T, row, v);
}
template <typename TabFn>
__device__ inline Call classify_normalised(const TabFn& T, const int2 row, int32_t v) {
  return classify_impl<true>(T, row, v);
}

// The same classification on the encoder's 16-bit LDS image (tfc_tables_create): hi16 is the upper
// bound modulo 2^16 — its only use is "upper - 1" in the call word, which is right either way.
__device__ inline Call classify_fast(const uint16_t* tab, const int2 row, int32_t v) {
  Call c;
  c.gamma = 0;
  c.neg = 0;
  c.bad = 0;
  const int len = row.y & 0x7FFFFFFF;
  int32_t sym = v;
  if (row.y >= 0) {
    if (v < 0 || v >= len - 2) {
      c.bad = 2;
      sym = 0;
    }
  } else {
    const int32_t vmax = len - 3;
    if (v < 0) {
      c.neg = 1;
      c.gamma = -v;
      sym = vmax;
    } else if (v >= vmax) {
      c.gamma = v - vmax + 1;
      sym = vmax;
    }
  }
  c.lo16 = tab[row.x + 1 + sym];
  c.hi16 = tab[row.x + 2 + sym];
  return c;
}

__device__ inline int escape_calls(int32_t gamma) {
  // 1 + 2*floor(log2 gamma) bits for the Elias-gamma code, plus one sign bit
  // (range_coder_kernels.cc:304-321).
  const int nb = 31 - __clz(gamma);
  return 2 * nb + 2;
}

// 16-bit digit collector: 64 digits per VGPR, one coalesced store per flush.
struct DigitSink {
  uint8_t* dst;        // 2-byte aligned
  unsigned int nbytes; // bytes already stored
  unsigned int cap;
  int n;               // digits waiting in reg
  int reg;
  unsigned int overflow;
};

__device__ inline void sink_flush(DigitSink& o, int lane) {
  if (o.nbytes + 2u * o.n > o.cap) {
    o.overflow = 1;
  } else if (lane < o.n) {
    const unsigned int d = static_cast<unsigned int>(o.reg);
    const unsigned short be = static_cast<unsigned short>(((d & 0xFF) << 8) | ((d >> 8) & 0xFF));
    reinterpret_cast<unsigned short*>(o.dst + o.nbytes)[lane] = be;
  }
  o.nbytes += 2u * o.n;
  o.n = 0;
}

__device__ inline void sink_put(DigitSink& o, unsigned int digit, int lane) {
  o.reg = tfc_writelane(static_cast<int>(digit), o.n, o.reg);
  ++o.n;
  if (o.n == 64) sink_flush(o, lane);
}

// One interval update on wave-uniform state; [lo16, hi16) / 2^16.
__device__ inline void enc_update(EncoderState& st, unsigned int lo16, unsigned int hi16,
                                  DigitSink& o, int lane) {
  const unsigned long long span = static_cast<unsigned long long>(st.span_m1) + 1;
  const unsigned int a = static_cast<unsigned int>((span * lo16) >> 16);
  const unsigned int b = static_cast<unsigned int>(((span * hi16) >> 16) - 1);
  st.base += a;
  st.span_m1 = b - a;
  const bool wrapped = st.base < a;
  if (static_cast<unsigned int>(st.base + st.span_m1) < st.base) {
    if ((st.span_m1 >> 16) == 0) {
      st.base <<= 16;
      st.span_m1 = (st.span_m1 << 16) | 0xFFFFu;
      st.pend_bytes += 2;
    }
    return;
  }
  if (st.pend_digit != 0) {
    unsigned int d = st.pend_digit;
    unsigned int fill = 0;
    if (!wrapped) {
      d -= 1;
      fill = 0xFFFFu;
    }
    sink_put(o, d, lane);
    for (unsigned int k = 0; k < st.pend_bytes; k += 2) sink_put(o, fill, lane);
    st.pend_digit = 0;
    st.pend_bytes = 0;
  }
  if ((st.span_m1 >> 16) == 0) {
    const unsigned int top = st.base >> 16;
    st.base <<= 16;
    st.span_m1 = (st.span_m1 << 16) | 0xFFFFu;
    if (st.base <= static_cast<unsigned int>(st.base + st.span_m1)) {
      sink_put(o, top, lane);
    } else {
      st.pend_digit = top + 1;
    }
  }
}

// RangeEncoder::Finalize (cc/lib/range_coder.cc:266-307) behind the digits already stored:
// returns the stream length.  One lane.
__device__ inline unsigned int finalize_bytes(const EncoderState& st, const DigitSink& o, uint8_t* out) {
  unsigned int n = o.nbytes;
  uint8_t* dst = out + n;
  if (st.pend_digit != 0) {
    dst[0] = (st.pend_digit >> 8) & 0xFF; ++n;
    if ((st.pend_digit & 0xFF) != 0) { dst[1] = st.pend_digit & 0xFF; ++n; }
  } else if (st.base != 0) {
    const unsigned int top = st.base + st.span_m1;
    const unsigned int r24 = ((st.base - 1) >> 24) + 1;
    if (r24 <= (top >> 24)) {
      dst[0] = r24 & 0xFF; ++n;
    } else {
      const unsigned int r16 = ((st.base - 1) >> 16) + 1;
      dst[0] = (r16 >> 8) & 0xFF; ++n;
      if ((r16 & 0xFF) != 0) { dst[1] = r16 & 0xFF; ++n; }
    }
  }
  return n;
}

// 64 upcoming big-endian digits of the stream, one per lane.
struct DigitWindow {
  const uint8_t* src;
  long long len;        // stream length in bytes
  unsigned int pulls;   // digits consumed so far (including the two of the ctor)
  unsigned int base;    // digit index held by lane 0
  int reg;
};

__device__ inline void window_load(DigitWindow& w, int lane) {
  const long long b = 2ll * (static_cast<long long>(w.base) + lane);
  unsigned int hi = b < w.len ? w.src[b] : 0u;
  unsigned int lo = b + 1 < w.len ? w.src[b + 1] : 0u;
  w.reg = static_cast<int>((hi << 8) | lo);
}

__device__ inline unsigned int window_pull(DigitWindow& w, int lane) {
  if (w.pulls - w.base >= 64u) {
    w.base = w.pulls;
    window_load(w, lane);
  }
  const unsigned int d = __builtin_amdgcn_readlane(w.reg, static_cast<int>(w.pulls - w.base));
  ++w.pulls;
  return d;
}

struct DecoderState {
  unsigned int base, span_m1, window;
};

// The two rules of the stream format at a decoder's ends, as (base, span_m1, window, pulls).  A stream opens on the
// whole interval with its first four bytes in the window, zeros behind its end (RangeDecoder's constructor,
// range_coder.h:79-83) ...
__host__ __device__ __forceinline__ uint4 dec_open_state(const uint8_t* const& src, const long long& len) {
  unsigned int w = 0;
  for (int i = 0; i < 4; ++i) w = (w << 8) | (i < len ? src[i] : 0u);
  return make_uint4(0u, 0xFFFFFFFFu, w, 2u);
}

// ... and closes well when no byte is left over and the window holds what the encoder's last flush wrote for this
// interval (RangeDecoder::Finalize, range_coder.h:144-169).
// (The arguments are references so that the callers' code comes out as it did with the rule written in place.)
__host__ __device__ __forceinline__ bool dec_finalize_ok(const unsigned int& base, const unsigned int& span_m1,
                                                         const unsigned int& window, const unsigned int& pulls,
                                                         const long long& len) {
  bool good;
  if (2ll * pulls < len) {
    good = false;
  } else {
    const unsigned int top = base + span_m1;
    if (base == 0 || top < base) {
      good = window == 0;
    } else {
      const int sh = (((base - 1) >> 24) < (top >> 24)) ? 24 : 16;
      const unsigned int r = ((base - 1) >> sh) + 1;
      good = (r << sh) == window;
    }
  }
  return good;
}

__device__ inline void dec_narrow(DecoderState& st, unsigned int lo, unsigned int hi, int prec,
                                  DigitWindow& w, int lane) {
  const unsigned long long span = static_cast<unsigned long long>(st.span_m1) + 1;
  const unsigned int a = static_cast<unsigned int>((span * lo) >> prec);
  const unsigned int b = static_cast<unsigned int>(((span * hi) >> prec) - 1);
  st.base += a;
  st.span_m1 = b - a;
  if ((st.span_m1 >> 16) == 0) {
    st.base <<= 16;
    st.span_m1 = (st.span_m1 << 16) | 0xFFFFu;
    st.window = (st.window << 16) | window_pull(w, lane);
  }
}

// Decode one binary digit with the uniform cdf {0,1,2}, precision 1
// (DecodeLinearly, range_coder.h:193-202 with the call at
// range_coder_kernels.cc:449-471).
__device__ inline int dec_bit(DecoderState& st, DigitWindow& w, int lane) {
  const unsigned long long span = static_cast<unsigned long long>(st.span_m1) + 1;
  const unsigned long long target =
      (static_cast<unsigned long long>(static_cast<unsigned int>(st.window - st.base)) + 1) << 1;
  const int bit = (target <= span) ? 0 : 1;
  dec_narrow(st, bit, bit + 1, 1, w, lane);
  return bit;
}

// Finds the first symbol k with target <= span * cdf[k + 1]; all 64 lanes test
// one candidate each.  `cdf0` = position of cdf[0], `ncdf` = number of cdf
// entries.  On damaged input (no candidate matches) the last symbol is taken.
template <typename TabFn>
__device__ inline int dec_symbol(const TabFn& T, DecoderState& st, int cdf0, int ncdf, int prec,
                                 DigitWindow& w, int lane) {
  const unsigned long long span = static_cast<unsigned long long>(st.span_m1) + 1;
  const unsigned long long target =
      (static_cast<unsigned long long>(static_cast<unsigned int>(st.window - st.base)) + 1) << prec;
  const int nsym = ncdf - 1;
  int sym = nsym - 1;
  unsigned int lo = 0, hi = 0;
  bool found = false;
  for (int c0 = 0; c0 < nsym; c0 += 64) {
    const int k = c0 + lane;
    unsigned int lo_k = 0, hi_k = 0;
    if (k < nsym) {
      lo_k = static_cast<unsigned int>(T(cdf0 + k));
      hi_k = static_cast<unsigned int>(T(cdf0 + k + 1));
    }
    const bool pred = (k < nsym) && (target <= span * hi_k);
    const unsigned long long m = __ballot(pred);
    if (m != 0) {
      const int kk = __builtin_ctzll(m);
      lo = __builtin_amdgcn_readlane(static_cast<int>(lo_k), kk);
      hi = __builtin_amdgcn_readlane(static_cast<int>(hi_k), kk);
      sym = c0 + kk;
      found = true;
      break;
    }
  }
  if (!found) {
    lo = static_cast<unsigned int>(T(cdf0 + nsym - 1));
    hi = static_cast<unsigned int>(T(cdf0 + nsym));
  }
  dec_narrow(st, lo, hi, prec, w, lane);
  return sym;
}

// The value behind the escape symbol of a row with negative precision (`nints` = ints of the row, header included):
// an Elias-gamma code and a sign bit (range_coder_kernels.cc:449-471).
__device__ inline int dec_escape(DecoderState& st, DigitWindow& w, int lane, int nints) {
  int nb = 0;
  // bound the unary prefix so damaged input cannot spin forever
  while (nb < 31 && dec_bit(st, w, lane) == 0) ++nb;
  int v = 1 << nb;
  while (--nb >= 0) v |= dec_bit(st, w, lane) << nb;
  const int neg = dec_bit(st, w, lane);
  return neg ? -v : v + (nints - 3) - 1;
}

struct OutInt32 {
  int32_t* out;
  __device__ void store(int64_t pos, int /*table*/, int32_t sym) const { tfc_gstore(out + pos, sym); }
  // split form for kernels that collect several elements per store
  using elem = int32_t;
  __device__ int32_t make(int /*table*/, int32_t sym) const { return sym; }
  __device__ int32_t* ptr() const { return out; }
};

template <typename T>
struct OutDequant {
  T* y;
  const float* qoffset;
  const int32_t* cdf_offset;
  __device__ void store(int64_t pos, int table, int32_t sym) const { tfc_gstore(y + pos, make(table, sym)); }
  using elem = T;
  __device__ T make(int table, int32_t sym) const {
    // outputs = cast(symbols + cdf_offset, dtype) (+ quantization_offset)
    T v = from_float<T>(static_cast<float>(sym + tfc_gload(cdf_offset + table)));
    if (qoffset) v = from_float<T>(to_float<T>(v) + to_float<T>(from_float<T>(tfc_gload(qoffset + table))));
    return v;
  }
  __device__ T* ptr() const { return y; }
};

}  // namespace tfc
