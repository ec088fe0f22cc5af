// Interleaved rANS: the call arithmetic, the element-to-calls expansion and a plain serial coder of a
// whole stream.  Plain C++17 with no HIP types: ans_coder.hip compiles the arithmetic for the device, the CPU tier
// (tests/native/ans_core_check.cc) compiles all of it for the host.
//
// A stream is coded by `lanes` states x in [2^16, 2^32), renormalised in 16-bit words; a call is (start, freq, P) with
// 1 <= P <= 16, 1 <= freq <= 2^P, start + freq <= 2^P.  The bytes are this project's own format, not the reference's.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define TFC_ANS_HD __host__ __device__
#else
#define TFC_ANS_HD
#endif

namespace tfc {
namespace ans {

constexpr int ANS_MAX_LANES = 64;
constexpr int ANS_MAX_CALLS = 4;            // table symbol, 6-bit escape head, low 16 bits, high bits
constexpr int ANS_WORD_BITS = 16;
constexpr int ANS_STATE_LOW = 65536;        // every lane starts, and has to end, here
// per-stream encoder status, or-ed
constexpr int ANS_STATUS_VALUE = 1;         // a value outside a row without escape (or a symbol of zero width)
constexpr int ANS_STATUS_INDEX = 2;         // a table index outside the lookup

struct Call {
  uint32_t start, freq;
  int prec;
};

TFC_ANS_HD inline uint32_t mulhi(uint32_t a, uint32_t b) {
  return static_cast<uint32_t>((static_cast<uint64_t>(a) * b) >> 32);
}

// 2^32 / d, a little low: the float reciprocal scaled just under 2^32, then one Newton step in integers.  mulhi(x, z)
// is then floor(x / d), floor(x / d) - 1 or floor(x / d) - 2 for every 32-bit x and d >= 1 (the sequence compilers emit
// for a 32-bit division on targets without one); divmod makes up the difference.
TFC_ANS_HD inline uint32_t reciprocal(uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float r = __builtin_amdgcn_rcpf(static_cast<float>(d));
#else
  const float r = 1.0f / static_cast<float>(d);
#endif
  uint32_t z = static_cast<uint32_t>(r * 4294966784.0f);      // 0x4F7FFFFE
  z += mulhi(z, (0u - d) * z);
  return z;
}

// x = q d + r with 0 <= r < d, exact for every x < 2^32 and 1 <= d <= 2^16 (z = reciprocal(d)).
TFC_ANS_HD inline void divmod(uint32_t x, uint32_t d, uint32_t z, uint32_t* q, uint32_t* r) {
  uint32_t qq = mulhi(x, z);
  uint32_t rr = x - qq * d;
  if (rr >= d) { ++qq; rr -= d; }
  if (rr >= d) { ++qq; rr -= d; }
  *q = qq;
  *r = rr;
}

// Encoder: whether the state gives up its low word in front of the call  (x >= freq << (32 - P)).
TFC_ANS_HD inline bool enc_emits(uint32_t x, const Call& c) { return (x >> (32 - c.prec)) >= c.freq; }
// ... and the call itself, on the renormalised state.
TFC_ANS_HD inline uint32_t enc_update(uint32_t x, const Call& c) {
  uint32_t q, r;
  divmod(x, c.freq, reciprocal(c.freq), &q, &r);
  return (q << c.prec) + r + c.start;
}

TFC_ANS_HD inline uint32_t dec_slot(uint32_t x, int prec) { return x & ((1u << prec) - 1u); }
// Decoder: the call on a state whose slot fell into [start, start + freq); a result below 2^16 takes a word next.
TFC_ANS_HD inline uint32_t dec_update(uint32_t x, uint32_t slot, const Call& c) {
  return c.freq * (x >> c.prec) + slot - c.start;
}
TFC_ANS_HD inline uint32_t dec_refill(uint32_t x, uint32_t word) { return (x << 16) | word; }

TFC_ANS_HD inline Call raw_call(uint32_t chunk, int bits) { return Call{chunk, 1u, bits}; }

// The reference's escape mapping (range_coder_kernels.cc:290-303), gamma as uint32: every int32 value has one.
TFC_ANS_HD inline uint32_t escape_gamma(int32_t v, int32_t max_value, int* sign) {
  *sign = v < 0;
  return v < 0 ? 0u - static_cast<uint32_t>(v) : static_cast<uint32_t>(v) - static_cast<uint32_t>(max_value) + 1u;
}
TFC_ANS_HD inline int32_t escape_value(uint32_t gamma, int sign, int32_t max_value) {
  return static_cast<int32_t>(sign ? 0u - gamma : gamma + static_cast<uint32_t>(max_value) - 1u);
}
TFC_ANS_HD inline int bit_length(uint32_t g) {
  int n = 0;
  while (g) { ++n; g >>= 1; }
  return n;
}
// Bits of the chunks behind the escape head, for k = bit_length(gamma) - 1.
TFC_ANS_HD inline int low_bits(int k) { return k < 16 ? k : 16; }
TFC_ANS_HD inline int high_bits(int k) { return k > 16 ? k - 16 : 0; }

// Element -> calls.  `row` points at a row's header, `row_size` counts header, boundaries and the closing 2^P.
// -> the number of calls, or 0 with ANS_STATUS_VALUE or-ed into *status.
TFC_ANS_HD inline int expand(const int32_t* row, int row_size, int32_t v, Call* out, int* status) {
  const int32_t h = row[0];
  const int prec = h < 0 ? -h : h;
  const int nsym = row_size - 2;
  const int32_t max_value = nsym - 1;
  int n = 1;
  int32_t sym = v;
  if (h < 0 && (v < 0 || v >= max_value)) {
    int sign;
    const uint32_t gamma = escape_gamma(v, max_value, &sign);
    const int k = bit_length(gamma) - 1;
    const uint32_t m = gamma - (1u << k);
    sym = max_value;
    // (fixed places: k > 16 implies k > 0)
    out[1] = raw_call(static_cast<uint32_t>(k) | (static_cast<uint32_t>(sign) << 5), 6);
    if (k > 0) out[2] = raw_call(m & ((1u << low_bits(k)) - 1u), low_bits(k));
    if (k > 16) out[3] = raw_call(m >> 16, high_bits(k));
    n = 2 + (k > 0) + (k > 16);
  } else if (v < 0 || v >= nsym) {
    *status |= ANS_STATUS_VALUE;
    return 0;
  }
  const uint32_t lo = static_cast<uint32_t>(row[1 + sym]), hi = static_cast<uint32_t>(row[2 + sym]);
  if (hi <= lo) {
    *status |= ANS_STATUS_VALUE;
    return 0;
  }
  out[0] = Call{lo, hi - lo, prec};
  return n;
}

// The last s in [0, nsym) with cdf[s] <= slot; cdf[0] = 0 and cdf[nsym] = 2^P > slot, so it never leaves the row.
template <typename Load>
TFC_ANS_HD inline int find_symbol(Load cdf, int nsym, uint32_t slot) {
  int lo = 0, hi = nsym;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (static_cast<uint32_t>(cdf(mid)) <= slot) lo = mid; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------------------------------
// A plain serial coder of one stream, the order of DESIGN.md §28 spelled out.  rows[2 j], rows[2 j + 1] = (start of row
// j's header in `lookup`, its size); `index` null: channel mode, element i takes row i mod nrows.

inline bool valid_lanes(int lanes) { return lanes >= 1 && lanes <= ANS_MAX_LANES && (lanes & (lanes - 1)) == 0; }

// -> status (0, or ANS_STATUS_VALUE and ANS_STATUS_INDEX or-ed); an element in error is coded with no call at all.
inline int encode_stream(const int32_t* lookup, const int32_t* rows, int64_t nrows, const int32_t* index,
                         const int32_t* value, int64_t n, int lanes, std::vector<uint8_t>* out) {
  out->clear();
  int status = 0;
  if (n <= 0) return 0;
  const int64_t used = n < lanes ? n : lanes;
  std::vector<uint32_t> x(static_cast<size_t>(used), static_cast<uint32_t>(ANS_STATE_LOW));
  std::vector<uint16_t> words;                              // in emission order
  const int64_t rounds = (n + lanes - 1) / lanes;
  std::vector<Call> calls(static_cast<size_t>(lanes) * ANS_MAX_CALLS);
  std::vector<int> ncalls(static_cast<size_t>(lanes));
  for (int64_t r = rounds - 1; r >= 0; --r) {
    for (int l = 0; l < lanes; ++l) {
      const int64_t i = r * lanes + l;
      ncalls[l] = 0;
      if (i >= n) continue;
      const int64_t row = index ? index[i] : i % nrows;
      if (row < 0 || row >= nrows) {
        status |= ANS_STATUS_INDEX;
        continue;
      }
      ncalls[l] = expand(lookup + rows[2 * row], rows[2 * row + 1], value[i], &calls[l * ANS_MAX_CALLS], &status);
    }
    for (int t = ANS_MAX_CALLS - 1; t >= 0; --t)
      for (int l = lanes - 1; l >= 0; --l) {
        if (ncalls[l] <= t) continue;
        const Call& c = calls[l * ANS_MAX_CALLS + t];
        if (enc_emits(x[l], c)) {
          words.push_back(static_cast<uint16_t>(x[l]));
          x[l] >>= 16;
        }
        x[l] = enc_update(x[l], c);
      }
  }
  out->reserve(4 * used + 2 * words.size());
  for (int64_t l = 0; l < used; ++l)
    for (int b = 0; b < 4; ++b) out->push_back(static_cast<uint8_t>(x[l] >> (8 * b)));
  for (size_t k = words.size(); k-- > 0;) {
    out->push_back(static_cast<uint8_t>(words[k]));
    out->push_back(static_cast<uint8_t>(words[k] >> 8));
  }
  return status;
}

// -> ok.  Whatever the bytes are, n values are written and nothing is read outside [data, data + len).
inline bool decode_stream(const int32_t* lookup, const int32_t* rows, int64_t nrows, const int32_t* index,
                          const uint8_t* data, int64_t len, int64_t n, int lanes, int32_t* out) {
  if (n <= 0) return len == 0;
  const int64_t used = n < lanes ? n : lanes;
  bool ok = len >= 4 * used && ((len - 4 * used) & 1) == 0;
  auto byte_at = [&](int64_t k) -> uint32_t { return k < len ? data[k] : 0u; };
  std::vector<uint32_t> x(static_cast<size_t>(used));
  for (int64_t l = 0; l < used; ++l)
    x[l] = byte_at(4 * l) | byte_at(4 * l + 1) << 8 | byte_at(4 * l + 2) << 16 | byte_at(4 * l + 3) << 24;
  const int64_t nwords = len >= 4 * used ? (len - 4 * used) / 2 : 0;
  int64_t wpos = 0;
  auto refill = [&](int first, int last, const std::vector<bool>& active) {
    for (int l = first; l < last; ++l) {
      if (!active[l] || x[l] >= static_cast<uint32_t>(ANS_STATE_LOW)) continue;
      uint32_t w = 0;
      if (wpos < nwords) w = byte_at(4 * used + 2 * wpos) | byte_at(4 * used + 2 * wpos + 1) << 8;
      else ok = false;
      ++wpos;
      x[l] = dec_refill(x[l], w);
    }
  };
  const int64_t rounds = (n + lanes - 1) / lanes;
  std::vector<bool> active(static_cast<size_t>(lanes));
  std::vector<int> k(static_cast<size_t>(lanes)), sign(static_cast<size_t>(lanes));
  std::vector<uint32_t> m(static_cast<size_t>(lanes));
  std::vector<int32_t> max_value(static_cast<size_t>(lanes));
  for (int64_t r = 0; r < rounds; ++r) {
    const int cnt = static_cast<int>(n - r * lanes < lanes ? n - r * lanes : lanes);
    // sub-step 0: the table symbol
    for (int l = 0; l < cnt; ++l) {
      const int64_t i = r * lanes + l;
      active[l] = false;
      k[l] = -1;
      const int64_t row = index ? index[i] : i % nrows;
      if (row < 0 || row >= nrows) {                        // the caller's error: no call, as the encoder
        out[i] = 0;
        ok = false;
        continue;
      }
      const int32_t* p = lookup + rows[2 * row];
      const int32_t h = p[0];
      const int prec = h < 0 ? -h : h;
      const int nsym = rows[2 * row + 1] - 2;
      const uint32_t slot = dec_slot(x[l], prec);
      const int s = find_symbol([&](int j) { return p[1 + j]; }, nsym, slot);
      const Call c{static_cast<uint32_t>(p[1 + s]), static_cast<uint32_t>(p[2 + s] - p[1 + s]), prec};
      x[l] = dec_update(x[l], slot, c);
      active[l] = true;
      out[i] = s;
      max_value[l] = nsym - 1;
      if (h < 0 && s == nsym - 1) k[l] = 0;                 // escaped: the head follows
    }
    refill(0, cnt, active);
    bool any = false;
    for (int l = 0; l < cnt; ++l) any = any || k[l] >= 0;
    if (!any) continue;
    // sub-step 1: the 6-bit head
    for (int l = 0; l < cnt; ++l) {
      active[l] = k[l] >= 0;
      if (!active[l]) continue;
      const uint32_t slot = dec_slot(x[l], 6);
      x[l] = dec_update(x[l], slot, raw_call(slot, 6));
      k[l] = static_cast<int>(slot & 31u);
      sign[l] = static_cast<int>(slot >> 5);
      m[l] = 0;
    }
    refill(0, cnt, active);
    // sub-steps 2 and 3: the low and the high bits of gamma - 2^k
    for (int part = 0; part < 2; ++part) {
      for (int l = 0; l < cnt; ++l) {
        const int bits = k[l] < 0 ? 0 : (part ? high_bits(k[l]) : low_bits(k[l]));
        active[l] = bits > 0;
        if (!active[l]) continue;
        const uint32_t slot = dec_slot(x[l], bits);
        x[l] = dec_update(x[l], slot, raw_call(slot, bits));
        m[l] |= slot << (16 * part);
      }
      refill(0, cnt, active);
    }
    for (int l = 0; l < cnt; ++l)
      if (k[l] >= 0) out[r * lanes + l] = escape_value((1u << k[l]) + m[l], sign[l], max_value[l]);
  }
  if (wpos != nwords) ok = false;
  for (int64_t l = 0; l < used; ++l) ok = ok && x[l] == static_cast<uint32_t>(ANS_STATE_LOW);
  return ok;
}

}  // namespace ans
}  // namespace tfc
