// Run-length gamma / Rice codec of tensorflow/compression on gfx950: RunLengthGammaEncode/Decode
// (cc/kernels/run_length_gamma_kernels.cc), RunLengthEncode/Decode (cc/kernels/run_length_kernels.cc), bit
// format of cc/lib/bit_coder.cc (LSB-first, zero-padded last byte).  See DESIGN.md §10 for the cost model.
//
// Encoder (five launches, one host synchronisation to size the blob):
//   rl_tile_kernel      per 1024-symbol tile: last non-zero, first zero (segment scans over the flat array)
//   rl_tile_scan        one workgroup: exclusive max / reverse min scans of those over tiles
//   rl_cost_kernel      per tile: every symbol's bit cost, tile sums, in-tile prefix at each unit start
//   rl_offsets_kernel   one workgroup: scan of tile sums -> unit bit starts -> byte offsets per string
//   rl_write_kernel     per tile: recompute costs, block scan, atomic-or of the set bits into a zeroed blob
// Zero bits are never written, so long unary runs cost nothing.
//
// Decoder: a lane per string (rl_decode_kernel), or, for long strings, chunk-parallel self-synchronising
// decode: every chunk of B bits is parsed speculatively from its first bit (rl_sync_kernel, round 0), re-parsed
// from its predecessor's exit for a bounded number of rounds (rl_sync_kernel, rounds 1..R), then one wave per string repairs any chunk
// still out of step sequentially and scans the symbol counts (rl_fix_kernel), and the chunks are decoded from
// their true entry points (rl_decode_kernel again).  Errors are only raised from that last, true, parse.
#include <hip/hip_fp16.h>

#include <cstdlib>
#include <cstring>

#include "bf16_io.h"
#include "launch.h"
#include "../../include/tfc_hip.h"

namespace tfc {
namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;
constexpr int kTile = kThreads * kPer;
constexpr int64_t kSentinel = int64_t(1) << 52;   // symbol count of a chunk whose parse failed

enum : int { kOk = 0, kOutOfBits = 1, kGammaWidth = 2, kPastEnd = 3, kRiceOverflow = 4 };

struct Codes {
  int rl;      // run-length code: Rice parameter, or < 0 for gamma(r + 1)
  int mag;     // magnitude code: Rice parameter, or < 0 for gamma(|x|)
  int runs;    // use_run_length_for_non_zeros
};

// ---------------------------------------------------------------------------------------------- encoder

__device__ __forceinline__ int bitw(uint32_t v) { return 32 - __clz(v); }
__device__ __forceinline__ int64_t gamma_bits(uint32_t v) { return 2 * bitw(v) - 1; }
__device__ __forceinline__ int64_t rice_bits(uint32_t v, int k) { return int64_t(v >> k) + 1 + k; }
__device__ __forceinline__ int64_t rl_bits(uint32_t r, const Codes& c) {
  return c.rl >= 0 ? rice_bits(r, c.rl) : gamma_bits(r + 1);
}
// sign bit + magnitude code (run_length_kernels.cc WriteNonZero; INT32_MIN as 2^31 - 1 under gamma)
__device__ __forceinline__ uint32_t mag_value(int32_t x, const Codes& c) {
  if (c.mag >= 0) return x > 0 ? uint32_t(x - 1) : uint32_t(-(x + 1));
  return x > 0 ? uint32_t(x) : (x == INT32_MIN ? 0x7fffffffu : uint32_t(-x));
}

template <int D> struct In;
template <> struct In<0> { static __device__ int32_t at(const void* p, int64_t i) { return static_cast<const int32_t*>(p)[i]; } };
template <> struct In<1> { static __device__ int32_t at(const void* p, int64_t i) { return int32_t(rintf(static_cast<const float*>(p)[i])); } };
template <> struct In<2> {
  static __device__ int32_t at(const void* p, int64_t i) {
    return int32_t(rintf(bf16_bits_to_float(static_cast<const uint16_t*>(p)[i])));
  }
};
template <> struct In<3> { static __device__ int32_t at(const void* p, int64_t i) { return int32_t(rintf(__half2float(static_cast<const __half*>(p)[i]))); } };

template <int D>
__device__ __forceinline__ void load4(const void* p, int64_t i0, int64_t n, int32_t (&x)[kPer]) {
  if (D == 0 && i0 + kPer <= n && (reinterpret_cast<uintptr_t>(static_cast<const int32_t*>(p) + i0) & 15) == 0) {
    const int4 v = *reinterpret_cast<const int4*>(static_cast<const int32_t*>(p) + i0);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    return;
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j) x[j] = i0 + j < n ? In<D>::at(p, i0 + j) : 0;
}

// Block-wide exclusive scans over kThreads threads (wave64 shuffles + one LDS round).
struct ScanSmem { int64_t w[kThreads / 64]; };
template <class Op>
__device__ int64_t block_excl(int64_t v, int64_t id, Op op, bool reverse, ScanSmem& s) {
  const int tid = threadIdx.x;
  const int t = reverse ? kThreads - 1 - tid : tid;        // position in scan order
  // inclusive wave scan in scan order: in reverse order the lane order is reversed too
  const int lane = t & 63, wave = t >> 6;
  int64_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t o = reverse ? __shfl_down(inc, d, 64) : __shfl_up(inc, d, 64);
    if (lane >= d) inc = op(inc, o);
  }
  int64_t excl = reverse ? __shfl_down(inc, 1, 64) : __shfl_up(inc, 1, 64);
  if (lane == 0) excl = id;
  __syncthreads();
  if (lane == 63) s.w[wave] = inc;
  __syncthreads();
  int64_t pre = id;
  for (int k = 0; k < wave; ++k) pre = op(pre, s.w[k]);
  return op(pre, excl);
}
struct OpMax { __device__ int64_t operator()(int64_t a, int64_t b) const { return a > b ? a : b; } };
struct OpMin { __device__ int64_t operator()(int64_t a, int64_t b) const { return a < b ? a : b; } };
struct OpAdd { __device__ int64_t operator()(int64_t a, int64_t b) const { return a + b; } };

struct EncParams {
  const void* x;
  int64_t n, L, units, tiles;
  Codes c;
  int64_t* tile_last_nz;    // [tiles] -> exclusive max scan (last non-zero before the tile)
  int64_t* tile_first_z;    // [tiles] -> reverse exclusive min scan (first zero after the tile)
  int64_t* tile_bits;       // [tiles] -> exclusive scan
  int64_t* unit_local;      // [units] in-tile exclusive bit prefix at the unit's first symbol
  int64_t* offsets;         // [units + 1] byte offsets of the strings
  uint32_t* blob;
};

template <int D>
__global__ __launch_bounds__(kThreads) void rl_tile_kernel(EncParams p) {
  __shared__ ScanSmem s;
  const int64_t i0 = blockIdx.x * int64_t(kTile) + threadIdx.x * kPer;
  int32_t x[kPer];
  load4<D>(p.x, i0, p.n, x);
  int64_t last = -1, first = INT64_MAX;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (i0 + j >= p.n) break;
    if (x[j] != 0) last = i0 + j;
    else if (first == INT64_MAX) first = i0 + j;
  }
  // block reductions through the scans (inclusive = op(exclusive, own))
  const int64_t lmax = OpMax()(block_excl(last, -1, OpMax(), false, s), last);
  const int64_t fmin = OpMin()(block_excl(first, INT64_MAX, OpMin(), true, s), first);
  if (threadIdx.x == kThreads - 1) p.tile_last_nz[blockIdx.x] = lmax;
  if (threadIdx.x == 0) p.tile_first_z[blockIdx.x] = fmin;
}

// One workgroup: every thread takes a contiguous segment of the tiles.
__global__ __launch_bounds__(kThreads) void rl_tile_scan(EncParams p) {
  __shared__ ScanSmem s;
  const int64_t seg = (p.tiles + kThreads - 1) / kThreads;
  const int64_t b = threadIdx.x * seg, e = b + seg < p.tiles ? b + seg : p.tiles;
  int64_t m = -1;
  for (int64_t t = b; t < e; ++t) m = OpMax()(m, p.tile_last_nz[t]);
  int64_t run = block_excl(m, -1, OpMax(), false, s);
  for (int64_t t = b; t < e; ++t) {
    const int64_t v = p.tile_last_nz[t];
    p.tile_last_nz[t] = run;
    run = OpMax()(run, v);
  }
  if (!p.c.runs) return;
  m = INT64_MAX;
  for (int64_t t = b; t < e; ++t) m = OpMin()(m, p.tile_first_z[t]);
  run = block_excl(m, INT64_MAX, OpMin(), true, s);
  for (int64_t t = e - 1; t >= b; --t) {
    const int64_t v = p.tile_first_z[t];
    p.tile_first_z[t] = run;
    run = OpMin()(run, v);
  }
}

// The symbols of one thread with their run context.  cost(j) is symbol j's bit cost, in write order.
struct Walk {
  int64_t i0, prev0;          // first index; last non-zero before it (or < unit start)
  int64_t nz_after[kPer];     // first zero after symbol j (or >= unit end)
};

template <int D>
__device__ __forceinline__ void walk_context(const EncParams& p, ScanSmem& s, int32_t (&x)[kPer], Walk& w) {
  const int64_t i0 = blockIdx.x * int64_t(kTile) + threadIdx.x * kPer;
  w.i0 = i0;
  load4<D>(p.x, i0, p.n, x);
  int64_t last = -1, first = INT64_MAX;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (i0 + j >= p.n) break;
    if (x[j] != 0) last = i0 + j;
    else if (first == INT64_MAX) first = i0 + j;
  }
  w.prev0 = OpMax()(block_excl(last, -1, OpMax(), false, s), p.tile_last_nz[blockIdx.x]);
  int64_t after = INT64_MAX;
  if (p.c.runs) after = OpMin()(block_excl(first, INT64_MAX, OpMin(), true, s), p.tile_first_z[blockIdx.x]);
#pragma unroll
  for (int j = kPer - 1; j >= 0; --j) {
    w.nz_after[j] = after;
    if (i0 + j < p.n && x[j] == 0) after = i0 + j;
  }
}

// Visits symbol j's codes in write order: f(kind, value) with kind 0 = run-length code, 1 = sign bit,
// 2 = magnitude code.  prev is the last non-zero before the symbol, ustart / uend its unit.
template <class F>
__device__ __forceinline__ void visit(const Codes& c, int64_t i, int32_t x, int64_t prev, int64_t nzafter,
                                      int64_t ustart, int64_t uend, F&& f) {
  const bool none = prev < ustart;
  if (x != 0) {
    if (!c.runs) {
      f(0, uint32_t(none ? i - ustart : i - prev - 1));
    } else if (none || prev != i - 1) {
      const int64_t z = none ? i - ustart : i - prev - 1;
      f(0, uint32_t(z - (none ? 0 : 1)));
      const int64_t nz_end = nzafter < uend ? nzafter : uend;
      f(0, uint32_t(nz_end - i - 1));
    }
    f(1, x > 0 ? 1u : 0u);
    f(2, mag_value(x, c));
  } else if (i == uend - 1) {
    const int64_t t = none ? uend - ustart : uend - 1 - prev;
    f(0, uint32_t(t - (c.runs && !none ? 1 : 0)));
  }
}

__device__ __forceinline__ int64_t code_bits(const Codes& c, int kind, uint32_t v) {
  if (kind == 0) return rl_bits(v, c);
  if (kind == 1) return 1;
  return c.mag >= 0 ? rice_bits(v, c.mag) : gamma_bits(v);
}

template <class F>
__device__ __forceinline__ void walk(const EncParams& p, const Walk& w, const int32_t (&x)[kPer], F&& f) {
  if (w.i0 >= p.n) return;
  int64_t u = w.i0 / p.L;
  int64_t ustart = u * p.L, uend = ustart + p.L;
  int64_t prev = w.prev0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t i = w.i0 + j;
    if (i >= p.n) break;
    while (i >= uend) { ++u; ustart = uend; uend += p.L; }
    f(j, i, u, ustart, uend, prev);
    if (x[j] != 0) prev = i;
  }
}

template <int D>
__global__ __launch_bounds__(kThreads) void rl_cost_kernel(EncParams p) {
  __shared__ ScanSmem s;
  int32_t x[kPer];
  Walk w;
  walk_context<D>(p, s, x, w);
  int64_t cost[kPer] = {0, 0, 0, 0};
  int64_t sum = 0;
  walk(p, w, x, [&](int j, int64_t i, int64_t, int64_t ustart, int64_t uend, int64_t prev) {
    int64_t b = 0;
    visit(p.c, i, x[j], prev, w.nz_after[j], ustart, uend, [&](int kind, uint32_t v) { b += code_bits(p.c, kind, v); });
    cost[j] = b;
    sum += b;
  });
  int64_t pre = block_excl(sum, 0, OpAdd(), false, s);
  walk(p, w, x, [&](int j, int64_t i, int64_t u, int64_t ustart, int64_t, int64_t) {
    if (i == ustart) p.unit_local[u] = pre;
    pre += cost[j];
  });
  if (threadIdx.x == kThreads - 1) p.tile_bits[blockIdx.x] = pre;
}

// One workgroup: tile prefixes, then every string's bit length -> bytes -> exclusive byte offsets.
__global__ __launch_bounds__(kThreads) void rl_offsets_kernel(EncParams p) {
  __shared__ ScanSmem s;
  __shared__ int64_t total;
  int64_t seg = (p.tiles + kThreads - 1) / kThreads;
  int64_t b = threadIdx.x * seg, e = b + seg < p.tiles ? b + seg : p.tiles;
  int64_t m = 0;
  for (int64_t t = b; t < e; ++t) m += p.tile_bits[t];
  int64_t run = block_excl(m, 0, OpAdd(), false, s);
  for (int64_t t = b; t < e; ++t) {
    const int64_t v = p.tile_bits[t];
    p.tile_bits[t] = run;
    run += v;
  }
  if (threadIdx.x == kThreads - 1) total = run;
  __syncthreads();
  auto start = [&](int64_t u) -> int64_t {
    if (u >= p.units) return total;
    return p.tile_bits[(u * p.L) / kTile] + p.unit_local[u];
  };
  seg = (p.units + kThreads - 1) / kThreads;
  b = threadIdx.x * seg;
  e = b + seg < p.units ? b + seg : p.units;
  m = 0;
  for (int64_t u = b; u < e; ++u) m += (start(u + 1) - start(u) + 7) >> 3;
  run = block_excl(m, 0, OpAdd(), false, s);
  for (int64_t u = b; u < e; ++u) {
    p.offsets[u] = run;
    run += (start(u + 1) - start(u) + 7) >> 3;
  }
  if (threadIdx.x == kThreads - 1) p.offsets[p.units] = run;
}

__device__ __forceinline__ void or_bits(uint32_t* blob, int64_t a, uint64_t v) {
  const uint64_t sh = v << (a & 31);
  uint32_t* w = blob + (a >> 5);
  atomicOr(w, uint32_t(sh));
  if (sh >> 32) atomicOr(w + 1, uint32_t(sh >> 32));
}

template <int D>
__global__ __launch_bounds__(kThreads) void rl_write_kernel(EncParams p) {
  __shared__ ScanSmem s;
  int32_t x[kPer];
  Walk w;
  walk_context<D>(p, s, x, w);
  int64_t sum = 0;
  walk(p, w, x, [&](int j, int64_t i, int64_t, int64_t ustart, int64_t uend, int64_t prev) {
    visit(p.c, i, x[j], prev, w.nz_after[j], ustart, uend, [&](int kind, uint32_t v) { sum += code_bits(p.c, kind, v); });
  });
  int64_t g = p.tile_bits[blockIdx.x] + block_excl(sum, 0, OpAdd(), false, s);   // global bit prefix
  int64_t cur_u = -1, base = 0;
  walk(p, w, x, [&](int j, int64_t i, int64_t u, int64_t ustart, int64_t uend, int64_t prev) {
    if (u != cur_u) {   // bit address of the unit's string = its byte offset * 8 - its global bit start
      cur_u = u;
      base = p.offsets[u] * 8 - (p.tile_bits[ustart / kTile] + p.unit_local[u]);
    }
    visit(p.c, i, x[j], prev, w.nz_after[j], ustart, uend, [&](int kind, uint32_t v) {
      const int64_t a = base + g;
      if (kind == 1) {
        if (v) or_bits(p.blob, a, 1);
        g += 1;
        return;
      }
      const int k = kind == 0 ? p.c.rl : p.c.mag;
      if (k >= 0) {                               // Rice: v >> k zeros, a 1, the low k bits
        const uint32_t q = v >> k;
        const uint64_t low = k ? (uint64_t(v) & ((uint64_t(1) << k) - 1)) : 0;
        or_bits(p.blob, a + q, 1 | (low << 1));
        g += int64_t(q) + 1 + k;
      } else {                                    // gamma: w - 1 zeros, a 1, the low w - 1 bits
        const uint32_t gv = kind == 0 ? v + 1 : v;
        const int bw = bitw(gv);
        const uint64_t low = uint64_t(gv) & ((uint64_t(1) << (bw - 1)) - 1);
        or_bits(p.blob, a + bw - 1, 1 | (low << 1));
        g += 2 * bw - 1;
      }
    });
  });
}

// ---------------------------------------------------------------------------------------------- decoder

struct DecParams {
  const uint8_t* blob;
  const int64_t* offsets;     // [units + 1] bytes
  const int64_t* chunk_base;  // [units + 1] first chunk of each string (chunked family)
  int64_t units, L, chunks, chunk_bits;
  Codes c;
  int64_t* entry;             // [chunks] bit where the chunk's first record starts
  int64_t* exit;              // [chunks] first record start at or past the chunk's end
  int64_t* count;             // [chunks] symbols the chunk's records advance (kSentinel on a parse error)
  int64_t* pos;               // [chunks] exclusive scan of count per string
  int* status;                // [units] (chunk << 3) | code of the first failure; INT_MAX = OK
  void* out;
  int out_dtype;              // 0 int32, 1 float32, 2 bfloat16
};

// A reader over one string: `end` bits in all, reads past it fail.  The blob is readable 16 bytes past its end.
struct Reader {
  const uint8_t* base;    // string start
  int64_t pos, end;
  __device__ uint64_t peek() const {     // 64 bits from pos, zero past end
    if (pos >= end) return 0;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(base) * 8 + pos;
    const uint64_t* w = reinterpret_cast<const uint64_t*>((addr >> 6) << 3);
    const int sh = addr & 63;
    uint64_t v = w[0] >> sh;
    if (sh) v |= w[1] << (64 - sh);
    const int64_t left = end - pos;
    if (left < 64) v = left <= 0 ? 0 : v & ((uint64_t(1) << left) - 1);
    return v;
  }
  // zeros before the next 1, consuming the 1 (BitReader::ReadGamma / ReadRice prefix); -1 = out of bits
  __device__ int64_t unary() {
    int64_t z = 0;
    while (true) {
      const uint64_t b = peek();
      if (b) {
        const int t = __ffsll(static_cast<unsigned long long>(b)) - 1;
        pos += t + 1;
        return z + t;
      }
      const int64_t left = end - pos;
      if (left <= 64) { pos = end; return -1; }
      z += 64;
      pos += 64;
    }
  }
  __device__ bool bits(int k, uint32_t& v) {
    if (end - pos < k) return false;
    v = k ? uint32_t(peek() & ((uint64_t(1) << k) - 1)) : 0;
    pos += k;
    return true;
  }
};

__device__ __forceinline__ int read_gamma(Reader& r, uint32_t& v) {
  const int64_t z = r.unary();
  if (z < 0) return kOutOfBits;
  if (z > 30) return kGammaWidth;
  uint32_t low;
  if (!r.bits(int(z), low)) return kOutOfBits;
  v = (1u << z) | low;
  return kOk;
}
__device__ __forceinline__ int read_rice(Reader& r, int k, uint32_t& v) {
  const int64_t z = r.unary();
  if (z < 0) return kOutOfBits;
  uint32_t low;
  if (!r.bits(k, low)) return kOutOfBits;
  if (z > (int64_t(INT32_MAX) >> k)) return kRiceOverflow;       // the reference's int32 arithmetic overflows
  const int64_t val = (z << k) | low;
  if (val > INT32_MAX) return kRiceOverflow;
  v = uint32_t(val);
  return kOk;
}
__device__ __forceinline__ int read_rl(Reader& r, const Codes& c, int64_t& v) {
  uint32_t t;
  int e;
  if (c.rl >= 0) {
    e = read_rice(r, c.rl, t);
    v = t;
  } else {
    e = read_gamma(r, t);
    v = int64_t(t) - 1;
  }
  return e;
}
__device__ __forceinline__ int read_nz(Reader& r, const Codes& c, int32_t& x) {
  uint32_t sgn, m;
  if (!r.bits(1, sgn)) return kOutOfBits;
  if (c.mag >= 0) {
    if (int e = read_rice(r, c.mag, m)) return e;
    if (sgn && m == uint32_t(INT32_MAX)) return kRiceOverflow;
    x = sgn ? int32_t(m) + 1 : -int32_t(m) - 1;
  } else {
    if (int e = read_gamma(r, m)) return e;
    x = sgn ? int32_t(m) : -int32_t(m);
  }
  return kOk;
}

__device__ __forceinline__ void store(const DecParams& p, int64_t i, int32_t v) {
  if (p.out_dtype == 0) {
    static_cast<int32_t*>(p.out)[i] = v;
  } else if (p.out_dtype == 1) {
    static_cast<float*>(p.out)[i] = float(v);
  } else {
    static_cast<unsigned short*>(p.out)[i] = float_to_bf16_bits(float(v));
  }
}

// Speculative parse of the records that start in [r.pos, stop): no position bound, no output.
__device__ void parse_records(Reader& r, int64_t stop, bool first, const Codes& c, int64_t& count) {
  int64_t n = 0;
  while (r.pos < stop) {
    int64_t run;
    if (read_rl(r, c, run)) { count = kSentinel; return; }
    if (!c.runs) {
      int32_t x;
      if (read_nz(r, c, x)) { count = kSentinel; return; }
      n += run + 1;
    } else {
      int64_t m;
      if (read_rl(r, c, m)) { count = kSentinel; return; }
      for (int64_t k = 0; k <= m; ++k) {
        int32_t x;
        if (read_nz(r, c, x)) { count = kSentinel; return; }
      }
      n += run + (first ? 0 : 1) + m + 1;
    }
    first = false;
  }
  count = n;
}

// The true parse of run_length_kernels.cc RunLengthDecodeOp::Compute from (bit, symbol position), records
// starting before `stop` (all of them when last).  -> error code.
__device__ int decode_records(const DecParams& p, Reader& r, int64_t stop, bool last, bool first, int64_t q,
                              int64_t out0) {
  const Codes& c = p.c;
  const int64_t n = p.L;
  while (q < n && (last || r.pos < stop)) {
    int64_t run;
    if (int e = read_rl(r, c, run)) return e;
    q += run + (c.runs && !first ? 1 : 0);
    first = false;
    if (q >= n) return q == n ? kOk : kPastEnd;
    if (c.runs) {
      int64_t m;
      if (int e = read_rl(r, c, m)) return e;
      if (q + m + 1 > n) return kPastEnd;
      for (int64_t k = 0; k <= m; ++k) {
        int32_t x;
        if (int e = read_nz(r, c, x)) return e;
        store(p, out0 + q++, x);
      }
    } else {
      int32_t x;
      if (int e = read_nz(r, c, x)) return e;
      store(p, out0 + q++, x);
    }
  }
  return kOk;
}

__device__ __forceinline__ int64_t unit_of_chunk(const DecParams& p, int64_t ch) {
  int64_t lo = 0, hi = p.units;               // chunk_base[lo] <= ch < chunk_base[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (p.chunk_base[mid] <= ch) lo = mid; else hi = mid;
  }
  return lo;
}

// Lane per string (chunks == 0) or lane per chunk from its true entry (after rl_fix_kernel).
__global__ __launch_bounds__(kThreads) void rl_decode_kernel(DecParams p) {
  const int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x;
  if (p.chunks == 0) {
    if (t >= p.units) return;
    Reader r{p.blob + p.offsets[t], 0, (p.offsets[t + 1] - p.offsets[t]) * 8};
    const int e = decode_records(p, r, r.end, true, true, 0, t * p.L);
    if (e) p.status[t] = e;
    return;
  }
  if (t >= p.chunks) return;
  const int64_t u = unit_of_chunk(p, t);
  const int64_t q = p.pos[t];
  if (q >= p.L || p.entry[t] < 0) return;
  const int64_t local = t - p.chunk_base[u];
  const bool last = t + 1 == p.chunk_base[u + 1];
  Reader r{p.blob + p.offsets[u], p.entry[t], (p.offsets[u + 1] - p.offsets[u]) * 8};
  const int e = decode_records(p, r, (local + 1) * p.chunk_bits, last, local == 0, q, u * p.L);
  if (e) atomicMin(p.status + u, int(local << 3) | e);
}

// Round 0: every chunk from its own first bit.  Round k > 0: every chunk from its predecessor's exit.
__global__ __launch_bounds__(kThreads) void rl_sync_kernel(DecParams p, int round) {
  const int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x;
  if (t >= p.chunks) return;
  const int64_t u = unit_of_chunk(p, t);
  const int64_t local = t - p.chunk_base[u];
  int64_t start = local * p.chunk_bits;
  if (round > 0) {
    if (local == 0) return;
    start = p.exit[t - 1];
    if (start == p.entry[t]) return;
  }
  Reader r{p.blob + p.offsets[u], start, (p.offsets[u + 1] - p.offsets[u]) * 8};
  int64_t cnt;
  if (start < 0) {
    cnt = kSentinel;
    r.pos = -1;
  } else {
    parse_records(r, (local + 1) * p.chunk_bits, local == 0, p.c, cnt);
    if (cnt == kSentinel) r.pos = -1;             // nothing after a failed parse is reachable
  }
  p.entry[t] = start;
  p.exit[t] = r.pos;
  p.count[t] = cnt;
}

// One wave per string: re-parses, in order, every chunk whose entry is not its predecessor's exit, then writes
// the exclusive scan of the symbol counts.
__global__ __launch_bounds__(64) void rl_fix_kernel(DecParams p) {
  const int64_t u = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t c0 = p.chunk_base[u], c1 = p.chunk_base[u + 1];
  const int64_t end = (p.offsets[u + 1] - p.offsets[u]) * 8;
  int64_t carry_exit = 0;     // exit of the chunk before the window
  int64_t carry_pos = 0;
  for (int64_t w = c0; w < c1;) {
    const int64_t c = w + lane;
    const bool in = c < c1;
    int64_t ent = in ? p.entry[c] : 0, ex = in ? p.exit[c] : 0, cnt = in ? p.count[c] : 0;
    int64_t prev_ex = __shfl_up(ex, 1, 64);
    if (lane == 0) prev_ex = carry_exit;
    const bool bad = in && c != c0 && ent != prev_ex;
    const uint64_t mask = __ballot(bad);
    int64_t upto = 64;                        // lanes of this window that are final
    if (mask) {
      const int b = __ffsll(static_cast<unsigned long long>(mask)) - 1;
      if (lane == b) {                        // repair chunk c from its predecessor's exit, sequentially
        Reader r{p.blob + p.offsets[u], prev_ex, end};
        const int64_t local = c - c0;
        if (prev_ex < 0) {
          cnt = kSentinel;
          r.pos = -1;
        } else {
          parse_records(r, (local + 1) * p.chunk_bits, false, p.c, cnt);
          if (cnt == kSentinel) r.pos = -1;
        }
        ent = prev_ex;
        ex = r.pos;
        p.entry[c] = ent;
        p.exit[c] = ex;
        p.count[c] = cnt;
      }
      upto = b + 1;
    }
    // exclusive scan of counts over the final lanes (saturating: a failed chunk makes the rest unreachable)
    int64_t v = lane < upto && in ? cnt : 0;
    int64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t o = __shfl_up(inc, d, 64);
      if (lane >= d) inc = inc + o > kSentinel ? kSentinel : inc + o;
    }
    int64_t excl = __shfl_up(inc, 1, 64);
    if (lane == 0) excl = 0;
    const int64_t pos = carry_pos + excl;
    if (lane < upto && in) p.pos[c] = pos > kSentinel ? kSentinel : pos;
    const int last = static_cast<int>((upto < c1 - w ? upto : c1 - w) - 1);
    carry_pos = __shfl(carry_pos + inc, last, 64);
    if (carry_pos > kSentinel) carry_pos = kSentinel;
    carry_exit = __shfl(ex, last, 64);
    w += last + 1;
  }
}

__global__ void rl_status_init(int* s, int64_t n) {
  const int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (t < n) s[t] = 0x7fffffff;
}
__global__ void rl_status_final(int* s, int64_t n) {
  const int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (t < n) s[t] = s[t] == 0x7fffffff ? 0 : (s[t] & 7);
}

int check_codes(const char* who, int rl, int mag) {
  if (rl > 31 || mag > 31)
    return fail("%s: run_length_code and magnitude_code must be at most 31 (a Rice parameter above 31 is "
                "undefined in bit_coder.cc); got %d and %d", who, rl, mag);
  return 0;
}

}  // namespace
}  // namespace tfc

extern "C" int tfc_run_length_encode_size(const void* data, int dtype, int64_t units, int64_t unit_len,
                                          int run_length_code, int magnitude_code, int nonzero_runs,
                                          int64_t* workspace, int64_t* offsets, int64_t* total_bytes,
                                          void* stream) {
  using namespace tfc;
  if (int rc = check_codes("tfc_run_length_encode_size", run_length_code, magnitude_code)) return rc;
  if (dtype < 0 || dtype > 3)
    return fail("tfc_run_length_encode_size: dtype must be 0 (int32), 1 (float32), 2 (bfloat16) or 3 (float16)");
  if (units < 0 || unit_len < 0 || unit_len > INT32_MAX - 1)
    return fail("tfc_run_length_encode_size: bad shape [%lld, %lld]", (long long)units, (long long)unit_len);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n = units * unit_len;
  if (n == 0) {
    TFC_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t) * (units + 1), st));
    *total_bytes = 0;
    return 0;
  }
  EncParams p{};
  p.x = data; p.n = n; p.L = unit_len; p.units = units;
  p.tiles = (n + kTile - 1) / kTile;
  p.c = Codes{run_length_code, magnitude_code, nonzero_runs ? 1 : 0};
  p.tile_last_nz = workspace;
  p.tile_first_z = workspace + p.tiles;
  p.tile_bits = workspace + 2 * p.tiles;
  p.unit_local = workspace + 3 * p.tiles;
  p.offsets = offsets;
  const dim3 g(static_cast<unsigned>(p.tiles));
  switch (dtype) {
    case 0: hipLaunchKernelGGL(rl_tile_kernel<0>, g, dim3(kThreads), 0, st, p); break;
    case 1: hipLaunchKernelGGL(rl_tile_kernel<1>, g, dim3(kThreads), 0, st, p); break;
    case 2: hipLaunchKernelGGL(rl_tile_kernel<2>, g, dim3(kThreads), 0, st, p); break;
    default: hipLaunchKernelGGL(rl_tile_kernel<3>, g, dim3(kThreads), 0, st, p); break;
  }
  hipLaunchKernelGGL(rl_tile_scan, dim3(1), dim3(kThreads), 0, st, p);
  switch (dtype) {
    case 0: hipLaunchKernelGGL(rl_cost_kernel<0>, g, dim3(kThreads), 0, st, p); break;
    case 1: hipLaunchKernelGGL(rl_cost_kernel<1>, g, dim3(kThreads), 0, st, p); break;
    case 2: hipLaunchKernelGGL(rl_cost_kernel<2>, g, dim3(kThreads), 0, st, p); break;
    default: hipLaunchKernelGGL(rl_cost_kernel<3>, g, dim3(kThreads), 0, st, p); break;
  }
  hipLaunchKernelGGL(rl_offsets_kernel, dim3(1), dim3(kThreads), 0, st, p);
  TFC_HIP(hipGetLastError());
  TFC_HIP(hipMemcpyAsync(total_bytes, offsets + units, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  TFC_HIP(hipStreamSynchronize(st));
  return 0;
}

extern "C" int tfc_run_length_encode_write(const void* data, int dtype, int64_t units, int64_t unit_len,
                                           int run_length_code, int magnitude_code, int nonzero_runs,
                                           const int64_t* workspace, const int64_t* offsets, uint8_t* blob,
                                           void* stream) {
  using namespace tfc;
  if (int rc = check_codes("tfc_run_length_encode_write", run_length_code, magnitude_code)) return rc;
  if (dtype < 0 || dtype > 3) return fail("tfc_run_length_encode_write: bad dtype");
  if (reinterpret_cast<uintptr_t>(blob) & 3) return fail("tfc_run_length_encode_write: blob must be 4-byte aligned");
  const int64_t n = units * unit_len;
  if (n <= 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  EncParams p{};
  p.x = data; p.n = n; p.L = unit_len; p.units = units;
  p.tiles = (n + kTile - 1) / kTile;
  p.c = Codes{run_length_code, magnitude_code, nonzero_runs ? 1 : 0};
  int64_t* ws = const_cast<int64_t*>(workspace);
  p.tile_last_nz = ws;
  p.tile_first_z = ws + p.tiles;
  p.tile_bits = ws + 2 * p.tiles;
  p.unit_local = ws + 3 * p.tiles;
  p.offsets = const_cast<int64_t*>(offsets);
  p.blob = reinterpret_cast<uint32_t*>(blob);
  const dim3 g(static_cast<unsigned>(p.tiles));
  switch (dtype) {
    case 0: hipLaunchKernelGGL(rl_write_kernel<0>, g, dim3(kThreads), 0, st, p); break;
    case 1: hipLaunchKernelGGL(rl_write_kernel<1>, g, dim3(kThreads), 0, st, p); break;
    case 2: hipLaunchKernelGGL(rl_write_kernel<2>, g, dim3(kThreads), 0, st, p); break;
    default: hipLaunchKernelGGL(rl_write_kernel<3>, g, dim3(kThreads), 0, st, p); break;
  }
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t tfc_run_length_workspace(int64_t units, int64_t unit_len) {
  const int64_t n = units * unit_len;
  const int64_t tiles = (n + tfc::kTile - 1) / tfc::kTile;
  return 3 * tiles + units + 1;
}

extern "C" int tfc_run_length_decode(const uint8_t* blob, const int64_t* offsets, const int64_t* host_offsets,
                                     int64_t units, int64_t unit_len, int run_length_code, int magnitude_code,
                                     int nonzero_runs, int out_dtype, void* out, int* status, void* stream) {
  using namespace tfc;
  if (int rc = check_codes("tfc_run_length_decode", run_length_code, magnitude_code)) return rc;
  if (out_dtype < 0 || out_dtype > 2)
    return fail("tfc_run_length_decode: out_dtype must be 0 (int32), 1 (float32) or 2 (bfloat16)");
  if (units < 0 || unit_len < 0 || unit_len > INT32_MAX - 1)
    return fail("tfc_run_length_decode: bad shape [%lld, %lld]", (long long)units, (long long)unit_len);
  if (units == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t esize = out_dtype == 2 ? 2 : 4;
  if (unit_len > 0) TFC_HIP(hipMemsetAsync(out, 0, esize * units * unit_len, st));
  TFC_HIP(hipMemsetAsync(status, 0, sizeof(int) * units, st));
  if (unit_len == 0) return 0;
  DecParams p{};
  p.blob = blob; p.offsets = offsets; p.units = units; p.L = unit_len;
  p.c = Codes{run_length_code, magnitude_code, nonzero_runs ? 1 : 0};
  p.status = status; p.out = out; p.out_dtype = out_dtype;
  // family: TFC_RL_DECODER = lane | chunk forces one, else chunks when the mean string is long
  const char* fam = env_str("TFC_RL_DECODER");
  const int64_t total_bits = host_offsets[units] * 8;
  bool chunked = total_bits / units >= env_int("TFC_RL_LONG_BITS", 16384);
  if (fam && !std::strcmp(fam, "lane")) chunked = false;
  if (fam && !std::strcmp(fam, "chunk")) chunked = true;
  if (!chunked) {
    hipLaunchKernelGGL(rl_decode_kernel, dim3(static_cast<unsigned>((units + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, st, p);
    TFC_HIP(hipGetLastError());
    return 0;
  }
  int64_t B = env_int("TFC_RL_CHUNK_BITS", 1024);
  if (B < 1) B = 1;
  const int rounds = env_int("TFC_RL_SYNC_ROUNDS", 2);
  std::vector<int64_t> base(units + 1);
  base[0] = 0;
  for (int64_t u = 0; u < units; ++u) {
    const int64_t bits = (host_offsets[u + 1] - host_offsets[u]) * 8;
    base[u + 1] = base[u] + std::max<int64_t>(1, (bits + B - 1) / B);   // an empty string still has a chunk
  }
  const int64_t chunks = base[units];
  DevBuf ws;
  TFC_HIP(ws.alloc(sizeof(int64_t) * (4 * chunks + units + 1), st));
  int64_t* w = static_cast<int64_t*>(ws.p);
  p.entry = w; p.exit = w + chunks; p.count = w + 2 * chunks; p.pos = w + 3 * chunks;
  p.chunk_base = w + 4 * chunks;
  p.chunks = chunks; p.chunk_bits = B;
  TFC_HIP(hipMemcpyAsync(const_cast<int64_t*>(p.chunk_base), base.data(), sizeof(int64_t) * (units + 1),
                         hipMemcpyHostToDevice, st));
  const unsigned cg = static_cast<unsigned>((chunks + kThreads - 1) / kThreads);
  for (int k = 0; k <= rounds; ++k) hipLaunchKernelGGL(rl_sync_kernel, dim3(cg), dim3(kThreads), 0, st, p, k);
  hipLaunchKernelGGL(rl_fix_kernel, dim3(static_cast<unsigned>(units)), dim3(64), 0, st, p);
  const unsigned ug = static_cast<unsigned>((units + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(rl_status_init, dim3(ug), dim3(kThreads), 0, st, status, units);
  hipLaunchKernelGGL(rl_decode_kernel, dim3(cg), dim3(kThreads), 0, st, p);
  hipLaunchKernelGGL(rl_status_final, dim3(ug), dim3(kThreads), 0, st, status, units);
  TFC_HIP(hipGetLastError());
  TFC_HIP(hipStreamSynchronize(st));    // the host copy of chunk_base must outlive the copy
  return 0;
}
