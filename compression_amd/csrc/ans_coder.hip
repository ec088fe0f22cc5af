// Interleaved rANS over the coder's lookup tables (ans_core.h): one wave per stream, the wave's lanes
// are the stream's coder states, so one step codes `lanes` consecutive elements where a range coder codes one.
//   encode: per round (descending) every lane expands its element into at most four calls; the sub-steps run in
//           reverse.  The emitters of a sub-step are one ballot, their places a lane-mask count; the words go backwards
//           into a per-stream slab sized for the worst case, a second launch packs states and words into blob + offsets.
//   decode: every lane takes its slot and searches its own row (lanes have different rows in index mode): in LDS where
//           the raw tables fit (table_lds_bytes), through L2 otherwise.  The words of a sub-step are handed out by a
//           ballot and a prefix count from a window of kWindowBlocks blocks of 64 words, one register per block;
//           sub-steps 1-3 run only in a round in which some lane escaped.
// Bounded by construction: a word behind the end of a string reads as zero, the search cannot leave its row
// (find_symbol), a stream_index outside the layout writes its verdict only.  The arithmetic is ans_core.h's; nothing
// of it is restated here.  No scratch.
#include <hip/hip_runtime.h>

#include "../../include/tfc_hip.h"
#include "ans_core.h"
#include "common.h"
#include "launch.h"
#include "range_tables.h"

namespace tfc {
namespace {

using namespace ans;

constexpr int kWavesPerBlock = 4;       // one wave per stream; a block stages the tables once for its four
constexpr int kBlock = kWavesPerBlock * 64;
constexpr long long kMaxStreams = 1ll << 23;
constexpr long long kMaxElems = 1ll << 27;
// The decoder's word window in blocks of 64 words (WordReader).
constexpr int kWindowBlocks = 4;

struct AnsParams {
  const int32_t* data;          // the raw lookup
  const int2* rows;             // (header, ints) per row
  int ntab, total;
  const int32_t* index;         // [streams, elems] or null (channel mode)
  long long streams;
  int elems, lanes;
  // encode
  const int32_t* value;         // [streams, elems]
  uint8_t* slabs;               // [streams][cap]: states in front, words at the end
  long long cap;
  unsigned int* lens;           // [streams]
  int32_t* status;              // [streams]
  // decode
  const uint8_t* blob;
  const int64_t* offsets;       // [nstrings + 1]
  const int32_t* stream_index;  // [nstrings] or null
  long long nstrings;
  int32_t* out;                 // [streams, elems]
  uint8_t* ok;                  // [nstrings]
};

__device__ inline int lanes_below(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<unsigned int>(m >> 32),
                                   __builtin_amdgcn_mbcnt_lo(static_cast<unsigned int>(m), 0u));
}

__global__ void __launch_bounds__(kBlock) ans_enc_kernel(AnsParams p) {
  const int lane = threadIdx.x & 63;
  const long long s = static_cast<long long>(blockIdx.x) * kWavesPerBlock +
                      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  if (s >= p.streams) return;
  const int n = p.elems, W = p.lanes;
  const long long at0 = s * n;
  uint16_t* slab = reinterpret_cast<uint16_t*>(p.slabs + s * p.cap);
  const int used = min(n, W);
  const long long first_word = 2ll * used;                  // the states' place
  long long wp = p.cap / 2;                                  // words are written below wp
  uint32_t x = static_cast<uint32_t>(ANS_STATE_LOW);
  int status = 0;
  bool over = false;
  const int rounds = (n + W - 1) / W;
  for (int r = rounds - 1; r >= 0; --r) {
    const int i = r * W + lane;
    Call c[ANS_MAX_CALLS];
#pragma unroll
    for (int t = 0; t < ANS_MAX_CALLS; ++t) c[t] = Call{0u, 1u, 1};
    int nc = 0;
    if (lane < W && i < n) {
      const int row = p.index ? p.index[at0 + i] : static_cast<int>(static_cast<unsigned int>(i) %
                                                                    static_cast<unsigned int>(p.ntab));
      if (row < 0 || row >= p.ntab) {
        status |= ANS_STATUS_INDEX;
      } else {
        const int2 rw = p.rows[row];
        nc = expand(p.data + rw.x, rw.y, p.value[at0 + i], c, &status);
      }
    }
#pragma unroll
    for (int t = ANS_MAX_CALLS - 1; t >= 0; --t) {
      const bool act = nc > t;
      if (!__any(act)) continue;
      const bool emit = act && enc_emits(x, c[t]);
      const unsigned long long m = __ballot(emit);
      if (m) {
        // emission runs from the highest lane down and the string holds the words in reverse: the lowest emitter's word
        // comes first
        wp -= __popcll(m);
        if (wp < first_word) over = true;
        else if (emit) slab[wp + lanes_below(m)] = static_cast<uint16_t>(x);
        if (emit) x >>= 16;
      }
      if (act) x = enc_update(x, c[t]);
    }
  }
  if (lane < used) reinterpret_cast<uint32_t*>(slab)[lane] = x;
  const unsigned long long bad_value = __ballot(status & ANS_STATUS_VALUE);
  const unsigned long long bad_index = __ballot(status & ANS_STATUS_INDEX);
  if (lane == 0) {
    p.lens[s] = over ? 0xFFFFFFFFu : static_cast<unsigned int>(4ll * used + 2 * (p.cap / 2 - wp));
    p.status[s] = (bad_value ? ANS_STATUS_VALUE : 0) | (bad_index ? ANS_STATUS_INDEX : 0);
  }
}

// Block b of a string's words: lane j holds word 64 b + j, zero behind the words' end; byte loads: a string starts
// wherever the one in front of it ended.
__device__ inline uint32_t block_words(const uint8_t* words, long long nwords, int block, int lane) {
  const long long k = 64ll * block + lane;
  return k < nwords ? words[2 * k] | static_cast<uint32_t>(words[2 * k + 1]) << 8 : 0u;
}

// The decoder's word window: the block the read position is in and the three behind it (kWindowBlocks blocks of 64
// words).  A sub-step takes at most 64 words, so it reads the first two; the fourth is requested when the position
// enters a new block and first moved one block later, which is what hides its load.
struct WordReader {
  const uint8_t* words;
  long long nwords;
  int pos, block;               // wave-uniform: the next word to hand out, the block it is in
  uint32_t b0, b1, b2, b3;
  bool missing;
};

// The lanes with `need` take the next words in ascending lane order.  Called by the whole wave.
__device__ inline void take_words(WordReader& w, bool need, uint32_t& x, int lane) {
  const unsigned long long m = __ballot(need);
  if (!m) return;
  const int at = w.pos + lanes_below(m);
  const int from = (at & 63) << 2;
  const uint32_t w0 = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(from, static_cast<int>(w.b0)));
  const uint32_t w1 = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(from, static_cast<int>(w.b1)));
  if (need) {
    w.missing |= at >= w.nwords;
    x = dec_refill(x, (at >> 6) == w.block ? w0 : w1);
  }
  w.pos += __popcll(m);
  if ((w.pos >> 6) != w.block) {                            // at most one block further: a take is 64 words at most
    ++w.block;
    w.b0 = w.b1;
    w.b1 = w.b2;
    w.b2 = w.b3;
    w.b3 = block_words(w.words, w.nwords, w.block + kWindowBlocks - 1, lane);
  }
}

template <bool kLds>
__global__ void __launch_bounds__(kBlock) ans_dec_kernel(AnsParams p) {
  extern __shared__ __attribute__((aligned(16))) int32_t tab[];
  if (kLds) {
    const int quads = p.total >> 2;                         // (both ends are 16-byte aligned)
    for (int i = threadIdx.x; i < quads; i += kBlock)
      reinterpret_cast<int4*>(tab)[i] = reinterpret_cast<const int4*>(p.data)[i];
    for (int i = 4 * quads + threadIdx.x; i < p.total; i += kBlock) tab[i] = p.data[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const long long j = static_cast<long long>(blockIdx.x) * kWavesPerBlock +
                      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  if (j >= p.nstrings) return;
  const long long s = p.stream_index ? static_cast<long long>(p.stream_index[j]) : j;
  if (s < 0 || s >= p.streams) {                            // no such stream: nothing is written but the verdict
    if (lane == 0) p.ok[j] = 0;
    return;
  }
  const uint8_t* src = p.blob + p.offsets[j];
  const long long len = max<long long>(p.offsets[j + 1] - p.offsets[j], 0);
  const int n = p.elems, W = p.lanes;
  if (n == 0) {
    if (lane == 0) p.ok[j] = len == 0;
    return;
  }
  const long long at0 = s * n;
  const int used = min(n, W);
  const bool framed = len >= 4ll * used && ((len - 4ll * used) & 1) == 0;
  uint32_t x = 0;
  if (lane < used)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (4ll * lane + b < len) x |= static_cast<uint32_t>(src[4 * lane + b]) << (8 * b);
  WordReader w;
  w.words = src + 4 * used;
  w.nwords = len >= 4ll * used ? (len - 4ll * used) >> 1 : 0;
  w.pos = 0;
  w.block = 0;
  w.missing = false;
  w.b0 = block_words(w.words, w.nwords, 0, lane);
  w.b1 = block_words(w.words, w.nwords, 1, lane);
  w.b2 = block_words(w.words, w.nwords, 2, lane);
  w.b3 = block_words(w.words, w.nwords, 3, lane);

  auto entry = [&](int at) -> int32_t { return kLds ? tab[at] : p.data[at]; };
  // the row of element i; -1: the index names none
  auto row_of = [&](int i) -> int {
    if (!(lane < W && i < n)) return -1;
    if (!p.index) return static_cast<int>(static_cast<unsigned int>(i) % static_cast<unsigned int>(p.ntab));
    const int row = p.index[at0 + i];
    return row < 0 || row >= p.ntab ? -1 : row;
  };
  bool bad = false;
  const int rounds = (n + W - 1) / W;
  // two rounds ahead: the index; one round ahead: the row's place
  int row_next = row_of(lane);
  int2 rw_next = p.rows[max(row_next, 0)];
  int row_after = row_of(W + lane);
  for (int r = 0; r < rounds; ++r) {
    const int i = r * W + lane;
    const bool act = lane < W && i < n;
    const int row = row_next;
    const int2 rw = rw_next;
    row_next = row_after;
    rw_next = p.rows[max(row_next, 0)];
    row_after = row_of(i + 2 * W);
    int32_t v = 0, max_value = 0;
    bool esc = false, need = false;
    if (act && row < 0) bad = true;
    if (act && row >= 0) {
      const int32_t h = entry(rw.x);
      const int prec = h < 0 ? -h : h;
      const int nsym = rw.y - 2;
      const uint32_t slot = dec_slot(x, prec);
      v = find_symbol([&](int k) { return entry(rw.x + 1 + k); }, nsym, slot);
      const uint32_t lo = static_cast<uint32_t>(entry(rw.x + 1 + v)), hi = static_cast<uint32_t>(entry(rw.x + 2 + v));
      x = dec_update(x, slot, Call{lo, hi - lo, prec});
      max_value = nsym - 1;
      esc = h < 0 && v == max_value;
      need = x < static_cast<uint32_t>(ANS_STATE_LOW);
    }
    take_words(w, need, x, lane);
    if (__any(esc)) {
      int k = 0, sign = 0;
      uint32_t m = 0;
      if (esc) {                                            // sub-step 1: the 6-bit head
        const uint32_t slot = dec_slot(x, 6);
        x = dec_update(x, slot, raw_call(slot, 6));
        k = static_cast<int>(slot & 31u);
        sign = static_cast<int>(slot >> 5);
      }
      take_words(w, esc && x < static_cast<uint32_t>(ANS_STATE_LOW), x, lane);
      const bool low = esc && k > 0;                        // sub-step 2: the low bits of gamma - 2^k
      if (low) {
        const uint32_t slot = dec_slot(x, low_bits(k));
        x = dec_update(x, slot, raw_call(slot, low_bits(k)));
        m = slot;
      }
      take_words(w, low && x < static_cast<uint32_t>(ANS_STATE_LOW), x, lane);
      const bool high = esc && k > 16;                      // sub-step 3: the bits above them
      if (__any(high)) {
        if (high) {
          const uint32_t slot = dec_slot(x, high_bits(k));
          x = dec_update(x, slot, raw_call(slot, high_bits(k)));
          m |= slot << 16;
        }
        take_words(w, high && x < static_cast<uint32_t>(ANS_STATE_LOW), x, lane);
      }
      if (esc) v = escape_value((1u << k) + m, sign, max_value);
    }
    if (act) p.out[at0 + i] = v;
  }
  const bool lane_good = !bad && !w.missing && (lane >= used || x == static_cast<uint32_t>(ANS_STATE_LOW));
  const unsigned long long all_good = __ballot(lane_good);
  if (lane == 0) p.ok[j] = (framed && all_good == ~0ull && w.pos == w.nwords) ? 1 : 0;
}

// offsets[0 .. n] = exclusive sums of lens (an overflowed stream counts as empty and raises *bad); one block.
__global__ void __launch_bounds__(256) ans_offsets_kernel(const unsigned int* lens, long long n, int64_t* offsets,
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

// string s: the states in front of its slab, then the words at the slab's end -> blob + offsets[s]; one block per string
__global__ void __launch_bounds__(256) ans_pack_kernel(const uint8_t* slabs, long long cap, int state_bytes,
                                                       const int64_t* offsets, uint8_t* blob) {
  const long long s = blockIdx.x;
  const long long n = min<long long>(offsets[s + 1] - offsets[s], cap);
  const uint8_t* src = slabs + s * cap;
  uint8_t* dst = blob + offsets[s];
  const long long shift = cap - n;                          // a word's byte i of the string sits at i + shift
  for (long long i = threadIdx.x; i < n; i += 256) dst[i] = src[i < state_bytes ? i : i + shift];
}

long long slab_bytes(long long elems, int lanes) {
  return 2ll * ANS_MAX_CALLS * elems + 4ll * std::min<long long>(elems, lanes);
}

int check_sizes(const char* who, int64_t streams, int64_t elems, int lanes) {
  if (!valid_lanes(lanes)) return fail("%s: lanes must be a power of two in [1, %d] (got %d)", who, ANS_MAX_LANES, lanes);
  if (streams < 0 || streams > kMaxStreams)
    return fail("%s: streams must be in [0, %lld] (got %lld)", who, kMaxStreams, static_cast<long long>(streams));
  if (elems < 0 || elems > kMaxElems)
    return fail("%s: elems must be in [0, %lld] (got %lld)", who, kMaxElems, static_cast<long long>(elems));
  return 0;
}

int fill_common(const char* who, const tfc_tables* tables, const int32_t* index, int64_t streams, int64_t elems,
                int lanes, AnsParams* p) {
  if (int rc = check_sizes(who, streams, elems, lanes)) return rc;
  if (!tables) return fail("%s: null tables", who);
  if (elems > 0 && tables->rows.empty()) return fail("%s: the lookup has no row", who);
  p->data = tables->d_data.as<int32_t>();
  p->rows = tables->d_rows.as<int2>();
  p->ntab = static_cast<int>(tables->rows.size());
  p->total = static_cast<int>(tables->host.size());
  p->index = index;
  p->streams = streams;
  p->elems = static_cast<int>(elems);
  p->lanes = lanes;
  return 0;
}

}  // namespace
}  // namespace tfc

using namespace tfc;

extern "C" int64_t tfc_ans_blob_capacity(int64_t streams, int64_t elems, int lanes) {
  if (check_sizes("tfc_ans_blob_capacity", streams, elems, lanes)) return -1;
  return streams * slab_bytes(elems, lanes);
}

extern "C" int tfc_ans_encode(const tfc_tables* tables, const int32_t* index, const int32_t* value, int64_t streams,
                              int64_t elems, int lanes, uint8_t* blob, int64_t* offsets, uint32_t* overflow,
                              int32_t* status, void* stream) {
  const char* who = "tfc_ans_encode";
  AnsParams p{};
  if (int rc = fill_common(who, tables, index, streams, elems, lanes, &p)) return rc;
  if (!offsets || !overflow) return fail("%s: null output pointer", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  TFC_HIP(hipMemsetAsync(overflow, 0, sizeof(uint32_t), st));
  if (streams == 0) {
    TFC_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t), st));
    return 0;
  }
  if (!status) return fail("%s: null status pointer", who);
  if (elems == 0) {
    TFC_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t) * (streams + 1), st));
    TFC_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * streams, st));
    return 0;
  }
  if (!value || !blob) return fail("%s: null pointer", who);
  p.value = value;
  p.cap = slab_bytes(elems, lanes);
  p.status = status;
  DevBuf slabs, lens;
  TFC_HIP(slabs.alloc(static_cast<size_t>(streams) * p.cap, st));
  TFC_HIP(lens.alloc(sizeof(unsigned int) * streams, st));
  p.slabs = slabs.as<uint8_t>();
  p.lens = lens.as<unsigned int>();
  {
    KernelTimer timer("ans_encode", st);
    hipLaunchKernelGGL(ans_enc_kernel, dim3(static_cast<unsigned>(ceil_div(streams, kWavesPerBlock))), dim3(kBlock), 0,
                       st, p);
  }
  hipLaunchKernelGGL(ans_offsets_kernel, dim3(1), dim3(256), 0, st, p.lens, static_cast<long long>(streams), offsets,
                     overflow);
  hipLaunchKernelGGL(ans_pack_kernel, dim3(static_cast<unsigned>(streams)), dim3(256), 0, st, p.slabs, p.cap,
                     4 * static_cast<int>(std::min<int64_t>(elems, lanes)), offsets, blob);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_ans_decode(const tfc_tables* tables, const uint8_t* blob, const int64_t* offsets,
                              const int32_t* stream_index, int64_t nstrings, const int32_t* index, int64_t streams,
                              int64_t elems, int lanes, int32_t* out, uint8_t* ok, void* stream) {
  const char* who = "tfc_ans_decode";
  AnsParams p{};
  if (int rc = fill_common(who, tables, index, streams, elems, lanes, &p)) return rc;
  if (nstrings < 0 || nstrings > kMaxStreams)
    return fail("%s: nstrings must be in [0, %lld] (got %lld)", who, kMaxStreams, static_cast<long long>(nstrings));
  if (!stream_index && nstrings != streams)
    return fail("%s: %lld strings for %lld streams and no stream_index", who, static_cast<long long>(nstrings),
                static_cast<long long>(streams));
  if (nstrings == 0) return 0;
  if (!blob || !offsets || !ok || (elems > 0 && !out)) return fail("%s: null pointer", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  p.blob = blob;
  p.offsets = offsets;
  p.stream_index = stream_index;
  p.nstrings = nstrings;
  p.out = out;
  p.ok = ok;
  const size_t lds = elems > 0 ? table_lds_bytes(tables) : 0;
  KernelTimer timer("ans_decode", st);
  const dim3 grid(static_cast<unsigned>(ceil_div(nstrings, kWavesPerBlock)));
  if (lds) return launch(ans_dec_kernel<true>, grid, dim3(kBlock), lds, st, p);
  return launch(ans_dec_kernel<false>, grid, dim3(kBlock), 0, st, p);
}
