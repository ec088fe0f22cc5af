// Multi-stream range coder for gfx950 (MI355X): one 64-lane wavefront per code
// stream.
//
// What runs where
//   * The arithmetic of one stream is a strict chain (every interval update
//     needs the previous span), so parallelism = number of streams.  Each
//     stream gets a whole wave; the wave's 64 lanes do everything that is NOT
//     on the chain in parallel — coalesced symbol loads, CDF gathers from the
//     LDS-resident table, escape detection, the decoder's CDF search
//     (64 candidate symbols per compare + ballot), byte-window refills and
//     coalesced output stores — while the chain itself runs on wave-uniform
//     values that hipcc keeps in scalar registers.
//   * Output is append-only 16-bit digits (the delayed-carry scheme never
//     rewrites emitted bytes), collected 64 at a time in one VGPR via
//     v_writelane and flushed as one coalesced 128-byte store.
//
// Behaviour follows (bit-exact, checked by tests/ against oracle/):
//   cc/lib/range_coder.cc:37-307, cc/lib/range_coder.h:79-282,
//   cc/kernels/range_coder_kernels.cc:101-471.
//
// This unit: the encoder and decoder handles and every kernel they launch (the kernel headers included below
// stay here with them: kernels of both sides write the __device__ counters that one host function reads, and the
// library has no relocatable device code).  The wave-per-stream device primitives are in range_wave.h, the
// tables and their image builders in range_tables.h / range_tables.hip, the deprecated single-stream ops in
// range_coder_legacy.hip, the library's error and timing plumbing in runtime.hip.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tfc_hip.h"
#include "launch.h"
#include "range_coder_device.h"
#include "range_plan.h"
#include "range_tables.h"
#include "range_wave.h"

using namespace tfc;

// ===========================================================================
// Kernels
// ===========================================================================

namespace tfc {

struct EncParams {
  TableView tab;
  const int32_t* index;     // null => channel mode
  int64_t streams;
  int64_t elems;
  // outputs of the counting pass / inputs of the coding pass
  unsigned long long* calls;        // [streams]
  unsigned long long* first_error;  // [1], linear position of the first range error
  // coding pass
  uint4* state;                     // [streams] base, span_m1, pend_digit, pend_bytes
  uint8_t* chunk;
  const long long* chunk_off;       // [streams + 1]
  unsigned int* chunk_len;          // [streams]
  unsigned int* overflow_flag;      // [1]
  // deferred-error handles (no read-back between the counting and the coding pass): the coding pass
  // itself looks at the counting pass's verdict — guard[0] = first range error (~0 = none), guard[1] =
  // bytes the per-stream slabs need — and appends nothing if there was an error or the slab the host
  // sized without knowing the data is too small (then it raises the overflow flag).  null: checked by the host.
  const unsigned long long* guard;
  unsigned long long cap_total;
};

// true: this call appends nothing (see EncParams::guard); the stream's piece gets length 0
__device__ inline bool enc_guard_skips(const EncParams& p, int64_t s, int lane) {
  if (!p.guard) return false;
  const unsigned long long err = p.guard[0], need = p.guard[1];
  if (err == ~0ull && need <= p.cap_total) return false;
  if (lane == 0) {
    p.chunk_len[s] = 0u;
    if (need > p.cap_total) atomicOr(p.overflow_flag, 1u);
  }
  return true;
}

// Counting + validation pass: fully parallel and HBM-bound (one coalesced read of the
// symbols).  Only the row's symbol count and escape flag are needed, so they are staged in
// LDS ((nsym << 1) | escape per table) instead of gathering table entries.
constexpr int kCountTile = 4096;      // elements of one stream per workgroup
constexpr int kCountLdsRows = 8192;

template <typename Src>
__global__ void __launch_bounds__(256) enc_count_kernel(EncParams p, Src src) {
  // rowinfo[min(ntab, kCountLdsRows)], sized at launch: this kernel runs beside the coding kernels of
  // other steps, and LDS it does not need is LDS their workgroups cannot get
  extern __shared__ int rowinfo[];
  __shared__ unsigned int part[4];
  const bool in_lds = p.tab.ntab <= kCountLdsRows;
  if (in_lds) {
    for (int i = threadIdx.x; i < p.tab.ntab; i += 256) {
      const int2 r = p.tab.rows[i];
      rowinfo[i] = ((r.y - 2) << 1) | (p.tab.data[r.x] < 0 ? 1 : 0);
    }
    __syncthreads();
  }
  const int64_t tiles = (p.elems + kCountTile - 1) / kCountTile;
  const int64_t s = blockIdx.x / tiles;
  const int64_t j0 = (blockIdx.x % tiles) * kCountTile;
  const unsigned int ntab = static_cast<unsigned int>(p.tab.ntab);
  unsigned int ch = static_cast<unsigned int>((j0 + threadIdx.x) % ntab);
  const unsigned int step = 256u % ntab;
  unsigned int calls = 0;
  for (int k = 0; k < kCountTile / 256; ++k) {
    const int64_t j = j0 + k * 256 + threadIdx.x;
    if (j < p.elems) {
      const int64_t pos = s * p.elems + j;
      int t = static_cast<int>(ch);
      bool bad = false;
      if (p.index) {
        t = p.index[pos];
        if (t < 0 || t >= p.tab.ntab) { bad = true; t = 0; }
      }
      int info;
      if (in_lds) {
        info = rowinfo[t];
      } else {
        const int2 r = p.tab.rows[t];
        info = ((r.y - 2) << 1) | (p.tab.data[r.x] < 0 ? 1 : 0);
      }
      const int nsym = info >> 1;
      const int32_t v = src.load(pos, t);
      unsigned int c = 1;
      if (info & 1) {
        const int vmax = nsym - 1;                  // last interval is the escape symbol
        const int gamma = v < 0 ? -v : (v >= vmax ? v - vmax + 1 : 0);
        if (gamma > 0) c += escape_calls(gamma);
      } else if (v < 0 || v >= nsym) {
        bad = true;
      }
      if (bad) atomicMin(p.first_error, static_cast<unsigned long long>(pos));
      calls += c;
    }
    ch += step;
    if (ch >= ntab) ch -= ntab;
  }
  for (int off = 32; off > 0; off >>= 1) calls += __shfl_down(calls, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = calls;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int tot = part[0] + part[1] + part[2] + part[3];
    atomicAdd(&p.calls[s], static_cast<unsigned long long>(tot));
    atomicAdd(p.first_error + 2, static_cast<unsigned long long>(tot));   // status[2]: calls of all streams
  }
}

// calls[s] -> byte capacity 2*calls + 4 rounded to 16, exclusive scan -> off.
__global__ void enc_offsets_kernel(const unsigned long long* calls, const uint4* state,
                                   int held_digits, int64_t streams,
                                   long long* off, unsigned long long* total) {
  // single block; streams is usually 1e2..1e5
  __shared__ long long carry;
  __shared__ long long tmp[1024];
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < streams; base += 1024) {
    const int64_t i = base + threadIdx.x;
    long long cap = 0;
    if (i < streams) {
      // 2 bytes per coder call, plus (fast kernels) the digits the previous calls held back
      long long digits = static_cast<long long>(calls[i]);
      if (held_digits) digits += 1 + static_cast<long long>(state[i].w);
      cap = ((2 * digits + 4 + 15) / 16) * 16;
    }
    tmp[threadIdx.x] = cap;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      long long v = threadIdx.x >= d ? tmp[threadIdx.x - d] : 0;
      __syncthreads();
      tmp[threadIdx.x] += v;
      __syncthreads();
    }
    if (i < streams) off[i] = carry + tmp[threadIdx.x] - cap;
    __syncthreads();
    if (threadIdx.x == 1023) carry += tmp[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    off[streams] = carry;
    *total = static_cast<unsigned long long>(carry);
  }
}

template <bool LDS_TAB, typename Src>
__global__ void __launch_bounds__(kBlock) enc_kernel(EncParams p, Src src) {
  extern __shared__ int32_t lds_tab[];
  if (LDS_TAB) {
    for (int i = threadIdx.x; i < p.tab.total; i += kBlock) lds_tab[i] = p.tab.data[i];
    __syncthreads();
  }
  auto T = [&](int i) -> int32_t { return LDS_TAB ? lds_tab[i] : p.tab.data[i]; };

  const int lane = threadIdx.x & 63;
  const int64_t s = __builtin_amdgcn_readfirstlane(
      static_cast<int>(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
  if (s >= p.streams) return;
  if (enc_guard_skips(p, s, lane)) return;

  const uint4 st0 = p.state[s];
  EncoderState st;
  st.base = __builtin_amdgcn_readfirstlane(st0.x);
  st.span_m1 = __builtin_amdgcn_readfirstlane(st0.y);
  st.pend_digit = __builtin_amdgcn_readfirstlane(st0.z);
  st.pend_bytes = __builtin_amdgcn_readfirstlane(st0.w);

  DigitSink o;
  const long long off0 = p.chunk_off[s];
  o.dst = p.chunk + off0;
  o.cap = static_cast<unsigned int>(p.chunk_off[s + 1] - off0);
  o.nbytes = 0;
  o.n = 0;
  o.reg = 0;
  o.overflow = 0;

  for (int64_t j0 = 0; j0 < p.elems; j0 += 64) {
    // ---- vector phase: 64 symbols at once --------------------------------
    const int64_t j = j0 + lane;
    Call c;
    c.lo16 = 0; c.hi16 = 0; c.gamma = 0; c.neg = 0; c.bad = 0;
    if (j < p.elems) {
      const int64_t pos = s * p.elems + j;
      int t = p.index ? p.index[pos] : static_cast<int>(j % p.tab.ntab);
      t = min(max(t, 0), p.tab.ntab - 1);  // range errors were reported by the counting pass
      const int2 row = p.tab.rows[t];
      c = classify(T, row, src.load(pos, t));
    }
    const unsigned long long esc_mask = __ballot(c.gamma > 0);
    const int cnt = static_cast<int>(min<int64_t>(64, p.elems - j0));
    // ---- serial phase: the chain -----------------------------------------
    for (int n = 0; n < cnt; ++n) {
      const unsigned int lo = __builtin_amdgcn_readlane(c.lo16, n);
      const unsigned int hi = __builtin_amdgcn_readlane(c.hi16, n);
      enc_update(st, lo, hi, o, lane);
      if ((esc_mask >> n) & 1) {
        const int g = __builtin_amdgcn_readlane(c.gamma, n);
        const int neg = __builtin_amdgcn_readlane(c.neg, n);
        int nb = 31 - __clz(g);             // floor(log2 g)
        for (int k = 0; k < nb; ++k) enc_update(st, 0, 0x8000u, o, lane);   // zeros
        for (int k = nb; k >= 0; --k) {
          const unsigned int bit = (g >> k) & 1;
          enc_update(st, bit << 15, (bit + 1) << 15, o, lane);
        }
        enc_update(st, static_cast<unsigned int>(neg) << 15,
                   static_cast<unsigned int>(neg + 1) << 15, o, lane);
      }
    }
  }
  sink_flush(o, lane);
  if (lane == 0) {
    p.state[s] = make_uint4(st.base, st.span_m1, st.pend_digit, st.pend_bytes);
    p.chunk_len[s] = o.nbytes;
    if (o.overflow) atomicOr(p.overflow_flag, 1u);
  }
}

}  // namespace tfc
#include "range_encoder_fast.h"
namespace tfc {

// ---- finalize -------------------------------------------------------------

struct ChunkRef {
  const uint8_t* data;
  const long long* off;      // start of every stream's piece, or null: stream s starts at s * stride
  const unsigned int* len;
  long long stride;
};
__device__ inline const uint8_t* chunk_piece(const ChunkRef& c, int64_t s) {
  return c.data + (c.off ? c.off[s] : s * c.stride);
}
// The pieces of a handle travel to the finalize kernels BY VALUE (kernel arguments are captured at
// launch): an asynchronous copy from a host vector would still be reading it after a stream-ordered
// finalize has returned.  Handles with more encode calls than this take a synchronising copy.
constexpr int kInlineChunks = 8;
struct ChunkList {
  ChunkRef inline_refs[kInlineChunks];
  const ChunkRef* more;      // all of them, when there are more than kInlineChunks
  int n;
  __device__ const ChunkRef& operator[](int i) const { return more ? more[i] : inline_refs[i]; }
};

// Tail of every stream per RangeEncoder::Finalize (range_coder.cc:266-307); one
// thread per stream.  tail[s] = {head bytes (<= 2), 0xFFFF digits to insert,
// end bytes (<= 2)}; also sums the stream's total length.
//   generic kernels:        state = (base, span-1, delay digit + 1, delayed bytes)
//   fast and lane kernels:  state = (base, span-1, valid<<31 | held digit, held 0xFFFF run)
struct Tail {
  unsigned char head[2];
  unsigned char end[2];
  unsigned int nhead, nend, run;
};

__device__ inline void enc_tail_one(const uint4* state, int64_t streams, const ChunkList& chunks,
                                    int nchunks, int fast_state, Tail* tail, long long* length) {
  const int64_t s = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (s >= streams) return;
  const uint4 st = state[s];
  Tail t;
  t.nhead = t.nend = t.run = 0;
  t.head[0] = t.head[1] = t.end[0] = t.end[1] = 0;
  const bool state1 = static_cast<unsigned int>(st.x + st.y) < st.x;   // carry still undecided
  unsigned int delay = 0;                                              // reference's delay_ & 0xFFFF
  if (fast_state) {
    if (state1) {
      delay = (st.z & 0xFFFFu) + 1u;
    } else if (st.z >> 31) {
      t.head[0] = (st.z >> 8) & 0xFF;
      t.head[1] = st.z & 0xFF;
      t.nhead = 2;
      t.run = st.w;
    }
  } else {
    delay = st.z;
  }
  if (delay != 0) {
    t.end[0] = (delay >> 8) & 0xFF;
    t.nend = 1;
    if ((delay & 0xFF) != 0) { t.end[1] = delay & 0xFF; t.nend = 2; }
  } else if (st.x != 0) {
    const unsigned int top = st.x + st.y;
    const unsigned int r24 = ((st.x - 1) >> 24) + 1;
    if (r24 <= (top >> 24)) {
      t.end[0] = r24 & 0xFF;
      t.nend = 1;
    } else {
      const unsigned int r16 = ((st.x - 1) >> 16) + 1;
      t.end[0] = (r16 >> 8) & 0xFF;
      t.nend = 1;
      if ((r16 & 0xFF) != 0) { t.end[1] = r16 & 0xFF; t.nend = 2; }
    }
  }
  tail[s] = t;
  long long len = static_cast<long long>(t.nhead) + 2ll * t.run + t.nend;
  for (int c = 0; c < nchunks; ++c) len += chunks[c].len[s];
  length[s] = len;
}
__global__ void enc_tail_kernel(const uint4* state, int64_t streams, const ChunkList chunks,
                                int nchunks, int fast_state, Tail* tail, long long* length) {
  enc_tail_one(state, streams, chunks, nchunks, fast_state, tail, length);
}

// Finalize of n single-call handles of the lane family in three launches (blockIdx.y = handle): their
// temporaries, offsets and packed blobs live at a fixed stride in ONE allocation.
constexpr int kMaxFinalizeJobs = 64;
struct FinalizeJobs {
  int64_t streams;
  int n;
  uint8_t* base;             // job k: base + k * job_bytes = [Tail x streams][length x streams][offsets x (streams + 1)][blob]
  long long job_bytes, length_off, offsets_off, blob_off;
  struct { const uint4* state; ChunkRef chunk; } job[kMaxFinalizeJobs];
};
__device__ inline Tail* fin_tail(const FinalizeJobs& f, int k) { return reinterpret_cast<Tail*>(f.base + k * f.job_bytes); }
__device__ inline long long* fin_length(const FinalizeJobs& f, int k) { return reinterpret_cast<long long*>(f.base + k * f.job_bytes + f.length_off); }
__device__ inline long long* fin_offsets(const FinalizeJobs& f, int k) { return reinterpret_cast<long long*>(f.base + k * f.job_bytes + f.offsets_off); }
__global__ void enc_tail_many_kernel(const FinalizeJobs f) {
  const int k = blockIdx.y;
  ChunkList one;
  one.inline_refs[0] = f.job[k].chunk;
  one.more = nullptr;
  one.n = 1;
  enc_tail_one(f.job[k].state, f.streams, one, 1, 1, fin_tail(f, k), fin_length(f, k));     // lane family: held-digit state
}

__device__ inline void scan_lengths_one(const long long* length, int64_t streams, long long* off) {
  __shared__ long long carry;
  __shared__ long long tmp[1024];
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < streams; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const long long v0 = i < streams ? length[i] : 0;
    tmp[threadIdx.x] = v0;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      long long v = threadIdx.x >= d ? tmp[threadIdx.x - d] : 0;
      __syncthreads();
      tmp[threadIdx.x] += v;
      __syncthreads();
    }
    if (i < streams) off[i] = carry + tmp[threadIdx.x] - v0;
    __syncthreads();
    if (threadIdx.x == 1023) carry += tmp[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) off[streams] = carry;
}
__global__ void scan_lengths_kernel(const long long* length, int64_t streams, long long* off) {
  scan_lengths_one(length, streams, off);
}
__global__ void scan_lengths_many_kernel(const FinalizeJobs f) {
  scan_lengths_one(fin_length(f, blockIdx.x), f.streams, fin_offsets(f, blockIdx.x));
}

// Wave-cooperative byte copy with 4-byte stores: dst is brought to dword alignment, the
// (generally misaligned) source is read as aligned dwords and funnel-shifted.  The source
// slabs carry >= 4 bytes of slack behind every stream, so reading one dword past n is safe.
__device__ inline void wave_copy(uint8_t* dst, const uint8_t* src, unsigned int n, int lane) {
  const unsigned int head = min(n, static_cast<unsigned int>((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));
  if (lane < static_cast<int>(head)) dst[lane] = src[lane];
  dst += head; src += head; n -= head;
  const unsigned int nd = n >> 2;
  const unsigned int sh = static_cast<unsigned int>(reinterpret_cast<uintptr_t>(src) & 3) * 8;
  const unsigned int* s32 = reinterpret_cast<const unsigned int*>(reinterpret_cast<uintptr_t>(src) & ~uintptr_t{3});
  unsigned int* d32 = reinterpret_cast<unsigned int*>(dst);
  if (sh == 0) {
    for (unsigned int i = lane; i < nd; i += 64) d32[i] = s32[i];
  } else {
    for (unsigned int i = lane; i < nd; i += 64) d32[i] = (s32[i] >> sh) | (s32[i + 1] << (32 - sh));
  }
  const unsigned int rem = n & 3;
  if (lane < static_cast<int>(rem)) dst[4 * nd + lane] = src[4 * nd + lane];
}

// One wave per stream: copy the stream's chunk pieces then its tail.
__device__ inline void enc_pack_one(int64_t streams, const ChunkList& chunks, int nchunks, const Tail* tail,
                                    const long long* off, uint8_t* blob) {
  const int lane = threadIdx.x & 63;
  const int64_t s = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (s >= streams) return;
  uint8_t* dst = blob + off[s];
  long long done = 0;
  for (int c = 0; c < nchunks; ++c) {
    const unsigned int n = chunks[c].len[s];
    wave_copy(dst + done, chunk_piece(chunks[c], s), n, lane);
    done += n;
  }
  const Tail t = tail[s];
  if (lane < static_cast<int>(t.nhead)) dst[done + lane] = t.head[lane];
  done += t.nhead;
  for (unsigned long long i = lane; i < 2ull * t.run; i += 64) dst[done + i] = 0xFF;
  done += 2ll * t.run;
  if (lane < static_cast<int>(t.nend)) dst[done + lane] = t.end[lane];
}
__global__ void __launch_bounds__(kBlock) enc_pack_kernel(int64_t streams, const ChunkList chunks,
                                                         int nchunks, const Tail* tail,
                                                         const long long* off, uint8_t* blob) {
  enc_pack_one(streams, chunks, nchunks, tail, off, blob);
}
__global__ void __launch_bounds__(kBlock) enc_pack_many_kernel(const FinalizeJobs f) {
  const int k = blockIdx.y;
  ChunkList one;
  one.inline_refs[0] = f.job[k].chunk;
  one.more = nullptr;
  one.n = 1;
  enc_pack_one(f.streams, one, 1, fin_tail(f, k), fin_offsets(f, k), f.base + k * f.job_bytes + f.blob_off);
}

// ---- decoder --------------------------------------------------------------

struct DecParams {
  TableView tab;
  const int32_t* index;
  int64_t streams;
  int64_t elems;
  const uint8_t* blob;
  const long long* off;            // [streams + 1]
  uint4* state;                    // base, span_m1, window, pulls
  unsigned long long* first_error; // index range error
  const unsigned int* only_flagged; // dec_fast_kernel: if set, decode only streams with a nonzero flag
  const unsigned int* job_guard;    // null, or a flag: the whole launch decodes only if it is set (fallback of range_pipe.h
                                    // for tables whose lane-per-stream image does not fit a CU)
  int blocks_after_escape;         // dec_fast_kernel: batches decoded as checked 8-symbol blocks after an escape
};

template <bool LDS_TAB, typename Dst>
__global__ void __launch_bounds__(kBlock) dec_kernel(DecParams p, Dst dst) {
  extern __shared__ int32_t lds_tab[];
  if (p.job_guard != nullptr && *p.job_guard == 0u) return;
  if (LDS_TAB) {
    for (int i = threadIdx.x; i < p.tab.total; i += kBlock) lds_tab[i] = p.tab.data[i];
    __syncthreads();
  }
  auto T = [&](int i) -> int32_t { return LDS_TAB ? lds_tab[i] : p.tab.data[i]; };

  const int lane = threadIdx.x & 63;
  const int64_t s = __builtin_amdgcn_readfirstlane(
      static_cast<int>(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
  if (s >= p.streams) return;

  const uint4 st0 = p.state[s];
  DecoderState st;
  st.base = __builtin_amdgcn_readfirstlane(st0.x);
  st.span_m1 = __builtin_amdgcn_readfirstlane(st0.y);
  st.window = __builtin_amdgcn_readfirstlane(st0.z);
  DigitWindow w;
  const long long o0 = p.off[s];
  w.src = p.blob + o0;
  w.len = p.off[s + 1] - o0;
  w.pulls = __builtin_amdgcn_readfirstlane(st0.w);
  w.base = w.pulls;
  window_load(w, lane);

  for (int64_t j0 = 0; j0 < p.elems; j0 += 64) {
    const int64_t j = j0 + lane;
    int t = 0;
    if (j < p.elems) {
      const int64_t pos = s * p.elems + j;
      if (p.index) {
        t = p.index[pos];
        if (t < 0 || t >= p.tab.ntab) {
          atomicMin(p.first_error, static_cast<unsigned long long>(pos));
          t = 0;
        }
      } else {
        t = static_cast<int>(j % p.tab.ntab);
      }
    }
    const int cnt = static_cast<int>(min<int64_t>(64, p.elems - j0));
    int outv = 0;
    for (int n = 0; n < cnt; ++n) {
      const int tn = __builtin_amdgcn_readlane(t, n);
      const int2 row = p.tab.rows[tn];
      const int start = __builtin_amdgcn_readfirstlane(row.x);
      const int nints = __builtin_amdgcn_readfirstlane(row.y);
      const int sp = __builtin_amdgcn_readfirstlane(T(start));
      const int prec = sp < 0 ? -sp : sp;
      int sym = dec_symbol(T, st, start + 1, nints - 1, prec, w, lane);
      if (sp < 0 && sym == nints - 3) sym = dec_escape(st, w, lane, nints);
      outv = tfc_writelane(sym, n, outv);
    }
    if (j < p.elems) dst.store(s * p.elems + j, t, outv);
  }
  if (lane == 0) p.state[s] = make_uint4(st.base, st.span_m1, st.window, w.pulls);
}

}  // namespace tfc
#include "range_decoder_fast.h"
#include "range_lanes.h"
#include "range_pipe.h"
namespace tfc {

// Opens every stream (dec_open_state, range_wave.h).
__device__ inline void dec_open_one(const uint8_t* blob, const long long* off, int64_t streams,
                                    uint4* state, unsigned long long* status) {
  const int64_t s = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (s == 0) *status = ~0ull;       // no index error met yet
  if (s >= streams) return;
  state[s] = dec_open_state(blob + off[s], off[s + 1] - off[s]);
}
__global__ void dec_open_kernel(const uint8_t* blob, const long long* off, int64_t streams,
                                uint4* state, unsigned long long* status) {
  dec_open_one(blob, off, streams, state, status);
}
// n decoders at once (blockIdx.y = handle): their control blocks ([status 16 B][state]) sit at a fixed
// stride in one allocation
constexpr int kMaxDecoderJobs = 64;
struct DecoderJobs {
  int64_t streams;
  int n;
  uint8_t* ctl;
  long long ctl_bytes;
  struct { const uint8_t* blob; const long long* off; uint8_t* ok; } job[kMaxDecoderJobs];
};
__global__ void dec_open_many_kernel(const DecoderJobs f) {
  const int k = blockIdx.y;
  uint8_t* ctl = f.ctl + k * f.ctl_bytes;
  dec_open_one(f.job[k].blob, f.job[k].off, f.streams, reinterpret_cast<uint4*>(ctl + 16),
               reinterpret_cast<unsigned long long*>(ctl));
}

// The Finalize verdict of every stream (dec_finalize_ok, range_wave.h).
__device__ inline void dec_close_one(const uint4* state, const long long* off, int64_t streams,
                                     uint8_t* ok) {
  const int64_t s = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (s >= streams) return;
  const uint4 st = state[s];
  ok[s] = dec_finalize_ok(st.x, st.y, st.z, st.w, off[s + 1] - off[s]) ? 1 : 0;
}
__global__ void dec_close_kernel(const uint4* state, const long long* off, int64_t streams,
                                 uint8_t* ok) {
  dec_close_one(state, off, streams, ok);
}
__global__ void dec_close_many_kernel(const DecoderJobs f) {
  const int k = blockIdx.y;
  dec_close_one(reinterpret_cast<const uint4*>(f.ctl + k * f.ctl_bytes + 16), f.job[k].off, f.streams, f.job[k].ok);
}

// Initial coder state of every stream, plus the handle's status words (first error position = none,
// value, index, filled flag) and overflow flag.
__device__ inline void fill_state_one(uint4* state, int64_t n, uint4 v, unsigned long long* status,
                                      unsigned int* oflag) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (i < n) state[i] = v;
  if (i == 0) {
    status[0] = ~0ull;
    status[1] = status[2] = status[3] = 0ull;
    *oflag = 0u;
  }
}
__global__ void fill_state_kernel(uint4* state, int64_t n, uint4 v, unsigned long long* status,
                                  unsigned int* oflag) {
  fill_state_one(state, n, v, status, oflag);
}
// n encoder control blocks ([status 32 B][overflow flag .. 64 B][state]) at a fixed stride (blockIdx.y)
__global__ void fill_state_many_kernel(uint8_t* ctl, long long ctl_bytes, int64_t n, uint4 v) {
  uint8_t* c = ctl + blockIdx.y * ctl_bytes;
  fill_state_one(reinterpret_cast<uint4*>(c + 64), n, v, reinterpret_cast<unsigned long long*>(c),
                 reinterpret_cast<unsigned int*>(c + 32));
}

}  // namespace tfc

// ===========================================================================
// Host side: the coder's switches and process-wide state
// ===========================================================================
// Everything in this section exists once per process, behind the function that names it.  (env_int and the table of all
// switches: launch.h.)

namespace {

constexpr int kLds = static_cast<int>(kLdsBytesPerCu);      // the lane and chain plans count LDS in int

// Which image the pipelined decoder's chain runs on — 1 "full" (the lane-per-stream kernels' image, one bit per quotient
// value), 2 "pairs" (the compact image, TFC_PDEC_STEP_H: half the bitmaps, ~10 % more cycles per row), 0: full where it
// fits and its chain waves all find a CU, else pairs — and the chain waves per workgroup (0: by launch size).
// tfc_set_pipe_format / TFC_PIPE_FORMAT, TFC_PIPE_WAVES: an A/B and test switch.
std::atomic<int>& pipe_format_value() {
  static std::atomic<int> v{[] {
    const char* e = env_str("TFC_PIPE_FORMAT");
    if (e && std::strcmp(e, "full") == 0) return 1;
    if (e && std::strcmp(e, "pairs") == 0) return 2;
    return 0;
  }()};
  return v;
}
std::atomic<int>& pipe_waves_value() {
  static std::atomic<int> v{std::max(0, env_int("TFC_PIPE_WAVES", 0))};
  return v;
}
inline int pipe_format() { return pipe_format_value().load(std::memory_order_relaxed); }
inline int pipe_waves_env() { return pipe_waves_value().load(std::memory_order_relaxed); }

// The pipelined kernels of range_pipe.h in front of the lane-per-stream kernels (TFC_PIPE=0: the latter alone —
// an A/B switch for measurements, not a product setting).
inline bool pipe_enabled() {
  static const bool on = env_int("TFC_PIPE", 1) != 0;
  return on;
}
// TFC_PIPE_NOFALLBACK=1 (tools/pipe_probe.py): the lane-per-stream kernel is NOT launched behind the pipelined ones, so
// that a job they gave up on shows as wrong output instead of being covered up
inline bool pipe_fallback_launch() {
  static const bool on = env_int("TFC_PIPE_NOFALLBACK", 0) == 0;
  return on;
}
// Launches of the pipelined kernels so far (tfc_pipe_counters)
std::atomic<long long>& pipe_launches() {
  static std::atomic<long long> n{0};
  return n;
}

// TFC_PIPE_OVERLAP (default 2): how the encoder's chain kernel is launched relative to the expansion that feeds it.
//   0  behind it, on the caller's stream (the chain starts when every call word is in memory);
//   1  on a stream of the library's own, enqueued behind the expansion;  2  the same, enqueued in front of it.
// On its own stream the chain consumes the call words tile by tile while the expansion is still producing them
// (range_pipe.h: `done` flags); whichever way the two kernels end up scheduled, the result is the same — a chain
// that went first and is not fed within TFC_PIPE_POLL_MS (default 250) gives its job to the lane-per-stream kernel.
inline int pipe_overlap() {
  static const int v = env_int("TFC_PIPE_OVERLAP", 2);
  return v;
}
inline long long pipe_poll_ticks() {
  static const long long v = static_cast<long long>(env_int("TFC_PIPE_POLL_MS", 250)) * 100000;     // wall_clock64(): 100 MHz
  return v;
}

// The library's own stream next to a caller's stream (one per caller stream and device, made on first use, never
// destroyed), with the two events that tie a launch on it into the caller's order.  It is a HIGH-priority stream
// (unless the caller's is): HIP multiplexes the streams of one priority onto a few hardware queues and kernels that
// share a queue run one after the other — a different priority is a different queue, and the chain is the critical
// path of an encode call.
struct SideStream {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
inline int side_stream(hipStream_t st, SideStream* out) {
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, SideStream> streams;
  int dev = 0;
  TFC_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  auto f = streams.find({dev, st});
  if (f == streams.end()) {
    SideStream ss;
    int least = 0, greatest = 0, mine = 0;
    TFC_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    if (hipStreamGetPriority(st, &mine) != hipSuccess) {
      (void)hipGetLastError();
      mine = least;
    }
    const int prio = (mine == greatest && least != greatest) ? least : greatest;
    TFC_HIP(hipStreamCreateWithPriority(&ss.stream, hipStreamNonBlocking, prio));
    TFC_HIP(hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming));
    TFC_HIP(hipEventCreateWithFlags(&ss.join, hipEventDisableTiming));
    f = streams.emplace(std::make_pair(dev, st), ss).first;
  }
  *out = f->second;
  return 0;
}
// Work beside the caller's stream `st`: after fork(), what goes to `stream` runs on the library's own stream, behind what
// `st` holds so far; join() puts `st` behind it again.  Without a fork `stream` is the caller's and join() does nothing.
struct SideFork {
  hipStream_t st, stream;
  SideStream side;
  bool forked = false;
  explicit SideFork(hipStream_t caller) : st(caller), stream(caller) {}
  int fork() {
    if (side_stream(st, &side)) return 1;
    TFC_HIP(hipEventRecord(side.fork, st));
    TFC_HIP(hipStreamWaitEvent(side.stream, side.fork, 0));
    stream = side.stream;
    forked = true;
    return 0;
  }
  int join() {
    if (!forked) return 0;
    TFC_HIP(hipEventRecord(side.join, side.stream));
    TFC_HIP(hipStreamWaitEvent(st, side.join, 0));
    return 0;
  }
};
// Temporaries of one pipelined launch (call words / raw rows: ~150 / ~125 MB per 512-stream job of BASELINE config 2) are
// bounded: more jobs than fit go out as several launches, one behind the other.  6 GB, at most an eighth of the device's
// memory; TFC_PIPE_TEMP_MB overrides.  Measured (round 5, bench.py `saturation`, profiles/r05_notes.md): a launch takes
// the same ~14 ms up to ~40 jobs, but more per launch does not help — with 24 GB, 64 jobs in ONE launch took 12.4 ms of
// encode (the expansion, 0.19 ms per job, is what bounds it beyond ~20 jobs) + 31 ms of decode (512 chain waves: two per
// CU behind one 149 KB table image, and the parse beside them finds no CU) against 12.0 + 28.6 ms as 39 + 25 jobs.
// A launch whose temporaries cannot be allocated runs on the lane-per-stream kernels, which need none.
// (per device ordinal: a process may drive several devices of different memory sizes)
struct PipeDeviceInfo {
  size_t temp_bytes = 0;
};
inline const PipeDeviceInfo& pipe_device_info() {
  constexpr int kMaxDevices = 64;
  static PipeDeviceInfo info[kMaxDevices];
  static std::once_flag once[kMaxDevices];
  int dev = 0;
  (void)hipGetDevice(&dev);
  dev = std::min(std::max(dev, 0), kMaxDevices - 1);
  std::call_once(once[dev], [dev] {
    PipeDeviceInfo& d = info[dev];
    if (env_str("TFC_PIPE_TEMP_MB")) {
      d.temp_bytes = static_cast<size_t>(std::max(1, env_int("TFC_PIPE_TEMP_MB", 0))) << 20;
      return;
    }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
      (void)hipGetLastError();
      d.temp_bytes = size_t{2} << 30;
      return;
    }
    d.temp_bytes = std::min<size_t>(size_t{6} << 30, total_b / 8);
  });
  return info[dev];
}
inline size_t pipe_temp_bytes() { return pipe_device_info().temp_bytes; }

// The facts the lane path's plans (range_plan.h) are functions of: the tables', the device's and the switches', and the
// kernels' compile-time sizes (WaveLds / kMaxJobs: of the lane kernel that is planned — EncWaveLds, EncLaneJobs or the
// decoder's).
inline plan::TableFacts table_facts(const tfc_tables* t) {
  plan::TableFacts f;
  f.lane_enc_bytes = t->lane_enc_bytes;
  f.lane_dec_bytes = t->lane_dec_bytes;
  f.pair_dec_bytes = t->pair_dec_bytes;
  f.pairs_ok = t->pairs_ok;
  f.any_escape = t->any_escape;
  f.lane_precision = t->lane_precision;
  f.entries = t->host.size();
  f.ntab = static_cast<int>(t->rows.size());
  return f;
}
inline plan::DeviceFacts device_facts() {
  plan::DeviceFacts f;
  f.cus = device_cus();
  f.lds_bytes = kLds;
  f.temp_bytes = pipe_temp_bytes();
  f.pipe_enabled = pipe_enabled();
  f.format = pipe_format();
  f.waves_override = pipe_waves_env();
  f.overlap = pipe_overlap();
  f.chip_shared = chip_shared();
  return f;
}
template <typename WaveLds, int kMaxJobs>
constexpr plan::KernelFacts kernel_facts() {
  plan::KernelFacts f;
  f.lane_wave_indexed = WaveLds::kBytes;
  f.lane_wave_plain = WaveLds::kIndex;
  f.dec_lds_bytes = PipeDecLds::kBytes;
  f.dec_lds_rows = PipeDecLds::kRows;
  f.dec_lds_stage = PipeDecLds::kStage;
  f.enc_chain_groups = PipeEncChainLds::kGroups;
  f.enc_chain_group = PipeEncChainLds::kGroup;
  f.enc_chain_rows = PipeEncChainLds::kRows;
  f.pipe_tile = kPipeTile;
  f.pipe_block = kPipeBlock;
  f.parse_rows = kParseRows;
  f.expand_tab_bytes = kExpandTabBytes;
  f.max_jobs = kMaxJobs;
  return f;
}
static_assert(sizeof(uint4) == plan::kStateBytes && sizeof(uint2) == plan::kStageOutBytes);      // range_plan.h's element sizes

// Kernel variants: run-time switches (index mode, the compact image, the staged tables) as std::bool_constant arguments
// of a generic lambda, which names the instantiation.  (Two flags: the first is the outer choice.  The variants are
// instantiated in that order, which is their order in the code object — tools/kernel_diff.py sees a swap as moved code.)
template <typename F>
auto with_flags(bool a, F&& f) {
  return a ? f(std::true_type{}) : f(std::false_type{});
}
template <typename F>
auto with_flags(bool a, bool b, F&& f) {
  return with_flags(a, [&](auto A) { return with_flags(b, [&](auto B) { return f(A, B); }); });
}

}  // namespace

// ===========================================================================
// Host side: encoder
// ===========================================================================

struct EncChunk {
  DevBuf data, off, len;
  long long stride = 0;         // lane kernels: stream s starts at s * stride (off unused)
  unsigned int* len_p = nullptr;    // the lengths: `len`, or the tail of `data` (lane kernels: one allocation)
  size_t data_bytes = 0;
};

// Kernel family of a handle (fixed at its first coding call; the families keep different state
// encodings between calls).
enum Family { kGeneric = 0, kFast = 1, kLanes = 2 };

struct tfc_encoder {
  const tfc_tables* tables = nullptr;
  int64_t streams = 0;
  int mode = TFC_MODE_AUTO;
  int family = -1;              // Family, chosen by the first encode call
  bool fast = false;            // wave-per-stream fast kernels are possible for these tables
  int fast_waves = 0;           // waves per workgroup for the fast kernels
  size_t fast_lds = 0;
  bool deferred = false;        // range errors are reported by finalize / status instead of encode
  bool poisoned = false;        // a range error was reported: the streams are no longer meaningful
  int64_t elems_last = 0;       // geometry of the call the recorded error belongs to
  bool indexed_last = false;
  DevBuf ctl;                   // one allocation behind the three views below ...
  std::shared_ptr<DevBuf> ctl_group;      // ... or a slice of the allocation shared by a create_many group
  DevView state;                // uint4 [streams]
  DevView oflag;                // unsigned int: a stream outgrew its output slab
  DevView status;               // u64[4]: first error position, its value, its index, filled flag
  std::vector<EncChunk> chunks;
  // results
  bool finalized = false;
  bool total_known = false;
  DevBuf blob_own, offsets_own;
  std::shared_ptr<DevBuf> result_group;   // finalize_device_many: blob / offsets are slices of one allocation
  DevView blob, offsets;
  int64_t total = 0;
  int64_t blob_capacity = 0;    // bytes behind `blob`
  // Every entry point that takes a stream retargets the handle's buffers to it: they are released in the
  // order of the stream that used them LAST, not of the one they were allocated under.
  void touch(hipStream_t s) {
    ctl.touch(s);
    if (ctl_group) ctl_group->touch(s);
    for (auto& c : chunks) { c.data.touch(s); c.off.touch(s); c.len.touch(s); }
    blob_own.touch(s);
    offsets_own.touch(s);
    if (result_group) result_group->touch(s);
  }
};

namespace {

// Waves (= code streams) of a workgroup of the wave-per-stream kernels, sharing one LDS copy of the tables: one wave
// per SIMD of a CU whenever there are that many streams.  Fewer, fuller workgroups: a CU that hosts even one coder wave
// is lost to a convolution workgroup — which wants all four SIMDs' registers — for as long as that wave runs, so with
// model steps in flight 128 streams as 64 workgroups of 2 waves cost the transforms twice the CUs of 32 workgroups of
// 4 (C4: 47.2 -> 45.2 ms per step; 8 or 16 waves per workgroup, two or four per SIMD: 51.2 / 63.5; measured in round 3).
inline int64_t waves_wanted(int64_t streams) {
  // tfc_set_chip_shared(1) — the caller keeps other kernels in flight beside the coder's: 512 streams and more get two
  // waves per SIMD, i.e. 64 instead of 128 CUs under a bls2017 batch (C1: 12.0 -> 11.1 ms per step with 8 steps in
  // flight; a lone 512-stream call is 1.4x slower that way, 6.5 -> 8.8 ms, hence not the default); for 128 streams the
  // same packing costs more than it frees (profiles/r03_notes.md)
  const bool shared = chip_shared();
  const int64_t limit = shared && streams >= 512 ? 8 : 4;
  return std::min<int64_t>(limit, std::max<int64_t>(1, streams));
}

// Which kernels a handle uses.  The lane-per-stream kernels issue ~1 vector instruction per symbol
// and 64 streams against 15-28 and 1 for the wave-per-stream kernels, but a lone call takes
// elems x ~400 cycles against elems x ~90-160: they win when the streams of all calls in flight
// outnumber the chip's SIMDs several times.  AUTO decides on the stream count of the handle alone;
// a caller that keeps many calls in flight asks for TFC_MODE_THROUGHPUT.
int select_family(const tfc_tables* t, int mode, int64_t streams, int64_t elems, bool fast_ok) {
  // the lane kernels address a stream's bytes with 32 bits, and their LDS plan (image + one wave's
  // staging planes, any variant of the encoder) has to fit the CU
  const bool lanes_ok = t->lanes_ok && elems < (int64_t{1} << 29) &&
                        plan::lanes_fit(t->lane_enc_bytes, EncWaveLds<int32_t>::kBytes, kLds);
  if (mode == TFC_MODE_AUTO) mode = tfc_get_default_mode();
  if (mode == TFC_MODE_THROUGHPUT && lanes_ok) return kLanes;
  if (mode == TFC_MODE_AUTO && lanes_ok && streams >= 4096) return kLanes;
  // tfc_set_chip_shared(1): a batch of 256 streams and more goes to the lane kernels where they fit — a wave per 64
  // streams on a handful of CUs instead of a wave per stream on 64-128 CUs that the convolutions then cannot use
  if (mode == TFC_MODE_AUTO && lanes_ok && streams >= 256 && chip_shared())
    return kLanes;
  return fast_ok ? kFast : kGeneric;
}

// Blocks a wave of the lane kernels lets lanes wait in front of an escape code before it takes the codes of all
// waiting lanes together (LaneArgs::defer; measured in round 3: 3).
inline int lanes_escape_defer() { return 3; }

// Slab bytes per stream that a lane-encoder call can never exceed, from the table headers alone (no
// counting pass, no read-back).  A call emits at most one 16-bit digit; and a call of probability P
// shrinks the span by at most 1 + log2(1/P) bits, a digit leaves every 16 bits: a symbol of a
// precision-p row costs <= p + 1 bits, each of the <= 64 binary calls of an escape code
// 1 + 2^-15 bits.  `carry` covers digits an earlier call left delayed.
// With escape rows that worst case is ~10 bytes per symbol against ~0.5 produced, so a call first
// runs with the no-escape bound (16 bits per symbol on average: exceeded only by streams that are
// mostly long escape codes); a stream that outgrows it raises the handle's overflow flag, and the call
// is repeated with the worst-case slab (handles that synchronise) or reported (deferred handles).
unsigned int lanes_slab_bytes(const tfc_tables* t, int64_t elems, bool worst) {
  const long long carry = 80;
  long long bytes = 2 * elems;
  if (t->any_escape && worst) bytes = (elems * (t->max_abs_prec + 1 + 65) + 7) / 8 + 8;
  bytes = (bytes + carry + 15) & ~15ll;
  return static_cast<unsigned int>(std::min<long long>(bytes, 0xFFFFFFF0ll));
}

// Records value / index of the first range error next to its position (stream-ordered, so the
// inputs are still alive whatever the caller does after the encode call returns).  One thread per job.
template <typename Src>
struct EncErrJobs {
  int64_t elems;
  int ntab, n;
  struct { unsigned long long* status; Src src; const int32_t* index; } job[EncLaneJobs<Src>::kMax];
};
template <typename Src>
__global__ void enc_error_kernel(const EncErrJobs<Src> jobs) {
  if (static_cast<int>(threadIdx.x) >= jobs.n) return;
  unsigned long long* status = jobs.job[threadIdx.x].status;
  const Src src = jobs.job[threadIdx.x].src;
  const int32_t* index = jobs.job[threadIdx.x].index;
  const unsigned long long pos = status[0];
  if (pos == ~0ull || status[3] != 0ull) return;
  int t = static_cast<int>((pos % static_cast<unsigned long long>(jobs.elems)) % static_cast<unsigned long long>(jobs.ntab));
  long long ix = 0;
  if (index) {
    ix = index[pos];
    t = (ix < 0 || ix >= jobs.ntab) ? 0 : static_cast<int>(ix);
  }
  status[1] = static_cast<unsigned long long>(static_cast<long long>(src.load(static_cast<int64_t>(pos), t)));
  status[2] = static_cast<unsigned long long>(ix);
  status[3] = 1ull;
}

// Builds the reference's range-error text for the element at `pos`.
int range_error_text(const tfc_tables* t, bool has_index, int32_t idx, int64_t channel,
                     int32_t value) {
  const int64_t ntab = static_cast<int64_t>(t->rows.size());
  if (has_index && (idx < 0 || idx >= ntab))
    return fail("index=%d not in range [0, %lld)", idx, static_cast<long long>(ntab));
  const int2 row = t->rows[has_index ? idx : channel];
  return fail("value=%d not in range [0, %d)", value, row.y - 2);
}

int encoder_error(tfc_encoder* e, const unsigned long long* host_status) {
  e->poisoned = true;
  const unsigned long long pos = host_status[0];
  const int64_t ch = static_cast<int64_t>((pos % static_cast<unsigned long long>(std::max<int64_t>(e->elems_last, 1))) %
                                          e->tables->rows.size());
  return range_error_text(e->tables, e->indexed_last, static_cast<int32_t>(static_cast<long long>(host_status[2])),
                          ch, static_cast<int32_t>(static_cast<long long>(host_status[1])));
}

// What a lane kernel is told of the tables and its LDS plan; `bytes`: of the direction's image (cap: the encoder's)
inline LaneArgs lane_args(const tfc_tables* t, int bytes, const plan::LanePlan& lanes) {
  LaneArgs la;
  la.image = t->d_lane_image.as<uint32_t>();
  la.bytes = bytes;
  la.ntab = static_cast<int>(t->rows.size());
  la.precision = t->lane_precision;
  la.cap = 0;
  la.defer = lanes_escape_defer();
  la.guard = nullptr;
  la.lds_image = lanes.lds_image;
  la.lds_wave = lanes.lds_wave;
  return la;
}

// The regions of a pipelined encode launch's workspace at `base`
inline void bind_workspace(PipeEncArgs* pa, uint8_t* base, const plan::EncLayout& lay, size_t groups) {
  pa->calls = reinterpret_cast<unsigned int*>(base + lay.calls);
  pa->stage_state = reinterpret_cast<uint4*>(base + lay.stage_state);
  pa->stage_out = reinterpret_cast<uint2*>(base + lay.stage_out);
  pa->status = reinterpret_cast<unsigned int*>(base + lay.status);
  pa->done = reinterpret_cast<unsigned int*>(base + lay.done);
  pa->fallback = reinterpret_cast<unsigned int*>(base + lay.fallback);
  pa->started = reinterpret_cast<unsigned int*>(base + lay.started);
  pa->groups = static_cast<int>(groups);
}

// The pipelined kernels of one encode launch (pa bound to its zeroed workspace): expansion, chain, commit.
// A large launch: the chain (workgroups of PipeEncChainLds::kGroups groups, helper waves: range_pipe.h) on the library's own stream
// next to the expansion.  A small one — a model step's few groups, next to other steps' convolutions — one-wave
// chain workgroups behind the expansion on the caller's stream: measured on bmshj2018 with steps in flight, the
// second stream, its events and the large workgroups cost more (45 against 36 ms per step) than the overlap of
// two short kernels gives.
template <typename Src>
int launch_enc_pipe(const EncLaneJobs<Src>& jobs, const PipeEncArgs& pa, const plan::EncPipePlan& pipe,
                    const plan::DeviceFacts& dev, bool indexed, hipStream_t st) {
  const size_t groups = static_cast<size_t>(pa.groups);
  const bool large = plan::large_launch(groups);
  const int overlap = plan::launch_overlap(dev, groups);
  PipeChainJobs cj;
  cj.streams = jobs.streams;
  for (int k = 0; k < jobs.n; ++k)
    cj.job[k] = PipeChainJob{jobs.job[k].state, jobs.job[k].chunk, jobs.job[k].chunk_len, jobs.job[k].overflow_flag};
  SideFork side(st);
  if (overlap && side.fork()) return 1;
  const hipStream_t cst = side.stream;
  const dim3 xgrid(static_cast<unsigned>(groups * pa.nt));
  auto expand = [&] {
    KernelTimer t2("enc_expand", st);
    with_flags(indexed, pa.tab_entries != 0, [&](auto I, auto T) {
      hipLaunchKernelGGL((enc_expand_kernel<decltype(I)::value, Src, decltype(T)::value>), xgrid, dim3(kExpandThreads), 0, st, jobs, pa);
    });
  };
  const int cgroups = PipeEncChainLds::kGroups;
  const unsigned cblocks = static_cast<unsigned>(ceil_div(static_cast<int64_t>(groups), cgroups));
  if (large)
    if (int rc = allow_dynamic_lds(reinterpret_cast<const void*>(&enc_chain_kernel), pipe.chain_lds)) return rc;
  auto chain = [&] {
    KernelTimer t2("enc_chain", cst);
    if (!large) {
      hipLaunchKernelGGL(enc_chain_direct_kernel, dim3(static_cast<unsigned>(groups)), dim3(64), 0, cst, cj, pa);
      return;
    }
    hipLaunchKernelGGL(enc_chain_kernel, dim3(cblocks), dim3(256 * cgroups), pipe.chain_lds, cst, cj, pa);
    // (the expansion behind the chain's workgroups, not in their way)
    if (overlap == 2)
      hipLaunchKernelGGL(enc_gate_kernel, dim3(1), dim3(1), 0, st, pa.started, cblocks, static_cast<long long>(20000));
  };
  if (overlap == 2) { chain(); expand(); }
  else { expand(); chain(); }
  if (int rc = side.join()) return rc;
  hipLaunchKernelGGL(enc_commit_kernel, dim3(static_cast<unsigned>(groups)), dim3(64), 0, st, cj, pa);
  return 0;
}

template <typename Src>
int encode_lanes_many(tfc_encoder* const* es, int n, const Src* srcs, const int32_t* const* indexes,
                      int64_t elems, hipStream_t st, bool worst_case_slab);

// Behind the launches of an encode call: the handles that want their range errors now are read back, and one whose
// stream outgrew the speculative slab (`backups`: the pre-call coder states, per handle) is coded again.
template <typename Src>
int settle_eager_encoders(tfc_encoder* const* es, int n, const Src* srcs, const int32_t* const* indexes, int64_t elems,
                          hipStream_t st, bool speculative, const DevBuf* backups) {
  const bool indexed = indexes && indexes[0];
  bool any_eager = false;
  for (int k = 0; k < n; ++k) any_eager |= !es[k]->deferred;
  if (!any_eager) return 0;
  TFC_HIP(hipStreamSynchronize(st));
  for (int k = 0; k < n; ++k) {
    tfc_encoder* e = es[k];
    if (e->deferred) continue;
    unsigned long long host_status[4];
    TFC_HIP(hipMemcpy(host_status, e->status.p, sizeof(host_status), hipMemcpyDeviceToHost));
    if (host_status[0] != ~0ull) return encoder_error(e, host_status);
    if (!speculative) continue;
    unsigned int oflag = 0;
    TFC_HIP(hipMemcpy(&oflag, e->oflag.p, sizeof(oflag), hipMemcpyDeviceToHost));
    if (oflag) {
      // a stream outgrew the speculative slab: back to the pre-call state, code again with the bound
      // that cannot be exceeded
      TFC_HIP(hipMemcpyAsync(e->state.p, backups[k].p, sizeof(uint4) * e->streams, hipMemcpyDeviceToDevice, st));
      TFC_HIP(hipMemsetAsync(e->oflag.p, 0, sizeof(unsigned int), st));
      e->chunks.pop_back();
      const int32_t* ix = indexed ? indexes[k] : nullptr;
      if (encode_lanes_many(&es[k], 1, &srcs[k], &ix, elems, st, true)) return 1;
    }
  }
  return 0;
}

// Lane-per-stream family: n handles (same tables, same stream count) coded by one launch per
// kMaxLaneJobs of them; no counting pass, no read-back unless a handle wants its range errors now.
// Where the geometry allows, the pipelined kernels (range_pipe.h: parallel expansion into call words, then the
// chain) take the launch and the lane-per-stream kernel behind them only codes the jobs they gave up on.
template <typename Src>
int encode_lanes_many(tfc_encoder* const* es, int n, const Src* srcs, const int32_t* const* indexes,
                      int64_t elems, hipStream_t st, bool worst_case_slab) {
  const tfc_tables* t = es[0]->tables;
  const int64_t streams = es[0]->streams;
  const bool indexed = indexes && indexes[0];
  // the facts, and the plans made of them (range_plan.h)
  const plan::TableFacts tf = table_facts(t);
  const plan::DeviceFacts dev = device_facts();
  constexpr plan::KernelFacts kf = kernel_facts<EncWaveLds<typename Src::raw_type>, EncLaneJobs<Src>::kMax>();
  const plan::LanePlan lanes = plan::lane_plan(tf.lane_enc_bytes, kf, dev, streams * n, indexed);
  const plan::EncPipePlan pipe = plan::enc_pipe_plan(tf, dev, kf, streams, elems);
  LaneArgs la = lane_args(t, t->lane_enc_bytes, lanes);
  la.cap = lanes_slab_bytes(t, elems, worst_case_slab);
  const bool speculative = t->any_escape && !worst_case_slab;
  std::vector<DevBuf> backups(speculative ? n : 0);     // pre-call coder states of the handles that can retry
  const void* fn = with_flags(indexed, [](auto I) { return reinterpret_cast<const void*>(&enc_lanes_kernel<decltype(I)::value, Src>); });
  if (int rc = allow_dynamic_lds(fn, lanes.lds_bytes)) return rc;
  PipeEncArgs pa;
  pa.nt = pipe.nt;
  pa.rows = pipe.rows;
  pa.groups_per_job = pipe.groups_per_job;
  pa.poll_ticks = pipe_poll_ticks();
  pa.fast16 = t->d_fast.as<uint16_t>();
  pa.rows_fast = t->d_rows_fast.as<int2>();
  pa.ntab = la.ntab;
  pa.tab_entries = pipe.tab_entries;
  pa.cap = la.cap;
  for (int g0 = 0; g0 < n; g0 += pipe.per_launch) {
    const int gn = std::min(pipe.per_launch, n - g0);
    // 1. the jobs
    EncLaneJobs<Src> jobs;
    EncErrJobs<Src> errs;
    jobs.streams = streams;
    jobs.elems = elems;
    jobs.blocks_per_job = static_cast<int>(ceil_div(streams, lanes.block));
    jobs.n = gn;
    errs.elems = elems;
    errs.ntab = la.ntab;
    errs.n = gn;
    for (int k = 0; k < gn; ++k) {
      tfc_encoder* e = es[g0 + k];
      e->elems_last = elems;
      e->indexed_last = indexed;
      if (speculative && !e->deferred) {
        TFC_HIP(backups[g0 + k].alloc(sizeof(uint4) * streams, st));
        TFC_HIP(hipMemcpyAsync(backups[g0 + k].p, e->state.p, sizeof(uint4) * streams, hipMemcpyDeviceToDevice, st));
      }
      EncChunk ch;
      ch.stride = la.cap;
      ch.data_bytes = static_cast<size_t>(la.cap) * streams;
      TFC_HIP(ch.data.alloc(ch.data_bytes + sizeof(unsigned int) * streams, st));
      ch.len_p = reinterpret_cast<unsigned int*>(ch.data.as<uint8_t>() + ch.data_bytes);
      EncLaneJob<Src>& J = jobs.job[k];
      J.src = srcs[g0 + k];
      J.index = indexed ? indexes[g0 + k] : nullptr;
      J.state = e->state.as<uint4>();
      J.chunk = ch.data.as<uint8_t>();
      J.chunk_len = ch.len_p;
      J.first_error = e->status.as<unsigned long long>();
      J.overflow_flag = e->oflag.as<unsigned int>();
      errs.job[k].status = J.first_error;
      errs.job[k].src = J.src;
      errs.job[k].index = J.index;
      e->chunks.push_back(std::move(ch));
    }
    {
      KernelTimer timer("enc_kernel", st);
      // 2. the workspace of the pipelined kernels
      DevBuf temp;
      const size_t groups = static_cast<size_t>(pipe.groups_per_job) * gn;
      const plan::EncLayout lay = plan::enc_layout(pipe, kf, groups);
      bool piped = pipe.enabled;
      la.guard = nullptr;
      if (piped && temp.alloc(lay.total, st) != hipSuccess) {
        // no room for the call words (a smaller or busier device): the lane-per-stream kernel codes this launch
        (void)hipGetLastError();
        temp.p = nullptr;
        piped = false;
      }
      if (piped) {
        bind_workspace(&pa, temp.as<uint8_t>(), lay, groups);
        // nothing known about any tile, no tile released, no fallback
        TFC_HIP(hipMemsetAsync(temp.as<uint8_t>() + lay.zero_offset, 0, lay.zero_bytes, st));
        // 3. the launches: expansion, chain, commit
        pipe_launches().fetch_add(1, std::memory_order_relaxed);
        if (int rc = launch_enc_pipe(jobs, pa, pipe, dev, indexed, st)) return rc;
        // 4. ... and the lane-per-stream kernel behind them for the jobs they gave up on
        la.guard = pa.fallback;
      }
      const dim3 grid(static_cast<unsigned>(jobs.blocks_per_job * gn));
      if (piped && !pipe_fallback_launch()) {}
      else with_flags(indexed, [&](auto I) {
        hipLaunchKernelGGL((enc_lanes_kernel<decltype(I)::value, Src>), grid, dim3(lanes.block), lanes.lds_bytes, st, jobs, la);
      });
      // `temp` goes back to the library's cache in stream order, behind these launches
    }
    hipLaunchKernelGGL((enc_error_kernel<Src>), dim3(1), dim3(64), 0, st, errs);
    TFC_HIP(hipGetLastError());
  }
  return settle_eager_encoders(es, n, srcs, indexes, elems, st, speculative, backups.data());
}

// Deferred-error handles, wave-per-stream families: the counting pass's first error goes to the handle's
// status word on the device (the value / index behind it are recorded by enc_error_kernel).
__global__ void enc_defer_kernel(const unsigned long long* count_status, unsigned long long* status) {
  if (count_status[0] != ~0ull && status[0] == ~0ull) status[0] = count_status[0];
}

// Slab bytes for a wave-per-stream call sized WITHOUT the counting pass's result: what the call needs
// when no symbol takes an escape code (2 bytes per coder call + 4, rounded per stream), a quarter more
// when the tables have escape rows (an escape adds 2 log2|overflow| + 3 calls; the tables' own tail mass
// is 2^-8 ... 2^-7 of the symbols), and room for digits earlier calls held back.
size_t speculative_slab_bytes(const tfc_tables* t, int64_t streams, int64_t elems) {
  const size_t per = ((2 * static_cast<size_t>(elems) + 4 + 15) / 16) * 16 + 32;
  size_t bytes = per * static_cast<size_t>(streams);
  if (t->any_escape) bytes += bytes / 4;
  bytes += 64u << 10;
  // test hook (tests/test_pipeline_gpu.py): TFC_SPECULATIVE_SLAB_DIV=n shrinks the slab so that the
  // "outgrown" path can be exercised with ordinary data
  // (read at every call: the test sets it around its own calls)
  const int n = env_int("TFC_SPECULATIVE_SLAB_DIV", 0);
  if (n > 1) bytes = std::max<size_t>(bytes / static_cast<size_t>(n), 256);
  return bytes;
}

// ---- fused quantise / dequantise for the lane family ----------------------------------------------
// The lane kernels' hand-scheduled blocks take plain int32 symbols in channel mode; their generic steps (which
// convert per element) are ~2.3x slower.  For bottleneck values the conversion therefore runs as its own
// elementwise pass — HBM-bound, ~25 us for the 25 M elements of config 2 against milliseconds of coding — into a
// stream-ordered temporary, and the blocks code int32: continuous_batched.py:370-380 / :416-422 at the speed of
// int32 channel mode (+ the pass).
// grid = (ceil(elems / 1024), streams): four elements per thread, 256 apart (every access of a wave is one
// contiguous run); 32-bit index arithmetic — the table of an element is its position in the stream modulo the
// table count, stepped by 256 mod ntab instead of divided per element
template <typename T>
__global__ void __launch_bounds__(256) lanes_quantize_kernel(tfc::SymQuant<T> src, unsigned int elems, unsigned int ntab,
                                                             int32_t* out) {
  const unsigned int j0 = blockIdx.x * 1024u + threadIdx.x;
  const long long base = static_cast<long long>(blockIdx.y) * elems;
  const unsigned int step = 256u % ntab;
  unsigned int t = j0 % ntab;
#pragma unroll
  for (unsigned int k = 0; k < 4u; ++k) {
    const unsigned int j = j0 + 256u * k;
    if (j < elems) out[base + j] = src.quant(src.y[base + j], static_cast<int>(t));
    t += step;
    t -= t >= ntab ? ntab : 0u;
  }
}
template <typename Dst>
__global__ void __launch_bounds__(256) lanes_dequantize_kernel(Dst dst, const int32_t* sym, unsigned int elems,
                                                               unsigned int ntab) {
  const unsigned int j0 = blockIdx.x * 1024u + threadIdx.x;
  const long long base = static_cast<long long>(blockIdx.y) * elems;
  const unsigned int step = 256u % ntab;
  unsigned int t = j0 % ntab;
#pragma unroll
  for (unsigned int k = 0; k < 4u; ++k) {
    const unsigned int j = j0 + 256u * k;
    if (j < elems) dst.store(base + j, static_cast<int>(t), sym[base + j]);
    t += step;
    t -= t >= ntab ? ntab : 0u;
  }
}

// Jobs on plain int32 symbols; the others quantise on load (SymQuant) or dequantise on store (OutDequant).
template <typename Job> struct is_plain_symbols : std::false_type {};
template <> struct is_plain_symbols<tfc::SymInt32> : std::true_type {};
template <> struct is_plain_symbols<tfc::OutInt32> : std::true_type {};

// Jobs per call of the lane path: a channel-mode batch that quantises or dequantises goes kMaxFinalizeJobs at a time
// (without the pipelined kernels it converts through an int32 temporary of the whole call); any other batch is one
// call, which the lane path splits into launches itself.
template <typename Job>
int lane_call_jobs(int n, bool indexed) {
  return is_plain_symbols<Job>::value || indexed ? n : std::min(n, kMaxFinalizeJobs);
}

// channel mode, bottleneck values: quantise pass, then the int32 blocks
template <typename Src>
int encode_lanes_prequantized(tfc_encoder* const* es, int n, const Src* srcs, int64_t elems, hipStream_t st) {
  const long long per = static_cast<long long>(es[0]->streams) * elems;
  const int ntab = static_cast<int>(es[0]->tables->rows.size());
  DevBuf tmp;
  TFC_HIP(tmp.alloc(sizeof(int32_t) * static_cast<size_t>(per) * n, st));
  std::vector<tfc::SymInt32> q(n);
  for (int k = 0; k < n; ++k) {
    int32_t* out = tmp.as<int32_t>() + static_cast<long long>(k) * per;
    hipLaunchKernelGGL((lanes_quantize_kernel<typename Src::raw_type>),
                       dim3(static_cast<unsigned>(ceil_div(elems, 1024)), static_cast<unsigned>(es[0]->streams)),
                       dim3(256), 0, st, srcs[k], static_cast<unsigned int>(elems), static_cast<unsigned int>(ntab), out);
    q[k] = tfc::SymInt32{out};
  }
  TFC_HIP(hipGetLastError());
  return encode_lanes_many(es, n, q.data(), static_cast<const int32_t* const*>(nullptr), elems, st, false);
  // `tmp` goes back to the pool in stream order, behind the coding launch
}

// n lane-family handles (same tables, same stream count), lane_call_jobs of them per call
template <typename Src>
int encode_lanes(tfc_encoder* const* es, int n, const Src* srcs, const int32_t* const* indexes, int64_t elems,
                 hipStream_t st) {
  const bool indexed = indexes && indexes[0];
  const int per_call = lane_call_jobs<Src>(n, indexed);
  for (int g0 = 0; g0 < n; g0 += per_call) {
    const int gn = std::min(per_call, n - g0);
    if constexpr (!is_plain_symbols<Src>::value) {
      // (the pipelined kernels quantise in their expansion pass)
      if (!indexed && !pipe_enabled()) {
        if (encode_lanes_prequantized(es + g0, gn, srcs + g0, elems, st)) return 1;
        continue;
      }
    }
    if (encode_lanes_many(es + g0, gn, srcs + g0, indexed ? indexes + g0 : nullptr, elems, st, false)) return 1;
  }
  return 0;
}

// One handle that encode_jobs did not batch (checked and touched there)
template <typename Src>
int run_encode(tfc_encoder* e, const int32_t* index, int64_t elems, const Src& src, hipStream_t st) {
  if (e->streams == 0 || elems == 0) return 0;
  const tfc_tables* t = e->tables;
  if (t->rows.empty()) return fail("index=0 not in range [0, 0)");
  if (e->family < 0) e->family = select_family(t, e->mode, e->streams, elems, e->fast);
  if (e->family == kLanes && elems >= (int64_t{1} << 29)) return fail("encode call too large for this handle");
  if (e->family == kLanes) return encode_lanes(&e, 1, &src, &index, elems, st);
  e->elems_last = elems;
  e->indexed_last = index != nullptr;

  EncChunk ch;
  TFC_HIP(ch.len.alloc(sizeof(unsigned int) * e->streams, st));
  ch.len_p = ch.len.as<unsigned int>();
  EncParams p;
  p.tab = view_of(t);
  p.index = index;
  p.streams = e->streams;
  p.elems = elems;
  p.calls = nullptr;
  p.first_error = e->status.as<unsigned long long>();
  p.state = e->state.as<uint4>();
  p.chunk = nullptr;
  p.chunk_off = nullptr;
  p.chunk_len = ch.len.as<unsigned int>();
  p.overflow_flag = e->oflag.as<unsigned int>();
  p.guard = nullptr;
  p.cap_total = 0;
  unsigned long long host_status[4] = {~0ull, 0ull, 0ull, 0ull};

  // wave-per-stream families: validation + exact output bound first (one read-back)
  DevBuf calls, cstat;
  TFC_HIP(calls.alloc(sizeof(unsigned long long) * e->streams, st));
  TFC_HIP(cstat.alloc(sizeof(unsigned long long) * 3, st));
  TFC_HIP(hipMemsetAsync(calls.p, 0, sizeof(unsigned long long) * e->streams, st));
  // cstat[0] = first error position, [1] = total capacity, [2] = coder calls of all streams
  TFC_HIP(hipMemsetAsync(cstat.p, 0xFF, sizeof(unsigned long long), st));
  TFC_HIP(hipMemsetAsync(cstat.as<unsigned long long>() + 1, 0, 2 * sizeof(unsigned long long), st));
  TFC_HIP(ch.off.alloc(sizeof(long long) * (e->streams + 1), st));
  p.calls = calls.as<unsigned long long>();
  p.first_error = cstat.as<unsigned long long>();
  p.chunk_off = ch.off.as<long long>();

  const int64_t tiles = ceil_div(elems, kCountTile);
  if (e->streams * tiles > kMaxGridX) return fail("encode call too large for one launch");
  const size_t count_lds = p.tab.ntab <= kCountLdsRows ? sizeof(int) * p.tab.ntab : 0;
  hipLaunchKernelGGL((enc_count_kernel<Src>), dim3(static_cast<unsigned>(e->streams * tiles)),
                     dim3(256), count_lds, st, p, src);
  hipLaunchKernelGGL(enc_offsets_kernel, dim3(1), dim3(1024), 0, st, p.calls, p.state,
                     e->family == kFast ? 1 : 0, e->streams, ch.off.as<long long>(),
                     cstat.as<unsigned long long>() + 1);
  unsigned long long count_status[3] = {~0ull, 0ull, 0ull};
  auto record_error = [&] {      // value / index behind the handle's first error position
    EncErrJobs<Src> errs;
    errs.elems = elems;
    errs.ntab = p.tab.ntab;
    errs.n = 1;
    errs.job[0].status = e->status.as<unsigned long long>();
    errs.job[0].src = src;
    errs.job[0].index = index;
    hipLaunchKernelGGL((enc_error_kernel<Src>), dim3(1), dim3(64), 0, st, errs);
  };
  if (e->deferred) {
    // no read-back: the slab is sized from the geometry alone and the coding pass checks the counting
    // pass's verdict on the device (EncParams::guard); an error or an outgrown slab surfaces at
    // tfc_encoder_status / tfc_encoder_finalize, as for the lane kernels
    count_status[1] = speculative_slab_bytes(t, e->streams, elems);
    p.guard = cstat.as<unsigned long long>();
    p.cap_total = count_status[1];
    hipLaunchKernelGGL(enc_defer_kernel, dim3(1), dim3(1), 0, st, cstat.as<unsigned long long>(),
                       e->status.as<unsigned long long>());
    record_error();
  } else {
  TFC_HIP(hipMemcpyAsync(count_status, cstat.p, sizeof(count_status), hipMemcpyDeviceToHost, st));
  TFC_HIP(hipStreamSynchronize(st));
  if (count_status[0] != ~0ull) {
    // nothing was appended; fetch the offending element for the message
    TFC_HIP(hipMemcpyAsync(e->status.p, count_status, sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    record_error();
    TFC_HIP(hipMemcpyAsync(host_status, e->status.p, sizeof(host_status), hipMemcpyDeviceToHost, st));
    const unsigned long long clear[4] = {~0ull, 0ull, 0ull, 0ull};
    TFC_HIP(hipStreamSynchronize(st));
    TFC_HIP(hipMemcpyAsync(e->status.p, clear, sizeof(clear), hipMemcpyHostToDevice, st));
    TFC_HIP(hipStreamSynchronize(st));
    const int rc = encoder_error(e, host_status);
    e->poisoned = false;      // the validation pass runs before anything is appended
    return rc;
  }

  }
  TFC_HIP(ch.data.alloc(count_status[1], st));
  ch.data_bytes = count_status[1];
  p.chunk = ch.data.as<uint8_t>();
  const size_t lds = table_lds_bytes(t);
  const unsigned blocks = static_cast<unsigned>(ceil_div(e->streams, kWavesPerBlock));
  if (e->family == kFast) {
    KernelTimer timer("enc_kernel", st);
    if (int rc = launch(&enc_fast_kernel<Src>, dim3(static_cast<unsigned>(ceil_div(e->streams, e->fast_waves))),
                        dim3(64 * e->fast_waves), e->fast_lds, st, p, src))
      return rc;
  } else {
    KernelTimer timer("enc_kernel", st);
    if (int rc = lds ? launch(&enc_kernel<true, Src>, dim3(blocks), dim3(kBlock), lds, st, p, src)
                     : launch(&enc_kernel<false, Src>, dim3(blocks), dim3(kBlock), 0, st, p, src))
      return rc;
  }
  e->chunks.push_back(std::move(ch));
  return 0;
}

// Every encode entry: n handles (same tables, same stream count) as one lane-path batch where all of them code on the
// lane family, else handle by handle.  `name` is the entry's, for its error texts.
template <typename Src>
int encode_jobs(tfc_encoder* const* es, int n, const Src* srcs, const int32_t* const* indexes, int64_t elems,
                hipStream_t st, const char* name) {
  bool batch = elems > 0 && elems < (int64_t{1} << 29);
  for (int k = 0; k < n; ++k) {
    tfc_encoder* e = es[k];
    if (e->finalized) return fail("encoder handle was already finalized");
    if (e->poisoned) return fail("encoder handle met a range error in an earlier call");
    if (elems < 0) return fail("negative element count");
    e->touch(st);
    if (e->tables != es[0]->tables || e->streams != es[0]->streams)
      return fail("%s: handles must share tables and stream count", name);
    if ((indexes && indexes[k]) != (indexes && indexes[0]))
      return fail("%s: either all jobs carry an index or none", name);
    if (e->streams == 0 || e->tables->rows.empty()) batch = false;
    if (batch && e->family < 0) e->family = select_family(e->tables, e->mode, e->streams * n, elems, e->fast);
    if (e->family != kLanes) batch = false;
  }
  if (batch) return encode_lanes(es, n, srcs, indexes, elems, st);
  for (int k = 0; k < n; ++k)
    if (run_encode(es[k], indexes ? indexes[k] : nullptr, elems, srcs[k], st)) return 1;
  return 0;
}

// Calls f(Dtype<T>{}) for the element type of a dtype code (0 float32, 1 bfloat16, 2 float16).
template <typename T> struct Dtype { using type = T; };
template <typename F>
int with_dtype(int dtype, F&& f) {
  switch (dtype) {
    case 0: return f(Dtype<float>{});
    case 1: return f(Dtype<__hip_bfloat16>{});
    case 2: return f(Dtype<__half>{});
    default: return fail("unsupported dtype code %d", dtype);
  }
}

// The quantising encode entries: channel mode (indexes null) or index mode
int encode_values(int n, tfc_encoder* const* es, const void* const* ys, int dtype, const float* qoffset,
                  const int32_t* const* indexes, const int32_t* cdf_offset, int64_t elems, void* stream,
                  const char* name) {
  return with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    std::vector<SymQuant<T>> srcs(n);
    for (int k = 0; k < n; ++k) srcs[k] = SymQuant<T>{static_cast<const T*>(ys[k]), qoffset, cdf_offset};
    return encode_jobs(es, n, srcs.data(), indexes, elems, static_cast<hipStream_t>(stream), name);
  });
}

int check_channels(const tfc_tables* t, int64_t channels) {
  if (channels != static_cast<int64_t>(t->rows.size()))
    return fail("channel count %lld does not match table count %lld",
                static_cast<long long>(channels), static_cast<long long>(t->rows.size()));
  return 0;
}

int check_indexes(int n, const int32_t* const* indexes) {
  if (!indexes) return fail("index is null");
  for (int k = 0; k < n; ++k)
    if (!indexes[k]) return fail("index is null");
  return 0;
}

// A new handle's tables, stream count and LDS plan of enc_fast_kernel: tables + row directory + one call ring per wave.
void plan_encoder(tfc_encoder* e, const tfc_tables* tables, int64_t streams) {
  e->tables = tables;
  e->streams = streams;
  const size_t fixed = sizeof(uint16_t) * ((tables->host.size() + 3) & ~size_t{3}) + sizeof(int2) * tables->rows.size();
  const size_t ring = sizeof(unsigned int) * kRingWords;
  if (!tables->rows.empty() && fixed + ring <= kLdsBytesPerCu) {
    e->fast = true;
    const size_t fit = (kLdsBytesPerCu - fixed) / ring;
    const size_t want = static_cast<size_t>(waves_wanted(streams));
    e->fast_waves = static_cast<int>(std::min(fit, want));
    e->fast_lds = fixed + ring * e->fast_waves;
  }
}

}  // namespace

extern "C" int tfc_encoder_create(const tfc_tables* tables, int64_t streams, void* stream,
                                  tfc_encoder** out) {
  *out = nullptr;
  if (!tables) return fail("tables is null");
  if (streams < 0) return fail("negative stream count");
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::unique_ptr<tfc_encoder> e(new tfc_encoder);
  plan_encoder(e.get(), tables, streams);
  TFC_HIP(e->ctl.alloc(64 + sizeof(uint4) * std::max<int64_t>(streams, 1), st));
  e->status.p = e->ctl.p;
  e->oflag.p = e->ctl.as<uint8_t>() + 32;
  e->state.p = e->ctl.as<uint8_t>() + 64;
  hipLaunchKernelGGL(fill_state_kernel, dim3(static_cast<unsigned>(std::max<int64_t>(1, ceil_div(streams, 256)))),
                     dim3(256), 0, st, e->state.as<uint4>(), streams, make_uint4(0u, 0xFFFFFFFFu, 0u, 0u),
                     e->status.as<unsigned long long>(), e->oflag.as<unsigned int>());
  *out = e.release();
  return 0;
}

// n handles with ONE allocation and ONE initialisation launch (the per-handle driver calls and small
// kernels are a measurable part of a step once the coding kernels of a group share a launch).
extern "C" int tfc_encoder_create_many(const tfc_tables* tables, int64_t streams, int n, void* stream,
                                       tfc_encoder** out) {
  if (!tables) return fail("tables is null");
  if (streams < 0 || n < 0) return fail("negative count");
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int k = 0; k < n; ++k) out[k] = nullptr;
  if (n == 0) return 0;
  const long long ctl_bytes = 64 + static_cast<long long>(sizeof(uint4)) * std::max<int64_t>(streams, 1);
  auto group = std::make_shared<DevBuf>();
  TFC_HIP(group->alloc(static_cast<size_t>(ctl_bytes) * n, st));
  std::vector<std::unique_ptr<tfc_encoder>> made;
  for (int k = 0; k < n; ++k) {
    std::unique_ptr<tfc_encoder> e(new tfc_encoder);
    plan_encoder(e.get(), tables, streams);
    e->ctl_group = group;
    uint8_t* c = group->as<uint8_t>() + k * ctl_bytes;
    e->status.p = c;
    e->oflag.p = c + 32;
    e->state.p = c + 64;
    made.push_back(std::move(e));
  }
  hipLaunchKernelGGL(fill_state_many_kernel,
                     dim3(static_cast<unsigned>(std::max<int64_t>(1, ceil_div(streams, 256))), static_cast<unsigned>(n)),
                     dim3(256), 0, st, group->as<uint8_t>(), ctl_bytes, streams, make_uint4(0u, 0xFFFFFFFFu, 0u, 0u));
  TFC_HIP(hipGetLastError());
  for (int k = 0; k < n; ++k) out[k] = made[k].release();
  return 0;
}

// EntropyEncodeFinalize of n handles without host synchronisation, in three launches where every handle
// holds exactly one piece from the lane-per-stream kernels (what tfc_encoder_encode_many leaves behind);
// otherwise handle by handle.
extern "C" int tfc_encoder_finalize_device_many(int n, tfc_encoder* const* es, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n <= 0) return 0;
  bool batch = n <= kMaxFinalizeJobs;
  for (int k = 0; k < n; ++k) es[k]->touch(st);
  for (int k = 0; k < n && batch; ++k) {
    const tfc_encoder* e = es[k];
    if (e->finalized || e->family != kLanes || e->chunks.size() != 1 || e->streams != es[0]->streams ||
        e->streams == 0 || e->chunks[0].stride != es[0]->chunks[0].stride)
      batch = false;
  }
  if (!batch) {
    for (int k = 0; k < n; ++k)
      if (tfc_encoder_finalize_device(es[k], stream)) return 1;
    return 0;
  }
  const int64_t streams = es[0]->streams;
  FinalizeJobs f;
  f.streams = streams;
  f.n = n;
  const size_t cap = es[0]->chunks[0].data_bytes + 4 * static_cast<size_t>(streams) + 64;     // pieces + Finalize bytes + slack
  f.length_off = static_cast<long long>((sizeof(Tail) * streams + 15) & ~size_t{15});
  f.offsets_off = f.length_off + static_cast<long long>(sizeof(long long)) * streams;
  f.blob_off = (f.offsets_off + static_cast<long long>(sizeof(long long)) * (streams + 1) + 15) & ~15ll;
  f.job_bytes = (f.blob_off + static_cast<long long>(cap) + 255) & ~255ll;
  auto group = std::make_shared<DevBuf>();
  TFC_HIP(group->alloc(static_cast<size_t>(f.job_bytes) * n, st));
  f.base = group->as<uint8_t>();
  for (int k = 0; k < n; ++k) {
    EncChunk& c = es[k]->chunks[0];
    f.job[k].state = es[k]->state.as<uint4>();
    f.job[k].chunk = ChunkRef{c.data.as<uint8_t>(), c.off.as<long long>(), c.len_p, c.stride};
  }
  hipLaunchKernelGGL(enc_tail_many_kernel, dim3(static_cast<unsigned>(ceil_div(streams, 256)), static_cast<unsigned>(n)),
                     dim3(256), 0, st, f);
  hipLaunchKernelGGL(scan_lengths_many_kernel, dim3(static_cast<unsigned>(n)), dim3(1024), 0, st, f);
  hipLaunchKernelGGL(enc_pack_many_kernel,
                     dim3(static_cast<unsigned>(ceil_div(streams, kWavesPerBlock)), static_cast<unsigned>(n)),
                     dim3(kBlock), 0, st, f);
  TFC_HIP(hipGetLastError());
  for (int k = 0; k < n; ++k) {
    tfc_encoder* e = es[k];
    e->result_group = group;
    e->offsets.p = f.base + k * f.job_bytes + f.offsets_off;
    e->blob.p = f.base + k * f.job_bytes + f.blob_off;
    e->blob_capacity = static_cast<int64_t>(cap);
    e->chunks.clear();       // stream-ordered frees behind the pack launch
    e->finalized = true;
  }
  return 0;
}

// (measurement aid, not part of the ABI: tools/chain_clock_probe.py)
extern "C" int tfc_debug_pipe_clocks(unsigned long long* out8) {
  TFC_HIP(hipDeviceSynchronize());
  TFC_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(tfc::g_pipe_clock), 8 * sizeof(unsigned long long)));
  return 0;
}
extern "C" int tfc_debug_pipe_window(int64_t* phases, int64_t* refills, int64_t* index_refills) {
  unsigned long long v[3] = {0, 0, 0};
  TFC_HIP(hipDeviceSynchronize());
  TFC_HIP(hipMemcpyFromSymbol(v, HIP_SYMBOL(tfc::g_pipe_window), sizeof(v)));
  if (phases) *phases = static_cast<int64_t>(v[0]);
  if (refills) *refills = static_cast<int64_t>(v[1]);
  if (index_refills) *index_refills = static_cast<int64_t>(v[2]);
  return 0;
}
extern "C" int tfc_debug_enc_clocks(unsigned long long* out4) {
  TFC_HIP(hipDeviceSynchronize());
  TFC_HIP(hipMemcpyFromSymbol(out4, HIP_SYMBOL(tfc::g_enc_clock), 4 * sizeof(unsigned long long)));
  return 0;
}

extern "C" int tfc_pipe_counters(int64_t* launches, int64_t* fallback_blocks) {
  if (launches) *launches = pipe_launches().load();
  if (fallback_blocks) {
    unsigned long long v = 0;
    TFC_HIP(hipDeviceSynchronize());
    TFC_HIP(hipMemcpyFromSymbol(&v, HIP_SYMBOL(tfc::g_pipe_fallback_blocks), sizeof(v)));
    *fallback_blocks = static_cast<int64_t>(v);
  }
  return 0;
}

extern "C" int tfc_set_pipe_format(int format, int waves_per_workgroup) {
  if (format < 0 || format > 2 || waves_per_workgroup < 0 || waves_per_workgroup > 8) {
    tfc::fail("tfc_set_pipe_format: format 0 ... 2, waves per workgroup 0 ... 8");
    return -1;
  }
  pipe_waves_value().store(waves_per_workgroup);
  return pipe_format_value().exchange(format);
}

extern "C" int tfc_encoder_set_mode(tfc_encoder* e, int mode) {
  if (mode != TFC_MODE_AUTO && mode != TFC_MODE_LATENCY && mode != TFC_MODE_THROUGHPUT)
    return fail("unknown mode %d", mode);
  if (e->family >= 0) return fail("the mode of a handle is fixed by its first coding call");
  e->mode = mode;
  return 0;
}

extern "C" int tfc_encoder_set_deferred_errors(tfc_encoder* e, int on) {
  e->deferred = on != 0;
  return 0;
}

extern "C" int tfc_encoder_encode(tfc_encoder* e, const int32_t* value, const int32_t* index,
                                  int64_t elems, void* stream) {
  const SymInt32 src{value};
  return encode_jobs(&e, 1, &src, &index, elems, static_cast<hipStream_t>(stream), "tfc_encoder_encode");
}

extern "C" int tfc_encoder_encode_many(int n, tfc_encoder* const* es, const int32_t* const* values,
                                       const int32_t* const* indexes, int64_t elems, void* stream) {
  if (n <= 0) return 0;
  std::vector<SymInt32> srcs(n);
  for (int k = 0; k < n; ++k) srcs[k] = SymInt32{values[k]};
  return encode_jobs(es, n, srcs.data(), indexes, elems, static_cast<hipStream_t>(stream), "tfc_encoder_encode_many");
}

extern "C" int tfc_encoder_encode_quantized(tfc_encoder* e, const void* y, int dtype,
                                            const float* qoffset, const int32_t* cdf_offset,
                                            int64_t channels, int64_t elems, void* stream) {
  if (check_channels(e->tables, channels)) return 1;
  return encode_values(1, &e, &y, dtype, qoffset, nullptr, cdf_offset, elems, stream, "tfc_encoder_encode_quantized");
}

extern "C" int tfc_encoder_encode_quantized_indexed(tfc_encoder* e, const void* y, int dtype,
                                                    const int32_t* index,
                                                    const int32_t* cdf_offset, int64_t elems,
                                                    void* stream) {
  if (check_indexes(1, &index)) return 1;
  return encode_values(1, &e, &y, dtype, nullptr, &index, cdf_offset, elems, stream,
                       "tfc_encoder_encode_quantized_indexed");
}

// EntropyEncodeChannel with the quantise prologue for n independent handles (same tables, same geometry) as one
// coding launch — tfc_encoder_encode_quantized x tfc_encoder_encode_many.
extern "C" int tfc_encoder_encode_quantized_many(int n, tfc_encoder* const* es, const void* const* ys, int dtype,
                                                 const float* qoffset, const int32_t* cdf_offset,
                                                 int64_t channels, int64_t elems, void* stream) {
  if (n <= 0) return 0;
  if (check_channels(es[0]->tables, channels)) return 1;
  return encode_values(n, es, ys, dtype, qoffset, nullptr, cdf_offset, elems, stream,
                       "tfc_encoder_encode_quantized_many");
}

// EntropyEncodeIndex with the quantise prologue for n independent handles (same tables, same geometry) as one
// coding launch — tfc_encoder_encode_quantized_indexed x tfc_encoder_encode_many: the main latents of several
// batches of a hyperprior model (continuous_indexed.py:355-386) behind one launch.
extern "C" int tfc_encoder_encode_quantized_indexed_many(int n, tfc_encoder* const* es, const void* const* ys, int dtype,
                                                         const int32_t* const* indexes, const int32_t* cdf_offset,
                                                         int64_t elems, void* stream) {
  if (n <= 0) return 0;
  if (check_indexes(n, indexes)) return 1;
  return encode_values(n, es, ys, dtype, nullptr, indexes, cdf_offset, elems, stream,
                       "tfc_encoder_encode_quantized_indexed_many");
}

namespace {

// Tail + lengths + offsets on the device; `exact` = synchronise to size the blob exactly, otherwise
// the blob gets the slabs' total capacity and nothing is read back.
int finalize_impl(tfc_encoder* e, hipStream_t st, bool exact) {
  e->touch(st);
  if (e->finalized) return 0;
  const int64_t n = e->streams;
  TFC_HIP(e->offsets_own.alloc(sizeof(long long) * (n + 1), st));
  e->offsets.p = e->offsets_own.p;
  if (n == 0) {
    TFC_HIP(hipMemsetAsync(e->offsets.p, 0, sizeof(long long), st));
    TFC_HIP(e->blob_own.alloc(0, st));
    e->blob.p = e->blob_own.p;
    e->blob_capacity = 0;
    e->total = 0;
    e->total_known = true;
    e->finalized = true;
    return 0;
  }
  std::vector<ChunkRef> refs;
  size_t capacity = 4 * static_cast<size_t>(n) + 64;   // Finalize bytes (<= 2 per stream) + slack
  for (auto& c : e->chunks) {
    refs.push_back(ChunkRef{c.data.as<uint8_t>(), c.off.as<long long>(), c.len_p, c.stride});
    capacity += c.data_bytes;
  }
  DevBuf d_refs, tail, length;
  ChunkList list;
  list.more = nullptr;
  list.n = static_cast<int>(refs.size());
  if (refs.size() <= static_cast<size_t>(kInlineChunks)) {
    for (size_t i = 0; i < refs.size(); ++i) list.inline_refs[i] = refs[i];
  } else {
    TFC_HIP(d_refs.alloc(sizeof(ChunkRef) * refs.size(), st));
    TFC_HIP(hipMemcpyAsync(d_refs.p, refs.data(), sizeof(ChunkRef) * refs.size(), hipMemcpyHostToDevice, st));
    TFC_HIP(hipStreamSynchronize(st));               // `refs` goes away with this frame
    list.more = d_refs.as<ChunkRef>();
  }
  TFC_HIP(tail.alloc((sizeof(Tail) + sizeof(long long)) * n + 16, st));
  long long* const length_p = reinterpret_cast<long long*>(tail.as<uint8_t>() + ((sizeof(Tail) * n + 15) & ~size_t{15}));
  const unsigned tb = static_cast<unsigned>(ceil_div(n, 256));
  hipLaunchKernelGGL(enc_tail_kernel, dim3(tb), dim3(256), 0, st, e->state.as<uint4>(), n,
                     list, static_cast<int>(refs.size()), e->family != kGeneric ? 1 : 0,
                     tail.as<Tail>(), length_p);
  hipLaunchKernelGGL(scan_lengths_kernel, dim3(1), dim3(1024), 0, st, length_p, n,
                     e->offsets.as<long long>());
  if (exact) {
    long long total = 0;
    unsigned int oflag = 0;
    unsigned long long host_status[4];
    TFC_HIP(hipMemcpyAsync(&total, e->offsets.as<long long>() + n, sizeof(long long),
                           hipMemcpyDeviceToHost, st));
    TFC_HIP(hipMemcpyAsync(&oflag, e->oflag.p, sizeof(oflag), hipMemcpyDeviceToHost, st));
    TFC_HIP(hipMemcpyAsync(host_status, e->status.p, sizeof(host_status), hipMemcpyDeviceToHost, st));
    TFC_HIP(hipStreamSynchronize(st));
    if (host_status[0] != ~0ull) return encoder_error(e, host_status);
    if (oflag) return fail("a stream outgrew its output slab (more than 16 bits per symbol on average with "
                           "deferred errors on: encode with tfc_encoder_set_deferred_errors(e, 0))");
    capacity = static_cast<size_t>(total) + 64;
    e->total = total;
    e->total_known = true;
  }
  TFC_HIP(e->blob_own.alloc(capacity, st));
  e->blob.p = e->blob_own.p;
  e->blob_capacity = static_cast<int64_t>(capacity);
  hipLaunchKernelGGL(enc_pack_kernel, dim3(static_cast<unsigned>(ceil_div(n, kWavesPerBlock))),
                     dim3(kBlock), 0, st, n, list, static_cast<int>(refs.size()),
                     tail.as<Tail>(), e->offsets.as<long long>(), e->blob.as<uint8_t>());
  TFC_HIP(hipGetLastError());
  e->chunks.clear();     // stream-ordered frees: no need to wait for the pack kernel here
  e->finalized = true;
  return 0;
}

}  // namespace

extern "C" int tfc_encoder_finalize(tfc_encoder* e, void* stream, int64_t* total_bytes) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (e->finalized && !e->total_known) {
    const int rc = tfc_encoder_status(e, stream, total_bytes);
    return rc;
  }
  if (finalize_impl(e, st, true)) return 1;
  *total_bytes = e->total;
  return 0;
}

extern "C" int tfc_encoder_finalize_device(tfc_encoder* e, void* stream) {
  return finalize_impl(e, static_cast<hipStream_t>(stream), false);
}

extern "C" int tfc_encoder_status(tfc_encoder* e, void* stream, int64_t* total_bytes) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  e->touch(st);
  unsigned int oflag = 0;
  unsigned long long host_status[4];
  long long total = 0;
  TFC_HIP(hipMemcpyAsync(&oflag, e->oflag.p, sizeof(oflag), hipMemcpyDeviceToHost, st));
  TFC_HIP(hipMemcpyAsync(host_status, e->status.p, sizeof(host_status), hipMemcpyDeviceToHost, st));
  if (e->finalized && !e->total_known)
    TFC_HIP(hipMemcpyAsync(&total, e->offsets.as<long long>() + e->streams, sizeof(long long),
                           hipMemcpyDeviceToHost, st));
  TFC_HIP(hipStreamSynchronize(st));
  if (host_status[0] != ~0ull) return encoder_error(e, host_status);
  if (oflag) return fail("a stream outgrew its output slab (more than 16 bits per symbol on average with "
                         "deferred errors on: encode with tfc_encoder_set_deferred_errors(e, 0))");
  if (e->finalized && !e->total_known) {
    e->total = total;
    e->total_known = true;
  }
  if (total_bytes) *total_bytes = e->finalized ? e->total : -1;
  return 0;
}

extern "C" int tfc_encoder_result(const tfc_encoder* e, const uint8_t** blob, const int64_t** offsets) {
  if (!e->finalized) return fail("encoder handle is not finalized");
  *blob = e->blob.as<uint8_t>();
  *offsets = e->offsets.as<int64_t>();
  return 0;
}

extern "C" int tfc_encoder_capacity(const tfc_encoder* e, int64_t* bytes) {
  if (!e->finalized) return fail("encoder handle is not finalized");
  *bytes = e->blob_capacity;
  return 0;
}

extern "C" int tfc_encoder_read(const tfc_encoder* e, uint8_t* blob_dst, int64_t* offsets_dst,
                                int dst_on_device, void* stream) {
  if (!e->finalized) return fail("encoder handle is not finalized");
  if (!e->total_known) return fail("tfc_encoder_status must read the size of a device-finalized handle first");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipMemcpyKind k = dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (offsets_dst)
    TFC_HIP(hipMemcpyAsync(offsets_dst, e->offsets.p, sizeof(int64_t) * (e->streams + 1), k, st));
  if (blob_dst && e->total)
    TFC_HIP(hipMemcpyAsync(blob_dst, e->blob.p, static_cast<size_t>(e->total), k, st));
  if (!dst_on_device) TFC_HIP(hipStreamSynchronize(st));
  return 0;
}

extern "C" void tfc_encoder_destroy(tfc_encoder* e) { delete e; }

// ===========================================================================
// Host side: decoder
// ===========================================================================

struct tfc_decoder {
  const tfc_tables* tables = nullptr;
  int64_t streams = 0;
  int mode = TFC_MODE_AUTO;
  DevBuf blob, offsets, ctl;               // blob / offsets: owned copies of host input only
  std::shared_ptr<DevBuf> ctl_group;       // create_many: ctl is a slice of a shared allocation
  DevView state, status;                   // uint4 [streams]; u64 first index error (views of ctl)
  const uint8_t* blob_p = nullptr;         // device bytes the kernels read (owned or borrowed)
  const long long* off_p = nullptr;
  void touch(hipStream_t s) {              // released in the order of the stream that used the handle last
    blob.touch(s);
    offsets.touch(s);
    ctl.touch(s);
    if (ctl_group) ctl_group->touch(s);
  }
};

extern "C" int tfc_decoder_create(const tfc_tables* tables, const uint8_t* blob,
                                  const int64_t* offsets, int64_t streams, int src_on_device,
                                  void* stream, tfc_decoder** out) {
  *out = nullptr;
  if (!tables) return fail("tables is null");
  if (streams < 0) return fail("negative stream count");
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::unique_ptr<tfc_decoder> d(new tfc_decoder);
  d->tables = tables;
  d->streams = streams;
  if (src_on_device) {
    // Borrowed, like the reference's decoder, which reads its source in place and requires the
    // caller to keep it alive (cc/lib/range_coder.h:74-77): no copy, no size read-back, no sync.
    d->blob_p = blob;
    d->off_p = reinterpret_cast<const long long*>(offsets);
  } else {
    const int64_t total = offsets[streams];
    TFC_HIP(d->offsets.alloc(sizeof(int64_t) * (streams + 1), st));
    TFC_HIP(hipMemcpyAsync(d->offsets.p, offsets, sizeof(int64_t) * (streams + 1), hipMemcpyHostToDevice, st));
    TFC_HIP(d->blob.alloc(static_cast<size_t>(total), st));
    if (total) TFC_HIP(hipMemcpyAsync(d->blob.p, blob, static_cast<size_t>(total), hipMemcpyHostToDevice, st));
    d->blob_p = d->blob.as<uint8_t>();
    d->off_p = d->offsets.as<long long>();
  }
  TFC_HIP(d->ctl.alloc(16 + sizeof(uint4) * std::max<int64_t>(streams, 1), st));
  d->status.p = d->ctl.p;
  d->state.p = d->ctl.as<uint8_t>() + 16;
  hipLaunchKernelGGL(dec_open_kernel, dim3(static_cast<unsigned>(std::max<int64_t>(1, ceil_div(streams, 256)))),
                     dim3(256), 0, st, d->blob_p, d->off_p, streams, d->state.as<uint4>(),
                     d->status.as<unsigned long long>());
  if (!src_on_device) TFC_HIP(hipStreamSynchronize(st));  // host buffers may go away
  *out = d.release();
  return 0;
}

// n decoders on the device-resident strings of n finalized encoders (borrowed, like tfc_decoder_create
// with src_on_device): one allocation, one launch.
extern "C" int tfc_decoder_create_many(const tfc_tables* tables, int n, tfc_encoder* const* from, void* stream,
                                       tfc_decoder** out) {
  if (!tables) return fail("tables is null");
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int k = 0; k < n; ++k) out[k] = nullptr;
  if (n <= 0) return 0;
  for (int k = 0; k < n; ++k) {
    if (!from[k]->finalized) return fail("encoder handle is not finalized");
    if (from[k]->streams != from[0]->streams) return fail("tfc_decoder_create_many: handles must share the stream count");
  }
  const int64_t streams = from[0]->streams;
  std::vector<std::unique_ptr<tfc_decoder>> made;
  for (int g0 = 0; g0 < n; g0 += kMaxDecoderJobs) {
    const int gn = std::min(kMaxDecoderJobs, n - g0);
    DecoderJobs f;
    f.streams = streams;
    f.n = gn;
    f.ctl_bytes = 16 + static_cast<long long>(sizeof(uint4)) * std::max<int64_t>(streams, 1);
    auto group = std::make_shared<DevBuf>();
    TFC_HIP(group->alloc(static_cast<size_t>(f.ctl_bytes) * gn, st));
    f.ctl = group->as<uint8_t>();
    for (int k = 0; k < gn; ++k) {
      std::unique_ptr<tfc_decoder> d(new tfc_decoder);
      d->tables = tables;
      d->streams = streams;
      d->blob_p = from[g0 + k]->blob.as<uint8_t>();
      d->off_p = from[g0 + k]->offsets.as<long long>();
      d->ctl_group = group;
      d->status.p = f.ctl + k * f.ctl_bytes;
      d->state.p = f.ctl + k * f.ctl_bytes + 16;
      f.job[k].blob = d->blob_p;
      f.job[k].off = d->off_p;
      f.job[k].ok = nullptr;
      made.push_back(std::move(d));
    }
    hipLaunchKernelGGL(dec_open_many_kernel,
                       dim3(static_cast<unsigned>(std::max<int64_t>(1, ceil_div(streams, 256))), static_cast<unsigned>(gn)),
                       dim3(256), 0, st, f);
  }
  TFC_HIP(hipGetLastError());
  for (int k = 0; k < n; ++k) out[k] = made[k].release();
  return 0;
}

// EntropyDecodeFinalize of n handles, no synchronisation: ok DEV uint8 [n, streams].
extern "C" int tfc_decoder_finalize_device_many(int n, tfc_decoder* const* ds, uint8_t* ok, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n <= 0) return 0;
  for (int k = 0; k < n; ++k) ds[k]->touch(st);
  const int64_t streams = ds[0]->streams;
  for (int g0 = 0; g0 < n; g0 += kMaxDecoderJobs) {
    const int gn = std::min(kMaxDecoderJobs, n - g0);
    // handles of one create_many group sit at a fixed stride; anything else goes handle by handle
    bool strided = streams > 0 && ds[g0]->ctl_group != nullptr;
    const long long ctl_bytes = 16 + static_cast<long long>(sizeof(uint4)) * std::max<int64_t>(streams, 1);
    for (int k = 0; k < gn && strided; ++k)
      if (ds[g0 + k]->ctl_group != ds[g0]->ctl_group || ds[g0 + k]->streams != streams ||
          ds[g0 + k]->status.as<uint8_t>() != ds[g0]->status.as<uint8_t>() + k * ctl_bytes)
        strided = false;
    if (!strided) {
      for (int k = 0; k < gn; ++k)
        if (tfc_decoder_finalize_device(ds[g0 + k], ok + (g0 + k) * ds[g0 + k]->streams, stream)) return 1;
      continue;
    }
    DecoderJobs f;
    f.streams = streams;
    f.n = gn;
    f.ctl_bytes = ctl_bytes;
    f.ctl = ds[g0]->status.as<uint8_t>();
    for (int k = 0; k < gn; ++k) {
      f.job[k].blob = ds[g0 + k]->blob_p;
      f.job[k].off = ds[g0 + k]->off_p;
      f.job[k].ok = ok + (g0 + k) * streams;
    }
    hipLaunchKernelGGL(dec_close_many_kernel,
                       dim3(static_cast<unsigned>(ceil_div(streams, 256)), static_cast<unsigned>(gn)), dim3(256), 0, st, f);
  }
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_decoder_set_mode(tfc_decoder* d, int mode) {
  if (mode != TFC_MODE_AUTO && mode != TFC_MODE_LATENCY && mode != TFC_MODE_THROUGHPUT)
    return fail("unknown mode %d", mode);
  d->mode = mode;      // the decoder state has one encoding: the mode may change between calls
  return 0;
}

namespace {

// One wave per stream (dec_fast_kernel where the tables qualify, else dec_kernel) for ONE handle; `job_guard` (or null): a
// device flag without which the launch does nothing.
template <typename Dst>
int launch_wave_decoder(tfc_decoder* d, const int32_t* index, int64_t elems, const Dst& dst, hipStream_t st,
                        const unsigned int* job_guard) {
  const tfc_tables* t = d->tables;
  DecParams p;
  p.tab = view_of(t);
  p.index = index;
  p.streams = d->streams;
  p.elems = elems;
  p.blob = d->blob_p;
  p.off = d->off_p;
  p.state = d->state.as<uint4>();
  p.first_error = d->status.as<unsigned long long>();
  p.only_flagged = nullptr;
  p.job_guard = job_guard;
  p.blocks_after_escape = 64;
  const size_t lds = table_lds_bytes(t);
  const unsigned blocks = static_cast<unsigned>(ceil_div(d->streams, kWavesPerBlock));
  const size_t fast_lds = dec_fast_lds(t);
  if (fast_lds) {
    const int waves = static_cast<int>(waves_wanted(d->streams));
    return launch(&dec_fast_kernel<Dst>, dim3(static_cast<unsigned>(ceil_div(d->streams, waves))), dim3(64 * waves), fast_lds,
                  st, p, dst);
  }
  return lds ? launch(&dec_kernel<true, Dst>, dim3(blocks), dim3(kBlock), lds, st, p, dst)
             : launch(&dec_kernel<false, Dst>, dim3(blocks), dim3(kBlock), 0, st, p, dst);
}

// The regions of a pipelined decode launch's workspace at `base`
inline void bind_workspace(PipeDecArgs* pa, uint8_t* base, const plan::DecLayout& lay, size_t groups) {
  pa->raw = reinterpret_cast<unsigned short*>(base + lay.raw);
  pa->posrec = reinterpret_cast<unsigned int*>(base + lay.posrec);
  pa->state_out = reinterpret_cast<uint4*>(base + lay.state_out);
  pa->kend = reinterpret_cast<unsigned int*>(base + lay.kend);
  pa->rowaddr = reinterpret_cast<unsigned short*>(base + lay.rowaddr);
  pa->fallback = reinterpret_cast<unsigned int*>(base + lay.fallback);
  pa->started = reinterpret_cast<unsigned int*>(base + lay.started);
  pa->progress = reinterpret_cast<unsigned int*>(base + lay.progress);
  pa->tile_done = reinterpret_cast<unsigned int*>(base + lay.tile_done);
  pa->groups = static_cast<int>(groups);
}

// The pipelined kernels of one decode launch (pa bound to its zeroed workspace; pla: the chain's image).
// The chain on the library's own stream, the parse next to it on the caller's: tiles of raw rows are turned
// into elements as the chain releases them, and a second pass behind the chain takes what the first left
// (the last rows, tiles it did not get in time) and commits the successor states.
// (a large launch only: see launch_enc_pipe)
template <typename Dst>
int launch_dec_pipe(const DecLaneJobs<Dst>& jobs, PipeDecArgs pa, const LaneArgs& pla, const plan::DecPipePlan& pipe,
                    const plan::DeviceFacts& dev, const tfc_tables* t, bool indexed, hipStream_t st) {
  const int gn = jobs.n;
  const size_t groups = static_cast<size_t>(pa.groups);
  const int overlap = plan::launch_overlap(dev, groups);
  PipeDecJobs cj;
  cj.streams = jobs.streams;
  cj.elems = jobs.elems;
  cj.blocks_per_job = static_cast<int>(ceil_div(pa.groups_per_job, pipe.pblock / 64));
  cj.n = gn;
  for (int k = 0; k < gn; ++k) cj.job[k] = PipeDecJob{jobs.job[k].blob, jobs.job[k].off, jobs.job[k].state};
  if (indexed) {
    PipeRowJobs rj;
    rj.per_job = jobs.streams * jobs.elems;
    rj.ntab = pla.ntab;
    rj.n = gn;
    for (int k = 0; k < gn; ++k) { rj.job[k].index = jobs.job[k].index; rj.job[k].first_error = jobs.job[k].first_error; }
    hipLaunchKernelGGL(dec_rows_kernel, dim3(static_cast<unsigned>(ceil_div(rj.per_job, 1024)), static_cast<unsigned>(gn)),
                       dim3(256), 0, st, rj, const_cast<unsigned short*>(pa.rowaddr));
  }
  SideFork side(st);
  if (overlap && side.fork()) return 1;
  const hipStream_t cst = side.stream;
  const dim3 cgrid(static_cast<unsigned>(cj.blocks_per_job * gn));
  const dim3 pgrid(static_cast<unsigned>(groups * pipe.tiles));
  const dim3 pgrid_next(static_cast<unsigned>(groups * pipe.ctiles));      // (the tiles every stream is sure to reach)
  {
    KernelTimer t2("dec_chain", cst);
    with_flags(pipe.pairs, indexed, [&](auto P, auto I) {
      hipLaunchKernelGGL((dec_chain_kernel<decltype(I)::value, decltype(P)::value>), cgrid, dim3(pipe.pblock), pipe.plds, cst, cj, pla, pa);
    });
  }
  const PipePairMap pm{t->d_pair_adjust.as<int>()};
  auto parse = [&](int concurrent) {
    pa.concurrent = concurrent;
    const dim3 g = concurrent ? pgrid_next : pgrid;
    const DecRow* dd = t->d_dec_dir.as<DecRow>();
    with_flags(pipe.pairs, indexed, [&](auto P, auto I) {
      hipLaunchKernelGGL((dec_parse_kernel<decltype(I)::value, decltype(P)::value, Dst>), g, dim3(256), 0, st, jobs, pa, dd, pla.ntab, pm);
    });
  };
  if (overlap) {
    KernelTimer t2("dec_parse_next", st);      // (next to the chain: as long as the chain, by construction)
    // (the chain's workgroups first: where one takes a CU's whole LDS it cannot be placed next to parse workgroups)
    hipLaunchKernelGGL(enc_gate_kernel, dim3(1), dim3(1), 0, st, pa.started, cgrid.x, static_cast<long long>(20000));
    parse(1);
  }
  if (int rc = side.join()) return rc;
  {
    KernelTimer t2("dec_parse", st);           // behind the chain: what the first pass left
    parse(0);
  }
  return 0;
}

// Lane-per-stream family: n handles (same tables, same stream count) decoded by one launch per
// kMaxLaneJobs of them.  Where the geometry allows, the pipelined kernels of range_pipe.h take the launch (chain into
// raw rows, then the parallel parse into `dsts`) and the lane-per-stream kernel behind them only decodes the jobs
// they gave up on.
template <typename Dst>
int decode_lanes_many(tfc_decoder* const* ds, int n, const Dst* dsts, const int32_t* const* indexes,
                      int64_t elems, hipStream_t st) {
  const tfc_tables* t = ds[0]->tables;
  const int64_t streams = ds[0]->streams;
  const bool indexed = indexes && indexes[0];
  // the facts, and the plans made of them (range_plan.h)
  const plan::TableFacts tf = table_facts(t);
  const plan::DeviceFacts dev = device_facts();
  constexpr plan::KernelFacts kf = kernel_facts<DecWaveLds<typename Dst::elem>, DecLaneJobs<Dst>::kMax>();
  const plan::LanePlan lanes = plan::lane_plan(tf.lane_dec_bytes, kf, dev, streams * n, indexed);
  const plan::DecPipePlan pipe = plan::dec_pipe_plan(tf, dev, kf, streams, elems, n, indexed);
  LaneArgs la = lane_args(t, t->lane_dec_bytes, lanes);
  if (lanes.fits) {
    const void* fn = with_flags(indexed, [](auto I) { return reinterpret_cast<const void*>(&dec_lanes_kernel<decltype(I)::value, Dst>); });
    if (int rc = allow_dynamic_lds(fn, lanes.lds_bytes)) return rc;
  }
  // the chain's view of the tables: the full image (the lane kernels') or the compact one
  LaneArgs pla = la;
  pla.lds_wave = pipe.lds_wave;
  pla.lds_image = pipe.lds_image;
  if (pipe.pairs) {
    pla.image = t->d_pair_image.as<uint32_t>();
    pla.bytes = t->pair_dec_bytes;
  }
  PipeDecArgs pa;
  pa.groups_per_job = pipe.groups_per_job;
  pa.rows = pipe.rows;
  pa.poll_ticks = 200000;         // 2 ms: the chain releases rows every ~0.2 ms
  if (pipe.enabled) {
    const void* pfn = with_flags(pipe.pairs, indexed, [](auto P, auto I) {
      return reinterpret_cast<const void*>(&dec_chain_kernel<decltype(I)::value, decltype(P)::value>);
    });
    if (int rc = allow_dynamic_lds(pfn, pipe.plds)) return rc;
  }
  if (!pipe.enabled && !lanes.fits) {
    // neither the pipelined kernels nor the lane-per-stream kernel can take the call: one wave per stream
    for (int k = 0; k < n; ++k) {
      KernelTimer timer("dec_kernel", st);
      if (launch_wave_decoder(ds[k], indexed ? indexes[k] : nullptr, elems, dsts[k], st, nullptr)) return 1;
    }
    return 0;
  }
  for (int g0 = 0; g0 < n; g0 += pipe.per_launch) {
    const int gn = std::min(pipe.per_launch, n - g0);
    // 1. the jobs
    DecLaneJobs<Dst> jobs;
    jobs.streams = streams;
    jobs.elems = elems;
    jobs.blocks_per_job = static_cast<int>(ceil_div(streams, lanes.block));
    jobs.n = gn;
    for (int k = 0; k < gn; ++k) {
      tfc_decoder* d = ds[g0 + k];
      DecLaneJob<Dst>& J = jobs.job[k];
      J.dst = dsts[g0 + k];
      J.index = indexed ? indexes[g0 + k] : nullptr;
      J.blob = d->blob_p;
      J.off = d->off_p;
      J.state = d->state.as<uint4>();
      J.first_error = d->status.as<unsigned long long>();
    }
    KernelTimer timer("dec_kernel", st);
    // 2. the workspace of the pipelined kernels
    DevBuf temp;
    const size_t groups = static_cast<size_t>(pipe.groups_per_job) * gn;
    const plan::DecLayout lay = plan::dec_layout(pipe, groups, gn, indexed, streams, elems);
    bool piped = pipe.enabled;
    la.guard = nullptr;
    if (piped && temp.alloc(lay.total, st) != hipSuccess) {
      // no room for the raw rows: the lane-per-stream kernel decodes this launch
      (void)hipGetLastError();
      temp.p = nullptr;
      piped = false;
    }
    if (piped) {
      bind_workspace(&pa, temp.as<uint8_t>(), lay, groups);
      // (kend of a group the chain gave up on stays unset: the parse skips the whole job under its fallback flag)
      TFC_HIP(hipMemsetAsync(temp.as<uint8_t>() + lay.zero_offset, 0, lay.zero_bytes, st));
      // 3. the launches: row addresses (index mode), chain, parse
      pipe_launches().fetch_add(1, std::memory_order_relaxed);
      if (int rc = launch_dec_pipe(jobs, pa, pla, pipe, dev, t, indexed, st)) return rc;
      // 4. ... and the fallback behind them for the jobs they gave up on
      la.guard = pa.fallback;
    }
    const dim3 grid(static_cast<unsigned>(jobs.blocks_per_job * gn));
    if (piped && !pipe_fallback_launch()) {}
    else if (!lanes.fits) {
      // (the tables' lane image does not fit a CU) what the pipelined kernels gave up on — or, without temporaries, the
      // whole launch — on the wave-per-stream kernels, handle by handle under its fallback flag
      for (int k = 0; k < gn; ++k)
        if (launch_wave_decoder(ds[g0 + k], jobs.job[k].index, elems, dsts[g0 + k], st, piped ? pa.fallback + k : nullptr)) return 1;
    }
    else with_flags(indexed, [&](auto I) {
      hipLaunchKernelGGL((dec_lanes_kernel<decltype(I)::value, Dst>), grid, dim3(lanes.block), lanes.lds_bytes, st, jobs, la);
    });
  }
  TFC_HIP(hipGetLastError());
  return 0;
}

// channel mode, bottleneck outputs: the int32 blocks into a stream-ordered temporary, then the dequantise pass
template <typename Dst>
int decode_lanes_dequantized(tfc_decoder* const* ds, int n, const Dst* dsts, int64_t elems, hipStream_t st) {
  const long long per = static_cast<long long>(ds[0]->streams) * elems;
  const int ntab = static_cast<int>(ds[0]->tables->rows.size());
  DevBuf tmp;
  TFC_HIP(tmp.alloc(sizeof(int32_t) * static_cast<size_t>(per) * n, st));
  std::vector<OutInt32> outs(n);
  for (int k = 0; k < n; ++k) outs[k] = OutInt32{tmp.as<int32_t>() + static_cast<long long>(k) * per};
  if (decode_lanes_many(ds, n, outs.data(), static_cast<const int32_t* const*>(nullptr), elems, st)) return 1;
  for (int k = 0; k < n; ++k)
    hipLaunchKernelGGL((lanes_dequantize_kernel<Dst>),
                       dim3(static_cast<unsigned>(ceil_div(elems, 1024)), static_cast<unsigned>(ds[0]->streams)), dim3(256), 0,
                       st, dsts[k], outs[k].out, static_cast<unsigned int>(elems), static_cast<unsigned int>(ntab));
  TFC_HIP(hipGetLastError());
  return 0;
}

// n lane-path handles (same tables, same stream count), lane_call_jobs of them per call
template <typename Dst>
int decode_lanes(tfc_decoder* const* ds, int n, const Dst* dsts, const int32_t* const* indexes, int64_t elems,
                 hipStream_t st) {
  const bool indexed = indexes && indexes[0];
  const int per_call = lane_call_jobs<Dst>(n, indexed);
  for (int g0 = 0; g0 < n; g0 += per_call) {
    const int gn = std::min(per_call, n - g0);
    if constexpr (!is_plain_symbols<Dst>::value) {
      // (the pipelined kernels dequantise in their parse pass)
      if (!indexed && !pipe_enabled()) {
        if (decode_lanes_dequantized(ds + g0, gn, dsts + g0, elems, st)) return 1;
        continue;
      }
    }
    if (decode_lanes_many(ds + g0, gn, dsts + g0, indexed ? indexes + g0 : nullptr, elems, st)) return 1;
  }
  return 0;
}

// Whether a decode call runs on the lane path: select_family chooses the lane family, and the tables' image plus one
// wave's staging fits the CU — the lane-per-stream kernels' own image, or (round 6) the compact image of the pipelined
// decoder, whose fallback is then the wave-per-stream kernel (decode_lanes_many).
template <typename Elem>
bool decodes_on_lanes(const tfc_decoder* d, int64_t streams_in_launch, int64_t elems, bool indexed) {
  const tfc_tables* t = d->tables;
  // (which wave-per-stream kernel runs otherwise is launch_wave_decoder's choice)
  if (select_family(t, d->mode, streams_in_launch, elems, false) != kLanes) return false;
  // (the job limit is no part of the question)
  constexpr plan::KernelFacts kf = kernel_facts<DecWaveLds<Elem>, 0>();
  return plan::decode_fits_lanes(table_facts(t), kf, indexed, kLds, pipe_enabled(), pipe_format());
}

// One handle that decode_jobs did not batch (checked and touched there)
template <typename Dst>
int run_decode(tfc_decoder* d, const int32_t* index, int64_t elems, const Dst& dst, hipStream_t st) {
  if (d->streams == 0 || elems == 0) return 0;
  if (d->tables->rows.empty()) return fail("index=0 not in range [0, 0)");
  if (decodes_on_lanes<typename Dst::elem>(d, d->streams, elems, index != nullptr))
    return decode_lanes(&d, 1, &dst, &index, elems, st);
  KernelTimer timer("dec_kernel", st);
  return launch_wave_decoder(d, index, elems, dst, st, nullptr);
}

// Every decode entry: n handles (same tables, same stream count) as one lane-path batch where all of them decode on
// the lane path, else handle by handle.  `name` is the entry's, for its error texts.
template <typename Dst>
int decode_jobs(tfc_decoder* const* ds, int n, const Dst* dsts, const int32_t* const* indexes, int64_t elems,
                hipStream_t st, const char* name) {
  if (elems < 0) return fail("negative element count");
  for (int k = 0; k < n; ++k) ds[k]->touch(st);
  const bool indexed = indexes && indexes[0];
  bool batch = elems > 0 && elems < (int64_t{1} << 29);
  for (int k = 0; k < n; ++k) {
    const tfc_decoder* d = ds[k];
    if (d->tables != ds[0]->tables || d->streams != ds[0]->streams)
      return fail("%s: handles must share tables and stream count", name);
    if ((indexes && indexes[k]) != indexed) return fail("%s: either all jobs carry an index or none", name);
    if (d->streams == 0 || d->tables->rows.empty()) batch = false;
    if (batch && !decodes_on_lanes<typename Dst::elem>(d, d->streams * n, elems, indexed)) batch = false;
  }
  if (batch) return decode_lanes(ds, n, dsts, indexes, elems, st);
  for (int k = 0; k < n; ++k)
    if (run_decode(ds[k], indexes ? indexes[k] : nullptr, elems, dsts[k], st)) return 1;
  return 0;
}

// The dequantising decode entries: channel mode (indexes null) or index mode
int decode_values(int n, tfc_decoder* const* ds, const int32_t* const* indexes, void* const* ys, int dtype,
                  const float* qoffset, const int32_t* cdf_offset, int64_t elems, void* stream, const char* name) {
  return with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    std::vector<OutDequant<T>> dsts(n);
    for (int k = 0; k < n; ++k) dsts[k] = OutDequant<T>{static_cast<T*>(ys[k]), qoffset, cdf_offset};
    return decode_jobs(ds, n, dsts.data(), indexes, elems, static_cast<hipStream_t>(stream), name);
  });
}

}  // namespace

extern "C" int tfc_decoder_decode(tfc_decoder* d, const int32_t* index, int32_t* out,
                                  int64_t elems, void* stream) {
  const OutInt32 dst{out};
  return decode_jobs(&d, 1, &dst, &index, elems, static_cast<hipStream_t>(stream), "tfc_decoder_decode");
}

extern "C" int tfc_decoder_decode_many(int n, tfc_decoder* const* ds, const int32_t* const* indexes,
                                       int32_t* const* outs, int64_t elems, void* stream) {
  if (n <= 0) return 0;
  std::vector<OutInt32> dsts(n);
  for (int k = 0; k < n; ++k) dsts[k] = OutInt32{outs[k]};
  return decode_jobs(ds, n, dsts.data(), indexes, elems, static_cast<hipStream_t>(stream), "tfc_decoder_decode_many");
}

extern "C" int tfc_decoder_decode_dequantized(tfc_decoder* d, const int32_t* index, void* y,
                                              int dtype, const float* qoffset,
                                              const int32_t* cdf_offset, int64_t channels,
                                              int64_t elems, void* stream) {
  if (!index && check_channels(d->tables, channels)) return 1;
  if (index && qoffset) return fail("qoffset is not supported in index mode");
  return decode_values(1, &d, &index, &y, dtype, qoffset, cdf_offset, elems, stream, "tfc_decoder_decode_dequantized");
}

// EntropyDecodeChannel with the dequantise epilogue for n independent handles as one coding launch.
extern "C" int tfc_decoder_decode_dequantized_many(int n, tfc_decoder* const* ds, void* const* ys, int dtype,
                                                   const float* qoffset, const int32_t* cdf_offset,
                                                   int64_t channels, int64_t elems, void* stream) {
  if (n <= 0) return 0;
  if (check_channels(ds[0]->tables, channels)) return 1;
  return decode_values(n, ds, nullptr, ys, dtype, qoffset, cdf_offset, elems, stream,
                       "tfc_decoder_decode_dequantized_many");
}

// EntropyDecodeIndex with the dequantise epilogue for n independent handles as one coding launch.
extern "C" int tfc_decoder_decode_dequantized_indexed_many(int n, tfc_decoder* const* ds, const int32_t* const* indexes,
                                                           void* const* ys, int dtype, const int32_t* cdf_offset,
                                                           int64_t elems, void* stream) {
  if (n <= 0) return 0;
  if (check_indexes(n, indexes)) return 1;
  return decode_values(n, ds, indexes, ys, dtype, nullptr, cdf_offset, elems, stream,
                       "tfc_decoder_decode_dequantized_indexed_many");
}

extern "C" int tfc_decoder_finalize_device(tfc_decoder* d, uint8_t* ok_dev, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  d->touch(st);
  const int64_t n = d->streams;
  if (n)
    hipLaunchKernelGGL(dec_close_kernel, dim3(static_cast<unsigned>(ceil_div(n, 256))), dim3(256),
                       0, st, d->state.as<uint4>(), d->off_p, n, ok_dev);
  TFC_HIP(hipGetLastError());
  return 0;
}

extern "C" int tfc_decoder_status(tfc_decoder* d, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  d->touch(st);
  unsigned long long first_error = ~0ull;
  TFC_HIP(hipMemcpyAsync(&first_error, d->status.p, sizeof(first_error), hipMemcpyDeviceToHost, st));
  TFC_HIP(hipStreamSynchronize(st));
  if (first_error != ~0ull)
    return fail("index=<element %llu> not in range [0, %lld)", first_error,
                static_cast<long long>(d->tables->rows.size()));
  return 0;
}

extern "C" int tfc_decoder_finalize(tfc_decoder* d, uint8_t* ok, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n = d->streams;
  DevBuf d_ok;
  TFC_HIP(d_ok.alloc(std::max<int64_t>(n, 1), st));
  if (tfc_decoder_finalize_device(d, d_ok.as<uint8_t>(), stream)) return 1;
  if (n) TFC_HIP(hipMemcpyAsync(ok, d_ok.p, n, hipMemcpyDeviceToHost, st));
  return tfc_decoder_status(d, stream);
}

extern "C" void tfc_decoder_destroy(tfc_decoder* d) { delete d; }
