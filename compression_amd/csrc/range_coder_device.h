// Device-side state of one range-coder stream (wave-uniform values), and the layout of the table images that their
// host builder (range_tables.hip) and the kernels reading them must agree on.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

// clang in ROCm 7.2 has no __builtin_amdgcn_writelane; bind the LLVM intrinsic
// (v_writelane_b32: write a wave-uniform value into one lane of a VGPR).
extern "C" __device__ int tfc_writelane(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

namespace tfc {

// Interval [base, base + span_m1] in a 32-bit window plus the unresolved carry:
// pend_digit = (undecided 16-bit digit + 1) or 0; pend_bytes = further
// undecided bytes behind it (always even).  Same information as
// RangeEncoder::{base_, size_minus1_, delay_} (cc/lib/range_coder.h:67-69).
struct EncoderState {
  unsigned int base;
  unsigned int span_m1;
  unsigned int pend_digit;
  unsigned int pend_bytes;
};

// Directory entry of the lane-per-stream kernels' LDS image (range_lanes.h): byte offsets inside the
// image of the row's cdf entries (minus 2: the lower bound of symbol s is at cdf + 2 s + 2), boundary
// bitmap and running counts, and
//   info = limit | has_escape << 31,  limit = number of plain symbols (= index of the escape symbol).
struct LaneRow { unsigned int cdf, info, bits, cum; };

// The directory of that image repeats its first entries behind its end: a hand-scheduled block of kEncCadence /
// kDecCadence steps (the steps between two memory phases) reads that many consecutive entries without a wrap test.
constexpr unsigned int kDirRepeat = 16;
constexpr unsigned int kEncCadence = 16;
constexpr unsigned int kDecCadence = 16;
static_assert(kEncCadence <= kDirRepeat && kDecCadence <= kDirRepeat, "a block reads cadence consecutive directory entries");

// Row directory entry of the wave-per-stream decoder's LDS image (range_decoder_fast.h).
//   x: index of the first stage-1 upper bound (narrow: cdf0 + 1, wide: pivot array)
//   y: index of cdf[0]
//   z: nsym | chunk << 16   (chunk = symbols per pivot; 1 for narrow rows)
//   w: escape symbol index (nsym - 1) if the row has negative precision, else -1
struct DecRow { int x, y, z, w; };

// Tables up to this many bytes are staged in LDS (160 KiB per CU on gfx950).
constexpr size_t kLdsTableBytes = 144 * 1024;

struct TableView {
  const int32_t* data;
  const uint16_t* fast16;     // encoder LDS image: entries scaled to 16-bit precision, modulo 2^16
  const int2* rows_fast;      // (offset, length | escape row << 31) per table, for that image
  const int32_t* dec_image;   // decoder LDS image (see tfc_tables_create, range_tables.hip)
  const DecRow* dec_dir;
  int dec_words;
  const int2* rows;
  int ntab;
  int total;
};

}  // namespace tfc
