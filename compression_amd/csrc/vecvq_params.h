// The tile sizes and route boundary of vecvq.hip.  ops/vq_ops.py reads this file (`constexpr int NAME = VALUE;` lines)
// and the tests derive their shapes from it, so a retune moves the cases with it.
#pragma once

namespace tfc {

constexpr int VQ_WAVE = 64;
constexpr int VQ_ROWS = 256;             // rows of x per workgroup, one per lane (both forward routes)
constexpr int VQ_NARROW_MAX_D = 32;      // D <= this: the narrow route (a lane's row in registers); above it the wide route
constexpr int VQ_NARROW_CHUNK = 256;     // codewords staged in LDS per step of the narrow route
constexpr int VQ_WIDE_KB = 32;           // codewords per step of the wide route (per-lane partial sums)
constexpr int VQ_WIDE_DT = 16;           // D tile of the wide route (codebook tile in LDS, the lane's x tile in registers)
constexpr int VQ_TARGET_BLOCKS = 512;    // fewer row tiles than this: the codebook is split over grid.y and merged
constexpr int VQ_MAX_SPLITS = 1024;
constexpr int VQ_BWD_KT = 8;             // codewords a backward workgroup owns
constexpr int VQ_BWD_DT = 256;           // D tile of the backward (a lane owns VQ_BWD_DT / VQ_WAVE columns)
constexpr int VQ_BWD_WAVES = 4;          // waves of a backward workgroup, each scanning one contiguous range of n
constexpr int VQ_BWD_BATCH = 4;          // matching rows whose loads are issued together
constexpr int VQ_BWD_SPLIT_ROWS = 2048;  // least rows per n-split of the backward (a multiple of VQ_BWD_WAVES * VQ_WAVE)
constexpr int VQ_BWD_TARGET_BLOCKS = 1024;
constexpr int VQ_BWD_MAX_SPLITS = 64;

}  // namespace tfc
