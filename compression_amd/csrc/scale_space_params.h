// The tile sizes and the argument limits of scale_space.hip.  ops/flow_ops.py reads this file (`constexpr int NAME =
// VALUE;` lines) and the tests derive their tile +- 1 shapes from it, so a retune moves the cases with it.
#pragma once

namespace tfc {

constexpr int SS_THREADS = 256;          // threads of every scale-space workgroup
constexpr int SS_MAX_C = 8;              // channels: [1, SS_MAX_C]
constexpr int SS_MAX_LEVELS = 8;         // blurred planes M: [1, SS_MAX_LEVELS]
constexpr int SS_MAX_SIGMA = 64;         // sigma0 * 2^(M-1) at most
constexpr int SS_MAX_RADIUS = 192;       // ceil(3 * SS_MAX_SIGMA)
constexpr int SS_MAX_TAPS = 400;         // sum over the planes of (radius + 1) at most: 383 + 8
constexpr int SS_MAX_DIM = 16384;        // H and W at most
constexpr int SS_ROW_TILE = 128;         // pixels of one image row per row-pass workgroup
constexpr int SS_COL_TILE_H = 64;        // rows per column-pass workgroup
constexpr int SS_COL_TILE_X = 32;        // floats of a W * C row per column-pass workgroup
constexpr int SS_WARP_TILE = 256;        // output pixels per warp workgroup (one per lane)
constexpr int SS_MAX_PARTS = 1024;       // partial maxima of the two-stage |g| reduction
constexpr int SS_FIXED_BITS = 40;        // a contribution is llrint(g w 2^(SS_FIXED_BITS - e))
constexpr int SS_MAX_HW_LOG2 = 22;       // backward: H * W <= 2^22, so that 2^22 contributions below 2^40 fit 63 bits

}  // namespace tfc
