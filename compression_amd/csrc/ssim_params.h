// The tap limit, tile sides and route boundaries of ssim.hip.  ops/image_ops.py reads this file (`constexpr int NAME =
// VALUE;` lines) and the tests derive their shapes from it, so a retune moves the cases with it.
#pragma once

namespace tfc {

constexpr int SSIM_MAX_TAPS = 31;        // the taps travel in the kernel arguments
constexpr int SSIM_TILE_SMALL_N = 32;    // tile side (positions forward, pixels backward) for n <= SSIM_TILE_SMALL_N_MAX
constexpr int SSIM_TILE_LARGE_N = 16;    // tile side above it
constexpr int SSIM_TILE_SMALL_N_MAX = 11;
constexpr int SSIM_FIXED_TAPS = 11;      // the tap count with kernels of its own (loops unrolled), on the larger tile

}  // namespace tfc
