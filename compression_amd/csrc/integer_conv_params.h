// The tile sizes and argument limits of integer_conv.hip.  ops/integer_ops.py reads this file (`constexpr int NAME =
// VALUE;` lines) and the tests derive their shapes from it, so a retune moves the cases with it.
#pragma once

namespace tfc {

constexpr int IC_TILE_PIXELS = 16;         // pixels of one v_mfma_i32_16x16x64_i8 tile (its N side, one per lane & 15)
constexpr int IC_TILE_COUTS = 16;          // output channels of one tile (its M side)
constexpr int IC_WAVE_PIXELS = 64;         // pixels a wave takes: four tiles side by side
constexpr int IC_WAVE_COUTS = 64;          // output channels a wave takes: four tiles; 16 accumulator tiles a wave
constexpr int IC_BLOCK_PIXELS = 256;       // pixels a workgroup takes: four waves, each with its own 64
constexpr int IC_CHUNK_CHANNELS = 16;      // input channels one lane hands the MFMA per step (16 bytes); 4 chunks a step
constexpr int IC_CIN_MULTIPLE = 32;        // Cin must be a multiple of this
constexpr int IC_MAX_REDUCTION = 32768;    // kh kw Cin at most: no sum leaves int32
constexpr int IC_MAX_SUPPORT = 9;          // kh, kw at most
constexpr int IC_MAX_DIVISOR_LOG2 = 24;    // 1 <= divisor <= 2^24
constexpr int IC_MAX_BIAS_LOG2 = 29;       // |bias| <= 2^29

}  // namespace tfc
