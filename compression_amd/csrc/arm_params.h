// The context offsets, tile sizes and argument limits of arm_bits.hip.  ops/arm_ops.py reads this file (the
// `constexpr int NAME = VALUE;` lines and the two offset tables), and the tests derive their shapes from it.
#pragma once

namespace tfc {

constexpr int ARM_MAX_C = 32;            // context size C is one of 8, 16, 24, 32 (= hidden width)
constexpr int ARM_MAX_L = 3;             // residual hidden layers, 1..3
constexpr int ARM_HALO = 4;              // rows above and columns to either side that C = 32 reaches
constexpr int ARM_ROWS = 4;              // rows of a workgroup's tile: one wave per row
constexpr int ARM_COLS = 64;             // columns of a tile: one lane per column
constexpr int ARM_THREADS = 256;         // ARM_ROWS * ARM_COLS, one pixel per thread
constexpr int ARM_TILE_W = 72;           // ARM_COLS + 2 * ARM_HALO: row stride of the staged tile in LDS
constexpr int ARM_GROUPS = 512;          // workgroups of the backward kernel: one partial parameter gradient each
constexpr int ARM_SUM_THREADS = 256;     // threads of the fixed-order sums
constexpr int ARM_MAX_B = 65535;         // grids of one call (the z extent of a launch)

// The causal half-plane (di < 0, or di == 0 and dj < 0) by ascending di^2 + dj^2, then di descending, then dj
// ascending; context k of pixel (i, j) is y[i + ARM_DI[k], j + ARM_DJ[k]], zero outside the grid.
constexpr int ARM_DI[32] = {0, -1, -1, -1, 0, -2, -1, -1, -2, -2, -2, -2, 0, -3, -1, -1,
                            -3, -3, -2, -2, -3, -3, 0, -4, -1, -1, -4, -4, -3, -3, -2, -2};
constexpr int ARM_DJ[32] = {-1, 0, -1, 1, -2, 0, -2, 2, -1, 1, -2, 2, -3, 0, -3, 3,
                            -1, 1, -3, 3, -2, 2, -4, 0, -4, 4, -1, 1, -3, 3, -4, 4};

// scale = exp(clamp(s, ARM_S_MIN, ARM_S_MAX)); bits = -log2(max(p, 2^-ARM_FLOOR_LOG2))
constexpr float ARM_S_MIN = -4.6f;
constexpr float ARM_S_MAX = 5.0f;
constexpr int ARM_FLOOR_LOG2 = 16;

}  // namespace tfc
