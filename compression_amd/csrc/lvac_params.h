// The tile sizes and the eligibility range of lvac.hip.  ops/lvac_ops.py reads this file (`constexpr int NAME = VALUE;`
// lines) and the tests derive their shapes from it, so a retune moves the cases with it.
#pragma once

namespace tfc {

constexpr int RAHT_THREADS = 256;        // threads of a RAHT workgroup
constexpr int RAHT_HEAD_ITEMS = 4096;    // consecutive levels of at most this many (child rows x channels) share one launch
constexpr int RAHT_MAX_LEVELS = 64;      // 3 x 21 Morton bits is the deepest tree
constexpr int RAHT_DESC = 10;            // int64 entries of a level's descriptor
constexpr int RAHT_MAX_BLOCKS = 4096;    // workgroups of a one-level launch (grid-stride above that)

constexpr int PM_WAVE = 64;
constexpr int PM_THREADS = 256;          // threads of a point-decoder workgroup: 16 point groups x 16 hidden groups
constexpr int PM_TILE = 128;             // points per workgroup tile (8 per thread)
constexpr int PM_HC = 64;                // hidden units per chunk (4 per thread)
constexpr int PM_DH = 68;                // row stride of the dH tile in LDS (PM_HC + 4: 16-byte rows, spread over banks)
constexpr int PM_MIN_C = 1;              // eligibility: latent channels
constexpr int PM_MAX_C = 32;
constexpr int PM_MIN_H = 1;              // eligibility: hidden units
constexpr int PM_MAX_H = 1024;
constexpr int PM_MAX_K = 35;             // PM_MAX_C + 3 position rows of W1
constexpr int PM_KG = 3;                 // rows of W1 a thread of the parameter kernel owns (16 * PM_KG >= PM_MAX_K)
constexpr int PM_PARAM_GROUPS = 128;     // tile groups of the parameter kernel: one partial gradient each
constexpr int PM_SUM_THREADS = 256;      // threads of the fixed-order sums (loss partials, gradient partials)

}  // namespace tfc
