// The tile sizes of window_attention.hip.  ops/attention_ops.py reads this file (`constexpr int NAME = VALUE;` lines) and
// the tests derive their shapes from it, so a retune moves the cases with it.
#pragma once

namespace tfc {

constexpr int WA_FWD_WINDOWS_WS8 = 2;      // windows of 8x8 tokens a forward workgroup takes (one lane per token)
constexpr int WA_FWD_WINDOWS_WS4 = 8;      // windows of 4x4 tokens a forward workgroup takes
constexpr int WA_MFMA_WINDOWS_WS8 = 1;     // windows one wave of the bfloat16 (MFMA) forward takes: 64 tokens, two 32-row tiles
constexpr int WA_MFMA_WINDOWS_WS4 = 2;     // 32 tokens, one tile; the cross-window pairs are excluded keys
constexpr int WA_BWD_WINDOWS_WS8 = 1;      // the same for the backward, whose workgroup also holds a [T, T + 1] tile
constexpr int WA_BWD_WINDOWS_WS4 = 4;
constexpr int WA_DTABLE_PARTIALS = 256;    // backward workgroups per head at most: each walks its window groups in a
                                           // fixed order and writes one partial dtable, merged in workgroup order
constexpr int WA_MERGE_THREADS = 256;      // threads of the dtable merge (one per table entry)

}  // namespace tfc
