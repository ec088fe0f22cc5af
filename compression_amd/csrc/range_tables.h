// The table set of a coder handle: the raw lookup and the four device images built from it (range_tables.hip).
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"
#include "range_coder_device.h"

struct tfc_tables {
  std::vector<int32_t> host;       // raw lookup
  std::vector<int2> rows;          // (start of header, ints incl. header)
  tfc::DevBuf d_data, d_rows;
  tfc::DevBuf d_fast, d_rows_fast;      // encoder LDS image (uint16, entries scaled to 16-bit precision) + its rows
  tfc::DevBuf d_dec_image, d_dec_dir;   // decoder LDS image: d_fast + pad + pivot arrays; row directory
  int dec_words = 0;
  bool dec_fast_ok = false;
  // lane-per-stream kernels (range_lanes.h): one LDS image; the encoder uses its first lane_enc_bytes
  tfc::DevBuf d_lane_image;
  int lane_enc_bytes = 0, lane_dec_bytes = 0, lane_precision = 0;
  bool lanes_ok = false;
  // the pipelined decoder's COMPACT image (range_pipe.h, dec_chain_kernel<..., true>): bitmaps of every second bound at
  // PAIR resolution (one bit per two quotient values: half the bitmaps' bytes), and per row what dec_parse_kernel adds
  // to a raw entry to have the symbol
  tfc::DevBuf d_pair_image, d_pair_adjust;
  int pair_dec_bytes = 0;
  bool pairs_ok = false;
  int max_abs_prec = 0;
  bool any_escape = false;
  int64_t max_row = 0;
};

namespace tfc {

TableView view_of(const tfc_tables* t);
// Bytes of the raw tables where the generic kernels stage them in LDS, else 0.
size_t table_lds_bytes(const tfc_tables* t);
// LDS bytes of dec_fast_kernel (decoder image + row directory), or 0 where the tables cannot take that kernel.
size_t dec_fast_lds(const tfc_tables* t);

}  // namespace tfc
