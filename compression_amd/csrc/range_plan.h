// Launch plans and workspace layouts of the lane path (range_coder.hip: encode_lanes_many, decode_lanes_many): plain
// functions of numbers.  No HIP header, no runtime call, no environment: the call site fills the facts — what the plans
// need of the tables, of the device and the switches, and of the kernels' compile-time sizes — and gets small structs
// back by value.  tests/test_coder_plan_cpu.py compiles this header for the host and holds it to tests/coder_plan_ref.py.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace tfc {
namespace plan {

// What the plans need of the tables (tfc_tables)
struct TableFacts {
  int lane_enc_bytes = 0, lane_dec_bytes = 0, pair_dec_bytes = 0;      // images of the lane kernels / the compact decoder image
  bool pairs_ok = false, any_escape = false;
  int lane_precision = 0;
  size_t entries = 0;          // of the tables scaled to 16 bits (tfc_tables::host)
  int ntab = 0;                // rows
};
// ... of the device and the switches
struct DeviceFacts {
  int cus = 0;
  int lds_bytes = 0;           // of one CU
  size_t temp_bytes = 0;       // temporaries one pipelined launch may take
  bool pipe_enabled = true;
  int format = 0;              // the chain's image: 0 by fit, 1 full, 2 pairs
  int waves_override = 0;      // chain waves per workgroup, 0: by launch size
  int overlap = 0;             // TFC_PIPE_OVERLAP
  bool chip_shared = false;
};
// ... of the kernels: the lane kernels' LDS per wave (of the direction and element type that is planned), the pipelined
// kernels' LDS and tile sizes, and the jobs one launch's argument struct holds
struct KernelFacts {
  int lane_wave_indexed = 0, lane_wave_plain = 0;                      // EncWaveLds / DecWaveLds: kBytes, kIndex
  int dec_lds_bytes = 0, dec_lds_rows = 0, dec_lds_stage = 0;          // PipeDecLds: kBytes, kRows, kStage
  int enc_chain_groups = 0, enc_chain_group = 0, enc_chain_rows = 0;   // PipeEncChainLds: kGroups, kGroup, kRows
  int pipe_tile = 0, pipe_block = 0, parse_rows = 0, expand_tab_bytes = 0;
  int max_jobs = 0;            // EncLaneJobs / DecLaneJobs: kMax
};
// bytes of a coder state (uint4), of a staged (bytes written, slab outgrown) pair (uint2), of a flag word
constexpr size_t kStateBytes = 16, kStageOutBytes = 8, kWord = sizeof(unsigned int);

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// A table image in LDS: whole KiB
inline int lane_image_bytes(int bytes) { return (bytes + 1023) & ~1023; }

// Streams per workgroup of the lane kernels: one wave (64 streams) until the launch fills the chip,
// so that a 512-stream call spreads over eight CUs (and XCDs), then more waves behind each LDS image.
inline int lanes_block(int64_t streams) {
  const int64_t waves = ceil_div(streams, 64);
  const int64_t per = std::min<int64_t>(8, std::max<int64_t>(1, waves / 256));
  return static_cast<int>(64 * per);
}

// A launch of 64 groups and more is a large one: its chain runs on the library's own stream (see launch_enc_pipe)
inline bool large_launch(size_t groups) { return groups >= 64; }
inline int launch_overlap(const DeviceFacts& d, size_t groups) { return large_launch(groups) ? d.overlap : 0; }

// ---- the lane-per-stream kernels ------------------------------------------------------------------------------------
// the lane-per-stream kernel (the pipelined kernels' fallback, or the launch's coder) needs its image + a wave's
// staging in a CU's LDS; tables whose image is larger (bls2017's 192 x 128 symbols: 176 KB) have the wave-per-stream
// kernels as the decoder's fallback, handle by handle (the encoder is given the lane family only where its image fits:
// select_family)
struct LanePlan {
  bool fits = false;
  int lds_image = 0, lds_wave = 0;
  int block = 64;              // threads of a workgroup
  int lds_bytes = 0;           // of a workgroup
};
inline bool lanes_fit(int image_bytes, int wave_bytes, int lds) { return lane_image_bytes(image_bytes) + wave_bytes <= lds; }
inline LanePlan lane_plan(int image_bytes, const KernelFacts& k, const DeviceFacts& d, int64_t streams_in_call, bool indexed) {
  LanePlan p;
  p.lds_image = lane_image_bytes(image_bytes);
  p.lds_wave = indexed ? k.lane_wave_indexed : k.lane_wave_plain;
  p.fits = lanes_fit(image_bytes, p.lds_wave, d.lds_bytes);
  p.block = p.fits ? std::min(lanes_block(streams_in_call), 64 * ((d.lds_bytes - p.lds_image) / p.lds_wave)) : 64;
  p.lds_bytes = p.lds_image + (p.block / 64) * p.lds_wave;
  return p;
}

// Jobs of one pipelined launch: as many as the launch's argument struct holds, as can be resident at once, and as the
// temporaries' budget hosts
inline int jobs_per_launch(bool pipe, int max_jobs, size_t resident_jobs, size_t temp_bytes, size_t job_bytes) {
  return !pipe ? max_jobs
               : static_cast<int>(std::max<size_t>(1, std::min<size_t>(std::min<size_t>(max_jobs, resident_jobs),
                                                                      temp_bytes / std::max<size_t>(job_bytes, 1))));
}

// A workspace is one allocation; its regions are taken one behind the other, each at its alignment.
struct Bump {
  size_t at = 0;
  size_t take(size_t bytes, size_t align) {
    at = (at + align - 1) & ~(align - 1);
    const size_t offset = at;
    at += bytes;
    return offset;
  }
};

// ---- encoder: expansion into call words, then the chain -------------------------------------------------------------
struct EncPipePlan {
  bool enabled = false;
  int nt = 0;                  // tiles per stream
  int rows = 0;                // row capacity of a stream
  int groups_per_job = 0;
  size_t job_bytes = 0;        // temporaries of a job
  int tab_entries = 0;         // PipeEncArgs::tab_entries
  int chain_lds = 0;           // LDS of a large launch's chain workgroup
  int per_launch = 0;          // jobs
};
inline EncPipePlan enc_pipe_plan(const TableFacts& t, const DeviceFacts& d, const KernelFacts& k, int64_t streams, int64_t elems) {
  EncPipePlan p;
  // pipelined launch plan: groups of 64 streams, tiles of kPipeTile symbols; rows (coder calls) per stream: one per
  // symbol, and room for escape codes when the tables have escape rows (half more than the symbols)
  p.nt = static_cast<int>(ceil_div(elems, k.pipe_tile));
  const int64_t rows64 = elems + (t.any_escape ? elems / 2 + 64 : 0);
  p.rows = static_cast<int>(std::min<int64_t>((rows64 + 31) / 32 * 32, int64_t{1} << 30));
  p.groups_per_job = static_cast<int>(ceil_div(streams, 64));
  const size_t group_bytes = static_cast<size_t>(p.rows) * 256 + (kWord * 65 * p.nt) + 64 * (kStateBytes + kStageOutBytes);
  p.job_bytes = group_bytes * p.groups_per_job;
  p.enabled = d.pipe_enabled && rows64 + 2048 < (int64_t{1} << 30) && p.job_bytes <= d.temp_bytes && t.entries <= 65536 &&
              static_cast<int64_t>(p.nt) * p.groups_per_job * k.max_jobs < (int64_t{1} << 31);
  // A launch's chain workgroups must all be resident at once, next to an expansion that needs CUs of its own: a chain
  // workgroup (PipeEncChainLds::kGroups groups) takes a CU's whole LDS, so at most half the CUs go to chains — beyond
  // that the chains starve the expansion they wait for (and time out into the fallback).
  const size_t resident_jobs = std::max<size_t>(1, static_cast<size_t>(d.cus / 2) * k.enc_chain_groups / std::max(1, p.groups_per_job));
  p.per_launch = jobs_per_launch(p.enabled, k.max_jobs, resident_jobs, d.temp_bytes, p.job_bytes);
  p.tab_entries = t.entries * 2 <= static_cast<size_t>(k.expand_tab_bytes) ? static_cast<int>(t.entries) : 0;
  p.chain_lds = k.enc_chain_groups * k.enc_chain_group;
  return p;
}

// The encoder's workspace (offsets in bytes).  Zeroed per launch — nothing known about any tile, no tile released, no
// fallback — are the flag regions: [zero_offset, zero_offset + zero_bytes).
struct EncLayout {
  size_t calls = 0, stage_state = 0, stage_out = 0, status = 0, done = 0, fallback = 0, started = 0;
  size_t total = 0, zero_offset = 0, zero_bytes = 0;
};
inline EncLayout enc_layout(const EncPipePlan& p, const KernelFacts& k, size_t groups) {
  EncLayout l;
  Bump b;
  // (room behind the last group: the one-wave chain requests an iteration's rows ahead)
  l.calls = b.take((groups * 64 * p.rows + 64 * k.enc_chain_rows) * kWord, 256);
  l.stage_state = b.take(groups * 64 * kStateBytes, 16);
  l.stage_out = b.take(groups * 64 * kStageOutBytes, 16);
  l.status = b.take(groups * p.nt * 64 * kWord, 256);
  l.done = b.take(groups * p.nt * kWord, 256);
  l.fallback = b.take(64 * kWord, 256);
  l.started = b.take(64 * kWord, kWord);          // (behind the 64 jobs' flags)
  l.total = b.at;
  l.zero_offset = l.status;
  l.zero_bytes = l.total - l.status;
  return l;
}

// ---- decoder: the chain into raw rows, then the parse -----------------------------------------------------------------
// LDS of a chain wave behind the image: the windows, and the raw entries of a block
inline int dec_chain_wave_bytes(const KernelFacts& k, bool indexed) {
  return (indexed ? k.dec_lds_bytes : k.dec_lds_rows) + k.dec_lds_stage;
}
struct DecPipePlan {
  bool enabled = false;
  bool pairs = false;          // the chain runs on the compact image
  int rows = 0;                // steps of the chain a stream may take
  int groups_per_job = 0;
  size_t raw_bytes = 0, rec_bytes = 0;       // of a group: raw rows, block records
  size_t job_bytes = 0;        // temporaries of a job
  int lds_image = 0, lds_wave = 0;           // the chain's image and its bytes per wave
  int pblock = 0;              // threads of a chain workgroup
  int plds = 0;                // LDS of a chain workgroup
  size_t tiles = 0;            // parse tiles of a group
  size_t ctiles = 0;           // ... that the pass next to the chain takes
  int per_launch = 0;          // jobs
};
inline DecPipePlan dec_pipe_plan(const TableFacts& t, const DeviceFacts& d, const KernelFacts& k, int64_t streams, int64_t elems,
                                 int n, bool indexed) {
  DecPipePlan p;
  const int kLds = d.lds_bytes;
  const int64_t kPipeBlock = k.pipe_block;
  // pipelined launch plan: groups of 64 streams; rows = steps of the chain (one per element, plus the bits of
  // escape codes: a quarter more is planned for when the tables have escape rows)
  p.groups_per_job = static_cast<int>(ceil_div(streams, 64));
  // (+ the blocks lanes sit out or spend finishing an escape code before the wave's tail pass, and the tail pass)
  const int64_t rows64 = ((elems + (t.any_escape ? elems / 4 + 64 + 24 * kPipeBlock : 2 * kPipeBlock)) + kPipeBlock - 1) / kPipeBlock * kPipeBlock;
  p.rows = static_cast<int>(std::min<int64_t>(rows64, (int64_t{1} << 30)));
  p.raw_bytes = static_cast<size_t>(p.rows) * 128;      // 16-bit entries, 64 lanes
  p.rec_bytes = (static_cast<size_t>(p.rows) / kPipeBlock + 1) * 256;
  const size_t group_bytes = p.raw_bytes + p.rec_bytes + 64 * kStateBytes + kWord;
  p.job_bytes = group_bytes * p.groups_per_job + (indexed ? 2 * static_cast<size_t>(streams) * elems : 0);
  p.lds_wave = dec_chain_wave_bytes(k, indexed);
  p.lds_image = lane_image_bytes(t.lane_dec_bytes);
  // Which image the chain runs on, and how many chain waves share a workgroup's copy of it.  A launch's chain
  // workgroups must all be resident at once (a second round doubles the launch's time and the parse next to the chain
  // gives up on groups that do not move), one wave per SIMD at most: the full image where it fits and hosts the call's
  // waves (BASELINE config 2: 150 KB, one wave per CU = 32 batches per launch), else the compact one (92 KB for config 2:
  // four waves per CU, 128 batches per launch; 115 KB for bls2017's tables, whose full image does not fit at all).
  const int64_t waves_call = static_cast<int64_t>(p.groups_per_job) * std::min(n, k.max_jobs);
  auto waves_fit = [&](int image_bytes) { return std::max(0, (kLds - image_bytes) / p.lds_wave); };
  const int pair_image = lane_image_bytes(t.pair_dec_bytes);
  const int fit_full = waves_fit(p.lds_image), fit_pairs = t.pairs_ok ? waves_fit(pair_image) : 0;
  switch (d.format) {
    case 1: p.pairs = false; break;
    case 2: p.pairs = fit_pairs >= 1; break;
    // (beyond three quarters of the CUs under full-image chain workgroups — each fills its CU's LDS — the parse next to the
    // chain finds no room and runs behind it: 32 batches of config 2 decode in 10.1 ms on the full image, 9.1 on the
    // compact one, whose workgroups leave 50 KB of every CU to two parse workgroups)
    default: p.pairs = fit_pairs >= 1 && (fit_full < 1 || 4 * waves_call > 3 * static_cast<int64_t>(d.cus) * std::min(fit_full, 4));
  }
  if (p.pairs) p.lds_image = pair_image;
  const int fit = p.pairs ? fit_pairs : fit_full;
  // waves per workgroup: as few as host the call on the chip's CUs (a chain wave wants a SIMD to itself); under
  // tfc_set_chip_shared — other kernels beside the coder's — four, so that the chains hold few CUs' LDS
  int per = static_cast<int>(std::min<int64_t>(8, std::max<int64_t>(1, ceil_div(waves_call, static_cast<int64_t>(d.cus)))));
  if (d.chip_shared) per = std::max(per, static_cast<int>(std::min<int64_t>(4, p.groups_per_job)));
  if (d.waves_override > 0) per = d.waves_override;
  per = std::min(per, std::min(fit, p.groups_per_job));
  p.pblock = 64 * std::max(per, 0);
  p.tiles = static_cast<size_t>(p.rows) / k.parse_rows + 1;
  // (precision 16: a quotient can equal the "no escape symbol" mark of dec_chain_kernel's directory, 0xFFFF)
  p.enabled = d.pipe_enabled && p.pblock >= 64 && rows64 < (int64_t{1} << 30) && p.job_bytes <= d.temp_bytes &&
              (!indexed || t.ntab < 4096) && t.lane_precision <= 15 &&
              (static_cast<int64_t>(p.rows) / k.parse_rows + 1) * p.groups_per_job * k.max_jobs < (int64_t{1} << 31);
  p.plds = p.lds_image + (p.pblock / 64) * p.lds_wave;
  const size_t chain_wgs_per_job = static_cast<size_t>(ceil_div(p.groups_per_job, std::max(1, p.pblock / 64)));
  const size_t resident_wgs = static_cast<size_t>(d.cus) * std::max<size_t>(1, kLds / std::max(1, p.plds));
  const size_t resident_jobs = std::max<size_t>(1, resident_wgs / std::max<size_t>(1, chain_wgs_per_job));
  p.per_launch = jobs_per_launch(p.enabled, k.max_jobs, resident_jobs, d.temp_bytes, p.job_bytes);
  // The pass next to the chain takes the tiles every stream is sure to reach (a row per element at least); the rows
  // beyond — escape codes' bit rows past the last element's place, a fraction of a percent — and the planned-for
  // capacity behind them (a quarter more) are the second pass's: workgroups of tiles that never fill would only be
  // dispatched behind the last real ones, wait for the chain's end and leave (16 000 of them in the 20-batch launch).
  p.ctiles = std::min<size_t>(p.tiles, static_cast<size_t>(ceil_div(elems, static_cast<int64_t>(k.parse_rows))));
  return p;
}

// Whether the LDS of a CU hosts a decode call on the lane path: the lane-per-stream kernels' own image plus one wave's
// staging, or the compact image of the pipelined decoder plus one chain wave (whose fallback is then the wave-per-stream
// kernel).  The expressions are lane_plan's `fits` and dec_pipe_plan's fit_pairs >= 1.  Asked once per handle of a call,
// so it takes the three device facts it reads (DeviceFacts: lds_bytes, pipe_enabled, format), not the struct.
inline bool decode_fits_lanes(const TableFacts& t, const KernelFacts& k, bool indexed, int lds_bytes, bool pipe_enabled, int format) {
  const bool compact_ok = t.pairs_ok && pipe_enabled && format != 1 &&
                          lanes_fit(t.pair_dec_bytes, dec_chain_wave_bytes(k, indexed), lds_bytes);
  return lanes_fit(t.lane_dec_bytes, indexed ? k.lane_wave_indexed : k.lane_wave_plain, lds_bytes) || compact_ok;
}

// The decoder's workspace (offsets in bytes) for a launch of gn jobs = `groups` groups.
// zeroed per launch: fallback flags (64 jobs), chain workgroups started, rows released per group, tiles taken
struct DecLayout {
  size_t raw = 0, posrec = 0, state_out = 0, kend = 0, rowaddr = 0, fallback = 0, started = 0, progress = 0, tile_done = 0;
  size_t total = 0, zero_offset = 0, zero_bytes = 0;
};
inline DecLayout dec_layout(const DecPipePlan& p, size_t groups, int gn, bool indexed, int64_t streams, int64_t elems) {
  DecLayout l;
  Bump b;
  l.raw = b.take(p.raw_bytes * groups, 256);
  l.posrec = b.take(p.rec_bytes * groups, 256);
  l.state_out = b.take(64 * kStateBytes * groups, 256);
  l.kend = b.take(kWord * groups, 256);
  l.rowaddr = b.take(indexed ? 2 * static_cast<size_t>(streams) * elems * gn : 0, 256);
  l.fallback = b.take(64 * kWord, 256);
  l.started = b.take(64 * kWord, kWord);
  l.progress = b.take(kWord * groups, kWord);
  l.tile_done = b.take(kWord * groups * p.tiles, kWord);
  l.total = b.take(0, 256);
  l.zero_offset = l.fallback;
  l.zero_bytes = l.total - l.fallback;
  return l;
}

}  // namespace plan
}  // namespace tfc
