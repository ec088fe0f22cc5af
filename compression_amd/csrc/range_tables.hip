// Host builders of the coder's table images: the raw lookup, the encoder's 16-bit image, the wave-per-stream
// decoder's image with its row directory, the lane-per-stream image and the pipelined decoder's compact image.
// No kernels: what the images must agree on with the kernels that read them is in range_coder_device.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tfc_hip.h"
#include "launch.h"
#include "range_coder_device.h"
#include "range_tables.h"

using namespace tfc;

namespace {

int scan_row(const std::vector<int32_t>& v, int64_t end, int64_t* cur, std::vector<int2>* rows) {
  int64_t p = *cur;
  if (end < p + 3) return fail("CDF ended prematurely.");
  const int64_t head = p;
  const int64_t ap = std::llabs(static_cast<long long>(v[head]));
  if (ap < 1 || ap >= 17)
    return fail("precision=%lld not in range [1, 17)", static_cast<long long>(ap));
  const int32_t last = 1 << ap;
  ++p;
  if (v[p] != 0) return fail("CDF must start with 0.");
  do {
    ++p;
    if (p == end) return fail("CDF must end with 1 << precision.");
    if (v[p] < v[p - 1]) return fail("CDF must be monotonically increasing.");
  } while (v[p] != last);
  ++p;
  rows->push_back(make_int2(static_cast<int>(head), static_cast<int>(p - head)));
  while (p != end && v[p] == last) ++p;
  *cur = p;
  return 0;
}

}  // namespace

extern "C" int tfc_tables_create(const int32_t* lookup, int rank, int64_t rows, int64_t cols,
                                 void* stream, tfc_tables** out) {
  *out = nullptr;
  if (rank != 1 && rank != 2) return fail("`lookup` must be rank 1 or 2: rank=%d", rank);
  const int64_t total = rank == 1 ? cols : rows * cols;
  if (total >= (int64_t{1} << 31)) return fail("`lookup` too large");
  std::unique_ptr<tfc_tables> t(new tfc_tables);
  t->host.assign(lookup, lookup + total);
  if (rank == 1) {
    for (int64_t cur = 0; cur != total;)
      if (scan_row(t->host, total, &cur, &t->rows)) return 1;
  } else {
    for (int64_t cur = 0; cur != total;) {
      const int64_t row_end = cur + cols;
      if (scan_row(t->host, row_end, &cur, &t->rows)) return 1;
      if (cur != row_end) return fail("CDF must end with 1 << precision.");
    }
  }
  for (const int2& r : t->rows) {
    const int32_t sp = t->host[r.x];
    t->max_abs_prec = std::max(t->max_abs_prec, std::abs(sp));
    t->any_escape |= sp < 0;
    t->max_row = std::max<int64_t>(t->max_row, r.y);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  TFC_HIP(t->d_data.alloc(sizeof(int32_t) * std::max<int64_t>(total, 1), st));
  TFC_HIP(t->d_rows.alloc(sizeof(int2) * std::max<size_t>(t->rows.size(), 1), st));
  if (total)
    TFC_HIP(hipMemcpyAsync(t->d_data.p, t->host.data(), sizeof(int32_t) * total,
                           hipMemcpyHostToDevice, st));
  if (!t->rows.empty())
    TFC_HIP(hipMemcpyAsync(t->d_rows.p, t->rows.data(), sizeof(int2) * t->rows.size(),
                           hipMemcpyHostToDevice, st));
  {
    std::vector<int32_t> fast(t->host);
    for (const int2& r : t->rows) {
      const int sh = 16 - std::abs(t->host[r.x]);
      for (int i = 1; i < r.y; ++i) fast[r.x + i] = t->host[r.x + i] << sh;
    }
    // Encoder image: 16 bits per entry.  A scaled entry is at most 65536 and only ever used as
    // "lower" (< 65536) or as "upper - 1" (the coder call word holds upper - 1), so it is stored modulo
    // 2^16; whether a row has the escape symbol moves from the header's sign into the row directory.
    // Half the LDS of the int32 image = twice the encoder workgroups per CU.
    std::vector<uint16_t> fast16(std::max<int64_t>(total, 1));
    for (int64_t i = 0; i < total; ++i) fast16[i] = static_cast<uint16_t>(fast[i]);
    std::vector<int2> rows_fast(t->rows);
    for (int2& r : rows_fast)
      if (t->host[r.x] < 0) r.y |= static_cast<int>(0x80000000u);
    TFC_HIP(t->d_fast.alloc(sizeof(uint16_t) * fast16.size(), st));
    TFC_HIP(hipMemcpyAsync(t->d_fast.p, fast16.data(), sizeof(uint16_t) * fast16.size(), hipMemcpyHostToDevice, st));
    TFC_HIP(t->d_rows_fast.alloc(sizeof(int2) * std::max<size_t>(rows_fast.size(), 1), st));
    if (!rows_fast.empty())
      TFC_HIP(hipMemcpyAsync(t->d_rows_fast.p, rows_fast.data(), sizeof(int2) * rows_fast.size(),
                             hipMemcpyHostToDevice, st));
    // Decoder image: the scaled table, 64 words of padding (lanes past a row's end
    // read harmless data), then 64 pivots per wide row (> 64 symbols).
    std::vector<int32_t> image(fast);
    image.resize(image.size() + 64, 65536);
    std::vector<int4> dir;
    bool ok = true;
    for (const int2& r : t->rows) {
      const int nsym = r.y - 2;
      const int cdf0 = r.x + 1;
      const int chunk = (nsym + 63) / 64;
      if (chunk > 64) ok = false;
      // a zero-width FIRST symbol has the upper bound 0, whose "bound - 1" form wraps and matches every
      // offset: such tables keep the generic decoder (64-bit comparison, range_coder.h:204-222)
      if (nsym > 1 && fast[cdf0 + 1] == 0) ok = false;
      int4 d;
      d.y = cdf0;
      d.z = nsym | (std::max(chunk, 1) << 16);
      d.w = t->host[r.x] < 0 ? nsym - 1 : -1;
      if (chunk <= 1) {
        d.x = cdf0 + 1;
      } else {
        d.x = static_cast<int>(image.size());
        for (int j = 0; j < 64; ++j)
          image.push_back(fast[cdf0 + std::min((j + 1) * chunk, nsym)]);
      }
      dir.push_back(d);
    }
    image.resize(image.size() + 64, 65536);
    t->dec_words = static_cast<int>(image.size());
    t->dec_fast_ok = ok && !t->rows.empty();
    TFC_HIP(t->d_dec_image.alloc(sizeof(int32_t) * image.size(), st));
    TFC_HIP(t->d_dec_dir.alloc(sizeof(int4) * std::max<size_t>(dir.size(), 1), st));
    TFC_HIP(hipMemcpyAsync(t->d_dec_image.p, image.data(), sizeof(int32_t) * image.size(),
                           hipMemcpyHostToDevice, st));
    if (!dir.empty())
      TFC_HIP(hipMemcpyAsync(t->d_dec_dir.p, dir.data(), sizeof(int4) * dir.size(),
                             hipMemcpyHostToDevice, st));
    TFC_HIP(hipStreamSynchronize(st));
  }
  {
    // Image of the lane-per-stream kernels: directory (one entry per table), 16-bit scaled cdf entries
    // (modulo 2^16: only a row's last entry is 2^16), then per row the bitmap of its boundaries over
    // [0, 2^precision) and the running count of boundaries before each 64-bit word.  The counts of a row have one
    // more entry, for the word BEHIND the row (the next row's first, or one empty word behind the last row): the
    // quotient estimate of an offset at the very top of the span is 2^precision, and the pipelined decoder
    // (range_pipe.h) reads that word — of which its shift keeps bit 0 only, which it has cleared in its own copy —
    // instead of clamping.  Rows must be strictly increasing (rank = popcount) and share one precision (the
    // quotient scale is a kernel constant) — other tables keep the wave-per-stream kernels.
    const size_t ntab = t->rows.size();
    bool ok = ntab > 0;
    const int prec = ok ? std::abs(t->host[t->rows[0].x]) : 0;
    const size_t nw = std::max<size_t>(1, (size_t{1} << prec) / 64);
    size_t cdf_entries = 0;
    for (const int2& r : t->rows) {
      const int nsym = r.y - 2;
      if (std::abs(t->host[r.x]) != prec) ok = false;
      if (nsym > 32767) ok = false;
      for (int k = 1; ok && k <= nsym; ++k)
        if (t->host[r.x + 1 + k] <= t->host[r.x + k]) ok = false;
      cdf_entries += static_cast<size_t>(nsym + 1);
    }
    // behind the tables' rows: the uniform binary row {0, 1/2, 1} the pipelined decoder (range_pipe.h) decodes the
    // bits of an escape code from (range_coder_kernels.cc:449-471: DecodeLinearly on {0, 1, 2} at precision 1)
    cdf_entries += 3;
    const size_t words = (ntab + 1) * nw + 1, counts = (ntab + 1) * (nw + 1);
    // the directory repeats its first entries behind its end: a block of kEncCadence / kDecCadence steps
    // reads that many consecutive entries without a wrap test per step (range_coder_device.h)
    const size_t dir_bytes = sizeof(tfc::LaneRow) * (ntab + kDirRepeat + 1);
    const size_t cdf_bytes = (2 * cdf_entries + 15) & ~size_t{15};
    const size_t enc_bytes = dir_bytes + cdf_bytes;
    const size_t dec_bytes = enc_bytes + 8 * words + ((2 * counts + 15) & ~size_t{15});
    // (the encoder needs directory + cdf entries only; a decoder image over the CU's LDS keeps the decoder on the
    // wave-per-stream kernels — decodes_on_lanes checks — and the encoder may still run lane-per-stream)
    if (enc_bytes > 128 * 1024) ok = false;
    if (ok) {
      std::vector<uint8_t> image(dec_bytes, 0);
      tfc::LaneRow* dir = reinterpret_cast<tfc::LaneRow*>(image.data());
      uint16_t* cdf16 = reinterpret_cast<uint16_t*>(image.data() + dir_bytes);
      uint64_t* bits = reinterpret_cast<uint64_t*>(image.data() + enc_bytes);
      uint16_t* cum = reinterpret_cast<uint16_t*>(image.data() + enc_bytes + 8 * words);
      size_t ce = 0;
      // per word: the boundaries before it MINUS ONE, as int16 (rank - 1 = symbol: the decoder adds the
      // popcount inside the word and has the symbol; -1 for the first word), and once more behind the row
      auto count_row = [&](size_t i) {
        unsigned int run = 0;
        for (size_t w = 0; w <= nw; ++w) {
          cum[i * (nw + 1) + w] = static_cast<uint16_t>(static_cast<int16_t>(static_cast<int>(run) - 1));
          if (w < nw) run += static_cast<unsigned int>(__builtin_popcountll(bits[i * nw + w]));
        }
      };
      auto place_row = [&](tfc::LaneRow& d, size_t i) {
        d.cdf = static_cast<unsigned int>(dir_bytes + 2 * ce) - 2u;     // of cdf[0], minus 2: lo / hi of symbol s at + 2 s + 2 / + 4
        d.bits = static_cast<unsigned int>(enc_bytes + 8 * i * nw);
        d.cum = static_cast<unsigned int>(enc_bytes + 8 * words + 2 * i * (nw + 1));
      };
      for (size_t i = 0; i < ntab; ++i) {
        const int2 r = t->rows[i];
        const int32_t* cdf = &t->host[r.x + 1];
        const int nsym = r.y - 2;
        const bool esc = t->host[r.x] < 0;
        tfc::LaneRow& d = dir[i];
        place_row(d, i);
        d.info = static_cast<unsigned int>(esc ? nsym - 1 : nsym) | (esc ? 0x80000000u : 0u);
        for (int k = 0; k <= nsym; ++k) cdf16[ce + k] = static_cast<uint16_t>(cdf[k] << (16 - prec));
        for (int k = 0; k < nsym; ++k) bits[i * nw + (cdf[k] >> 6)] |= uint64_t{1} << (cdf[k] & 63);
        count_row(i);
        ce += static_cast<size_t>(nsym + 1);
      }
      for (size_t i = 0; i < kDirRepeat; ++i) dir[ntab + i] = dir[i % ntab];
      {
        // the binary row, at the table set's precision (the quotient scale is a kernel constant); at precision 0
        // (no such tables: precision >= 1) its two boundaries would coincide
        tfc::LaneRow& d = dir[ntab + kDirRepeat];
        place_row(d, ntab);
        d.info = 2u;
        cdf16[ce] = 0; cdf16[ce + 1] = 0x8000; cdf16[ce + 2] = 0;
        const unsigned int mid = 1u << (prec - 1);
        bits[ntab * nw] |= 1ull;
        bits[ntab * nw + (mid >> 6)] |= uint64_t{1} << (mid & 63);
        count_row(ntab);
      }
      TFC_HIP(t->d_lane_image.alloc(image.size(), st));
      TFC_HIP(hipMemcpyAsync(t->d_lane_image.p, image.data(), image.size(), hipMemcpyHostToDevice, st));
      TFC_HIP(hipStreamSynchronize(st));
      t->lane_enc_bytes = static_cast<int>(enc_bytes);
      t->lane_dec_bytes = static_cast<int>(dec_bytes);
      t->lane_precision = prec;
      t->lanes_ok = true;
    }
  }
  if (t->lanes_ok && t->lane_precision <= 15) {
    // Compact image of the pipelined decoder (round 6).  The boundary bitmaps are 2/3 of the lane image (98 of 154 KB for
    // BASELINE config 2's tables; bls2017's 192 x 128-symbol tables need 176 KB and do not fit a CU at all): one bit per
    // quotient value, because two bounds may be neighbours.  EVERY SECOND bound of a strictly increasing row is at least
    // two apart from the next one marked, so a bitmap of those needs one bit per PAIR of quotient values {2 j, 2 j + 1}
    // only — half the bytes — and its rank i says: bound k = 2 i + o is the last marked one whose pair is not behind
    // q's, hence  cdf[k] - 1 <= q < cdf[k + 2]  and the symbol is k - 1, k or k + 1.  The step (TFC_PDEC_STEP_H) reads
    // the four entries cdf[k - 1 .. k + 2] with one ds_read2_b32 and settles it with two comparisons of the quotient
    // (t0 = [q >= cdf[k]], t1 = [q >= cdf[k + 1]]: lower / upper bound by four selects, symbol = k - 1 + t0 + t1) —
    // verified by the exact interval test like every estimate.
    //   * which bounds are marked: those with k = o (mod 2), o = symbols of the row (mod 2) — then the last marked one is
    //     k = n - 2 and the row's END (2^16, stored as 0: the only entry a comparison must not meet) is only ever an
    //     upper bound;
    //   * in front of cdf[0] a row has two zero entries (an even row's first window starts at cdf[-1]; a row of one symbol
    //     takes k = -1: both comparisons true, the window slides to (cdf[0], cdf[1])), and rows are placed so that the
    //     window of rank i starts at a multiple of four bytes: the directory's cdf pointer is that address for i = 0;
    //   * the step's raw entry is 2 i + t0 + t1 = symbol - (o - 1): dec_parse_kernel adds the row's o - 1 (pair_adjust).
    // Layout: directory (final form: what dec_chain_kernel<..., false> makes of its copy of the lane image), entries,
    // bitmaps (row i at word i * nw2, one spare word behind the last row), counts (nw2 + 1 per row).
    const size_t ntab = t->rows.size();
    const int prec = t->lane_precision, sh = 16 - prec;
    const size_t npairs = size_t{1} << (prec - 1);
    const size_t nw2 = std::max<size_t>(1, npairs / 64);
    const size_t dir_bytes = sizeof(tfc::LaneRow) * (ntab + kDirRepeat + 1);
    std::vector<uint16_t> entries;            // all rows: [pad ... 0, 0, cdf[0] ... cdf[n]]
    std::vector<int> adjust(ntab);
    std::vector<uint64_t> bits((ntab + 1) * nw2 + 1, 0);
    std::vector<uint16_t> cum((ntab + 1) * (nw2 + 1), 0);
    std::vector<size_t> window0(ntab + 1);    // entry index of the window of rank 0: cdf[o - 1]
    auto add_row = [&](size_t i, const int32_t* cdf, int nsym, unsigned int carry) {
      // (a row of ONE symbol has no bound a comparison may meet — cdf[1] is its end: its window starts two entries in
      // front of cdf[0], in the pad: o = -1, both comparisons true)
      const int o = nsym == 1 ? -1 : (nsym & 1);
      // entry index of cdf[0] such that the byte address of cdf[o - 1] (dir_bytes is a multiple of 16) is a multiple of 4
      size_t at0 = entries.size() + 2;
      if (((at0 + o - 1) & 1) != 0) ++at0;
      entries.resize(at0, 0);
      for (int k = 0; k <= nsym; ++k) entries.push_back(static_cast<uint16_t>(static_cast<unsigned int>(cdf[k]) << sh));
      window0[i] = at0 + o - 1;
      // (the first marked bound, k = o, is left out: the rank is then the index i of the last marked bound, and the
      // quotients below it share its window)
      for (int k = o + 2; k < nsym; k += 2) {
        const unsigned int pair = static_cast<unsigned int>(cdf[k]) >> 1;
        bits[i * nw2 + (pair >> 6)] |= uint64_t{1} << (pair & 63);
      }
      unsigned int run = carry;
      for (size_t w = 0; w <= nw2; ++w) {
        cum[i * (nw2 + 1) + w] = static_cast<uint16_t>(run);
        if (w < nw2) run += static_cast<unsigned int>(__builtin_popcountll(bits[i * nw2 + w]));
      }
    };
    for (size_t i = 0; i < ntab; ++i) {
      const int2 r = t->rows[i];
      const int nsym = r.y - 2;
      adjust[i] = (nsym == 1 ? -1 : (nsym & 1)) - 1;
      add_row(i, &t->host[r.x + 1], nsym, 0u);
    }
    {
      // the binary row of an escape code's bits {0, 1/2, 1}: two symbols, bound 0 marked, window (pad, 0, 1/2, end):
      // t0 = 1, t1 = the bit; its ranks carry 0x4000, so that 2 i + t0 + t1 = 0x8001 + bit — the raw entry of a bit row
      // as it is stored (the bit is entry >> 1 & 1; 0xFFFF stays the mark of a row a lane sat out)
      const int32_t bin[3] = {0, 1 << (prec - 1), 1 << prec};
      add_row(ntab, bin, 2, 0x4000u);
    }
    entries.resize(entries.size() + 2, 0);    // (the last window's fourth entry)
    const size_t cdf_bytes = (2 * entries.size() + 15) & ~size_t{15};
    const size_t bits_off = dir_bytes + cdf_bytes;
    const size_t cum_off = bits_off + 8 * bits.size();
    const size_t total = cum_off + ((2 * cum.size() + 15) & ~size_t{15});
    if (total <= kLdsBytesPerCu) {
      std::vector<uint8_t> image(total, 0);
      tfc::LaneRow* dir = reinterpret_cast<tfc::LaneRow*>(image.data());
      auto entry_of = [&](size_t i, unsigned int limit, bool esc, unsigned int esclo, bool binary) {
        tfc::LaneRow d;
        // (the step addresses the window as cdf + 4 i; the binary row's ranks carry 0x4000)
        d.cdf = static_cast<unsigned int>(dir_bytes + 2 * window0[i]) - (binary ? 0x10000u : 0u);
        d.info = (limit & 0x7FFFu) | (esc ? 0x8000u : 0u) | ((0xFFFFu - esclo) << 16);
        d.bits = static_cast<unsigned int>(bits_off + 8 * i * nw2) - 8u;
        d.cum = static_cast<unsigned int>(cum_off + 2 * i * (nw2 + 1)) - 2u;
        return d;
      };
      for (size_t i = 0; i < ntab; ++i) {
        const int2 r = t->rows[i];
        const bool esc = t->host[r.x] < 0;
        const int nsym = r.y - 2;
        // limit: plain symbols (= the escape symbol's index), as in the lane image; ESCLO: the escape symbol's lower bound
        // on the tables' own scale (0xFFFF, which no quotient reaches at precision <= 15, for a row without one)
        dir[i] = entry_of(i, static_cast<unsigned int>(esc ? nsym - 1 : nsym), esc,
                          esc ? static_cast<unsigned int>(t->host[r.x + 1 + nsym - 1]) : 0xFFFFu, false);
      }
      for (size_t i = 0; i < kDirRepeat; ++i) dir[ntab + i] = dir[i % ntab];
      dir[ntab + kDirRepeat] = entry_of(ntab, 2u, false, 1u << (prec - 1), true);
      std::memcpy(image.data() + dir_bytes, entries.data(), 2 * entries.size());
      std::memcpy(image.data() + bits_off, bits.data(), 8 * bits.size());
      std::memcpy(image.data() + cum_off, cum.data(), 2 * cum.size());
      TFC_HIP(t->d_pair_image.alloc(image.size(), st));
      TFC_HIP(hipMemcpyAsync(t->d_pair_image.p, image.data(), image.size(), hipMemcpyHostToDevice, st));
      TFC_HIP(t->d_pair_adjust.alloc(sizeof(int) * ntab, st));
      TFC_HIP(hipMemcpyAsync(t->d_pair_adjust.p, adjust.data(), sizeof(int) * ntab, hipMemcpyHostToDevice, st));
      TFC_HIP(hipStreamSynchronize(st));
      t->pair_dec_bytes = static_cast<int>(total);
      t->pairs_ok = true;
    }
  }
  TFC_HIP(hipStreamSynchronize(st));
  *out = t.release();
  return 0;
}

extern "C" int64_t tfc_tables_count(const tfc_tables* t) { return static_cast<int64_t>(t->rows.size()); }
extern "C" void tfc_tables_destroy(tfc_tables* t) { delete t; }

namespace tfc {

size_t table_lds_bytes(const tfc_tables* t) {
  const size_t b = t->host.size() * sizeof(int32_t);
  return b <= kLdsTableBytes ? b : 0;
}

TableView view_of(const tfc_tables* t) {
  TableView v;
  v.data = t->d_data.as<int32_t>();
  v.fast16 = t->d_fast.as<uint16_t>();
  v.rows_fast = t->d_rows_fast.as<int2>();
  v.dec_image = t->d_dec_image.as<int32_t>();
  v.dec_dir = t->d_dec_dir.as<DecRow>();
  v.dec_words = t->dec_words;
  v.rows = t->d_rows.as<int2>();
  v.ntab = static_cast<int>(t->rows.size());
  v.total = static_cast<int>(t->host.size());
  return v;
}

// LDS bytes of dec_fast_kernel (decoder image + row directory), or 0 where the tables cannot take that kernel.
size_t dec_fast_lds(const tfc_tables* t) {
  const size_t b = sizeof(int32_t) * ((t->dec_words + 3) & ~3) + sizeof(int4) * t->rows.size();
  return t->dec_fast_ok && b <= kLdsBytesPerCu ? b : 0;
}

}  // namespace tfc
