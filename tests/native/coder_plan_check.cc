// Host build of compression_amd/csrc/range_plan.h for tests/test_coder_plan_cpu.py: every plan and layout of `count`
// cases, numbers in, numbers out (the order of both is the test's IN / OUT name lists).
#include <initializer_list>

#include "../../compression_amd/csrc/range_plan.h"

using namespace tfc::plan;

namespace {

long long* put_lane(long long* o, const LanePlan& p) {
  *o++ = p.fits; *o++ = p.lds_image; *o++ = p.lds_wave; *o++ = p.block; *o++ = p.lds_bytes;
  return o;
}
long long* put_enc_layout(long long* o, const EncLayout& l) {
  for (size_t v : {l.calls, l.stage_state, l.stage_out, l.status, l.done, l.fallback, l.started, l.total, l.zero_offset, l.zero_bytes})
    *o++ = static_cast<long long>(v);
  return o;
}
long long* put_dec_layout(long long* o, const DecLayout& l) {
  for (size_t v : {l.raw, l.posrec, l.state_out, l.kend, l.rowaddr, l.fallback, l.started, l.progress, l.tile_done, l.total,
                   l.zero_offset, l.zero_bytes})
    *o++ = static_cast<long long>(v);
  return o;
}

}  // namespace

extern "C" int coder_plan_check(int count, int n_in, int n_out, const long long* in_all, long long* out_all) {
  for (int c = 0; c < count; ++c) {
    const long long* i = in_all + static_cast<size_t>(c) * n_in;
    long long* const out = out_all + static_cast<size_t>(c) * n_out;
    TableFacts t;
    t.lane_enc_bytes = static_cast<int>(*i++); t.lane_dec_bytes = static_cast<int>(*i++); t.pair_dec_bytes = static_cast<int>(*i++);
    t.pairs_ok = *i++ != 0; t.any_escape = *i++ != 0; t.lane_precision = static_cast<int>(*i++);
    t.entries = static_cast<size_t>(*i++); t.ntab = static_cast<int>(*i++);
    DeviceFacts d;
    d.cus = static_cast<int>(*i++); d.lds_bytes = static_cast<int>(*i++); d.temp_bytes = static_cast<size_t>(*i++);
    d.pipe_enabled = *i++ != 0; d.format = static_cast<int>(*i++); d.waves_override = static_cast<int>(*i++);
    d.overlap = static_cast<int>(*i++); d.chip_shared = *i++ != 0;
    KernelFacts ke, kd;      // encoder's, decoder's: they differ in the lane kernels' LDS per wave and in the job limit
    ke.lane_wave_indexed = static_cast<int>(*i++); ke.lane_wave_plain = static_cast<int>(*i++);
    kd.lane_wave_indexed = static_cast<int>(*i++); kd.lane_wave_plain = static_cast<int>(*i++);
    ke.dec_lds_bytes = static_cast<int>(*i++); ke.dec_lds_rows = static_cast<int>(*i++); ke.dec_lds_stage = static_cast<int>(*i++);
    ke.enc_chain_groups = static_cast<int>(*i++); ke.enc_chain_group = static_cast<int>(*i++); ke.enc_chain_rows = static_cast<int>(*i++);
    ke.pipe_tile = static_cast<int>(*i++); ke.pipe_block = static_cast<int>(*i++); ke.parse_rows = static_cast<int>(*i++);
    ke.expand_tab_bytes = static_cast<int>(*i++);
    const int enc_max = static_cast<int>(*i++), dec_max = static_cast<int>(*i++);
    const int wi = kd.lane_wave_indexed, wp = kd.lane_wave_plain;
    kd = ke;
    kd.lane_wave_indexed = wi; kd.lane_wave_plain = wp;
    ke.max_jobs = enc_max; kd.max_jobs = dec_max;
    const long long streams = *i++, elems = *i++;
    const int n = static_cast<int>(*i++);
    const bool indexed = *i++ != 0;
    if (i - (in_all + static_cast<size_t>(c) * n_in) != n_in) return 1;

    long long* o = out;
    o = put_lane(o, lane_plan(t.lane_enc_bytes, ke, d, streams * n, indexed));
    o = put_lane(o, lane_plan(t.lane_dec_bytes, kd, d, streams * n, indexed));
    const EncPipePlan e = enc_pipe_plan(t, d, ke, streams, elems);
    *o++ = e.enabled; *o++ = e.nt; *o++ = e.rows; *o++ = e.groups_per_job; *o++ = static_cast<long long>(e.job_bytes);
    *o++ = e.tab_entries; *o++ = e.chain_lds; *o++ = e.per_launch;
    const DecPipePlan p = dec_pipe_plan(t, d, kd, streams, elems, n, indexed);
    *o++ = p.enabled; *o++ = p.pairs; *o++ = p.rows; *o++ = p.groups_per_job; *o++ = static_cast<long long>(p.raw_bytes);
    *o++ = static_cast<long long>(p.rec_bytes); *o++ = static_cast<long long>(p.job_bytes); *o++ = p.lds_image; *o++ = p.lds_wave;
    *o++ = p.pblock; *o++ = p.plds; *o++ = static_cast<long long>(p.tiles); *o++ = static_cast<long long>(p.ctiles);
    *o++ = p.per_launch;
    *o++ = decode_fits_lanes(t, kd, indexed, d.lds_bytes, d.pipe_enabled, d.format);
    // the layouts of a call's first and last launch
    for (int last = 0; last < 2; ++last) {
      const int gn_e = last ? n - (n - 1) / e.per_launch * e.per_launch : std::min(e.per_launch, n);
      const int gn_d = last ? n - (n - 1) / p.per_launch * p.per_launch : std::min(p.per_launch, n);
      const size_t groups_e = static_cast<size_t>(e.groups_per_job) * gn_e, groups_d = static_cast<size_t>(p.groups_per_job) * gn_d;
      *o++ = gn_e; *o++ = launch_overlap(d, groups_e);
      o = put_enc_layout(o, enc_layout(e, ke, groups_e));
      *o++ = gn_d; *o++ = launch_overlap(d, groups_d);
      o = put_dec_layout(o, dec_layout(p, groups_d, gn_d, indexed, streams, elems));
    }
    if (o - out != n_out) return 2;
  }
  return 0;
}
