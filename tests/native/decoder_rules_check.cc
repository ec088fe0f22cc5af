// The two stream-format rules of csrc/range_wave.h, dec_open_state and dec_finalize_ok, compiled for the host
// (hipcc --offload-host-only) so that tests/test_context_models_cpu.py can hold them against tests/context_ref.py.
#include "../../compression_amd/csrc/range_wave.h"

extern "C" int decoder_finalize_ok(unsigned int base, unsigned int span_m1, unsigned int window, unsigned int pulls,
                                   long long len) {
  return tfc::dec_finalize_ok(base, span_m1, window, pulls, len) ? 1 : 0;
}

extern "C" void decoder_open_state(const uint8_t* src, long long len, unsigned int* out) {
  const uint4 s = tfc::dec_open_state(src, len);
  out[0] = s.x;
  out[1] = s.y;
  out[2] = s.z;
  out[3] = s.w;
}
