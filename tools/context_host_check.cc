// Host-side checks of the context-model entry points as a stand-alone program, for sanitizer builds:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I compression_amd/csrc
//       tools/context_host_check.cc -o /tmp/context_host_check && /tmp/context_host_check
//
// It runs what tfc_context_workspace / tfc_context_scan / tfc_context_decode do before they touch the device
// (ctx_layout, ctx_check_shape, ctx_workspace_bytes of csrc/context_params.h) over a sweep of sizes, packs a weight
// buffer section by section the way ops/context_ops.py does, and checks that the sections tile the buffer: aligned, in
// order, inside `total`, every real element written once and every padding element left zero.  Exit status 0 and
// "context_host_check ok" on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "context_params.h"

namespace {

int failures = 0;

#define EXPECT(cond, ...)                      \
  do {                                         \
    if (!(cond)) {                             \
      std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);       \
      std::fprintf(stderr, "\n");              \
      ++failures;                              \
    }                                          \
  } while (0)

struct Section {
  const char* name;
  int64_t at, rows, padded, cols;
};

// one matrix [rows][cols] into its section: value = a running counter, so that overlaps show
void put(std::vector<float>& buf, std::vector<unsigned char>& hits, const Section& s, float* counter) {
  for (int64_t r = 0; r < s.rows; ++r)
    for (int64_t c = 0; c < s.cols; ++c) {
      const int64_t i = s.at + r * s.cols + c;
      buf.at(static_cast<size_t>(i)) = (*counter += 1.f);
      hits.at(static_cast<size_t>(i)) += 1;
    }
}

void check_sizes(int m, int p, int h1, int h2) {
  tfc::ContextLayout L;
  const char* e = tfc::ctx_layout(m, p, h1, h2, &L);
  if (e) {
    // the only refusals inside the sweep: a position that does not fit the LDS budget
    EXPECT(std::strstr(e, "do not fit") != nullptr, "unexpected refusal for %d %d %d %d: %s", m, p, h1, h2, e);
    return;
  }
  EXPECT(L.waves >= 1 && L.waves <= tfc::CTX_MAX_WAVES, "waves %d", L.waves);
  EXPECT(static_cast<int64_t>(L.waves) * L.pos_floats <= tfc::CTX_LDS_FLOATS, "LDS %d x %d", L.waves, L.pos_floats);
  EXPECT(L.a_floats % 4 == 0 && L.b_floats % 4 == 0 && L.pp % 4 == 0, "row strides must be multiples of 4");
  EXPECT(L.a_floats >= L.c2p && L.a_floats >= L.h2p && L.b_floats >= L.h1p && L.b_floats >= L.c2, "buffer sizes");
  EXPECT(L.pos_floats >= L.pp && tfc::CTX_LDS_FLOATS / L.pp >= 1, "the precomputation's tile");
  // the 12 taps are [tap][Mp][2M]: tap t, channel k at row t * Mp + k
  const Section sections[] = {
      {"wc", L.wc, static_cast<int64_t>(tfc::CTX_TAPS) * L.mp, static_cast<int64_t>(tfc::CTX_TAPS) * L.mp, L.c2},
      {"bc", L.bc, 1, 1, L.c2},          {"w1c", L.w1c, L.c2, L.c2p, L.h1}, {"w1p", L.w1p, L.p, L.pp, L.h1},
      {"b1", L.b1, 1, 1, L.h1},          {"w2", L.w2, L.h1, L.h1p, L.h2},   {"b2", L.b2, 1, 1, L.h2},
      {"w3", L.w3, L.h2, L.h2p, L.c2},   {"b3", L.b3, 1, 1, L.c2}};
  std::vector<float> buf(static_cast<size_t>(L.total), 0.f);
  std::vector<unsigned char> hits(static_cast<size_t>(L.total), 0);
  float counter = 0.f;
  int64_t end = 0;
  for (const Section& s : sections) {
    EXPECT(s.at % tfc::CTX_KPAD == 0, "%s starts at %lld", s.name, static_cast<long long>(s.at));
    EXPECT(s.at >= end, "%s overlaps its predecessor", s.name);
    end = s.at + s.padded * s.cols;
    EXPECT(end <= L.total, "%s ends at %lld of %lld", s.name, static_cast<long long>(end), static_cast<long long>(L.total));
    if (std::strcmp(s.name, "wc") == 0) {
      // only the M real channels of every tap are written
      for (int t = 0; t < tfc::CTX_TAPS; ++t) {
        const Section tap = {"tap", s.at + static_cast<int64_t>(t) * L.mp * L.c2, L.m, L.mp, L.c2};
        put(buf, hits, tap, &counter);
      }
    } else {
      put(buf, hits, s, &counter);
    }
  }
  EXPECT(L.total - end < tfc::CTX_KPAD, "slack behind the last section");
  int64_t written = 0;
  for (size_t i = 0; i < hits.size(); ++i) {
    EXPECT(hits[i] <= 1, "element %zu written %d times", i, hits[i]);
    EXPECT(hits[i] == 1 || buf[i] == 0.f, "padding element %zu is not zero", i);
    written += hits[i];
  }
  const int64_t want = static_cast<int64_t>(tfc::CTX_TAPS) * L.m * L.c2 + 2 * L.c2 + static_cast<int64_t>(L.c2 + L.p) * L.h1 +
                       L.h1 + static_cast<int64_t>(L.h1) * L.h2 + L.h2 + static_cast<int64_t>(L.h2) * L.c2;
  EXPECT(written == want, "%lld elements written, %lld expected", static_cast<long long>(written), static_cast<long long>(want));

  // the shape checks and the workspace
  EXPECT(tfc::ctx_check_shape(3, 5, 7, 64, L.total, L) == nullptr, "a plain shape was refused");
  EXPECT(tfc::ctx_check_shape(3, 5, 7, 64, L.total + 1, L) != nullptr, "a wrong packed size was accepted");
  EXPECT(tfc::ctx_check_shape(-1, 5, 7, 64, L.total, L) != nullptr, "a negative batch was accepted");
  EXPECT(tfc::ctx_check_shape(3, 0, 7, 64, L.total, L) != nullptr, "Hl = 0 was accepted");
  EXPECT(tfc::ctx_check_shape(3, 5, 7, 0, L.total, L) != nullptr, "num_scales = 0 was accepted");
  EXPECT(tfc::ctx_check_shape(1ll << 30, 1 << 20, 1 << 20, 64, L.total, L) != nullptr, "2^70 positions were accepted");
  EXPECT(tfc::ctx_check_shape(0, 1, 1, 1, L.total, L) == nullptr, "an empty batch was refused");
  const int64_t ws = tfc::ctx_workspace_bytes(3, 5, 7, L.h1);
  EXPECT(ws % 16 == 0 && ws >= 3 * 5 * 7 * static_cast<int64_t>(L.h1) * 4 + 3 * 5 * 16, "workspace %lld", static_cast<long long>(ws));
}

}  // namespace

int main() {
  // odd sizes, sizes around the padding, the test widths and the model's (M 192: P 384, H1 640, H2 512)
  int layouts = 0;
  for (int m : {1, 2, 3, 5, 16, 192})
    for (int p : {1, 6, 33, 384})
      for (int h1 : {1, 7, 26, 640})
        for (int h2 : {1, 5, 21, 512}) {
          check_sizes(m, p, h1, h2);
          ++layouts;
        }
  tfc::ContextLayout L;
  EXPECT(tfc::ctx_layout(0, 1, 1, 1, &L) != nullptr, "M = 0 was accepted");
  EXPECT(tfc::ctx_layout(1, 1, 1, 1 << 20, &L) != nullptr, "H2 = 2^20 was accepted");
  EXPECT(tfc::ctx_layout(4000, 8000, 13000, 10000, &L) != nullptr, "a position beyond the LDS budget was accepted");
  EXPECT(tfc::ctx_layout(192, 384, 640, 512, &L) == nullptr && L.waves == 8, "the model's widths run 8 positions at a time");
  if (failures) {
    std::fprintf(stderr, "context_host_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("context_host_check ok: %d layouts\n", layouts);
  return 0;
}
