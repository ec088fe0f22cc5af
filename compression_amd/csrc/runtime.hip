// Library plumbing of the C ABI that is not a kernel: the last error text, slow-call and kernel timing, the profile
// table, the process-wide mode switches, the per-device CU count, and the library's cache of released device memory.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tfc_hip.h"
#include "launch.h"

namespace tfc {

BlockCache::BlockCache() {
  const char* e = std::getenv("TFC_CACHE_LIMIT_MB");
  limit = static_cast<size_t>(e ? std::atoll(e) : 65536) << 20;
}

// (per device ordinal: a process may drive several devices)
int device_cus() {
  constexpr int kMaxDevices = 64;
  static int cus[kMaxDevices];
  static std::once_flag once[kMaxDevices];
  int dev = 0;
  (void)hipGetDevice(&dev);
  dev = std::min(std::max(dev, 0), kMaxDevices - 1);
  std::call_once(once[dev], [dev] {
    if (hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
      (void)hipGetLastError();
      cus[dev] = 256;
    }
  });
  return cus[dev];
}

std::string& last_error() {
  static thread_local std::string e;
  return e;
}

double slow_call_threshold_ms() {
  static const double ms = [] {
    const char* e = std::getenv("TFC_SLOW_CALL_MS");
    return e ? std::atof(e) : 0.0;
  }();
  return ms;
}

namespace {
double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

SlowCall::SlowCall(const char* w, const char* f, int l)
    : what(w), file(f), line(l), t0(slow_call_threshold_ms() > 0.0 ? now_ms() : 0.0) {}

SlowCall::~SlowCall() {
  if (t0 == 0.0) return;
  const double dt = now_ms() - t0;
  if (dt >= slow_call_threshold_ms())
    std::fprintf(stderr, "[tfc slow call] %8.2f ms  %s:%d  %s  (%llu)\n", dt, file, line, what, detail);
}

int fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  last_error() = buf;
  return 1;
}

// ---- optional kernel timing --------------------------------------------------
namespace {
struct ProfileEntry {
  std::string name;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double total_ms = 0;
  int64_t launches = 0;
};
bool g_profile_on = false;
std::mutex g_profile_mutex;      // encoders / decoders may run on several host threads
std::vector<ProfileEntry>& profile_table() {
  static std::vector<ProfileEntry> t;
  return t;
}
ProfileEntry& profile_entry(const char* name) {
  for (auto& e : profile_table())
    if (e.name == name) return e;
  profile_table().push_back(ProfileEntry{name, {}, 0, 0});
  return profile_table().back();
}
}  // namespace

bool profiling_enabled() { return g_profile_on; }

KernelTimer::KernelTimer(const char* n, hipStream_t s) : name(n), st(s), on(g_profile_on), slow(n, "launch scope", 0) {
  if (!on) return;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  (void)hipEventRecord(a, st);
}

KernelTimer::~KernelTimer() {
  if (!on) return;
  (void)hipEventRecord(b, st);
  std::lock_guard<std::mutex> lock(g_profile_mutex);
  profile_entry(name).pending.emplace_back(a, b);
}

}  // namespace tfc

using namespace tfc;

namespace {
std::atomic<int> g_chip_shared{0};      // tfc_set_chip_shared
}

// -> the previous value, so that nested users can restore it
extern "C" int tfc_set_chip_shared(int shared) {
  return g_chip_shared.exchange(shared ? 1 : 0, std::memory_order_relaxed);
}
bool tfc::chip_shared() { return g_chip_shared.load(std::memory_order_relaxed) != 0; }

namespace {
std::atomic<int>& default_mode() {
  static std::atomic<int> mode{[] {
    const char* e = std::getenv("TFC_DEFAULT_MODE");
    if (e && !std::strcmp(e, "latency")) return TFC_MODE_LATENCY;
    if (e && !std::strcmp(e, "throughput")) return TFC_MODE_THROUGHPUT;
    return TFC_MODE_AUTO;
  }()};
  return mode;
}
}  // namespace
extern "C" int tfc_set_default_mode(int mode) {
  if (mode != TFC_MODE_AUTO && mode != TFC_MODE_LATENCY && mode != TFC_MODE_THROUGHPUT)
    return fail("unknown mode %d", mode);
  default_mode().store(mode);
  return 0;
}
extern "C" int tfc_get_default_mode(void) { return default_mode().load(); }

extern "C" void tfc_profile_enable(int on) {
  std::lock_guard<std::mutex> lock(g_profile_mutex);
  g_profile_on = on != 0;
  if (on) {
    for (auto& e : profile_table()) {
      for (auto& p : e.pending) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
      e.pending.clear();
      e.total_ms = 0;
      e.launches = 0;
    }
  }
}

extern "C" int tfc_profile_query(const char* kernel, double* total_ms, int64_t* launches) {
  std::lock_guard<std::mutex> lock(g_profile_mutex);
  ProfileEntry& e = profile_entry(kernel);
  for (auto& p : e.pending) {
    float ms = 0;
    if (hipEventSynchronize(p.second) == hipSuccess && hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) {
      e.total_ms += ms;
      e.launches += 1;
    }
    (void)hipEventDestroy(p.first);
    (void)hipEventDestroy(p.second);
  }
  e.pending.clear();
  *total_ms = e.total_ms;
  *launches = e.launches;
  return 0;
}

extern "C" int tfc_abi_version(void) { return TFC_ABI_VERSION; }
extern "C" const char* tfc_last_error(void) { return last_error().c_str(); }
extern "C" void tfc_free(void* p) { std::free(p); }

extern "C" int tfc_cache_bytes(long long* bytes) {
  if (!bytes) return tfc::fail("tfc_cache_bytes: null argument");
  tfc::BlockCache& c = tfc::BlockCache::get();
  std::lock_guard<std::mutex> lock(c.mu);
  *bytes = static_cast<long long>(c.cached);
  return 0;
}

extern "C" int tfc_cache_trim(long long* released) {
  const size_t n = tfc::BlockCache::get().trim();
  if (released) *released = static_cast<long long>(n);
  return 0;
}
