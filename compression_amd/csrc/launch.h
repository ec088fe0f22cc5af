// Launch plumbing every unit shares: the device's CU count and LDS size, the dynamic-LDS launch, the "fits one launch"
// limits, and the environment switches.  State (the per-device CU count) lives in runtime.hip.
//
// The environment switches of the library (csrc/), all of them.  "once": read at first use, fixed for the process;
// "call": read on every call, so a test can flip it inside one process.
//
//   name                      values                     default   read  file
//   TFC_CACHE_LIMIT_MB        MB of released blocks kept 65536     once  runtime.hip (BlockCache)
//   TFC_CNORM_NT              0 / 1: non-temporal stores by size   once  channel_norm.hip
//   TFC_CONV_DOWN3            0: no gen-3 stride-2 route on        once  conv_gemm3.hip
//   TFC_CONV_F32              native: the float32 MFMA   planes    call  signal_conv.hip
//   TFC_CONV_F32_CHUNK_BYTES  bytes of planes per chunk  2 GiB     call  conv_shared.h
//   TFC_CONV_GEN              < 3: no gen 3; 4: all of it 3        call  conv_gemm3.hip
//   TFC_CONV_NT               0 / 1: non-temporal stores by size   once  conv_gemm3.hip
//   TFC_CONV_UP_PHASE         0: no per-phase route      on        once  signal_conv.hip
//   TFC_CONV_XCD              0: blocks in launch order  on        once  signal_conv.hip
//   TFC_DEFAULT_MODE          latency / throughput       auto      once  runtime.hip
//   TFC_GDN_NT                0 / 1: non-temporal stores by size   once  gdn_common.h
//   TFC_PIPE                  0: lane kernels alone      1         once  range_coder.hip
//   TFC_PIPE_FORMAT           full / pairs               by fit    once  range_coder.hip
//   TFC_PIPE_NOFALLBACK       1: no lane kernel behind   0         once  range_coder.hip
//   TFC_PIPE_OVERLAP          0 / 1 / 2                  2         once  range_coder.hip
//   TFC_PIPE_POLL_MS          ms a chain waits for words 250       once  range_coder.hip
//   TFC_PIPE_TEMP_MB          MB of temporaries a launch by memory once  range_coder.hip (per device)
//   TFC_PIPE_WAVES            chain waves per workgroup  0: by size once  range_coder.hip
//   TFC_RL_CHUNK_BITS         bits per decode chunk      1024      call  run_length.hip
//   TFC_RL_DECODER            lane / chunk               by length call  run_length.hip
//   TFC_RL_LONG_BITS          bits per unit: chunked     16384     call  run_length.hip
//   TFC_RL_SYNC_ROUNDS        synchronisation rounds     2         call  run_length.hip
//   TFC_SLOW_CALL_MS          ms: report slower calls    0: off    once  runtime.hip
//   TFC_SPECULATIVE_SLAB_DIV  slab = need / n            0: off    call  range_coder.hip
//   TFC_SSIM_RUNTIME_TAPS     1: taps as an argument     0         call  ssim.hip
//   TFC_WGRAD_TR              0: no transposed wgrad     on        once  signal_conv_backward.hip
#pragma once
#include <cstdlib>

#include "common.h"

namespace tfc {

// CUs of the current device: queried once per device ordinal; 256 where the query fails (the error is cleared).
int device_cus();

// LDS of one CU (gfx950): the most a workgroup's static + dynamic LDS can take.
constexpr size_t kLdsBytesPerCu = 160 * 1024;

// An integer switch; `fallback` where it is not set or empty.
inline int env_int(const char* name, int fallback) {
  const char* e = std::getenv(name);
  return e && *e ? std::atoi(e) : fallback;
}
// An on/off switch: -1 not set, 0 where the value starts with '0', 1 otherwise.
inline int env_switch(const char* name) {
  const char* e = std::getenv(name);
  return e ? (e[0] == '0' ? 0 : 1) : -1;
}
// A switch with a value of its own (a name, a count beyond int); null where it is not set.
inline const char* env_str(const char* name) { return std::getenv(name); }

// Whether a kernel's streamed traffic of `bytes` leaves non-temporal: beyond half the 256 MB Infinity Cache it would
// only push out lines that something else still reads.  env_override (env_switch of the kernel's *_NT): >= 0 decides.
inline bool beyond_cache(long long bytes, int env_override) {
  return env_override >= 0 ? env_override != 0 : bytes > (128ll << 20);
}

// What fits one launch: the x extent of a grid, and its y and z extents.  A site compares against these and fails with
// a text of its own (or, in a route's eligibility test, returns -1).
constexpr long long kMaxGridX = (1ll << 31) - 1;
constexpr long long kMaxGridYZ = 65535;

// Raises a kernel's limit of dynamic LDS to lds_bytes.  launch() does it for its own launch; the coder calls it once in
// front of the several launches of a batch.
inline int allow_dynamic_lds(const void* kernel, size_t lds_bytes) {
  TFC_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes)));
  return 0;
}

// Launches `kernel`; with dynamic LDS it first raises the kernel's limit (every call: the attribute is the driver's, and
// nothing here remembers what was set).
template <typename... P, typename... A>
int launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, A&&... args) {
  if (lds_bytes > 0)
    if (int rc = allow_dynamic_lds(reinterpret_cast<const void*>(kernel), lds_bytes)) return rc;
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, st, static_cast<P>(args)...);
  TFC_HIP(hipGetLastError());
  return 0;
}

}  // namespace tfc
