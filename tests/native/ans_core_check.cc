// Host build of compression_amd/csrc/ans_core.h for tests/test_ans_format_cpu.py: the serial coder of a whole stream
// and the quotient/remainder helper, behind a C interface for ctypes.
#include "../../compression_amd/csrc/ans_core.h"

#include <cstring>

using namespace tfc::ans;

extern "C" {

// -> the string's length (it is written where it fits `cap`), *status as encode_stream returns it
long long ans_check_encode(const int32_t* lookup, const int32_t* rows, long long nrows, const int32_t* index,
                           const int32_t* value, long long n, int lanes, uint8_t* out, long long cap, int* status) {
  std::vector<uint8_t> bytes;
  *status = encode_stream(lookup, rows, nrows, index, value, n, lanes, &bytes);
  if (static_cast<long long>(bytes.size()) <= cap && !bytes.empty()) std::memcpy(out, bytes.data(), bytes.size());
  return static_cast<long long>(bytes.size());
}

int ans_check_decode(const int32_t* lookup, const int32_t* rows, long long nrows, const int32_t* index,
                     const uint8_t* data, long long len, long long n, int lanes, int32_t* out) {
  return decode_stream(lookup, rows, nrows, index, data, len, n, lanes, out) ? 1 : 0;
}

void ans_check_divmod(const uint32_t* x, const uint32_t* d, long long n, uint32_t* q, uint32_t* r) {
  for (long long i = 0; i < n; ++i) divmod(x[i], d[i], reciprocal(d[i]), &q[i], &r[i]);
}

}  // extern "C"
