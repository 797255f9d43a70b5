// abi_util.h — what the units behind the C ABI (include/sezkp_stark.h) share
// and need no HIP header for: the error an entry point's body throws, the
// wrapper that turns it into a return code and a message, and the copies into
// a caller-owned sezkp_buf. abi_host.cpp sees only this; the units that touch
// the device get it through prover_ctx.h.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <exception>
#include <string>
#include <vector>

#include "../../include/sezkp_stark.h"

#define SEZKP_LOCAL __attribute__((visibility("hidden")))

// one type and one copy of each helper per library, none among its symbols
#pragma GCC visibility push(hidden)

namespace sezkp::detail {
struct Err {
  int32_t code;
  std::string msg;
};

inline void set_err(char* err, size_t len, const std::string& m) {
  if (err && len) {
    snprintf(err, len, "%s", m.c_str());
  }
}
}  // namespace sezkp::detail
using namespace sezkp::detail;

// Runs an entry point's body: SEZKP_OK, or an Err's code and message, or
// `other` with the message of any other exception (SEZKP_E_NOMEM everywhere
// but sezkp_ctx_dist_ntt).
template <class F>
int32_t guarded(char* err, size_t err_len, int32_t other, F&& body) {
  try {
    body();
    return SEZKP_OK;
  } catch (const Err& e) {
    set_err(err, err_len, e.msg);
    return e.code;
  } catch (const std::exception& e) {
    set_err(err, err_len, e.what());
    return other;
  }
}

inline void to_buf(const std::vector<uint8_t>& v, sezkp_buf* out) {
  out->data = (uint8_t*)malloc(v.size() ? v.size() : 1);
  if (!out->data) throw Err{SEZKP_E_NOMEM, "out of host memory"};
  memcpy(out->data, v.data(), v.size());
  out->len = v.size();
}
inline void to_buf(const std::string& s, sezkp_buf* out) { to_buf(std::vector<uint8_t>(s.begin(), s.end()), out); }
#pragma GCC visibility pop
