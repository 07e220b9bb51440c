// letkf_api_error.hip -- C ABI, the error text of the calling thread: fail(), the exception barrier of the entries, and the
// two entries that need neither a context nor a barrier.  Host code without any HIP include (tests/test_entry_barrier.py
// builds it with the host compiler and throws into the barrier).

#include "letkf_api_error.h"

#include <exception>

namespace {
thread_local std::string g_last_error;
thread_local const char* g_fixed_error = nullptr;   // in place of g_last_error where no text could be built
}  // namespace

namespace letkf::api {

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  g_fixed_error = nullptr;
  return code;
}

int fail_exception(const char* entry) noexcept {
  try {
    try {
      throw;
    } catch (const std::exception& e) {
      return fail(LETKF_E_INVALID, std::string(entry) + ": " + e.what());
    } catch (...) {
      return fail(LETKF_E_INVALID, std::string(entry) + ": unknown exception");
    }
  } catch (...) {
    g_fixed_error = "a C++ exception, and no memory for its text";
    return LETKF_E_INVALID;
  }
}

}  // namespace letkf::api

extern "C" {

int letkf_amd_abi_version(void) { return LETKF_AMD_ABI_VERSION; }

const char* letkf_amd_last_error(void) { return g_fixed_error ? g_fixed_error : g_last_error.c_str(); }

}  // extern "C"
