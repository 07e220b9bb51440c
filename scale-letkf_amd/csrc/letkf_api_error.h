// letkf_api_error.h -- the calling thread's error text and the barrier that closes every C entry (letkf_api_error.hip).
// No HIP in here: a host compiler builds that unit alone.
#pragma once
#include <string>

#include "../../include/letkf_amd.h"

namespace letkf::api {

// sets the text that letkf_amd_last_error() returns on this thread; returns code
int fail(int code, const std::string& msg);
// Inside a catch (...) handler: the exception in flight becomes LETKF_E_INVALID with "<entry>: <what()>" (or "<entry>: unknown
// exception") as the error text.  Nothing leaves it: where building that text throws again, the text is a fixed one.
int fail_exception(const char* entry) noexcept;

}  // namespace letkf::api

// Closes the function-try-block of a C entry: `int letkf_x(...) try { ... } LETKF_ENTRY_END(letkf_x)`.  No C++ exception
// crosses extern "C" -- a bad_alloc that unwinds through bind(C) aborts a Fortran host.  LETKF_ENTRY_END_TO names where the
// code goes instead of `return` (letkf_core_c has a status argument and no result).
#define LETKF_ENTRY_END_TO(name, ...) catch (...) { __VA_ARGS__ letkf::api::fail_exception(#name); }
#define LETKF_ENTRY_END(name) LETKF_ENTRY_END_TO(name, return)
