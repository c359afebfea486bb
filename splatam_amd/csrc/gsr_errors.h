// gsr_errors.h -- error reporting and argument tests shared by the C entry points of every file.
#pragma once
#include <string>

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

// error reporting shared by the C entry points (gsr_last_error)
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* where);
// the sequence steps' argument tests: an image whose pixel index fits an int, a workspace's alignment
inline bool image_size_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL; }
inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }
// the `terms` output of the gsr_track_*_terms entries (two floats): not NULL, 4-byte aligned (gsr_capi.hip)
int check_terms(const char* entry, const float* terms);

}  // namespace gsr
