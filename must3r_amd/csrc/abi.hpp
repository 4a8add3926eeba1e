// C ABI plumbing shared by every file that defines must3r_hip_* entry points.  A stateless entry point lives in the file of its
// kernels: a new one means include/must3r_hip.h, that file and must3r_amd/_lib.py, nothing else.
#pragma once
#include "../../include/must3r_hip.h"

namespace m3r {
// records the text for the calling thread (must3r_hip_last_error) and returns 1; defined in model.hip
int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
}  // namespace m3r
