// orbfe_internal.h — what the kernel files need of each other (orbfe_kernels.h is orbfe_host.hip's interface).
// Not exported from the library.
#pragma once

#include "orbfe_kernels.h"

namespace orbfe {
#pragma GCC visibility push(hidden)
// The per-device dynamic-LDS limit of a kernel that asks for more than 64 KiB (orbfe_kernels.hip).  raise_lds: to
// at least `bytes` on the current device (never lowered; at most 160 KiB); lds_limit: what was raised there.
hipError_t raise_lds(const void* fn, int bytes);
int lds_limit(const void* fn);
#pragma GCC visibility pop
}  // namespace orbfe
