// Host-side helpers of the extraction-side translation units (label statistics, contact sites, object segmentation, the dataset
// merges, the probe): the error hook of sd_api.hip, the rounding rules for capacities, scratch arrays and 1D grids, the steps every
// entry point opens with (reject, zero the counts, check the scratch), the 1D launch, and the check behind the last launch of an
// entry point.  The CNN path has its own (differently shaped) helpers and does not include this.
#pragma once
#include "../../include/syconn_dense.h"
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string>

int sd_fail_msg(int code, const char* msg);      // sd_api.hip: sets sd_last_error()

namespace {

inline bool pow2(unsigned long long v) { return v && !(v & (v - 1)); }
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
// blocks of 256 threads for n items walked with a grid stride: at least one, at most `cap`
inline int grid_for(unsigned long long n, int cap) { const unsigned long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > (unsigned long long)cap ? cap : g)); }
// kernel<<<grid_for(n, cap), 256, 0, s>>>(args...): THE launch of a __launch_bounds__(256) kernel that walks n items with a grid stride
template <class... P, class... A> inline void launch_1d(void (*kernel)(P...), unsigned long long n, int cap, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(n, cap)), dim3(256), 0, s, args...);
}
inline int launch_status(const char* what) { return hipGetLastError() == hipSuccess ? SD_OK : sd_fail_msg(SD_ERR_HIP, what); }

// ---- the opening of an entry point `who`: the first check that fails decides the message ---------------------------------------------
inline int fail(const char* who, const char* what) { return sd_fail_msg(SD_ERR_INVALID, (std::string(who) + what).c_str()); }
// the first n_slots 64-bit counts to 0, in stream order before the kernels that raise them
inline int zero_counts(void* counts, size_t n_slots, hipStream_t s) {
    return hipMemsetAsync(counts, 0, n_slots * sizeof(unsigned long long), s) == hipSuccess ? SD_OK : sd_fail_msg(SD_ERR_HIP, "memset failed");
}
// `query` names the size query with its arguments as the caller would write it: "sd_x_temp_bytes(n)"
inline int check_scratch(const char* who, const void* temp, size_t temp_bytes, size_t need, const char* query) {
    return temp && temp_bytes >= need ? SD_OK : fail(who, (std::string(": scratch smaller than ") + query).c_str());
}

}  // namespace
