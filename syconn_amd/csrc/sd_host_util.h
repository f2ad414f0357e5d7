// Host-side helpers of the extraction-side translation units (label statistics, contact sites, object segmentation, the dataset
// merges, the probe): the error hook of sd_api.hip, the rounding rules for capacities, scratch arrays and 1D grids, and the check
// behind the last launch of an entry point.  The CNN path has its own (differently shaped) helpers and does not include this.
#pragma once
#include "../../include/syconn_dense.h"
#include <hip/hip_runtime.h>
#include <stddef.h>

int sd_fail_msg(int code, const char* msg);      // sd_api.hip: sets sd_last_error()

namespace {

inline bool pow2(unsigned long long v) { return v && !(v & (v - 1)); }
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
// blocks of 256 threads for n items walked with a grid stride: at least one, at most `cap`
inline int grid_for(unsigned long long n, int cap) { const unsigned long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > (unsigned long long)cap ? cap : g)); }
inline int launch_status(const char* what) { return hipGetLastError() == hipSuccess ? SD_OK : sd_fail_msg(SD_ERR_HIP, what); }

}  // namespace
