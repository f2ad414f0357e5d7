// Helpers shared by the dataset merges (sd_propmerge.hip, sd_cs_merge.hip): records are ordered by a stable rocPRIM radix sort of
// their u64 ids with a u32 permutation as payload, a head flag marks the first record of every id and an inclusive scan of the
// flags numbers the segments.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>
#include <algorithm>

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

__global__ __launch_bounds__(256) void k_iota(u32* p, u64 n) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) p[i] = (u32)i;
}
// head[i] = 1 where a new key starts in the sorted order
__global__ __launch_bounds__(256) void k_heads(const u64* ka, const u64* kb /* may be nullptr */, u32* head, u64 n) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
        head[i] = (i == 0 || ka[i] != ka[i - 1] || (kb && kb[i] != kb[i - 1])) ? 1u : 0u;
}

inline int grid_for(u64 n, int cap = 4096) { u64 g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > (u64)cap ? (u64)cap : g)); }
inline bool pow2(u64 v) { return v && !(v & (v - 1)); }
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// rocPRIM scratch for n records (radix sort of u64 keys with u32 values, inclusive scan of u32)
inline size_t prim_bytes(size_t n) {
    size_t a = 0, b = 0;
    u64* k = nullptr; u32* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, a, k, k, v, v, n, 0, 64, (hipStream_t)0);
    (void)rocprim::inclusive_scan(nullptr, b, v, v, n, rocprim::plus<u32>(), (hipStream_t)0);
    return up256(std::max(a, b));
}

}  // namespace
