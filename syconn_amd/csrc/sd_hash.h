// Device hash-table helpers shared by the label-statistics passes (sd_segstats.hip, sd_cs_syntype.hip): open addressing with
// linear probing over u64 keys in caller-owned device memory, key 0 = empty slot (label 0 is background and never inserted),
// and the run structure of a wave that lets a pass issue one table update per run of equal labels instead of one per voxel.
#pragma once
#include "sd_host_util.h"
#include <stdint.h>

namespace {

typedef unsigned long long u64;
constexpr u64 EMPTY = 0ull;

__device__ __forceinline__ u64 mix64(u64 k) {             // murmur3 finaliser
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

// slot of `k` in an open-addressing table (linear probing), inserting it if absent; -1 when the table is full
__device__ __forceinline__ long find_or_insert(u64* keys, u64 cap, u64 k) {
    const u64 mask = cap - 1;
    u64 h = mix64(k) & mask;
    for (u64 probe = 0; probe < cap; ++probe, h = (h + 1) & mask) {
        u64 cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == k) return (long)h;
        if (cur == EMPTY) {
            const u64 old = atomicCAS(&keys[h], EMPTY, k);
            if (old == EMPTY || old == k) return (long)h;
        }
    }
    return -1;
}

// run structure of a wave: `head` lanes start a run of equal values inside one z-row; returns the run length for head lanes
__device__ __forceinline__ int run_length(bool head, int lane, int nvalid) {
    const u64 m = __ballot(head);
    const u64 later = (lane == 63) ? 0ull : (m >> (lane + 1));
    int next = later ? (lane + 1 + __builtin_ctzll(later)) : 64;
    if (next > nvalid) next = nvalid;
    return next - lane;
}

// the grid-stride launches over a table or a volume in the files that include this header share one cap (sd_host_util.h defines
// grid_for; this declaration only gives it the default, and the label-statistics tests read the figure from here)
inline int grid_for(u64 n, int cap = 4096);

}  // namespace
