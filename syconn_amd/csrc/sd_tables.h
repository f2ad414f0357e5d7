// What the table and graph kernels of the dataset stage share (sd_skeleton.hip, sd_cell_assembly.hip, sd_syn_ssv.hip, sd_cs_merge.hip,
// the union-find also sd_objseg.hip): the grid-stride walk, binary searches over ascending arrays, the checks of offset and id tables,
// and the union-find.  Plain device code over sd_host_util.h: sd_sortseg.h (the sorts, with rocPRIM) and sd_pointtiles.h (the point
// queries) build on it, and a file that only labels components (sd_objseg.hip) takes it without either.
//   searches    lower_bound / upper_bound / find_exact over an ascending a[0 .. n); segment_of turns an item into the segment that owns
//               it under offsets begin[0 .. n_segments].  Results are clamped, so a bad table can mislead a kernel but never send it
//               outside the table.
//   checks      k_check_offsets / k_check_ascending raise counts[7] (the "bad input table" slot of every entry point that has 8 count
//               slots); which slot it is belongs to these kernels, not to their callers.
//   union-find  ONE link rule: the larger root goes under the smaller one, so the root of a set is its smallest member.  That is a
//               contract, not a detail: it is the cell id of sd_cell_assembly.hip, the first voxel in raster order of sd_objseg.hip and
//               the component numbering of sd_syn_ssv.hip.
#pragma once
#include "sd_host_util.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

const size_t LIM31 = (size_t)1 << 31;                        // counts per call stay below it (32-bit permutations, int grids)

// bits that hold every value of [0, n), n < 2^31: the segment field of a key
inline int bits_for(u64 n) {
    int b = 0;
    while (b < 31 && ((n - 1) >> b)) ++b;
    return b;
}

// ---- the grid-stride walk of a kernel with 256-thread blocks: for (u64 i = grid_tid(); i < n; i += grid_stride()) -----------------------
__device__ __forceinline__ u64 grid_tid() { return (u64)blockIdx.x * 256 + threadIdx.x; }
__device__ __forceinline__ u64 grid_stride() { return (u64)gridDim.x * 256; }

__device__ __forceinline__ u64 clamp_u64(u64 v, u64 hi) { return v < hi ? v : hi; }

// ---- searches over an ascending a[0 .. n) -----------------------------------------------------------------------------------------
// first index whose element is >= key (n if none)
template <class T> __device__ __forceinline__ u64 lower_bound(const T* a, u64 n, u64 key) {
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if ((u64)a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first index whose element is > key (n if none)
template <class T> __device__ __forceinline__ u64 upper_bound(const T* a, u64 n, u64 key) {
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if ((u64)a[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first index that holds `key`, or -1
template <class T> __device__ __forceinline__ long find_exact(const T* a, u64 n, u64 key) {
    const u64 lo = lower_bound(a, n, key);
    return (lo < n && (u64)a[lo] == key) ? (long)lo : -1;
}
// the segment of item j under the offsets begin[0 .. n_segments]; clamped into [0, n_segments) whatever the table holds
template <class T> __device__ __forceinline__ u64 segment_of(const T* begin, u64 n_segments, u64 j) {
    u64 s = upper_bound(begin, n_segments + 1, j);
    s = s ? s - 1 : 0;
    return s < n_segments ? s : n_segments - 1;
}

// ---- table checks: a table that fails sets counts[7] ------------------------------------------------------------------------------
// offsets begin[0 .. n + 1) must ascend from 0 to n_items
__global__ __launch_bounds__(256) void k_check_offsets(const u64* __restrict__ begin, u64 n, u64 n_items, u64* counts) {
    for (u64 c = grid_tid(); c < n; c += grid_stride()) {
        const u64 b0 = begin[c], b1 = begin[c + 1];
        if (b1 < b0 || b1 > n_items || (c == 0 && b0 != 0) || (c == n - 1 && b1 != n_items)) counts[7] = 1;
    }
}
// ids must ascend strictly
__global__ __launch_bounds__(256) void k_check_ascending(const u64* __restrict__ ids, u64 n, u64* counts) {
    for (u64 i = grid_tid() + 1; i < n; i += grid_stride())
        if (ids[i] <= ids[i - 1]) counts[7] = 1;
}

// ---- union-find over L[0 .. n), L[i] = i at the start; I = int or u32 --------------------------------------------------------------
// A link only ever lowers an entry (atomicMin), so L[a] <= a always and every chain descends strictly: uf_find ends, whatever else runs.
// The loads are relaxed atomics of agent scope, which keeps them out of the CU's L1, where a line may be older than a link another CU
// has sent to the L2.  Nothing stronger is needed: a value that is out of date is still an ancestor of `a` (at worst no longer a root),
// and the only step that must see the present is the link itself, a read-modify-write at the L2.  Roots are final once the kernel that
// unites has ended; the callers read them in a later kernel.
template <class I> __device__ __forceinline__ I uf_find(const I* L, I a) {
    I p = __hip_atomic_load(&L[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != a) { a = p; p = __hip_atomic_load(&L[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    return a;
}
template <class I> __device__ __forceinline__ void uf_union(I* L, I a, I b) {
    while (true) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) { const I t = a; a = b; b = t; }          // link the larger root under the smaller one
        const I old = atomicMin(&L[a], b);
        if (old == a) return;                                // a was still a root: linked
        a = old;                                             // somebody else re-linked a meanwhile; L[a] = min(old, b) now keeps one of the
    }                                                        // two links, and uniting (old, b) makes the other: retry from there
}

}  // namespace
