// The scratch rule and the sort / segment sequence of the dataset merges (sd_propmerge.hip, sd_cs_merge.hip, sd_syn_ssv.hip, ...), over
// the types, the grid-stride walk and the searches of sd_tables.h.
//   scratch   a merge lists its scratch arrays ONCE, in a function that takes them from a ScratchAlloc: without a base pointer that
//             function is the size query (*_temp_bytes), over the caller's buffer it hands out the pointers.  Every array starts on a
//             256-byte boundary; the rocPRIM scratch (take_prim) serves every sort and scan of the call.
//   sequence  stable rocPRIM radix sort of u64 keys with a u32 permutation as payload (sort_by_key: the identity, sort_carry: one
//             that exists already), a head flag at the first record of every key and an inclusive scan of the flags that numbers the
//             segments (number_segments); scan_u32 is the bare scan.  Failures read "<entry point>: radix sort failed" / ": scan failed".
#pragma once
#include "sd_tables.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>
#include <algorithm>
#include <string>

namespace {

__global__ __launch_bounds__(256) void k_iota(u32* p, u64 n) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) p[i] = (u32)i;
}
// head[i] = 1 where a new key starts in the sorted order
__global__ __launch_bounds__(256) void k_heads(const u64* ka, const u64* kb /* may be nullptr */, u32* head, u64 n) {
    for (u64 i = grid_tid(); i < n; i += grid_stride())
        head[i] = (i == 0 || ka[i] != ka[i - 1] || (kb && kb[i] != kb[i - 1])) ? 1u : 0u;
}

// bump allocator over the caller's scratch; without a base it only adds up the sizes
struct ScratchAlloc {
    char* base; size_t used;
    explicit ScratchAlloc(void* b = nullptr) : base(reinterpret_cast<char*>(b)), used(0) {}
    template <class T> T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += up256(count * sizeof(T));
        return p;
    }
    template <class... T> void take_into(size_t count, T*&... p) { ((p = take<T>(count)), ...); }       // `count` elements for each
};

// rocPRIM scratch for n records (radix sort of u64 keys with u32 values, inclusive scan of u32)
struct PrimScratch { void* p; size_t bytes; };
inline PrimScratch take_prim(ScratchAlloc& a, size_t n) {
    size_t sb = 0, cb = 0;
    u64* k = nullptr; u32* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, sb, k, k, v, v, n, 0, 64, (hipStream_t)0);
    (void)rocprim::inclusive_scan(nullptr, cb, v, v, n, rocprim::plus<u32>(), (hipStream_t)0);
    const size_t bytes = up256(std::max(sb, cb));
    return PrimScratch{a.take<char>(bytes), bytes};
}

inline int sortseg_fail(const char* who, const char* what) { return sd_fail_msg(SD_ERR_HIP, (std::string(who) + what).c_str()); }

// stable sort of (keys, perm_in) by bits [0, bits) of the keys; Keys = u64* or const u64* (rocPRIM's kernels carry the type)
template <class Keys>
inline int sort_carry(const char* who, const PrimScratch& prim, Keys keys, u64* keys_sorted, u32* perm_in, u32* perm_out, size_t n,
                      int bits, hipStream_t s) {
    size_t pb = prim.bytes;
    if (rocprim::radix_sort_pairs(prim.p, pb, keys, keys_sorted, perm_in, perm_out, n, 0, bits, s) != hipSuccess)
        return sortseg_fail(who, ": radix sort failed");
    return SD_OK;
}
// the same with the identity permutation (written to `iota`) as payload: perm_out[i] is where sorted record i came from
template <class Keys>
inline int sort_by_key(const char* who, const PrimScratch& prim, Keys keys, u64* keys_sorted, u32* iota, u32* perm_out, size_t n, int bits,
                       hipStream_t s) {
    launch_1d(k_iota, n, 4096, s, iota, (u64)n);
    return sort_carry(who, prim, keys, keys_sorted, iota, perm_out, n, bits, s);
}
inline int scan_u32(const char* who, const PrimScratch& prim, u32* in, u32* out, size_t n, hipStream_t s) {
    size_t pb = prim.bytes;
    if (rocprim::inclusive_scan(prim.p, pb, in, out, n, rocprim::plus<u32>(), s) != hipSuccess) return sortseg_fail(who, ": scan failed");
    return SD_OK;
}
// head flags of the sorted keys (ka, and kb where given) and the 1-based segment number of every record
inline int number_segments(const char* who, const PrimScratch& prim, const u64* ka, const u64* kb, u32* head, u32* seg, size_t n,
                           hipStream_t s) {
    launch_1d(k_heads, n, 4096, s, ka, kb, head, (u64)n);
    return scan_u32(who, prim, head, seg, n, s);
}

}  // namespace
