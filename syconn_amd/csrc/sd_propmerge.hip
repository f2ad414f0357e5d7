// Dataset-wide merge of per-chunk label statistics on the device (the chunk driver around the natives):
// what /root/reference/syconn/proc/sd_proc.py does with Python dictionaries per chunk (_map_subcell_extract_props_thread :617-678:
// the "purely inside this chunk and below min_obj_vx" filter; merge_prop_dicts :1248-1273; merge_map_dicts :1300-1322) is done here
// on RECORD ARRAYS that never leave HBM until the dataset is finished:
//
//   per chunk   sd_chunkprops_append / sd_chunkpairs_append read the hash tables sd_segstats_scan filled, apply the filter from the
//               table's own bounding boxes (an id lies on one of the six faces of the chunk  <=>  its box touches that face), shift
//               coordinates by the chunk's origin and append records at a device-side cursor -- no host synchronisation per chunk;
//   per dataset sd_propmerge_objects / sd_propmerge_pairs: stable LSD radix sort by id (rocPRIM), head flags, scan, one thread per
//               segment: voxel counts add up, the representative coordinate is the LAST chunk's (dict.update order), the bounding
//               boxes stay one per chunk, listed in chunk order (the reference appends them to a list per id).
//
// Records of one chunk are appended in table order (arbitrary) but chunks are appended in stream order and an id occurs at most once
// per chunk, so a STABLE sort by id alone yields chunk order inside every segment.
#include "../../include/syconn_dense.h"
#include "sd_sortseg.h"

namespace {

// view of an object table as sd_segstats.hip lays it out: keys | first | size | bbmin[3][cap] | bbmax[3][cap]
struct TabView {
    const u64* keys; const u64* first; const u64* size; const int* bbmin; const int* bbmax; u64 cap;
};
inline TabView tab_view(const void* base, u64 cap) {
    TabView t;
    t.keys = reinterpret_cast<const u64*>(base);
    t.first = t.keys + cap;
    t.size = t.first + cap;
    t.bbmin = reinterpret_cast<const int*>(t.size + cap);
    t.bbmax = t.bbmin + 3 * cap;
    t.cap = cap;
    return t;
}

// "purely inside this chunk and smaller than the threshold" (sd_proc.py:640-650 / :657-670); min_vx <= 1 disables the filter
__device__ __forceinline__ bool dropped(const TabView& t, u64 slot, u64 min_vx, int X, int Y, int Z) {
    if (min_vx <= 1 || t.size[slot] >= min_vx) return false;
    const bool on_face = t.bbmin[slot] == 0 || t.bbmin[t.cap + slot] == 0 || t.bbmin[2 * t.cap + slot] == 0 ||
                         t.bbmax[slot] == X || t.bbmax[t.cap + slot] == Y || t.bbmax[2 * t.cap + slot] == Z;
    return !on_face;
}

__global__ __launch_bounds__(256) void k_chunkprops_append(TabView t, int X, int Y, int Z, int ox, int oy, int oz, u64 min_vx,
                                                           u64* ids, int* rc, int* bb, u64* sizes, u64 max_rec, u64* cursor) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < t.cap; i += (u64)gridDim.x * 256) {
        const u64 k = t.keys[i];
        if (k == 0ull || t.size[i] == 0ull) continue;          // size 0: the id was only inserted for the overlap table
        if (dropped(t, i, min_vx, X, Y, Z)) continue;
        const u64 o = atomicAdd(cursor, 1ull);
        if (o >= max_rec) continue;                             // the caller sees cursor > max_rec and repeats with more room
        ids[o] = k; sizes[o] = t.size[i];
        const u64 f = t.first[i];                               // raster index in the (X,Y,Z) chunk, z fastest
        const u64 fxy = f / (u64)Z;
        rc[3 * o + 0] = (int)(fxy / (u64)Y) + ox; rc[3 * o + 1] = (int)(fxy % (u64)Y) + oy; rc[3 * o + 2] = (int)(f % (u64)Z) + oz;
        const int off[3] = {ox, oy, oz};
#pragma unroll
        for (int a = 0; a < 3; ++a) { bb[6 * o + a] = t.bbmin[a * t.cap + i] + off[a]; bb[6 * o + 3 + a] = t.bbmax[a * t.cap + i] + off[a]; }
    }
}

__global__ __launch_bounds__(256) void k_chunkpairs_append(const u64* pkeys, const u64* pcnt, u64 pcap, TabView sub, const u64* cell_keys,
                                                           int X, int Y, int Z, u64 min_vx, u64* out_sub, u64* out_cell, u64* out_cnt,
                                                           u64 max_rec, u64* cursor) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < pcap; i += (u64)gridDim.x * 256) {
        const u64 k = pkeys[i];
        if (k == 0ull) continue;
        const u64 ss = (k - 1) >> 32, cs = (k - 1) & 0xffffffffull;
        if (dropped(sub, ss, min_vx, X, Y, Z)) continue;       // a dropped organelle object leaves the overlap table as well (:668-669)
        const u64 o = atomicAdd(cursor, 1ull);
        if (o >= max_rec) continue;
        out_sub[o] = sub.keys[ss]; out_cell[o] = cell_keys[cs]; out_cnt[o] = pcnt[i];
    }
}

__global__ __launch_bounds__(256) void k_gather64(const u64* src, const u32* idx, u64* dst, u64 n) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) dst[i] = src[idx[i]];
}

// one thread per segment of equal ids: total voxel count, representative coordinate of the last chunk; every thread also moves its own
// record's box into sorted order
__global__ __launch_bounds__(256) void k_reduce_objects(const u64* skey, const u32* perm, const u32* head, const u32* seg, const u64* sizes,
                                                        const int* rc, const int* bb, u64 n, u64* uniq, u64* tot, int* last_rc,
                                                        u32* seg_begin, int* bb_sorted, u64* n_unique) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        const u32 src = perm[i];
#pragma unroll
        for (int a = 0; a < 6; ++a) bb_sorted[6 * i + a] = bb[6 * (u64)src + a];
        if (i == n - 1) *n_unique = (u64)seg[i];
        if (!head[i]) continue;
        const u64 k = skey[i];
        u64 sum = 0, j = i;
        for (; j < n && skey[j] == k; ++j) sum += sizes[perm[j]];
        const u32 s = seg[i] - 1u, last = perm[j - 1];
        uniq[s] = k; tot[s] = sum; seg_begin[s] = (u32)i;
        last_rc[3 * s] = rc[3 * (u64)last]; last_rc[3 * s + 1] = rc[3 * (u64)last + 1]; last_rc[3 * s + 2] = rc[3 * (u64)last + 2];
    }
}

__global__ __launch_bounds__(256) void k_reduce_pairs(const u64* ssub, const u64* scell, const u32* perm, const u32* head, const u32* seg,
                                                      const u64* counts, u64 n, u64* out_sub, u64* out_cell, u64* out_cnt, u64* n_unique) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        if (i == n - 1) *n_unique = (u64)seg[i];
        if (!head[i]) continue;
        const u64 a = ssub[i], b = scell[i];
        u64 sum = 0;
        for (u64 j = i; j < n && ssub[j] == a && scell[j] == b; ++j) sum += counts[perm[j]];
        const u32 s = seg[i] - 1u;
        out_sub[s] = a; out_cell[s] = b; out_cnt[s] = sum;
    }
}

struct Scratch { u64 *k0, *k1, *k2; u32 *i0, *i1, *head, *seg; PrimScratch prim; };
size_t layout(Scratch& w, void* base, size_t n) {
    ScratchAlloc a(base);
    a.take_into(n, w.k0, w.k1, w.k2, w.i0, w.i1, w.head, w.seg);
    w.prim = take_prim(a, n);
    return a.used;
}

}  // namespace

extern "C" {

int sd_chunkprops_append(const void* table, size_t cap_obj, int X, int Y, int Z, int ox, int oy, int oz, uint64_t min_obj_vx,
                         uint64_t* ids_dev, int32_t* rc_dev, int32_t* bbox_dev, uint64_t* sizes_dev, size_t max_records,
                         uint64_t* cursor_dev, void* stream) {
    if (!table || !pow2(cap_obj) || X <= 0 || Y <= 0 || Z <= 0 || !ids_dev || !rc_dev || !bbox_dev || !sizes_dev || !cursor_dev)
        return sd_fail_msg(SD_ERR_INVALID, "sd_chunkprops_append: bad argument");
    launch_1d(k_chunkprops_append, cap_obj, 4096, reinterpret_cast<hipStream_t>(stream), tab_view(table, cap_obj), X, Y, Z, ox, oy, oz,
              (u64)min_obj_vx, reinterpret_cast<u64*>(ids_dev), rc_dev, bbox_dev, reinterpret_cast<u64*>(sizes_dev), (u64)max_records,
              reinterpret_cast<u64*>(cursor_dev));
    return launch_status("sd_chunkprops_append: launch failed");
}

int sd_chunkpairs_append(const void* pair_table, size_t cap_pair, const void* sub_table, const void* cell_table, size_t cap_obj,
                         int X, int Y, int Z, uint64_t min_obj_vx, uint64_t* sub_ids_dev, uint64_t* cell_ids_dev, uint64_t* counts_dev,
                         size_t max_records, uint64_t* cursor_dev, void* stream) {
    if (!pair_table || !pow2(cap_pair) || !sub_table || !cell_table || !pow2(cap_obj) || X <= 0 || Y <= 0 || Z <= 0 || !sub_ids_dev ||
        !cell_ids_dev || !counts_dev || !cursor_dev)
        return sd_fail_msg(SD_ERR_INVALID, "sd_chunkpairs_append: bad argument");
    const u64* pk = reinterpret_cast<const u64*>(pair_table);
    launch_1d(k_chunkpairs_append, cap_pair, 4096, reinterpret_cast<hipStream_t>(stream), pk, pk + cap_pair, (u64)cap_pair,
              tab_view(sub_table, cap_obj), reinterpret_cast<const u64*>(cell_table), X, Y, Z, (u64)min_obj_vx, reinterpret_cast<u64*>(sub_ids_dev),
              reinterpret_cast<u64*>(cell_ids_dev), reinterpret_cast<u64*>(counts_dev), (u64)max_records, reinterpret_cast<u64*>(cursor_dev));
    return launch_status("sd_chunkpairs_append: launch failed");
}

size_t sd_propmerge_temp_bytes(size_t n_records) { Scratch w; return layout(w, nullptr, n_records ? n_records : 1); }

int sd_propmerge_objects(const uint64_t* ids_dev, const uint64_t* sizes_dev, const int32_t* rc_dev, const int32_t* bbox_dev, size_t n,
                         uint64_t* uniq_ids_dev, uint64_t* tot_sizes_dev, int32_t* last_rc_dev, uint32_t* seg_begin_dev,
                         int32_t* bbox_sorted_dev, uint64_t* n_unique_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    if (!n_unique_dev) return sd_fail_msg(SD_ERR_INVALID, "sd_propmerge_objects: null count");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int rc = zero_counts(n_unique_dev, 1, s); rc != SD_OK) return rc;
    if (n == 0) return SD_OK;
    if (n >= (1ull << 32)) return sd_fail_msg(SD_ERR_INVALID, "sd_propmerge_objects: < 2^32 records per call");
    Scratch w;
    if (!ids_dev || !sizes_dev || !rc_dev || !bbox_dev || !uniq_ids_dev || !tot_sizes_dev || !last_rc_dev || !seg_begin_dev ||
        !bbox_sorted_dev || !temp_dev || temp_bytes < layout(w, temp_dev, n))
        return sd_fail_msg(SD_ERR_INVALID, "sd_propmerge_objects: bad argument / scratch smaller than sd_propmerge_temp_bytes(n)");
    const char* who = "sd_propmerge_objects";
    if (int rc = sort_by_key(who, w.prim, reinterpret_cast<const u64*>(ids_dev), w.k0, w.i0, w.i1, n, 64, s); rc != SD_OK) return rc;
    if (int rc = number_segments(who, w.prim, w.k0, nullptr, w.head, w.seg, n, s); rc != SD_OK) return rc;
    launch_1d(k_reduce_objects, n, 4096, s, w.k0, w.i1, w.head, w.seg, reinterpret_cast<const u64*>(sizes_dev), rc_dev, bbox_dev, (u64)n,
              reinterpret_cast<u64*>(uniq_ids_dev), reinterpret_cast<u64*>(tot_sizes_dev), last_rc_dev, seg_begin_dev, bbox_sorted_dev,
              reinterpret_cast<u64*>(n_unique_dev));
    return launch_status("sd_propmerge_objects: launch failed");
}

int sd_propmerge_pairs(const uint64_t* sub_ids_dev, const uint64_t* cell_ids_dev, const uint64_t* counts_dev, size_t n,
                       uint64_t* out_sub_dev, uint64_t* out_cell_dev, uint64_t* out_counts_dev, uint64_t* n_unique_dev, void* temp_dev,
                       size_t temp_bytes, void* stream) {
    if (!n_unique_dev) return sd_fail_msg(SD_ERR_INVALID, "sd_propmerge_pairs: null count");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int rc = zero_counts(n_unique_dev, 1, s); rc != SD_OK) return rc;
    if (n == 0) return SD_OK;
    if (n >= (1ull << 32)) return sd_fail_msg(SD_ERR_INVALID, "sd_propmerge_pairs: < 2^32 records per call");
    Scratch w;
    if (!sub_ids_dev || !cell_ids_dev || !counts_dev || !out_sub_dev || !out_cell_dev || !out_counts_dev || !temp_dev ||
        temp_bytes < layout(w, temp_dev, n))
        return sd_fail_msg(SD_ERR_INVALID, "sd_propmerge_pairs: bad argument / scratch smaller than sd_propmerge_temp_bytes(n)");
    const char* who = "sd_propmerge_pairs";
    const u64* sub = reinterpret_cast<const u64*>(sub_ids_dev);
    const u64* cell = reinterpret_cast<const u64*>(cell_ids_dev);
    // lexicographic (subcell id, cell id): stable sort by the minor key first, then by the major key
    if (int rc = sort_by_key(who, w.prim, cell, w.k0, w.i0, w.i1, n, 64, s); rc != SD_OK) return rc;
    launch_1d(k_gather64, n, 4096, s, sub, w.i1, w.k1, (u64)n);
    if (int rc = sort_carry(who, w.prim, w.k1, w.k2, w.i1, w.i0, n, 64, s); rc != SD_OK) return rc;
    launch_1d(k_gather64, n, 4096, s, cell, w.i0, w.k0, (u64)n);                               // k2 = sorted subcell ids, k0 = their cell ids
    if (int rc = number_segments(who, w.prim, w.k2, w.k0, w.head, w.seg, n, s); rc != SD_OK) return rc;
    launch_1d(k_reduce_pairs, n, 4096, s, w.k2, w.k0, w.i0, w.head, w.seg, reinterpret_cast<const u64*>(counts_dev), (u64)n,
              reinterpret_cast<u64*>(out_sub_dev), reinterpret_cast<u64*>(out_cell_dev), reinterpret_cast<u64*>(out_counts_dev),
              reinterpret_cast<u64*>(n_unique_dev));
    return launch_status("sd_propmerge_pairs: launch failed");
}

}  // extern "C"
