// Dataset-wide merge of contact sites and synapses on the device: the record form of what
// extraction/cs_extraction_steps.py does with Python dictionaries -- the running merges of
// _contact_site_extraction_thread (:484-492, merge_prop_dicts / merge_type_dicts / merge_voxel_dicts per chunk), the pickles its
// workers write, _write_props_collect_helper (:631-673, which loads them again per storage bucket and worker) and the merging,
// joining and filtering half of _write_props_to_syn_thread (:544-623).  As in sd_propmerge.hip nothing per object exists on the host
// before the dataset is finished:
//
//   per chunk   sd_cs_merge_append turns the int64[n][SD_CST_COLS] records of sd_cs_syntype_records and the voxel rows of
//               sd_cs_syntype_voxels into cs records, syn records (sites with syn voxels only) and uint32 voxel rows appended at
//               device-side cursors, coordinates shifted by the origin of the chunk core -- no host synchronisation;
//   per dataset sd_cs_merge_objects, then sd_cs_merge_synapses: stable radix sort by id, head flags, segment numbers, one thread per
//               id: sizes (and type counts) add up, the representative coordinate is the LAST chunk's, the boxes stay one per chunk
//               in chunk order next to their union.  Ids below the size threshold -- for synapses also those whose cs object was
//               dropped (:579, :593) -- leave the compacted output: three scans over the sorted records (kept heads, kept
//               records, kept voxel rows) give every id its output row, every box its slot and every voxel run its position, and
//               the runs of an id are copied into one contiguous run, chunks in chunk order.
//
// Chunks are appended in processing order and an id occurs at most once per chunk, so the STABLE sort by id yields chunk order
// inside every segment whatever order the records of one chunk were appended in.
#include "../../include/syconn_dense.h"
#include "sd_sortseg.h"
#include "sd_tables.h"

namespace {

// cursors[0] cs records, [1] syn records, [2] voxel rows.  Records are counted past their maximum (the caller sees the overrun);
// nothing is written beyond it.
__global__ __launch_bounds__(256) void k_csm_append(const int64_t* __restrict__ rec, u64 n, int ox, int oy, int oz, u64* cs_ids,
                                                    int* cs_rc, int* cs_bb, u64* cs_sizes, u64 max_cs, u64* syn_ids, int* syn_rc,
                                                    int* syn_bb, u64* syn_sizes, u64* syn_asym, u64* syn_sym, u64* syn_vpos, u64 max_syn,
                                                    u64* cursors) {
    const int off[3] = {ox, oy, oz};
    const u64 vbase = cursors[2];                           // advanced by k_csm_vox_advance after this kernel
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        const int64_t* r = rec + i * SD_CST_COLS;
        const u64 o = atomicAdd(&cursors[0], 1ull);
        if (o < max_cs) {
            cs_ids[o] = (u64)r[0]; cs_sizes[o] = (u64)r[4];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                cs_rc[3 * o + a] = (int)r[1 + a] + off[a];
                cs_bb[6 * o + a] = (int)r[5 + a] + off[a]; cs_bb[6 * o + 3 + a] = (int)r[8 + a] + off[a];
            }
        }
        if (r[14] <= 0) continue;                           // no syn voxels: the site has no syn record
        const u64 s = atomicAdd(&cursors[1], 1ull);
        if (s >= max_syn) continue;
        syn_ids[s] = (u64)r[0]; syn_sizes[s] = (u64)r[14]; syn_asym[s] = (u64)r[21]; syn_sym[s] = (u64)r[22];
        syn_vpos[s] = vbase + (u64)r[23];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            syn_rc[3 * s + a] = (int)r[11 + a] + off[a];
            syn_bb[6 * s + a] = (int)r[15 + a] + off[a]; syn_bb[6 * s + 3 + a] = (int)r[18 + a] + off[a];
        }
    }
}

// the chunk's voxel rows (int64, origin included) behind the rows of the chunks before it, as uint32
__global__ __launch_bounds__(256) void k_csm_vox_append(const int64_t* __restrict__ vox, u64 n_rows, u32* __restrict__ dst, u64 max_rows,
                                                        const u64* cursors) {
    const u64 base = cursors[2];
    for (u64 i = grid_tid(); i < 3 * n_rows; i += grid_stride()) {
        const u64 row = base + i / 3;
        if (row < max_rows) dst[3 * base + i] = (u32)vox[i];
    }
}
__global__ void k_csm_vox_advance(u64* cursors, u64 n_rows) { cursors[2] += n_rows; }

// one thread per segment: does the id stay?  Its merged size must reach min_vx; with a join table (the kept cs objects) the id must
// be in it, and its size there is kept for the output.
__global__ __launch_bounds__(256) void k_csm_keep(const u64* skey, const u32* perm, const u32* head, const u32* seg, const u64* sizes, u64 n,
                                                  u64 min_vx, const u64* join_ids, const u64* join_sizes, u64 n_join, int join,
                                                  u32* keepseg, u64* joined) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        if (!head[i]) continue;
        const u64 k = skey[i];
        u64 sum = 0;
        for (u64 j = i; j < n && skey[j] == k; ++j) sum += sizes[perm[j]];
        const u32 s = seg[i] - 1u;
        bool keep = sum >= min_vx;
        u64 jsz = 0;
        if (join) {
            const long at = find_exact(join_ids, n_join, k);
            if (at < 0) keep = false; else jsz = join_sizes[at];
        }
        keepseg[s] = keep ? 1u : 0u; joined[s] = jsz;
    }
}

// per sorted record: kept head, kept record, kept voxel rows (the inputs of the three scans)
__global__ __launch_bounds__(256) void k_csm_flags(const u32* perm, const u32* head, const u32* seg, const u32* keepseg, const u64* sizes,
                                                   int with_vox, u64 n, u32* f_head, u32* f_rec, u32* f_vox) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        const u32 keep = keepseg[seg[i] - 1u];
        f_head[i] = keep & head[i]; f_rec[i] = keep;
        f_vox[i] = (keep && with_vox) ? (u32)sizes[perm[i]] : 0u;
    }
}

struct CsmOut {
    u64 *uniq, *tot; int *last_rc, *ubox; u32* seg_begin; int* bb_sorted;
    u64 *asym_tot, *sym_tot, *join_size; u32* vox_begin;      // synapses only (nullptr otherwise)
    u64* counts;                                              // kept ids, kept boxes, kept voxel rows, ids before the filter
};

// every kept record moves its box to its slot; the head of a kept segment reduces it into output row (kept heads before it)
__global__ __launch_bounds__(256) void k_csm_reduce(const u64* skey, const u32* perm, const u32* head, const u32* seg, const u32* keepseg,
                                                    const u32* s_head, const u32* s_rec, const u32* s_vox, const u64* joined,
                                                    const u64* sizes, const int* rc, const int* bb, const u64* asym, const u64* sym, u64 n,
                                                    CsmOut o) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        if (i == n - 1) { o.counts[0] = s_head[i]; o.counts[1] = s_rec[i]; o.counts[2] = s_vox[i]; o.counts[3] = seg[i]; }
        const u32 s = seg[i] - 1u;
        if (!keepseg[s]) continue;
        const u32 src = perm[i], slot = s_rec[i] - 1u;
#pragma unroll
        for (int a = 0; a < 6; ++a) o.bb_sorted[6 * (u64)slot + a] = bb[6 * (u64)src + a];
        if (!head[i]) continue;
        const u64 k = skey[i];
        u64 sum = 0, na = 0, ns = 0, j = i;
        int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
        for (; j < n && skey[j] == k; ++j) {
            const u64 p = perm[j];
            sum += sizes[p];
            if (asym) { na += asym[p]; ns += sym[p]; }
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], bb[6 * p + a]); hi[a] = max(hi[a], bb[6 * p + 3 + a]); }
        }
        const u64 last = perm[j - 1], row = s_head[i] - 1u;
        o.uniq[row] = k; o.tot[row] = sum; o.seg_begin[row] = slot;
#pragma unroll
        for (int a = 0; a < 3; ++a) { o.last_rc[3 * row + a] = rc[3 * last + a]; o.ubox[6 * row + a] = lo[a]; o.ubox[6 * row + 3 + a] = hi[a]; }
        if (asym) {
            o.asym_tot[row] = na; o.sym_tot[row] = ns; o.join_size[row] = joined[s];
            o.vox_begin[row] = s_vox[i] - (u32)sizes[src];       // exclusive: rows kept before this id's first run
        }
    }
}

// segmented copy of the voxel runs: output row r belongs to the first sorted record whose inclusive scan value exceeds r (records
// without kept rows repeat their predecessor's value and are never first)
__global__ __launch_bounds__(256) void k_csm_copy_runs(const u32* perm, const u32* s_vox, const u64* sizes, const u64* vpos, u64 n,
                                                       const u32* __restrict__ vox_src, u64 n_vox_src, u32* __restrict__ vox_out) {
    const u64 total = min((u64)s_vox[n - 1], n_vox_src);    // kept rows never exceed the rows there are: vox_out holds n_vox_src
    for (u64 r = grid_tid(); r < total; r += grid_stride()) {
        u64 lo = 0, hi = n - 1;                             // s_vox[n - 1] > r
        while (lo < hi) {
            const u64 mid = lo + (hi - lo) / 2;
            if ((u64)s_vox[mid] > r) hi = mid; else lo = mid + 1;
        }
        const u64 p = perm[lo], len = sizes[p];
        const u64 from = vpos[p] + (r - ((u64)s_vox[lo] - len));
        if (from >= n_vox_src) continue;                    // cannot happen for records of sd_cs_merge_append; never read outside
        vox_out[3 * r] = vox_src[3 * from]; vox_out[3 * r + 1] = vox_src[3 * from + 1]; vox_out[3 * r + 2] = vox_src[3 * from + 2];
    }
}

struct CsmScratch { u64 *skey, *joined; u32 *i0, *perm, *head, *seg, *keepseg, *f_head, *f_rec, *f_vox, *s_head, *s_rec, *s_vox; PrimScratch prim; };
size_t layout(CsmScratch& w, void* base, size_t n) {
    ScratchAlloc a(base);
    a.take_into(n, w.skey, w.joined, w.i0, w.perm, w.head, w.seg, w.keepseg, w.f_head, w.f_rec, w.f_vox, w.s_head, w.s_rec, w.s_vox);
    w.prim = take_prim(a, n);
    return a.used;
}

struct CsmIn {
    const u64 *ids, *sizes; const int *rc, *bb; const u64 *asym, *sym, *vpos;
    const u32* vox; u64 n_vox;
    const u64 *join_ids, *join_sizes; u64 n_join; int join;
};

int csm_merge(const char* what, const CsmIn& in, size_t n, u64 min_vx, const CsmOut& o, u32* vox_out, void* temp, size_t temp_bytes,
              hipStream_t s) {
    const char* who = "sd_cs_merge";
    if (!o.counts) return fail(who, ": null counts");
    if (int rc = zero_counts(o.counts, 4, s); rc != SD_OK) return rc;
    if (n == 0) return SD_OK;
    if (n >= (1ull << 32) || in.n_vox >= (1ull << 32)) return fail(who, ": < 2^32 records and voxel rows per call");
    CsmScratch w;
    if (int rc = check_scratch(who, temp, temp_bytes, layout(w, temp, n), "sd_cs_merge_temp_bytes(n)"); rc != SD_OK) return rc;
    if (int rc = sort_by_key(who, w.prim, in.ids, w.skey, w.i0, w.perm, n, 64, s); rc != SD_OK) return rc;
    if (int rc = number_segments(who, w.prim, w.skey, nullptr, w.head, w.seg, n, s); rc != SD_OK) return rc;
    launch_1d(k_csm_keep, n, 4096, s, w.skey, w.perm, w.head, w.seg, in.sizes, (u64)n, min_vx, in.join_ids, in.join_sizes, in.n_join, in.join,
              w.keepseg, w.joined);
    launch_1d(k_csm_flags, n, 4096, s, w.perm, w.head, w.seg, w.keepseg, in.sizes, in.vpos ? 1 : 0, (u64)n, w.f_head, w.f_rec, w.f_vox);
    if (int rc = scan_u32(who, w.prim, w.f_head, w.s_head, n, s); rc != SD_OK) return rc;
    if (int rc = scan_u32(who, w.prim, w.f_rec, w.s_rec, n, s); rc != SD_OK) return rc;
    if (int rc = scan_u32(who, w.prim, w.f_vox, w.s_vox, n, s); rc != SD_OK) return rc;
    launch_1d(k_csm_reduce, n, 4096, s, w.skey, w.perm, w.head, w.seg, w.keepseg, w.s_head, w.s_rec, w.s_vox, w.joined, in.sizes, in.rc, in.bb,
              in.asym, in.sym, (u64)n, o);
    if (in.vpos && in.n_vox)
        launch_1d(k_csm_copy_runs, in.n_vox, 4096, s, w.perm, w.s_vox, in.sizes, in.vpos, (u64)n, in.vox, in.n_vox, vox_out);
    return launch_status(what);
}

}  // namespace

extern "C" {

int sd_cs_merge_append(const int64_t* rec_dev, size_t n, const int64_t* vox_dev, size_t n_vox, int ox, int oy, int oz,
                       uint64_t* cs_ids_dev, int32_t* cs_rc_dev, int32_t* cs_bbox_dev, uint64_t* cs_sizes_dev, size_t max_cs,
                       uint64_t* syn_ids_dev, int32_t* syn_rc_dev, int32_t* syn_bbox_dev, uint64_t* syn_sizes_dev, uint64_t* syn_asym_dev,
                       uint64_t* syn_sym_dev, uint64_t* syn_vpos_dev, size_t max_syn, uint32_t* vox_all_dev, size_t max_vox,
                       uint64_t* cursors_dev, void* stream) {
    if (!cursors_dev || (n && !rec_dev) || (n_vox && !vox_dev))
        return sd_fail_msg(SD_ERR_INVALID, "sd_cs_merge_append: bad argument");
    if ((max_cs && (!cs_ids_dev || !cs_rc_dev || !cs_bbox_dev || !cs_sizes_dev)) ||
        (max_syn && (!syn_ids_dev || !syn_rc_dev || !syn_bbox_dev || !syn_sizes_dev || !syn_asym_dev || !syn_sym_dev || !syn_vpos_dev)) ||
        (max_vox && !vox_all_dev))
        return sd_fail_msg(SD_ERR_INVALID, "sd_cs_merge_append: null record array");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    u64* cur = reinterpret_cast<u64*>(cursors_dev);
    if (n)
        launch_1d(k_csm_append, n, 4096, s, rec_dev, (u64)n, ox, oy, oz, reinterpret_cast<u64*>(cs_ids_dev), cs_rc_dev, cs_bbox_dev,
                  reinterpret_cast<u64*>(cs_sizes_dev), (u64)max_cs, reinterpret_cast<u64*>(syn_ids_dev), syn_rc_dev, syn_bbox_dev,
                  reinterpret_cast<u64*>(syn_sizes_dev), reinterpret_cast<u64*>(syn_asym_dev), reinterpret_cast<u64*>(syn_sym_dev),
                  reinterpret_cast<u64*>(syn_vpos_dev), (u64)max_syn, cur);
    if (n_vox) {
        launch_1d(k_csm_vox_append, 3 * (u64)n_vox, 4096, s, vox_dev, (u64)n_vox, vox_all_dev, (u64)max_vox, cur);
        hipLaunchKernelGGL(k_csm_vox_advance, dim3(1), dim3(1), 0, s, cur, (u64)n_vox);
    }
    return launch_status("sd_cs_merge_append: launch failed");
}

size_t sd_cs_merge_temp_bytes(size_t n_records) { CsmScratch w; return layout(w, nullptr, n_records ? n_records : 1); }

int sd_cs_merge_objects(const uint64_t* ids_dev, const uint64_t* sizes_dev, const int32_t* rc_dev, const int32_t* bbox_dev, size_t n,
                        uint64_t min_obj_vx, uint64_t* uniq_ids_dev, uint64_t* tot_sizes_dev, int32_t* last_rc_dev,
                        int32_t* union_bbox_dev, uint32_t* seg_begin_dev, int32_t* bbox_sorted_dev, uint64_t* counts_dev, void* temp_dev,
                        size_t temp_bytes, void* stream) {
    if (n && (!ids_dev || !sizes_dev || !rc_dev || !bbox_dev || !uniq_ids_dev || !tot_sizes_dev || !last_rc_dev || !union_bbox_dev ||
              !seg_begin_dev || !bbox_sorted_dev))
        return sd_fail_msg(SD_ERR_INVALID, "sd_cs_merge_objects: bad argument");
    CsmIn in{};
    in.ids = reinterpret_cast<const u64*>(ids_dev); in.sizes = reinterpret_cast<const u64*>(sizes_dev); in.rc = rc_dev; in.bb = bbox_dev;
    CsmOut o{};
    o.uniq = reinterpret_cast<u64*>(uniq_ids_dev); o.tot = reinterpret_cast<u64*>(tot_sizes_dev); o.last_rc = last_rc_dev;
    o.ubox = union_bbox_dev; o.seg_begin = seg_begin_dev; o.bb_sorted = bbox_sorted_dev; o.counts = reinterpret_cast<u64*>(counts_dev);
    return csm_merge("sd_cs_merge_objects: launch failed", in, n, (u64)min_obj_vx, o, nullptr, temp_dev, temp_bytes,
                     reinterpret_cast<hipStream_t>(stream));
}

int sd_cs_merge_synapses(const uint64_t* ids_dev, const uint64_t* sizes_dev, const int32_t* rc_dev, const int32_t* bbox_dev,
                         const uint64_t* asym_dev, const uint64_t* sym_dev, const uint64_t* vpos_dev, size_t n,
                         const uint32_t* vox_all_dev, size_t n_vox, const uint64_t* cs_ids_dev, const uint64_t* cs_sizes_dev, size_t n_cs,
                         uint64_t min_obj_vx, uint64_t* uniq_ids_dev, uint64_t* tot_sizes_dev, int32_t* last_rc_dev,
                         int32_t* union_bbox_dev, uint32_t* seg_begin_dev, int32_t* bbox_sorted_dev, uint64_t* asym_tot_dev,
                         uint64_t* sym_tot_dev, uint64_t* cs_size_dev, uint32_t* vox_begin_dev, uint32_t* vox_out_dev,
                         uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    if (n && (!ids_dev || !sizes_dev || !rc_dev || !bbox_dev || !asym_dev || !sym_dev || !vpos_dev || !uniq_ids_dev || !tot_sizes_dev ||
              !last_rc_dev || !union_bbox_dev || !seg_begin_dev || !bbox_sorted_dev || !asym_tot_dev || !sym_tot_dev || !cs_size_dev ||
              !vox_begin_dev || (n_vox && (!vox_all_dev || !vox_out_dev)) || (n_cs && (!cs_ids_dev || !cs_sizes_dev))))
        return sd_fail_msg(SD_ERR_INVALID, "sd_cs_merge_synapses: bad argument");
    CsmIn in{};
    in.ids = reinterpret_cast<const u64*>(ids_dev); in.sizes = reinterpret_cast<const u64*>(sizes_dev); in.rc = rc_dev; in.bb = bbox_dev;
    in.asym = reinterpret_cast<const u64*>(asym_dev); in.sym = reinterpret_cast<const u64*>(sym_dev);
    in.vpos = reinterpret_cast<const u64*>(vpos_dev); in.vox = vox_all_dev; in.n_vox = (u64)n_vox;
    in.join_ids = reinterpret_cast<const u64*>(cs_ids_dev); in.join_sizes = reinterpret_cast<const u64*>(cs_sizes_dev);
    in.n_join = (u64)n_cs; in.join = 1;
    CsmOut o{};
    o.uniq = reinterpret_cast<u64*>(uniq_ids_dev); o.tot = reinterpret_cast<u64*>(tot_sizes_dev); o.last_rc = last_rc_dev;
    o.ubox = union_bbox_dev; o.seg_begin = seg_begin_dev; o.bb_sorted = bbox_sorted_dev; o.counts = reinterpret_cast<u64*>(counts_dev);
    o.asym_tot = reinterpret_cast<u64*>(asym_tot_dev); o.sym_tot = reinterpret_cast<u64*>(sym_tot_dev);
    o.join_size = reinterpret_cast<u64*>(cs_size_dev); o.vox_begin = vox_begin_dev;
    return csm_merge("sd_cs_merge_synapses: launch failed", in, n, (u64)min_obj_vx, o, vox_out_dev, temp_dev, temp_bytes,
                     reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
