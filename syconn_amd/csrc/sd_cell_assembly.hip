// Cells from the supervoxel graph and organelles to cells: the array form of what the reference does object by object in Python --
// exec/exec_init.py run_create_rag (:299-367) and the size-threshold branch of run_create_neuron_ssd (:61-80) over networkx with
// proc/graphs.py create_ccsize_dict (:220-249); the cell properties of reps/super_segmentation_object.py (:713-727, :1148-1168); the
// overlap ratios of proc/sd_proc.py (:1063-1084) summed with a Counter per cell and decided by proc/ssd_proc.py (:55-91, :126-238);
// map_synssv_objects_thread (:315-342).
//
//   components  the node universe = the table ids and every edge endpoint without 0: one 64-bit sort of both, a head per distinct id,
//               a scan; row r of the universe is the r-th smallest id, an id finds its row by binary search.  Union-find over the rows
//               (uf_union of sd_tables.h: the root is the smallest id of the component, which is the reference's cell id),
//               then one pass that writes every node's root before anything reads one.  Boxes and voxel counts of the table's
//               supervoxels go to their root by integer atomics; the size of a component is the float64 norm of its scaled extent
//               with every product and sum rounded on its own, and a correctly rounded square root.  The cells in CSR form are a
//               stable sort of the kept nodes by root row: cells ascending, supervoxels ascending inside.  The surviving edges are a
//               flag, a scan and a scatter.  The number of nodes is known only on the device: every later kernel reads it from the
//               counts and clamps it to the capacity.
//   properties  per supervoxel of a cell list: its table row by binary search, size and boxes to the cell by integer atomics.
//   mapping     the supervoxel -> (cell, position) lookup is a sort of the cell lists (an id seen twice sets counts[6]).  A record
//               (organelle, supervoxel, voxels) that finds both gets ratio = voxels / size; two stable sorts (by the position in the
//               concatenated cell lists, then by (cell row, organelle row)) leave every (cell, organelle) run in the order of the cell's
//               supervoxel list, and ONE thread adds a run from its first record on: float order is part of the contract, so there is no
//               float atomic and no tree sum here.
//   synapses    the 2 n half records (slot 0 first), keyed by the cell row of their partner: one stable sort.
//
// Every index read from device memory is clamped or checked before it is used.  No scalar memory writes, no inline assembly.
#include "../../include/syconn_dense.h"
#include "sd_sortseg.h"
#include "sd_tables.h"
#include <limits.h>

namespace {

constexpr int GRID = SD_CELLASM_GRID;
constexpr int CELL_SHIFT = 31;                               // pair key = cell row << 31 | organelle row
constexpr u64 NO_PAIR = 1ull << 62;                          // above every pair key: a dropped record
constexpr u64 ORG_MASK = (1ull << CELL_SHIFT) - 1;

// ---- components -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cc_universe(const u64* __restrict__ ids, u64 n_ids, const u64* __restrict__ edges, u64 m, u64* key) {
    for (u64 i = grid_tid(); i < m; i += grid_stride()) key[i] = i < n_ids ? ids[i] : edges[i - n_ids];
}
// row r = the r-th smallest id that is not 0; counts[0] = their number
__global__ __launch_bounds__(256) void k_cc_rows(const u64* __restrict__ skey, const u32* __restrict__ head, const u32* __restrict__ seg, u64 m,
                                                 u64* node_ids, u64* counts) {
    const u64 z = skey[0] == 0 ? 1 : 0;
    for (u64 i = grid_tid(); i < m; i += grid_stride()) {
        if (head[i] && skey[i] != 0) node_ids[clamp_u64((u64)seg[i] - 1 - z, m - 1)] = skey[i];
        if (i == m - 1) counts[0] = (u64)seg[i] - z;
    }
}
__global__ __launch_bounds__(256) void k_cc_union(const u64* __restrict__ edges, u64 n_edges, const u64* __restrict__ node_ids, u64 m, u32* parent,
                                                  u64* counts) {
    const u64 n = clamp_u64(counts[0], m);
    for (u64 e = grid_tid(); e < n_edges; e += grid_stride()) {
        const u64 a = edges[2 * e], b = edges[2 * e + 1];
        if (!a || !b) continue;                                                  // node 0 is removed, and its edges with it
        const long ra = find_exact(node_ids, n, a), rb = find_exact(node_ids, n, b);
        if (ra < 0 || rb < 0) { counts[7] = 1; continue; }
        uf_union(parent, (u32)ra, (u32)rb);
    }
}
__global__ __launch_bounds__(256) void k_cc_roots(const u32* __restrict__ parent, u64 m, u32* root, int* cbox, u64* cvox, const u64* counts) {
    const u64 n = clamp_u64(counts[0], m);
    for (u64 r = grid_tid(); r < n; r += grid_stride()) {
        root[r] = uf_find(parent, (u32)r);
        for (int a = 0; a < 3; ++a) { cbox[6 * r + a] = INT_MAX; cbox[6 * r + 3 + a] = INT_MIN; }
        cvox[r] = 0;
    }
}
__global__ __launch_bounds__(256) void k_cc_boxes(const u64* __restrict__ ids, const long long* __restrict__ sizes, const u64* __restrict__ box_begin,
                                                  const int* __restrict__ boxes, u64 n_ids, u64 n_boxes, const u64* __restrict__ node_ids,
                                                  const u32* __restrict__ root, u64 m, int* cbox, u64* cvox, u64* counts) {
    const u64 n = clamp_u64(counts[0], m);
    for (u64 i = grid_tid(); i < n_ids; i += grid_stride()) {
        const u64 id = ids[i];
        if (!id) continue;
        const long r = find_exact(node_ids, n, id);
        if (r < 0) { counts[7] = 1; continue; }
        const u64 rt = clamp_u64(root[r], n - 1);
        atomicAdd(&cvox[rt], (u64)sizes[i]);
        const u64 b1 = clamp_u64(box_begin[i + 1], n_boxes), b0 = clamp_u64(box_begin[i], b1);
        for (u64 b = b0; b < b1; ++b)
            for (int a = 0; a < 3; ++a) {                                        // np.min / np.max over BOTH corners of every box
                const int lo = boxes[6 * b + a], hi = boxes[6 * b + 3 + a];
                atomicMin(&cbox[6 * rt + a], lo < hi ? lo : hi);
                atomicMax(&cbox[6 * rt + 3 + a], lo < hi ? hi : lo);
            }
    }
}
// np.linalg.norm((max - min) of the scaled corners): max * s - min * s, then ((dx dx) + dy dy) + dz dz and its square root
__device__ __forceinline__ double extent_norm(const int* bx, double sx, double sy, double sz) {
#pragma clang fp contract(off)
    const double dx = (double)bx[3] * sx - (double)bx[0] * sx, dy = (double)bx[4] * sy - (double)bx[1] * sy, dz = (double)bx[5] * sz - (double)bx[2] * sz;
    return __builtin_sqrt(((dx * dx) + dy * dy) + dz * dz);
}
__global__ __launch_bounds__(256) void k_cc_sizes(const u32* __restrict__ root, const int* __restrict__ cbox, const u64* __restrict__ cvox,
                                                  const u64* __restrict__ node_ids, u64 m, double sx, double sy, double sz, double min_size, int strict,
                                                  double* csize, u32* keep, u64* counts) {
    const u64 n = clamp_u64(counts[0], m);
    for (u64 r = grid_tid(); r < n; r += grid_stride()) {
        if (root[r] != r) continue;
        if (cbox[6 * r] == INT_MAX) {                                            // no supervoxel of the component is in the table
            counts[6] = 1;
            counts[5] = node_ids[r];
            csize[r] = 0.0;
            keep[r] = 0;
            continue;
        }
        const double size = extent_norm(cbox + 6 * r, sx, sy, sz);
        const bool k = strict ? size > min_size : size >= min_size;
        csize[r] = size;
        keep[r] = k ? 1u : 0u;
        if (k) atomicAdd(&counts[4], cvox[r]);
    }
}
__global__ __launch_bounds__(256) void k_cc_nodes(const u32* __restrict__ root, const u32* __restrict__ keep, const double* __restrict__ csize,
                                                  const u64* __restrict__ node_ids, u64 m, u64* node_comp, double* node_size, u64* key, const u64* counts) {
    const u64 n = clamp_u64(counts[0], m);
    for (u64 r = grid_tid(); r < m; r += grid_stride()) {
        if (r >= n) { key[r] = m; continue; }
        const u64 rt = clamp_u64(root[r], n - 1);
        const bool k = keep[rt] != 0;
        node_comp[r] = k ? node_ids[rt] : 0;
        node_size[r] = csize[rt];
        key[r] = k ? rt : m;
    }
}
// the kept nodes sorted by root row: cell numbers from the heads; the first dropped record (or the end) closes the table
__global__ __launch_bounds__(256) void k_cc_csr(const u64* __restrict__ skey, const u32* __restrict__ perm, const u32* __restrict__ head,
                                                const u32* __restrict__ seg, const u64* __restrict__ node_ids, u64 m, u64* ssv_ids, u64* sv_begin,
                                                u64* sv_ids, u64* counts) {
    for (u64 i = grid_tid(); i < m; i += grid_stride()) {
        const u64 k = skey[i];
        if (k >= m) {
            if (i == 0 || skey[i - 1] < m) {
                const u64 cells = i ? seg[i - 1] : 0;
                counts[1] = cells;
                counts[2] = i;
                sv_begin[clamp_u64(cells, m)] = i;
            }
            continue;
        }
        sv_ids[i] = node_ids[clamp_u64(perm[i], m - 1)];
        const u64 c = clamp_u64((u64)seg[i] - 1, m - 1);
        if (head[i]) { ssv_ids[c] = node_ids[k]; sv_begin[c] = i; }
        if (i == m - 1) { counts[1] = c + 1; counts[2] = m; sv_begin[c + 1] = m; }
    }
}
__global__ __launch_bounds__(256) void k_cc_edge_flags(const u64* __restrict__ edges, u64 n_edges, const u64* __restrict__ node_ids,
                                                       const u32* __restrict__ root, const u32* __restrict__ keep, u64 m, u32* flag, const u64* counts) {
    const u64 n = clamp_u64(counts[0], m);
    for (u64 e = grid_tid(); e < n_edges; e += grid_stride()) {
        const u64 a = edges[2 * e], b = edges[2 * e + 1];
        u32 f = 0;
        if (a && b) {
            const long ra = find_exact(node_ids, n, a);
            if (ra >= 0) f = keep[clamp_u64(root[ra], n - 1)];
        }
        flag[e] = f;
    }
}
__global__ __launch_bounds__(256) void k_cc_edges_out(const u64* __restrict__ edges, u64 n_edges, const u32* __restrict__ flag, const u32* __restrict__ pos,
                                                      u64* edges_out, u64* counts) {
    for (u64 e = grid_tid(); e < n_edges; e += grid_stride()) {
        if (flag[e]) {
            const u64 o = clamp_u64((u64)pos[e] - 1, n_edges - 1);
            edges_out[2 * o] = edges[2 * e];
            edges_out[2 * o + 1] = edges[2 * e + 1];
        }
        if (e == n_edges - 1) counts[3] = pos[e];
    }
}

// ---- cell properties --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_props_init(const u64* __restrict__ sv_begin, const u64* __restrict__ sv_ids, u64 n_cells, u64 n_sv,
                                                    const u64* __restrict__ ids, const int* __restrict__ rep, u64 n_ids, long long* cell_size,
                                                    int* cell_box, int* cell_rep) {
    for (u64 c = grid_tid(); c < n_cells; c += grid_stride()) {
        const u64 b1 = clamp_u64(sv_begin[c + 1], n_sv), b0 = clamp_u64(sv_begin[c], b1);
        cell_size[c] = 0;
        for (int a = 0; a < 3; ++a) { cell_box[6 * c + a] = INT_MAX; cell_box[6 * c + 3 + a] = INT_MIN; }
        const long t = b0 < b1 ? find_exact(ids, n_ids, sv_ids[b0]) : -1;       // the first supervoxel in the cell's order
        for (int a = 0; a < 3; ++a) cell_rep[3 * c + a] = t >= 0 ? rep[3 * t + a] : 0;
    }
}
__global__ __launch_bounds__(256) void k_props_sv(const u64* __restrict__ sv_begin, const u64* __restrict__ sv_ids, u64 n_cells, u64 n_sv,
                                                  const u64* __restrict__ ids, const long long* __restrict__ sizes, const u64* __restrict__ box_begin,
                                                  const int* __restrict__ boxes, u64 n_ids, u64 n_boxes, long long* cell_size, int* cell_box, u64* counts) {
    for (u64 j = grid_tid(); j < n_sv; j += grid_stride()) {
        const u64 c = segment_of(sv_begin, n_cells, j);
        if (j < sv_begin[c] || j >= sv_begin[c + 1]) { counts[7] = 1; continue; }
        const u64 id = sv_ids[j];
        const long t = find_exact(ids, n_ids, id);
        if (t < 0) { atomicAdd(&counts[0], 1ull); counts[5] = id; continue; }
        atomicAdd(reinterpret_cast<u64*>(&cell_size[c]), (u64)sizes[t]);
        const u64 b1 = clamp_u64(box_begin[t + 1], n_boxes), b0 = clamp_u64(box_begin[t], b1);
        for (u64 b = b0; b < b1; ++b)
            for (int a = 0; a < 3; ++a) {
                atomicMin(&cell_box[6 * c + a], boxes[6 * b + a]);
                atomicMax(&cell_box[6 * c + 3 + a], boxes[6 * b + 3 + a]);
            }
    }
}
__global__ __launch_bounds__(256) void k_props_finish(u64 n_cells, int* cell_box) {
    for (u64 c = grid_tid(); c < n_cells; c += grid_stride())
        if (cell_box[6 * c] == INT_MAX)                                          // no known supervoxel: the zero box (:1158-1161)
            for (int a = 0; a < 6; ++a) cell_box[6 * c + a] = 0;
}

// ---- mapping ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_map_lookup_check(const u64* __restrict__ lsv, u64 n_sv, u64* counts) {
    for (u64 p = grid_tid(); p < n_sv; p += grid_stride())
        if (lsv[p] == 0 || (p && lsv[p] == lsv[p - 1])) counts[6] = 1;
}
__global__ __launch_bounds__(256) void k_map_records(const u64* __restrict__ rec_sub, const u64* __restrict__ rec_sv, const long long* __restrict__ rec_cnt,
                                                     u64 n_rec, const u64* __restrict__ org_ids, const long long* __restrict__ org_sizes, u64 n_org,
                                                     const u64* __restrict__ lsv, const u32* __restrict__ lperm, const u64* __restrict__ sv_begin,
                                                     u64 n_cells, u64 n_sv, u64* key_pos, u64* key_pair, double* ratio) {
    for (u64 i = grid_tid(); i < n_rec; i += grid_stride()) {
        const u64 sv = rec_sv[i];
        const long long cnt = rec_cnt[i];
        const long o = find_exact(org_ids, n_org, rec_sub[i]);
        const long p = sv ? find_exact(lsv, n_sv, sv) : -1;
        if (o < 0 || p < 0 || cnt <= 0) { key_pos[i] = n_sv; key_pair[i] = NO_PAIR; ratio[i] = 0.0; continue; }
        const u64 j = clamp_u64(lperm[p], n_sv - 1);
        key_pos[i] = j;
        key_pair[i] = segment_of(sv_begin, n_cells, j) << CELL_SHIFT | (u64)o;
        ratio[i] = (double)cnt / (double)org_sizes[o];
    }
}
__global__ __launch_bounds__(256) void k_map_gather(const u64* __restrict__ key_pair, const u32* __restrict__ perm, u64 n_rec, u64* out) {
    for (u64 i = grid_tid(); i < n_rec; i += grid_stride()) out[i] = key_pair[clamp_u64(perm[i], n_rec - 1)];
}
// one thread per (cell, organelle) run: the ratios added one after another from the first record of the run on
__global__ __launch_bounds__(256) void k_map_sum(const u64* __restrict__ skey, const u32* __restrict__ perm, const u32* __restrict__ head,
                                                 const u32* __restrict__ seg, const double* __restrict__ ratio, u64 n_rec, const u64* __restrict__ org_ids,
                                                 const long long* __restrict__ org_sizes, u64 n_org, double lower, double upper, double size_thresh,
                                                 u64* pair_key, u64* pair_org, double* pair_ratio, uint8_t* pair_acc, u32* acc_flag, u32* org_n,
                                                 u32* org_first, u64* counts) {
    for (u64 i = grid_tid(); i < n_rec; i += grid_stride()) {
        const u64 k = skey[i];
        if (k >= NO_PAIR) {
            if (i == 0 || skey[i - 1] < NO_PAIR) { counts[0] = i; counts[1] = i ? seg[i - 1] : 0; }
            continue;
        }
        if (i == n_rec - 1) { counts[0] = n_rec; counts[1] = seg[i]; }
        if (!head[i]) continue;
        double sum = 0.0;
        for (u64 t = i; t < n_rec && skey[t] == k; ++t) sum += ratio[clamp_u64(perm[t], n_rec - 1)];
        const u64 p = clamp_u64((u64)seg[i] - 1, n_rec - 1), o = clamp_u64(k & ORG_MASK, n_org - 1), c = k >> CELL_SHIFT;
        const bool acc = sum > lower && (upper >= 1.0 || sum <= upper) && (double)org_sizes[o] > size_thresh;
        pair_key[p] = k;
        pair_org[p] = org_ids[o];
        pair_ratio[p] = sum;
        pair_acc[p] = acc ? 1 : 0;
        acc_flag[p] = acc ? 1u : 0u;
        if (acc) { atomicAdd(&org_n[o], 1u); atomicMin(&org_first[o], (u32)c); }
    }
}
__global__ __launch_bounds__(256) void k_map_out(const u64* __restrict__ pair_key, const u64* __restrict__ pair_org, const u32* __restrict__ acc_flag,
                                                 const u32* __restrict__ acc_pos, u64 n_rec, u64 n_cells, u64* cell_begin, u64* acc_begin, u64* acc_org,
                                                 u64* counts) {
    const u64 n_pairs = clamp_u64(counts[1], n_rec);
    for (u64 p = grid_tid(); p < n_rec; p += grid_stride()) {
        if (p < n_pairs && acc_flag[p]) acc_org[clamp_u64((u64)acc_pos[p] - 1, n_rec - 1)] = pair_org[p];
        if (p == n_rec - 1) counts[2] = acc_pos[p];
    }
    for (u64 c = grid_tid(); c <= n_cells; c += grid_stride()) {
        const u64 b = lower_bound(pair_key, n_pairs, c << CELL_SHIFT);
        cell_begin[c] = b;
        acc_begin[c] = b ? acc_pos[b - 1] : 0;
    }
}

// ---- synapses ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_syn_keys(const u64* __restrict__ partners, const uint8_t* __restrict__ keep, u64 n_syn,
                                                  const u64* __restrict__ ssv_ids, u64 n_cells, u64* key) {
    for (u64 h = grid_tid(); h < 2 * n_syn; h += grid_stride()) {
        const u64 slot = h >= n_syn ? 1 : 0, i = h - slot * n_syn;
        const long row = keep[i] ? find_exact(ssv_ids, n_cells, partners[2 * i + slot]) : -1;
        key[h] = row >= 0 ? (u64)row : n_cells;
    }
}
__global__ __launch_bounds__(256) void k_syn_out(const u64* __restrict__ skey, const u32* __restrict__ perm, const u64* __restrict__ syn_ids, u64 n_syn,
                                                 u64 n_cells, u64* syn_begin, u64* out_ids, u64* counts) {
    for (u64 k = grid_tid(); k < 2 * n_syn; k += grid_stride()) {
        if (skey[k] >= n_cells) continue;
        const u64 h = clamp_u64(perm[k], 2 * n_syn - 1);
        out_ids[k] = syn_ids[h >= n_syn ? h - n_syn : h];
    }
    for (u64 c = grid_tid(); c <= n_cells; c += grid_stride()) {
        const u64 b = lower_bound(skey, 2 * n_syn, c);
        syn_begin[c] = b;
        if (c == n_cells) counts[0] = b;
    }
}

// ---- scratch ----------------------------------------------------------------------------------------------------------------------
struct CompScratch { u64 *key, *skey, *cvox; u32 *i0, *perm, *head, *seg, *parent, *root, *keep, *eflag, *epos; int* cbox; double* csize; PrimScratch prim; };
size_t layout(CompScratch& w, void* base, size_t m, size_t n_edges) {
    ScratchAlloc a(base);
    a.take_into(m, w.key, w.skey, w.cvox);
    a.take_into(m, w.i0, w.perm, w.head, w.seg, w.parent, w.root, w.keep);
    a.take_into(6 * m, w.cbox);
    a.take_into(m, w.csize);
    a.take_into(std::max<size_t>(n_edges, 1), w.eflag, w.epos);
    w.prim = take_prim(a, std::max(m, n_edges));
    return a.used;
}
struct MapScratch { u64 *lsv, *ka, *kb, *kc; u32 *li0, *lperm, *i0, *pa, *pb, *head, *seg, *aflag, *apos; double* ratio; PrimScratch prim; };
size_t layout(MapScratch& w, void* base, size_t n_rec, size_t n_sv) {
    ScratchAlloc a(base);
    a.take_into(std::max<size_t>(n_sv, 1), w.lsv);
    a.take_into(std::max<size_t>(n_sv, 1), w.li0, w.lperm);
    a.take_into(n_rec, w.ka, w.kb, w.kc);
    a.take_into(n_rec, w.i0, w.pa, w.pb, w.head, w.seg, w.aflag, w.apos);
    a.take_into(n_rec, w.ratio);
    w.prim = take_prim(a, std::max<size_t>(std::max(n_rec, n_sv), 1));
    return a.used;
}
struct SynScratch { u64 *key, *skey; u32 *i0, *perm; PrimScratch prim; };
size_t layout(SynScratch& w, void* base, size_t n_half) {
    ScratchAlloc a(base);
    a.take_into(n_half, w.key, w.skey);
    a.take_into(n_half, w.i0, w.perm);
    w.prim = take_prim(a, n_half);
    return a.used;
}

}  // namespace

extern "C" {

size_t sd_svgraph_components_temp_bytes(size_t n_ids, size_t n_edges) {
    CompScratch w;
    return layout(w, nullptr, std::max<size_t>(n_ids + 2 * n_edges, 1), n_edges);
}

int sd_svgraph_components(const uint64_t* edges_dev, size_t n_edges, const uint64_t* ids_dev, const int64_t* sizes_dev, const uint64_t* box_begin_dev,
                          const int32_t* boxes_dev, size_t n_ids, size_t n_boxes, const double* scaling_xyz, double min_cc_size, int strict,
                          uint64_t* node_ids_dev, uint64_t* node_comp_dev, double* node_size_dev, uint64_t* ssv_ids_dev, uint64_t* sv_begin_dev,
                          uint64_t* sv_ids_dev, uint64_t* edges_out_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_svgraph_components";
    if (!counts_dev || !sv_begin_dev) return fail(who, ": null counts or sv_begin");
    if (n_ids >= LIM31 || n_edges >= LIM31 / 2 || n_ids + 2 * n_edges >= LIM31 || n_boxes >= LIM31) return fail(who, ": ids + endpoints and boxes < 2^31 per call");
    if (!scaling_xyz || !(scaling_xyz[0] > 0.0) || !(scaling_xyz[1] > 0.0) || !(scaling_xyz[2] > 0.0)) return fail(who, ": scaling must be positive");
    if (min_cc_size != min_cc_size) return fail(who, ": min_cc_size is NaN");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (hipMemsetAsync(sv_begin_dev, 0, sizeof(u64), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    const size_t m = n_ids + 2 * n_edges;
    if (m == 0) return SD_OK;
    if ((n_ids && (!ids_dev || !sizes_dev || !box_begin_dev || (n_boxes && !boxes_dev))) || (n_edges && (!edges_dev || !edges_out_dev)) || !node_ids_dev ||
        !node_comp_dev || !node_size_dev || !ssv_ids_dev || !sv_ids_dev)
        return fail(who, ": bad argument");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_svgraph_components_temp_bytes(n_ids, n_edges), "sd_svgraph_components_temp_bytes(n_ids, n_edges)"); rc != SD_OK)
        return rc;
    CompScratch w;
    layout(w, temp_dev, m, n_edges);
    const u64 M = m, E = n_edges, I = n_ids, B = n_boxes;
    const u64 *edges = reinterpret_cast<const u64*>(edges_dev), *ids = reinterpret_cast<const u64*>(ids_dev), *bb = reinterpret_cast<const u64*>(box_begin_dev);
    const long long* sizes = reinterpret_cast<const long long*>(sizes_dev);
    u64 *node_ids = reinterpret_cast<u64*>(node_ids_dev), *node_comp = reinterpret_cast<u64*>(node_comp_dev), *ssv_ids = reinterpret_cast<u64*>(ssv_ids_dev),
        *sv_begin = reinterpret_cast<u64*>(sv_begin_dev), *sv_ids = reinterpret_cast<u64*>(sv_ids_dev), *edges_out = reinterpret_cast<u64*>(edges_out_dev);
    if (I) {
        launch_1d(k_check_ascending, I, GRID, s, ids, I, counts);
        launch_1d(k_check_offsets, I, GRID, s, bb, I, B, counts);
    }
    launch_1d(k_cc_universe, M, GRID, s, ids, I, edges, M, w.key);
    if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, m, 64, s); rc != SD_OK) return rc;
    if (int rc = number_segments(who, w.prim, w.skey, nullptr, w.head, w.seg, m, s); rc != SD_OK) return rc;
    launch_1d(k_cc_rows, M, GRID, s, w.skey, w.head, w.seg, M, node_ids, counts);
    launch_1d(k_iota, M, GRID, s, w.parent, M);
    if (E) launch_1d(k_cc_union, E, GRID, s, edges, E, node_ids, M, w.parent, counts);
    launch_1d(k_cc_roots, M, GRID, s, w.parent, M, w.root, w.cbox, w.cvox, counts);
    if (I) launch_1d(k_cc_boxes, I, GRID, s, ids, sizes, bb, boxes_dev, I, B, node_ids, w.root, M, w.cbox, w.cvox, counts);
    launch_1d(k_cc_sizes, M, GRID, s, w.root, w.cbox, w.cvox, node_ids, M, scaling_xyz[0], scaling_xyz[1], scaling_xyz[2], min_cc_size, strict, w.csize, w.keep, counts);
    launch_1d(k_cc_nodes, M, GRID, s, w.root, w.keep, w.csize, node_ids, M, node_comp, node_size_dev, w.key, counts);
    if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, m, bits_for(M + 1), s); rc != SD_OK) return rc;
    if (int rc = number_segments(who, w.prim, w.skey, nullptr, w.head, w.seg, m, s); rc != SD_OK) return rc;
    launch_1d(k_cc_csr, M, GRID, s, w.skey, w.perm, w.head, w.seg, node_ids, M, ssv_ids, sv_begin, sv_ids, counts);
    if (E) {
        launch_1d(k_cc_edge_flags, E, GRID, s, edges, E, node_ids, w.root, w.keep, M, w.eflag, counts);
        if (int rc = scan_u32(who, w.prim, w.eflag, w.epos, n_edges, s); rc != SD_OK) return rc;
        launch_1d(k_cc_edges_out, E, GRID, s, edges, E, w.eflag, w.epos, edges_out, counts);
    }
    return launch_status("sd_svgraph_components: launch failed");
}

int sd_cell_props(const uint64_t* sv_begin_dev, const uint64_t* sv_ids_dev, size_t n_cells, size_t n_sv, const uint64_t* ids_dev, const int64_t* sizes_dev,
                  const int32_t* rep_coords_dev, const uint64_t* box_begin_dev, const int32_t* boxes_dev, size_t n_ids, size_t n_boxes,
                  int64_t* cell_size_dev, int32_t* cell_box_dev, int32_t* cell_rep_dev, uint64_t* counts_dev, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_cell_props";
    if (!counts_dev) return fail(who, ": null counts");
    if (n_cells >= LIM31 || n_sv >= LIM31 || n_ids >= LIM31 || n_boxes >= LIM31) return fail(who, ": cells, supervoxels, ids and boxes < 2^31 per call");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (n_cells == 0) return n_sv ? fail(who, ": supervoxels without cells") : SD_OK;
    if (!sv_begin_dev || (n_sv && !sv_ids_dev) || (n_ids && (!ids_dev || !sizes_dev || !rep_coords_dev || !box_begin_dev || (n_boxes && !boxes_dev))) ||
        !cell_size_dev || !cell_box_dev || !cell_rep_dev)
        return fail(who, ": bad argument");
    const u64 Cn = n_cells, S = n_sv, I = n_ids, B = n_boxes;
    const u64 *sv_begin = reinterpret_cast<const u64*>(sv_begin_dev), *sv_ids = reinterpret_cast<const u64*>(sv_ids_dev),
              *ids = reinterpret_cast<const u64*>(ids_dev), *bb = reinterpret_cast<const u64*>(box_begin_dev);
    const long long* sizes = reinterpret_cast<const long long*>(sizes_dev);
    long long* cell_size = reinterpret_cast<long long*>(cell_size_dev);
    launch_1d(k_check_offsets, Cn, GRID, s, sv_begin, Cn, S, counts);
    if (I) {
        launch_1d(k_check_ascending, I, GRID, s, ids, I, counts);
        launch_1d(k_check_offsets, I, GRID, s, bb, I, B, counts);
    }
    launch_1d(k_props_init, Cn, GRID, s, sv_begin, sv_ids, Cn, S, ids, rep_coords_dev, I, cell_size, cell_box_dev, cell_rep_dev);
    if (S) launch_1d(k_props_sv, S, GRID, s, sv_begin, sv_ids, Cn, S, ids, sizes, bb, boxes_dev, I, B, cell_size, cell_box_dev, counts);
    launch_1d(k_props_finish, Cn, GRID, s, Cn, cell_box_dev);
    return launch_status("sd_cell_props: launch failed");
}

size_t sd_cell_mapping_temp_bytes(size_t n_records, size_t n_sv) {
    MapScratch w;
    return layout(w, nullptr, std::max<size_t>(n_records, 1), n_sv);
}

int sd_cell_mapping(const uint64_t* rec_sub_dev, const uint64_t* rec_sv_dev, const int64_t* rec_count_dev, size_t n_records, const uint64_t* org_ids_dev,
                    const int64_t* org_sizes_dev, size_t n_org, const uint64_t* sv_begin_dev, const uint64_t* sv_ids_dev, size_t n_cells, size_t n_sv,
                    double lower_ratio, double upper_ratio, double size_threshold, uint64_t* cell_begin_dev, uint64_t* pair_org_dev,
                    double* pair_ratio_dev, uint8_t* pair_accepted_dev, uint64_t* acc_begin_dev, uint64_t* acc_org_dev, uint32_t* org_n_cells_dev,
                    uint32_t* org_first_cell_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_cell_mapping";
    if (!counts_dev) return fail(who, ": null counts");
    if (n_records >= LIM31 || n_org >= LIM31 || n_cells >= LIM31 || n_sv >= LIM31) return fail(who, ": records, organelles, cells and supervoxels < 2^31 per call");
    if (lower_ratio != lower_ratio || upper_ratio != upper_ratio || size_threshold != size_threshold) return fail(who, ": a threshold is NaN");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (n_cells == 0 && n_sv) return fail(who, ": supervoxels without cells");
    if (!cell_begin_dev || !acc_begin_dev || (n_org && (!org_ids_dev || !org_sizes_dev || !org_n_cells_dev || !org_first_cell_dev)) ||
        (n_cells && !sv_begin_dev) || (n_sv && !sv_ids_dev))
        return fail(who, ": bad argument");
    if (hipMemsetAsync(cell_begin_dev, 0, (n_cells + 1) * sizeof(u64), s) != hipSuccess || hipMemsetAsync(acc_begin_dev, 0, (n_cells + 1) * sizeof(u64), s) != hipSuccess ||
        (n_org && (hipMemsetAsync(org_n_cells_dev, 0, n_org * sizeof(u32), s) != hipSuccess ||
                   hipMemsetAsync(org_first_cell_dev, 0xff, n_org * sizeof(u32), s) != hipSuccess)))
        return sd_fail_msg(SD_ERR_HIP, "memset failed");
    const u64 R = n_records, O = n_org, Cn = n_cells, S = n_sv;
    const u64 *org_ids = reinterpret_cast<const u64*>(org_ids_dev), *sv_begin = reinterpret_cast<const u64*>(sv_begin_dev),
              *sv_ids = reinterpret_cast<const u64*>(sv_ids_dev);
    const long long* org_sizes = reinterpret_cast<const long long*>(org_sizes_dev);
    if (Cn) launch_1d(k_check_offsets, Cn, GRID, s, sv_begin, Cn, S, counts);
    if (O) launch_1d(k_check_ascending, O, GRID, s, org_ids, O, counts);
    if (R || S)
        if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_cell_mapping_temp_bytes(n_records, n_sv), "sd_cell_mapping_temp_bytes(n_records, n_sv)"); rc != SD_OK) return rc;
    MapScratch w;
    layout(w, temp_dev, std::max<size_t>(n_records, 1), n_sv);
    if (S) {                                                                     // checked even without records: a supervoxel in two cells
        if (int rc = sort_by_key(who, w.prim, sv_ids, w.lsv, w.li0, w.lperm, n_sv, 64, s); rc != SD_OK) return rc;
        launch_1d(k_map_lookup_check, S, GRID, s, w.lsv, S, counts);
    }
    if (R == 0) return launch_status("sd_cell_mapping: launch failed");
    if (!rec_sub_dev || !rec_sv_dev || !rec_count_dev || !pair_org_dev || !pair_ratio_dev || !pair_accepted_dev || !acc_org_dev)
        return fail(who, ": bad argument");
    launch_1d(k_map_records, R, GRID, s, reinterpret_cast<const u64*>(rec_sub_dev), reinterpret_cast<const u64*>(rec_sv_dev),
              reinterpret_cast<const long long*>(rec_count_dev), R, org_ids, org_sizes, O, w.lsv, w.lperm, sv_begin, Cn, S, w.ka, w.kb, w.ratio);
    if (int rc = sort_by_key(who, w.prim, w.ka, w.kc, w.i0, w.pa, n_records, std::max(1, bits_for(S + 1)), s); rc != SD_OK) return rc;
    launch_1d(k_map_gather, R, GRID, s, w.kb, w.pa, R, w.ka);
    if (int rc = sort_carry(who, w.prim, w.ka, w.kc, w.pa, w.pb, n_records, 63, s); rc != SD_OK) return rc;
    if (int rc = number_segments(who, w.prim, w.kc, nullptr, w.head, w.seg, n_records, s); rc != SD_OK) return rc;
    if (hipMemsetAsync(w.aflag, 0, n_records * sizeof(u32), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    launch_1d(k_map_sum, R, GRID, s, w.kc, w.pb, w.head, w.seg, w.ratio, R, org_ids, org_sizes, O, lower_ratio, upper_ratio, size_threshold, w.kb,
              reinterpret_cast<u64*>(pair_org_dev), pair_ratio_dev, pair_accepted_dev, w.aflag, org_n_cells_dev, org_first_cell_dev, counts);
    if (int rc = scan_u32(who, w.prim, w.aflag, w.apos, n_records, s); rc != SD_OK) return rc;
    launch_1d(k_map_out, std::max<u64>(R, Cn + 1), GRID, s, w.kb, reinterpret_cast<const u64*>(pair_org_dev), w.aflag, w.apos, R, Cn,
              reinterpret_cast<u64*>(cell_begin_dev), reinterpret_cast<u64*>(acc_begin_dev), reinterpret_cast<u64*>(acc_org_dev), counts);
    return launch_status("sd_cell_mapping: launch failed");
}

size_t sd_cell_synapses_temp_bytes(size_t n_syn) {
    SynScratch w;
    return layout(w, nullptr, std::max<size_t>(2 * n_syn, 1));
}

int sd_cell_synapses(const uint64_t* partners_dev, const uint8_t* keep_dev, const uint64_t* syn_ids_dev, size_t n_syn, const uint64_t* ssv_ids_dev,
                     size_t n_cells, uint64_t* syn_begin_dev, uint64_t* out_ids_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_cell_synapses";
    if (!counts_dev || !syn_begin_dev) return fail(who, ": null counts or syn_begin");
    if (n_syn >= LIM31 / 2 || n_cells >= LIM31) return fail(who, ": cells and half records < 2^31 per call");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (hipMemsetAsync(syn_begin_dev, 0, (n_cells + 1) * sizeof(u64), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    if (n_cells && !ssv_ids_dev) return fail(who, ": bad argument");
    const u64 N = n_syn, Cn = n_cells;
    const u64* ssv_ids = reinterpret_cast<const u64*>(ssv_ids_dev);
    if (Cn) launch_1d(k_check_ascending, Cn, GRID, s, ssv_ids, Cn, counts);
    if (N == 0) return launch_status("sd_cell_synapses: launch failed");
    if (!partners_dev || !keep_dev || !syn_ids_dev || !out_ids_dev) return fail(who, ": bad argument");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_cell_synapses_temp_bytes(n_syn), "sd_cell_synapses_temp_bytes(n_syn)"); rc != SD_OK) return rc;
    SynScratch w;
    layout(w, temp_dev, 2 * n_syn);
    launch_1d(k_syn_keys, 2 * N, GRID, s, reinterpret_cast<const u64*>(partners_dev), keep_dev, N, ssv_ids, Cn, w.key);
    if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, 2 * n_syn, std::max(1, bits_for(Cn + 1)), s); rc != SD_OK) return rc;
    launch_1d(k_syn_out, std::max<u64>(2 * N, Cn + 1), GRID, s, w.skey, w.perm, reinterpret_cast<const u64*>(syn_ids_dev), N, Cn,
              reinterpret_cast<u64*>(syn_begin_dev), reinterpret_cast<u64*>(out_ids_dev), counts);
    return launch_status("sd_cell_synapses: launch failed");
}

}  // extern "C"
