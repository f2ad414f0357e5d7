// Properties of the partner cells at every cell-level synapse, and the synapse classifier: the array form of what the reference's
// extraction/cs_processing_steps.py does per cell and per synapse in Python -- _collect_properties_from_ssv_partners_thread (:109-174:
// per cell one cKDTree over the mesh vertices, k = 50 with a Counter vote (reps/rep_helper.py:281-334), and one over the skeleton
// nodes, k = 1 (reps/super_segmentation_object.py:2923-3003)) and _classify_synssv_objects_thread (:1129-1161: one
// rfc.predict_proba([feats]) per synapse).
//
//   knn      segmented k nearest neighbours with vote.  Cell c owns points[begin[c] : begin[c + 1]]; a query is (cell row, float64
//            coordinate).  The neighbours of a query are the min(k, points of the cell) points of ITS cell with the smallest
//            (d^2, original index), d^2 = ((dx dx) + dy dy) + dz dz in float64 with nothing fused; the vote is the label with the
//            highest count among them, on equal counts the one whose first occurrence is nearest (Counter.most_common(1)).
//     build  one wave per cell: the cell's box.  The tile index of sd_pointtiles.h with the cells as segments and, per point, the
//            30-bit Morton code of its position inside the cell's box as the spatial key.
//     query  one wave per query.  Lane i holds entry i of the candidate list, ascending by (d^2, index); the k-th best is lane k - 1.
//            The list is seeded from the tile whose box is nearest; then the lanes test 64 tile boxes at a time, and a tile is
//            skipped when its box distance^2 (box_dist2: never above the d^2 of a point inside) is strictly above the k-th best (a
//            tie on d^2 is still decided by the index).  (d^2, index) is a total order: the result depends neither on the tiling nor
//            on the visit order.
//   forest   one thread per row: the row cast to float32, in every tree left iff x[feature] <= threshold (the float32 widened to
//            float64), the leaf's class fractions added in tree order in float64, divided by the number of trees: sklearn's
//            predict_proba with n_jobs = 1.
//
// Every index read from device memory is clamped before it is used; counts[7] != 0 says that one was out of range.  No scalar memory
// writes, no inline assembly.
#include "../../include/syconn_dense.h"
#include "sd_sortseg.h"
#include "sd_pointtiles.h"

namespace {

constexpr int KNN_BITS = 10;                                 // key bits per axis
constexpr u32 NO_IX = 0xffffffffu;
static_assert(SD_SYN_PROPS_MAX_K == 64 && TILE == 64, "one list entry and one point of a tile per lane");

__device__ __forceinline__ double ld_coord(const void* pts, int f32, u64 i) {
    return f32 ? (double)reinterpret_cast<const float*>(pts)[i] : reinterpret_cast<const double*>(pts)[i];
}
__device__ __forceinline__ u64 spread3(u32 v) {              // bit i of v -> bit 3 i
    u64 r = 0;
#pragma unroll
    for (int i = 0; i < KNN_BITS; ++i) r |= (u64)((v >> i) & 1u) << (3 * i);
    return r;
}

// ---- build ------------------------------------------------------------------------------------------------------------------------
// one wave per cell: offsets checked, cbox[c] = the smallest coordinates and the factor that maps the longest extent to 2^KNN_BITS
__global__ __launch_bounds__(256) void k_knn_cell_box(const void* __restrict__ pts, int f32, const u64* __restrict__ begin, u64 n_cells, u64 n_pts,
                                                      double* cbox, u64* counts) {
    const int lane = threadIdx.x & 63;
    const u64 wave = grid_tid() >> 6, n_waves = grid_stride() >> 6;
    for (u64 c = wave; c < n_cells; c += n_waves) {
        const u64 b0 = begin[c], b1 = begin[c + 1];
        const bool bad = b1 < b0 || b1 > n_pts || (c == 0 && b0 != 0) || (c == n_cells - 1 && b1 != n_pts);
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        if (!bad)
            for (u64 i = b0 + lane; i < b1; i += 64)
#pragma unroll
                for (int a = 0; a < 3; ++a) { const double v = ld_coord(pts, f32, 3 * i + a); lo[a] = fmin(lo[a], v); hi[a] = fmax(hi[a], v); }
        wave_minmax3(lo, hi);
        if (lane == 0) {
            if (bad) counts[7] = 1;
            const double ext = fmax(hi[0] - lo[0], fmax(hi[1] - lo[1], hi[2] - lo[2]));
#pragma unroll
            for (int a = 0; a < 3; ++a) cbox[4 * c + a] = lo[a];
            cbox[4 * c + 3] = (ext > 0.0 && ext < INFINITY) ? (double)(1 << KNN_BITS) / ext : 0.0;
        }
    }
}
__global__ __launch_bounds__(256) void k_knn_keys(const void* __restrict__ pts, int f32, const u64* __restrict__ begin, const double* __restrict__ cbox,
                                                  u64 n_cells, u64 n_pts, u64* key) {
    for (u64 j = grid_tid(); j < n_pts; j += grid_stride()) {
        const u64 c = segment_of(begin, n_cells, j);
        const double g = cbox[4 * c + 3];
        u64 k = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double f = (ld_coord(pts, f32, 3 * j + a) - cbox[4 * c + a]) * g;
            const u32 v = f > 0.0 ? (f < (double)((1 << KNN_BITS) - 1) ? (u32)f : (u32)((1 << KNN_BITS) - 1)) : 0u;      // NaN -> 0
            k |= spread3(v) << a;
        }
        key[j] = (c << (3 * KNN_BITS)) | k;
    }
}
__global__ __launch_bounds__(256) void k_knn_place(const void* __restrict__ pts, int f32, const u32* __restrict__ perm, u64 n_pts, double* spts) {
    for (u64 i = grid_tid(); i < n_pts; i += grid_stride()) {
        u64 j = perm[i];
        if (j >= n_pts) j = n_pts - 1;
#pragma unroll
        for (int a = 0; a < 3; ++a) spts[3 * i + a] = ld_coord(pts, f32, 3 * j + a);                    // float32 widens exactly
    }
}

// ---- query ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool before(double d, u32 ix, double kd, u32 ki) { return d < kd || (d == kd && ix < ki); }

// the points of one tile (sorted rows t0 .. t0 + 63 below i1) against the list: the ones before the k-th best are inserted one by one
__device__ __forceinline__ void knn_visit(const double* __restrict__ spts, const u32* __restrict__ perm, u64 t0, u64 i1, const double* qp, int k,
                                          int lane, double& e_d2, u32& e_ix) {
    const u64 i = t0 + lane;
    double d = INFINITY;
    u32 ix = NO_IX;
    if (i < i1) {
        const double p[3] = {spts[3 * i], spts[3 * i + 1], spts[3 * i + 2]};
        d = sq_dist(p, qp);
        ix = perm[i];
    }
    const double kd0 = __shfl(e_d2, k - 1);                                      // read by all lanes, outside any lane-dependent branch
    const u32 ki0 = (u32)__shfl((int)e_ix, k - 1);
    u64 m = __ballot(i < i1 && before(d, ix, kd0, ki0));
    while (m) {                                                                  // m and all that follows is the same in every lane
        const int b = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const double cd = __shfl(d, b);
        const u32 ci = (u32)__shfl((int)ix, b);
        const double kd = __shfl(e_d2, k - 1);
        const u32 ki = (u32)__shfl((int)e_ix, k - 1);
        if (!before(cd, ci, kd, ki)) continue;                                   // the k-th best has moved since
        const int pos = __popcll(__ballot(before(e_d2, e_ix, cd, ci)));          // the list is ascending: these lanes are a prefix
        const double ud = __shfl_up(e_d2, 1);
        const u32 ui = (u32)__shfl_up((int)e_ix, 1);
        if (lane == pos) { e_d2 = cd; e_ix = ci; }
        else if (lane > pos) { e_d2 = ud; e_ix = ui; }
    }
}

__global__ __launch_bounds__(256) void k_knn_query(const double* __restrict__ spts, const u32* __restrict__ perm, const int* __restrict__ labels,
                                                   const u64* __restrict__ begin, u64 n_cells, u64 n_pts, const double* __restrict__ tbox, u64 n_slots,
                                                   const u32* __restrict__ q_cell, const double* __restrict__ q_xyz, u64 n_q, int k, int* vote,
                                                   int* nn_idx, double* nn_d2, u64* counts) {
    const int lane = threadIdx.x & 63;
    const u64 wave = grid_tid() >> 6, n_waves = grid_stride() >> 6;
    u64 n_visit = 0, n_skip = 0;
    bool bad = false;
    for (u64 q = wave; q < n_q; q += n_waves) {
        const u64 c = q_cell[q];
        double e_d2 = INFINITY;                                                  // entry `lane` of the list
        u32 e_ix = NO_IX;
        int keff = 0;
        if (c < n_cells) {
            const u64 i1 = begin[c + 1] < n_pts ? begin[c + 1] : n_pts, i0 = begin[c] < i1 ? begin[c] : i1;
            const u64 n = i1 - i0, n_tiles = (n + TILE - 1) / TILE, slot0 = tile_slot0(i0, c);
            keff = n < (u64)k ? (int)n : k;
            const double qp[3] = {q_xyz[3 * q], q_xyz[3 * q + 1], q_xyz[3 * q + 2]};
            // the tile with the nearest box seeds the list
            double bd = INFINITY;
            u64 bt = 0;
            for (u64 t = lane; t < n_tiles; t += 64) {
                const double d = box_dist2(qp, tile_box(tbox, n_slots, slot0, t));
                if (d < bd) { bd = d; bt = t; }
            }
            for (int msk = 32; msk; msk >>= 1) {
                const double od = __shfl_xor(bd, msk);
                const u64 ot = __shfl_xor(bt, msk);
                if (od < bd || (od == bd && ot < bt)) { bd = od; bt = ot; }
            }
            if (n_tiles) { knn_visit(spts, perm, i0 + bt * TILE, i1, qp, k, lane, e_d2, e_ix); ++n_visit; }
            for (u64 t0 = 0; t0 < n_tiles; t0 += 64) {
                const u64 t = t0 + lane;
                const bool live = t < n_tiles && t != bt;
                double d = INFINITY;
                if (live) d = box_dist2(qp, tile_box(tbox, n_slots, slot0, t));
                const double kth0 = __shfl(e_d2, k - 1);
                u64 m = __ballot(live && !(d > kth0));
                n_skip += (u64)__popcll(__ballot(live)) - (u64)__popcll(m);
                while (m) {
                    const int b = __ffsll((unsigned long long)m) - 1;
                    m &= m - 1;
                    const double db = __shfl(d, b), kth = __shfl(e_d2, k - 1);
                    if (db > kth) { ++n_skip; continue; }                          // strictly above the k-th best
                    knn_visit(spts, perm, i0 + (t0 + b) * TILE, i1, qp, k, lane, e_d2, e_ix);
                    ++n_visit;
                }
            }
        } else {
            bad = true;
        }
        // Counter(labels in list order).most_common(1): the highest count, then the earliest first occurrence
        const bool in = lane < keff;
        int lab = 0;
        if (in) {
            const u64 ix = e_ix < n_pts ? e_ix : n_pts - 1;
            if (e_ix >= n_pts) bad = true;
            lab = labels ? labels[ix] : (int)ix;
        }
        int cnt = 0, first = 64;
        for (int j = 0; j < keff; ++j) {
            const int lj = __shfl(lab, j);
            if (in && lj == lab) { ++cnt; if (first == 64) first = j; }
        }
        int best = in ? cnt * 64 + (63 - first) : -1;
        for (int msk = 32; msk; msk >>= 1) best = max(best, __shfl_xor(best, msk));
        const int win = __shfl(lab, best >= 0 ? 63 - (best & 63) : 0);
        if (lane == 0) vote[q] = keff ? win : -1;
        if (nn_idx && lane < k) nn_idx[q * (u64)k + lane] = in ? (int)e_ix : -1;
        if (nn_d2 && lane < k) nn_d2[q * (u64)k + lane] = in ? e_d2 : INFINITY;
    }
    if (lane == 0) {
        if (n_visit) atomicAdd(&counts[0], n_visit);
        if (n_skip) atomicAdd(&counts[1], n_skip);
    }
    if (bad) counts[7] = 1;
}

// ---- forest -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_forest(const double* __restrict__ rows, u64 n_rows, int n_feat, const int* __restrict__ feature,
                                                const double* __restrict__ thr, const int* __restrict__ left, const int* __restrict__ right,
                                                const double* __restrict__ proba, const int* __restrict__ tree_begin, int n_trees, int n_nodes,
                                                int n_classes, double* out, u64* counts) {
    bool bad = false;
    for (u64 r = grid_tid(); r < n_rows; r += grid_stride()) {
        double* o = out + r * (u64)n_classes;
        for (int c = 0; c < n_classes; ++c) o[c] = 0.0;
        for (int t = 0; t < n_trees; ++t) {
            int node = tree_begin[t];
            if (node < 0 || node >= n_nodes) { bad = true; node = 0; }
            for (;;) {
                const int l = left[node];
                if (l < 0) break;
                int f = feature[node];
                if (f < 0 || f >= n_feat) { bad = true; f = 0; }
                const double x = (double)(float)rows[r * (u64)n_feat + f];
                const int next = x <= thr[node] ? l : right[node];
                if (next <= node || next >= n_nodes) { bad = true; break; }        // children follow their parent: no cycle, no way out
                node = next;
            }
            for (int c = 0; c < n_classes; ++c) o[c] += proba[(u64)node * n_classes + c];
        }
        for (int c = 0; c < n_classes; ++c) o[c] /= (double)n_trees;
    }
    if (bad) counts[7] = 1;
}

// ---- scratch ----------------------------------------------------------------------------------------------------------------------
struct KnnScratch { double *spts, *tbox, *cbox; u64 *key, *skey; u32 *i0, *perm; size_t n_slots; PrimScratch prim; };
size_t layout(KnnScratch& w, void* base, size_t n_pts, size_t n_cells) {
    ScratchAlloc a(base);
    w.n_slots = tile_slots(n_pts, n_cells);
    a.take_into(3 * n_pts, w.spts);
    a.take_into(6 * w.n_slots, w.tbox);
    a.take_into(4 * n_cells, w.cbox);
    a.take_into(n_pts, w.key, w.skey);
    a.take_into(n_pts, w.i0, w.perm);
    w.prim = take_prim(a, n_pts);
    return a.used;
}

}  // namespace

extern "C" {

size_t sd_syn_props_knn_temp_bytes(size_t n_points, size_t n_cells) {
    KnnScratch w;
    return layout(w, nullptr, n_points ? n_points : 1, n_cells ? n_cells : 1);
}

int sd_syn_props_knn(const void* points_dev, int points_f32, const uint64_t* begin_dev, size_t n_cells, size_t n_points,
                     const int32_t* labels_dev, const uint32_t* q_cell_dev, const double* q_xyz_dev, size_t n_q, int k, int stages,
                     int32_t* vote_dev, int32_t* nn_idx_dev, double* nn_d2_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes,
                     void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_syn_props_knn";
    if (!counts_dev) return fail(who, ": null counts");
    if (k < 1 || k > SD_SYN_PROPS_MAX_K) return fail(who, ": 1 <= k <= 64");
    if (n_points >= LIM31 || n_q >= LIM31 || n_cells >= LIM31)
        return fail(who, ": points, queries and cells < 2^31 per call");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (n_cells == 0 || !(stages & 3)) {
        if (n_q) return fail(who, ": queries without cells");
        return SD_OK;
    }
    if (!begin_dev || (n_points && !points_dev)) return fail(who, ": bad argument");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_syn_props_knn_temp_bytes(n_points, n_cells), "sd_syn_props_knn_temp_bytes(n_points, n_cells)"); rc != SD_OK)
        return rc;
    KnnScratch w;
    layout(w, temp_dev, n_points ? n_points : 1, n_cells);
    const u64 N = n_points, Cn = n_cells, Q = n_q;
    const u64* begin = reinterpret_cast<const u64*>(begin_dev);
    const int f32 = points_f32 ? 1 : 0;
    if (stages & 1) {
        const int cbits = bits_for(Cn);
        launch_1d(k_knn_cell_box, 64 * Cn, SD_SYN_PROPS_CELL_GRID, s, points_dev, f32, begin, Cn, N, w.cbox, counts);
        if (N) {
            launch_1d(k_knn_keys, N, SD_SYN_PROPS_POINT_GRID, s, points_dev, f32, begin, w.cbox, Cn, N, w.key);
            if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, n_points, cbits + 3 * KNN_BITS, s); rc != SD_OK) return rc;
            launch_1d(k_knn_place, N, SD_SYN_PROPS_POINT_GRID, s, points_dev, f32, w.perm, N, w.spts);
            launch_1d(k_tile_boxes<false>, 64 * Cn, SD_SYN_PROPS_CELL_GRID, s, w.spts, begin, Cn, N, (u64)w.n_slots, w.tbox, (double*)nullptr);
        }
    }
    if ((stages & 2) && Q) {
        if (!q_cell_dev || !q_xyz_dev || !vote_dev) return fail(who, ": bad argument");
        launch_1d(k_knn_query, 64 * Q, SD_SYN_PROPS_QUERY_GRID, s, w.spts, w.perm, labels_dev, begin, Cn, N, w.tbox, (u64)w.n_slots, q_cell_dev,
                  q_xyz_dev, Q, k, vote_dev, nn_idx_dev, nn_d2_dev, counts);
    }
    return launch_status("sd_syn_props_knn: launch failed");
}

int sd_syn_props_forest(const double* rows_dev, size_t n_rows, int n_features, const int32_t* feature_dev, const double* threshold_dev,
                        const int32_t* left_dev, const int32_t* right_dev, const double* proba_dev, const int32_t* tree_begin_dev, int n_trees,
                        int n_nodes, int n_classes, double* out_dev, uint64_t* counts_dev, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_syn_props_forest";
    if (!counts_dev) return fail(who, ": null counts");
    if (n_features < 1 || n_trees < 1 || n_nodes < n_trees || n_classes < 1 || n_rows >= LIM31)
        return fail(who, ": features, trees, classes >= 1, a node per tree, rows < 2^31");
    if (int rc = zero_counts(counts_dev, 8, s); rc != SD_OK) return rc;
    if (n_rows == 0) return SD_OK;
    if (!rows_dev || !feature_dev || !threshold_dev || !left_dev || !right_dev || !proba_dev || !tree_begin_dev || !out_dev)
        return fail(who, ": bad argument");
    launch_1d(k_forest, n_rows, SD_SYN_PROPS_FOREST_GRID, s, rows_dev, (u64)n_rows, n_features, feature_dev, threshold_dev, left_dev, right_dev,
              proba_dev, tree_begin_dev, n_trees, n_nodes, n_classes, out_dev, reinterpret_cast<u64*>(counts_dev));
    return launch_status("sd_syn_props_forest: launch failed");
}

}  // extern "C"
