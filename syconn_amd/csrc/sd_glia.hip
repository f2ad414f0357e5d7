// Astrocyte splitting of the supervoxel graph, all cells of a dataset in one launch set: the array form of what the reference does cell by
// cell in Python over networkx -- proc/graphs.py remove_glia_nodes (:278-360) with create_ccsize_dict (:220-249) behind split_glia_graph
// (:173-195), proc/glia_splitting.py collect_glia_sv (:37-63) and write_astrocyte_svgraph (:77-161) -- and the supervoxel glia decision of
// reps/segmentation_helper.py glia_pred_so / glia_proba_so (:32-78) with reps/segmentation.py glia_pred (:799-814).
//
//   universe    the nodes = every edge endpoint and every extra node: one 64-bit sort, a head per distinct id, a scan; row r is the r-th
//               smallest id.  Every node finds its table row and both endpoints of every edge their node rows ONCE; all passes read those.
//   passes      four times the same three kernels over a per-node group number (edges unite two nodes of one group, nodes of the group
//               SKIP take no part): union (uf_union of sd_tables.h: the root of a set is its smallest row, so its smallest id), roots (every
//               node's root written before anything reads one), boxes (the box of every node to its root by integer atomicMin / atomicMax
//               over order-preserving 64-bit keys of the doubles).  The groups: (A) one for all: the cells; (B) the glia class: the
//               components of steps 1 and 2, whose "is significant" goes to the cell root by an atomicOr; (C) neuron or tiny glia fragment
//               of the cells that step 3 decides; (D) the final class: the output components.
//   sizes       sqrt(((dx dx) + dy dy) + dz dz) of d = max - min over BOTH corners of all boxes of a component, float64, every product and
//               sum rounded on its own, the root correctly rounded (extent_norm of sd_cell_assembly.hip, without a scaling: boxes are nm).
//   tables      the components of a class in CSR form are one stable sort of its nodes by root row: components ascending by their smallest
//               id, supervoxels ascending inside.  The split graphs are a flag, a scan and a scatter per class, in input order.
//
// The number of nodes is known only on the device: every kernel reads it from counts[0] and clamps it to the scratch.  Every index read from
// device memory is clamped or checked before it is used, every output write is guarded by the capacity given.  No float atomics, no scalar
// memory writes, no inline assembly.
#include "../../include/syconn_dense.h"
#include "sd_sortseg.h"
#include "sd_tables.h"

namespace {

constexpr int GRID = SD_GLIA_GRID;
constexpr u32 SKIP = 0xffffffffu;                            // group of a node that takes no part in a pass
constexpr u32 NO_ROW = 0xffffffffu;                          // a node that is not in the table
constexpr u64 KEY_MAX = ~0ull;
// counts slots
enum { C_NODES = 0, C_CELLS, C_NCC, C_NSV, C_GCC, C_GSV, C_NEDGES, C_BAD, C_GEDGES, C_GVOX, C_UNKNOWN, C_UNKNOWN_ID, C_LOST, C_OUT1, C_OUT2, C_OUT3, N_COUNTS };

// doubles <-> u64 keys with the same order (-0.0 below +0.0; NaN is the caller's to keep out)
__device__ __forceinline__ u64 key_of(double v) {
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : b | (1ull << 63);
}
__device__ __forceinline__ double value_of(u64 k) { return __longlong_as_double((long long)((k >> 63) ? k & ~(1ull << 63) : ~k)); }

// ---- universe ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gl_universe(const u64* __restrict__ edges, u64 n_ends, const u64* __restrict__ nodes, u64 m, u64* key, u64* counts) {
    for (u64 i = grid_tid(); i < m; i += grid_stride()) key[i] = i < n_ends ? edges[i] : nodes[i - n_ends];
    if (grid_tid() == 0) counts[C_UNKNOWN_ID] = KEY_MAX;                          // lowered by atomicMin, set to 0 at the end if nothing did
}
__global__ __launch_bounds__(256) void k_gl_rows(const u64* __restrict__ skey, const u32* __restrict__ head, const u32* __restrict__ seg, u64 m, u64 node_cap,
                                                 u64* nid, u64* counts) {
    for (u64 i = grid_tid(); i < m; i += grid_stride()) {
        if (head[i]) nid[clamp_u64((u64)seg[i] - 1, m - 1)] = skey[i];
        if (i == m - 1) {
            counts[C_NODES] = seg[i];
            if (seg[i] > node_cap) counts[C_LOST] = 1;
        }
    }
}
// per node: its table row, glia class, whether its ORIGINAL cell passes the size filter of write_astrocyte_svgraph (:125-127, :147-149)
__global__ __launch_bounds__(256) void k_gl_resolve(const u64* __restrict__ nid, u64 m, const u64* __restrict__ ids, const uint8_t* __restrict__ glia,
                                                    u64 n_ids, const double* __restrict__ cell_size, double min_cell_size, u32* row, u32* cls, u32* alive,
                                                    u32* grp, u32* cellflag, u64* counts) {
    const u64 n = clamp_u64(counts[C_NODES], m);
    for (u64 r = grid_tid(); r < n; r += grid_stride()) {
        const long t = find_exact(ids, n_ids, nid[r]);
        if (t < 0) { counts[C_UNKNOWN] = 1; atomicMin(&counts[C_UNKNOWN_ID], nid[r]); }
        row[r] = t < 0 ? NO_ROW : (u32)t;
        cls[r] = t >= 0 && glia[t] != 0 ? 1u : 0u;
        alive[r] = (t >= 0 && cell_size && cell_size[t] < min_cell_size) ? 0u : 1u;
        grp[r] = 0;                                                              // pass A: one group
        cellflag[r] = 0;
    }
}
__global__ __launch_bounds__(256) void k_gl_endpoints(const u64* __restrict__ edges, u64 n_edges, const u64* __restrict__ nid, u64 m, u32* ea, u32* eb,
                                                      const u64* counts) {
    const u64 n = clamp_u64(counts[C_NODES], m);
    for (u64 e = grid_tid(); e < n_edges; e += grid_stride()) {
        ea[e] = (u32)clamp_u64(lower_bound(nid, n, edges[2 * e]), n - 1);           // an endpoint is a node by construction
        eb[e] = (u32)clamp_u64(lower_bound(nid, n, edges[2 * e + 1]), n - 1);
    }
}

// ---- one pass ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gl_union(const u32* __restrict__ ea, const u32* __restrict__ eb, u64 n_edges, const u32* __restrict__ grp, u64 m,
                                                  u32* parent) {
    for (u64 e = grid_tid(); e < n_edges; e += grid_stride()) {
        const u32 a = (u32)clamp_u64(ea[e], m - 1), b = (u32)clamp_u64(eb[e], m - 1);
        const u32 g = grp[a];
        if (g == SKIP || g != grp[b] || a == b) continue;
        uf_union(parent, a, b);
    }
}
__global__ __launch_bounds__(256) void k_gl_roots(const u32* __restrict__ parent, u64 m, u32* root, u64* bk /* may be nullptr */, const u64* counts) {
    const u64 n = clamp_u64(counts[C_NODES], m);
    for (u64 r = grid_tid(); r < n; r += grid_stride()) {
        root[r] = uf_find(parent, (u32)r);
        if (bk)
            for (int a = 0; a < 3; ++a) { bk[6 * r + a] = KEY_MAX; bk[6 * r + 3 + a] = 0; }
    }
}
__global__ __launch_bounds__(256) void k_gl_boxes(const u32* __restrict__ row, const u32* __restrict__ grp, const u32* __restrict__ root,
                                                  const double* __restrict__ boxes, u64 n_ids, u64 m, u64* bk, const u64* counts) {
    const u64 n = clamp_u64(counts[C_NODES], m);
    for (u64 r = grid_tid(); r < n; r += grid_stride()) {
        const u64 t = row[r];
        if (grp[r] == SKIP || t >= n_ids) continue;
        const u64 rt = clamp_u64(root[r], n - 1);
        for (int a = 0; a < 3; ++a) {                                            // np.min / np.max over BOTH corners of every box
            const double lo = boxes[6 * t + a], hi = boxes[6 * t + 3 + a];
            atomicMin(&bk[6 * rt + a], key_of(lo < hi ? lo : hi));
            atomicMax(&bk[6 * rt + 3 + a], key_of(lo < hi ? hi : lo));
        }
    }
}
// np.linalg.norm(max - min) of the corners: ((dx dx) + dy dy) + dz dz and its square root; a root without any box (an unknown node) has 0
__device__ __forceinline__ double extent_norm(const u64* k) {
#pragma clang fp contract(off)
    if (k[0] > k[3]) return 0.0;
    const double dx = value_of(k[3]) - value_of(k[0]), dy = value_of(k[4]) - value_of(k[1]), dz = value_of(k[5]) - value_of(k[2]);
    return __builtin_sqrt(((dx * dx) + dy * dy) + dz * dz);
}
// sizes of the roots of a pass; where cellflag is given (pass B) a root with size > min_size marks its cell: bit 0 a neuron, bit 1 a glia one
__global__ __launch_bounds__(256) void k_gl_sizes(const u32* __restrict__ root, const u32* __restrict__ grp, const u64* __restrict__ bk, u64 m,
                                                  const u32* __restrict__ cls, const u32* __restrict__ cellroot, double min_size, double* csize,
                                                  u32* cellflag /* may be nullptr */, const u64* counts) {
    const u64 n = clamp_u64(counts[C_NODES], m);
    for (u64 r = grid_tid(); r < n; r += grid_stride()) {
        if (root[r] != r || grp[r] == SKIP) continue;
        const double size = extent_norm(bk + 6 * r);
        csize[r] = size;
        if (cellflag && size > min_size) atomicOr(&cellflag[clamp_u64(cellroot[r], n - 1)], cls[r] ? 2u : 1u);
    }
}
__device__ __forceinline__ int outcome_of(u32 flag) { return !(flag & 1u) ? 1 : (!(flag & 2u) ? 2 : 3); }

// after pass B: the size of steps 1 / 2 per node; the group of pass C = neuron or tiny glia fragment (size < min_size) of an outcome-3 cell
__global__ __launch_bounds__(256) void k_gl_classify(const u32* __restrict__ cls, const u32* __restrict__ root, const double* __restrict__ csize,
                                                     const u32* __restrict__ cellroot, const u32* __restrict__ cellflag, u64 m, double min_size, double* s1,
                                                     u32* grp, const u64* counts) {
    const u64 n = clamp_u64(counts[C_NODES], m);
    for (u64 r = grid_tid(); r < n; r += grid_stride()) {
        const double size = csize[clamp_u64(root[r], n - 1)];
        s1[r] = size;
        const bool three = outcome_of(cellflag[clamp_u64(cellroot[r], n - 1)]) == 3;
        grp[r] = three && (cls[r] == 0 || size < min_size) ? 0u : SKIP;
    }
}
// after pass C: the size of the neuron-or-tiny pass (NaN where the node took no part) and the final class, which is the group of pass D
__global__ __launch_bounds__(256) void k_gl_final(const u32* __restrict__ root, const double* __restrict__ csize, const u32* __restrict__ cellroot,
                                                  const u32* __restrict__ cellflag, u64 m, double min_size, double* s2, u32* grp, const u64* counts) {
    const u64 n = clamp_u64(counts[C_NODES], m);
    for (u64 r = grid_tid(); r < n; r += grid_stride()) {
        const bool part = grp[r] != SKIP;
        const double size = part ? csize[clamp_u64(root[r], n - 1)] : __builtin_nan("");
        const int oc = outcome_of(cellflag[clamp_u64(cellroot[r], n - 1)]);
        s2[r] = size;
        grp[r] = oc == 1 ? 1u : (oc == 2 ? 0u : (part && !(size < min_size) ? 0u : 1u));
    }
}

// ---- outputs -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gl_nodes_out(const u64* __restrict__ nid, const u32* __restrict__ row, const u32* __restrict__ cellroot,
                                                      const u32* __restrict__ fcls, const u32* __restrict__ root, const u32* __restrict__ alive,
                                                      const double* __restrict__ s1, const double* __restrict__ s2, const long long* __restrict__ sv_sizes,
                                                      u64 n_ids, u64 m, u64 cap, u64* node_ids, u64* node_cell, uint8_t* node_class, u64* node_comp,
                                                      double* node_size1, double* node_size2, u32* chead, u64* counts) {
    const u64 n = clamp_u64(counts[C_NODES], m);
    for (u64 r = grid_tid(); r < m; r += grid_stride()) {
        if (r >= n) { chead[r] = 0; continue; }
        chead[r] = cellroot[r] == r ? 1u : 0u;
        if (sv_sizes && fcls[r] == 1 && alive[r] && row[r] < n_ids) atomicAdd(&counts[C_GVOX], (u64)sv_sizes[row[r]]);
        if (r >= cap) continue;
        node_ids[r] = nid[r];
        node_cell[r] = nid[clamp_u64(cellroot[r], n - 1)];
        node_class[r] = (uint8_t)fcls[r];
        node_comp[r] = nid[clamp_u64(root[r], n - 1)];
        node_size1[r] = s1[r];
        node_size2[r] = s2[r];
    }
}
__global__ __launch_bounds__(256) void k_gl_cells_out(const u64* __restrict__ nid, const u32* __restrict__ chead, const u32* __restrict__ cpos,
                                                      const u32* __restrict__ cellflag, u64 m, u64 cap, u64* cell_ids, uint8_t* cell_outcome, u64* counts) {
    const u64 n = clamp_u64(counts[C_NODES], m);
    for (u64 r = grid_tid(); r < n; r += grid_stride()) {
        if (chead[r]) {
            const u64 c = (u64)cpos[r] - 1;
            const int oc = outcome_of(cellflag[r]);
            atomicAdd(&counts[C_OUT1 + oc - 1], 1ull);
            if (c < cap) { cell_ids[c] = nid[r]; cell_outcome[c] = (uint8_t)oc; }
        }
        if (r == n - 1) {
            counts[C_CELLS] = cpos[r];
            if (counts[C_UNKNOWN_ID] == KEY_MAX && !counts[C_UNKNOWN]) counts[C_UNKNOWN_ID] = 0;
        }
    }
}
// sort key of the component table of class c: the root row of the nodes that are in it, m for all others
__global__ __launch_bounds__(256) void k_gl_cc_keys(const u32* __restrict__ fcls, const u32* __restrict__ root, const u32* __restrict__ alive, u64 m, u32 c,
                                                    u64* key, const u64* counts) {
    const u64 n = clamp_u64(counts[C_NODES], m);
    for (u64 r = grid_tid(); r < m; r += grid_stride()) key[r] = (r < n && fcls[r] == c && alive[r]) ? clamp_u64(root[r], n - 1) : m;
}
// the nodes of a class sorted by root row: component numbers from the heads; the first other record (or the end) closes the table
__global__ __launch_bounds__(256) void k_gl_csr(const u64* __restrict__ skey, const u32* __restrict__ perm, const u32* __restrict__ head,
                                                const u32* __restrict__ seg, const u64* __restrict__ nid, const u32* __restrict__ cellroot, u64 m, u64 cap,
                                                u64* cc_ids, u64* cc_cell, u64* sv_begin, u64* sv_ids, u64* counts, int slot_cc, int slot_sv) {
    for (u64 i = grid_tid(); i < m; i += grid_stride()) {
        const u64 k = skey[i];
        if (k >= m) {
            if (i == 0 || skey[i - 1] < m) {
                const u64 ccs = i ? seg[i - 1] : 0;
                counts[slot_cc] = ccs;
                counts[slot_sv] = i;
                if (ccs <= cap) sv_begin[ccs] = i;
            }
            continue;
        }
        if (i < cap) sv_ids[i] = nid[clamp_u64(perm[i], m - 1)];
        const u64 c = clamp_u64((u64)seg[i] - 1, m - 1);
        if (head[i] && c < cap) { cc_ids[c] = nid[k]; cc_cell[c] = nid[clamp_u64(cellroot[k], m - 1)]; sv_begin[c] = i; }
        if (i == m - 1) {
            counts[slot_cc] = c + 1;
            counts[slot_sv] = m;
            if (c + 1 <= cap) sv_begin[c + 1] = m;
        }
    }
}
__global__ __launch_bounds__(256) void k_gl_edge_flags(const u32* __restrict__ ea, const u32* __restrict__ eb, u64 n_edges, const u32* __restrict__ fcls,
                                                       const u32* __restrict__ alive, u64 m, u32 c, u32* flag) {
    for (u64 e = grid_tid(); e < n_edges; e += grid_stride()) {
        const u64 a = clamp_u64(ea[e], m - 1), b = clamp_u64(eb[e], m - 1);
        flag[e] = (fcls[a] == c && fcls[b] == c && alive[a] && alive[b]) ? 1u : 0u;
    }
}
__global__ __launch_bounds__(256) void k_gl_edges_out(const u64* __restrict__ edges, u64 n_edges, const u32* __restrict__ flag, const u32* __restrict__ pos,
                                                      u64 cap, u64* edges_out, u64* counts, int slot) {
    for (u64 e = grid_tid(); e < n_edges; e += grid_stride()) {
        if (flag[e]) {
            const u64 o = (u64)pos[e] - 1;
            if (o < cap) { edges_out[2 * o] = edges[2 * e]; edges_out[2 * o + 1] = edges[2 * e + 1]; }
        }
        if (e == n_edges - 1) {
            counts[slot] = pos[e];
            if (pos[e] > cap) counts[C_LOST] = 1;
        }
    }
}

// ---- glia_pred_so / glia_proba_so: one thread per supervoxel ------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void k_gl_pred(const T* __restrict__ probas, const u64* __restrict__ view_begin, u64 n_sv, u64 n_views, double thresh,
                                                 int point_model, uint8_t* cls, double* mean) {
#pragma clang fp contract(off)
    for (u64 i = grid_tid(); i < n_sv; i += grid_stride()) {
        const u64 b1 = clamp_u64(view_begin[i + 1], n_views), b0 = clamp_u64(view_begin[i], b1);
        double sum = 0.0;
        long long votes = 0;
        for (u64 v = b0; v < b1; ++v) {
            const double p = (double)probas[v];
            sum += p;
            votes += p > thresh ? 1 : 0;
        }
        const double mu = b1 > b0 ? sum / (double)(b1 - b0) : __builtin_nan("");
        mean[i] = mu;
        const bool g = b1 > b0 && (point_model ? mu >= thresh : (mu > thresh && votes > (long long)((double)(b1 - b0) * 0.7)));
        cls[i] = g ? 1 : 0;
    }
}

// ---- scratch ----------------------------------------------------------------------------------------------------------------------
struct GliaScratch {
    u64 *key, *skey, *nid, *bk;
    double *csize, *s1, *s2;
    u32 *i0, *perm, *head, *seg, *row, *cls, *alive, *grp, *parent, *cellroot, *root, *cellflag, *ea, *eb, *eflag, *epos;
    PrimScratch prim;
};
size_t layout(GliaScratch& w, void* base, size_t m, size_t n_edges) {
    ScratchAlloc a(base);
    a.take_into(m, w.key, w.skey, w.nid);
    a.take_into(6 * m, w.bk);
    a.take_into(m, w.csize, w.s1, w.s2);
    a.take_into(m, w.i0, w.perm, w.head, w.seg, w.row, w.cls, w.alive, w.grp, w.parent, w.cellroot, w.root, w.cellflag);
    a.take_into(std::max<size_t>(n_edges, 1), w.ea, w.eb, w.eflag, w.epos);
    w.prim = take_prim(a, std::max(m, n_edges));
    return a.used;
}

}  // namespace

extern "C" {

size_t sd_glia_split_temp_bytes(size_t n_ids, size_t n_edges, size_t n_nodes) {
    (void)n_ids;
    GliaScratch w;
    return layout(w, nullptr, std::max<size_t>(2 * n_edges + n_nodes, 1), n_edges);
}

int sd_glia_split(const uint64_t* edges_dev, size_t n_edges, const uint64_t* nodes_dev, size_t n_nodes, const uint64_t* ids_dev, const double* boxes_dev,
                  const uint8_t* glia_dev, size_t n_ids, double min_size, const double* cell_size_dev, double min_cell_size, const int64_t* sv_sizes_dev,
                  size_t node_cap, size_t edge_cap, uint64_t* node_ids_dev, uint64_t* node_cell_dev, uint8_t* node_class_dev, uint64_t* node_comp_dev,
                  double* node_size1_dev, double* node_size2_dev, uint64_t* cell_ids_dev, uint8_t* cell_outcome_dev, uint64_t* ncc_ids_dev,
                  uint64_t* ncc_cell_dev, uint64_t* ncc_begin_dev, uint64_t* ncc_sv_dev, uint64_t* gcc_ids_dev, uint64_t* gcc_cell_dev,
                  uint64_t* gcc_begin_dev, uint64_t* gcc_sv_dev, uint64_t* neuron_edges_dev, uint64_t* astrocyte_edges_dev, uint64_t* counts_dev,
                  void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_glia_split";
    if (!counts_dev || !ncc_begin_dev || !gcc_begin_dev) return fail(who, ": null counts or component offsets");
    if (n_ids >= LIM31 || n_edges >= LIM31 / 2 || n_nodes >= LIM31 || 2 * n_edges + n_nodes >= LIM31) return fail(who, ": ids and endpoints + nodes < 2^31 per call");
    if (min_size != min_size || (cell_size_dev && min_cell_size != min_cell_size)) return fail(who, ": a threshold is NaN");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, N_COUNTS, s); rc != SD_OK) return rc;
    if (hipMemsetAsync(ncc_begin_dev, 0, sizeof(u64), s) != hipSuccess || hipMemsetAsync(gcc_begin_dev, 0, sizeof(u64), s) != hipSuccess)
        return sd_fail_msg(SD_ERR_HIP, "memset failed");
    const size_t m = 2 * n_edges + n_nodes;
    if (m == 0) return SD_OK;
    if ((n_ids && (!ids_dev || !boxes_dev || !glia_dev)) || (n_edges && !edges_dev) || (n_nodes && !nodes_dev) ||
        (edge_cap && (!neuron_edges_dev || !astrocyte_edges_dev)) ||
        (node_cap && (!node_ids_dev || !node_cell_dev || !node_class_dev || !node_comp_dev || !node_size1_dev || !node_size2_dev || !cell_ids_dev ||
                      !cell_outcome_dev || !ncc_ids_dev || !ncc_cell_dev || !ncc_sv_dev || !gcc_ids_dev || !gcc_cell_dev || !gcc_sv_dev)))
        return fail(who, ": bad argument");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_glia_split_temp_bytes(n_ids, n_edges, n_nodes), "sd_glia_split_temp_bytes(n_ids, n_edges, n_nodes)"); rc != SD_OK)
        return rc;
    GliaScratch w;
    layout(w, temp_dev, m, n_edges);
    const u64 M = m, E = n_edges, I = n_ids, NC = node_cap, EC = edge_cap;
    const u64 *edges = reinterpret_cast<const u64*>(edges_dev), *nodes = reinterpret_cast<const u64*>(nodes_dev), *ids = reinterpret_cast<const u64*>(ids_dev);
    if (I) launch_1d(k_check_ascending, I, GRID, s, ids, I, counts);
    // universe
    launch_1d(k_gl_universe, M, GRID, s, edges, 2 * E, nodes, M, w.key, counts);
    if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, m, 64, s); rc != SD_OK) return rc;
    if (int rc = number_segments(who, w.prim, w.skey, nullptr, w.head, w.seg, m, s); rc != SD_OK) return rc;
    launch_1d(k_gl_rows, M, GRID, s, w.skey, w.head, w.seg, M, NC, w.nid, counts);
    launch_1d(k_gl_resolve, M, GRID, s, w.nid, M, ids, glia_dev, I, cell_size_dev, min_cell_size, w.row, w.cls, w.alive, w.grp, w.cellflag, counts);
    if (E) launch_1d(k_gl_endpoints, E, GRID, s, edges, E, w.nid, M, w.ea, w.eb, counts);
    // the passes: groups in w.grp, roots to `root`, boxes of the roots to w.bk where `boxes` is set
    auto pass = [&](u32* root, bool boxes) {
        launch_1d(k_iota, M, GRID, s, w.parent, M);
        if (E) launch_1d(k_gl_union, E, GRID, s, w.ea, w.eb, E, w.grp, M, w.parent);
        launch_1d(k_gl_roots, M, GRID, s, w.parent, M, root, boxes ? w.bk : nullptr, counts);
        if (boxes) launch_1d(k_gl_boxes, M, GRID, s, w.row, w.grp, root, boxes_dev, I, M, w.bk, counts);
    };
    pass(w.cellroot, false);                                                     // A: the cells
    if (hipMemcpyAsync(w.grp, w.cls, m * sizeof(u32), hipMemcpyDeviceToDevice, s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "copy failed");
    pass(w.root, true);                                                          // B: components of one class (steps 1 and 2)
    launch_1d(k_gl_sizes, M, GRID, s, w.root, w.grp, w.bk, M, w.cls, w.cellroot, min_size, w.csize, w.cellflag, counts);
    launch_1d(k_gl_classify, M, GRID, s, w.cls, w.root, w.csize, w.cellroot, w.cellflag, M, min_size, w.s1, w.grp, counts);
    pass(w.root, true);                                                          // C: neurons and tiny glia fragments (step 3)
    launch_1d(k_gl_sizes, M, GRID, s, w.root, w.grp, w.bk, M, w.cls, w.cellroot, min_size, w.csize, (u32*)nullptr, counts);
    launch_1d(k_gl_final, M, GRID, s, w.root, w.csize, w.cellroot, w.cellflag, M, min_size, w.s2, w.grp, counts);
    pass(w.root, false);                                                         // D: components of the final classes
    // outputs
    launch_1d(k_gl_nodes_out, M, GRID, s, w.nid, w.row, w.cellroot, w.grp, w.root, w.alive, w.s1, w.s2, reinterpret_cast<const long long*>(sv_sizes_dev), I, M,
              NC, reinterpret_cast<u64*>(node_ids_dev), reinterpret_cast<u64*>(node_cell_dev), node_class_dev, reinterpret_cast<u64*>(node_comp_dev),
              node_size1_dev, node_size2_dev, w.head, counts);
    if (int rc = scan_u32(who, w.prim, w.head, w.seg, m, s); rc != SD_OK) return rc;
    launch_1d(k_gl_cells_out, M, GRID, s, w.nid, w.head, w.seg, w.cellflag, M, NC, reinterpret_cast<u64*>(cell_ids_dev), cell_outcome_dev, counts);
    for (u32 c = 0; c < 2; ++c) {
        launch_1d(k_gl_cc_keys, M, GRID, s, w.grp, w.root, w.alive, M, c, w.key, counts);
        if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, m, bits_for(M + 1), s); rc != SD_OK) return rc;
        if (int rc = number_segments(who, w.prim, w.skey, nullptr, w.head, w.seg, m, s); rc != SD_OK) return rc;
        launch_1d(k_gl_csr, M, GRID, s, w.skey, w.perm, w.head, w.seg, w.nid, w.cellroot, M, NC, reinterpret_cast<u64*>(c ? gcc_ids_dev : ncc_ids_dev),
                  reinterpret_cast<u64*>(c ? gcc_cell_dev : ncc_cell_dev), reinterpret_cast<u64*>(c ? gcc_begin_dev : ncc_begin_dev),
                  reinterpret_cast<u64*>(c ? gcc_sv_dev : ncc_sv_dev), counts, (int)(c ? C_GCC : C_NCC), (int)(c ? C_GSV : C_NSV));
        if (E) {
            launch_1d(k_gl_edge_flags, E, GRID, s, w.ea, w.eb, E, w.grp, w.alive, M, c, w.eflag);
            if (int rc = scan_u32(who, w.prim, w.eflag, w.epos, n_edges, s); rc != SD_OK) return rc;
            launch_1d(k_gl_edges_out, E, GRID, s, edges, E, w.eflag, w.epos, EC, reinterpret_cast<u64*>(c ? astrocyte_edges_dev : neuron_edges_dev), counts,
                      (int)(c ? C_GEDGES : C_NEDGES));
        }
    }
    return launch_status("sd_glia_split: launch failed");
}

int sd_glia_pred(const void* probas_dev, int is_f64, const uint64_t* view_begin_dev, size_t n_sv, size_t n_views, double thresh, int point_model,
                 uint8_t* class_dev, double* mean_dev, uint64_t* counts_dev, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_glia_pred";
    if (!counts_dev) return fail(who, ": null counts");
    if (n_sv >= LIM31) return fail(who, ": supervoxels < 2^31 per call");
    if (thresh != thresh) return fail(who, ": thresh is NaN");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (n_sv == 0) return n_views ? fail(who, ": views without supervoxels") : SD_OK;
    if (!view_begin_dev || (n_views && !probas_dev) || !class_dev || !mean_dev) return fail(who, ": bad argument");
    const u64 N = n_sv, V = n_views;
    const u64* vb = reinterpret_cast<const u64*>(view_begin_dev);
    launch_1d(k_check_offsets, N, GRID, s, vb, N, V, counts);
    if (is_f64) launch_1d(k_gl_pred<double>, N, GRID, s, reinterpret_cast<const double*>(probas_dev), vb, N, V, thresh, point_model, class_dev, mean_dev);
    else launch_1d(k_gl_pred<float>, N, GRID, s, reinterpret_cast<const float*>(probas_dev), vb, N, V, thresh, point_model, class_dev, mean_dev);
    return launch_status("sd_glia_pred: launch failed");
}

}  // extern "C"
