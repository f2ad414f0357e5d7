// Majority votes along skeletons: the array form of what the reference's reps/super_segmentation_helper.py does per node in Python --
// majorityvote_skeleton_property (:1270-1302: one nx.single_source_dijkstra_path(g, n, max_dist) and one np.unique per node, over the
// graph of SuperSegmentationObject.weighted_graph, reps/super_segmentation_object.py:1440-1451) and majority_vote_compartments
// (:1233-1266: connected components of the graph without its soma nodes, one np.unique per component).
//
//   csr      all cells in one call.  Cell c owns nodes node_begin[c] .. node_begin[c + 1] and edges edge_begin[c] .. edge_begin[c + 1];
//            an edge names two nodes by their index INSIDE the cell.  Every edge gives two half edges keyed by the table row of their
//            first node; sort_by_key (sd_sortseg.h, stable) orders them, row g of the adjacency is the key range of g.  An edge that
//            names a node outside its cell gets the key n_nodes, behind every row, and sets counts[7]: it is never walked.
//   vote     one wave per source node: a label-correcting search.  dist(v) = the smallest left-to-right float64 sum of edge weights
//            over all paths from the source, the least fixed point of dist[v] = min(dist[u] + w), which a relaxation reaches with the
//            same bits in any order (Dijkstra's result).  The reached nodes live in an open-addressed table of the wave (node ->
//            distance, linear probing) in LDS; a distance is lowered with a 64-bit integer atomic minimum on its bits (non-negative
//            doubles order like their bit patterns), and a node whose distance went down is queued again unless it is queued already
//            (bit 31 of its key).  The wave takes ONE queued node at a time and relaxes its adjacency row 64 entries per step, one per
//            lane.  Only nodes with dist <= max_dist are ever entered: when the queue is empty the table IS the window.  The vote:
//            per class a ballot over the list of reached nodes, lane c keeps the count of class c, the highest count wins and on
//            equal counts the smaller class (np.unique + argmax).
//            A window of more than SD_SKEL_LDS_NODES nodes does not fit: the source is flagged, counted in counts[0], and redone by
//            the second kernel over per-wave arrays in the scratch that are indexed by the node's index inside its cell (no hashing),
//            sized by the largest cell.  Nothing is truncated.
//   comps    union-find over the edges whose two nodes are not soma (uf_union of sd_tables.h), key (root, class) per node, sort_by_key,
//            the length of every (root, class) run by a search for its end, the best (count, smallest class) of every root by a 64-bit atomic maximum, then per node the rule 50 c1 < 33 total.
//
// Every index read from device memory is clamped or checked before it is used.  No scalar memory writes, no inline assembly.
#include "../../include/syconn_dense.h"
#include "sd_sortseg.h"
#include "sd_tables.h"

namespace {

constexpr u32 CAP = SD_SKEL_LDS_NODES;                       // reached nodes an LDS table holds
constexpr u32 SLOTS = 2 * CAP;                               // its slots: never more than (CAP + 64) / SLOTS full
constexpr u32 LISTN = CAP + 64;                              // a step enters up to 64 nodes before the overflow test
constexpr int LOG_SLOTS = 10;
constexpr u32 INQ = 0x80000000u, IDMASK = 0x7fffffffu, EMPTY = 0x7fffffffu;
constexpr u64 FAR = ~0ull;                                   // above the bits of every double >= 0, +inf included
static_assert(SLOTS == (1u << LOG_SLOTS) && SLOTS <= 65536, "slots are a power of two and fit the 16-bit queue entries");
static_assert(SD_SKEL_MAX_CLASSES == 64, "one class count per lane");
static_assert(4 * (SLOTS * (8 + 4 + 2) + LISTN * 2) <= 65536, "four waves' tables in one block's LDS");

// ---- csr --------------------------------------------------------------------------------------------------------------------------
// the two table rows of edge e, or false where one of them is outside the cell
__device__ __forceinline__ bool edge_rows(const long long* __restrict__ edges, const u64* __restrict__ edge_begin, const u64* __restrict__ node_begin,
                                          u64 n_cells, u64 n_nodes, u64 e, u64& ga, u64& gb) {
    const u64 c = segment_of(edge_begin, n_cells, e);
    const u64 n1 = clamp_u64(node_begin[c + 1], n_nodes), n0 = clamp_u64(node_begin[c], n1);
    const long long a = edges[2 * e], b = edges[2 * e + 1], n = (long long)(n1 - n0);
    if (a < 0 || a >= n || b < 0 || b >= n) return false;
    ga = n0 + (u64)a;
    gb = n0 + (u64)b;
    return true;
}
__global__ __launch_bounds__(256) void k_csr_keys(const long long* __restrict__ edges, const u64* __restrict__ edge_begin, const u64* __restrict__ node_begin,
                                                  u64 n_cells, u64 n_nodes, u64 n_edges, u64* key, u64* counts) {
    for (u64 j = grid_tid(); j < 2 * n_edges; j += grid_stride()) {
        u64 ga = 0, gb = 0;
        const bool ok = edge_rows(edges, edge_begin, node_begin, n_cells, n_nodes, j >> 1, ga, gb);
        if (!ok) counts[7] = 1;
        key[j] = ok ? ((j & 1) ? gb : ga) : n_nodes;
    }
}
__global__ __launch_bounds__(256) void k_csr_place(const long long* __restrict__ edges, const double* __restrict__ weight, const u64* __restrict__ skey,
                                                   const u32* __restrict__ perm, u64 n_nodes, u64 n_edges, u32* adj_nbr, double* adj_w, u64* counts) {
    for (u64 i = grid_tid(); i < 2 * n_edges; i += grid_stride()) {
        const u64 j = clamp_u64(perm[i], 2 * n_edges - 1), e = j >> 1;
        double w = weight[e];
        if (!(w >= 0.0)) { w = INFINITY; counts[7] = 1; }                        // negative or NaN: never relaxed below a finite max_dist
        adj_nbr[i] = skey[i] < n_nodes ? (u32)edges[2 * e + ((j & 1) ^ 1)] : 0u;
        adj_w[i] = w;
    }
}
__global__ __launch_bounds__(256) void k_csr_rows(const u64* __restrict__ skey, u64 n_nodes, u64 n_adj, u64* adj_begin) {
    for (u64 g = grid_tid(); g <= n_nodes; g += grid_stride()) adj_begin[g] = n_adj ? lower_bound(skey, n_adj, g) : 0;
}

// ---- vote -------------------------------------------------------------------------------------------------------------------------
// the arrays of one wave: in LDS (GLOBAL = false: `key` maps slots to nodes) or in the scratch (GLOBAL = true: slot = node, `key`
// only carries the queued bit).  Every access is a relaxed atomic of the matching scope: in LDS that is the plain instruction, in
// global memory it keeps the reads out of the CU's L1, where a line may be older than an atomic another lane has sent to the L2.
template <bool GLOBAL, class IX> struct WaveTab {
    static constexpr int SCOPE = GLOBAL ? __HIP_MEMORY_SCOPE_AGENT : __HIP_MEMORY_SCOPE_WORKGROUP;
    u64* dist; u32* key; IX* queue; IX* list; u32 slots;
    template <class T> __device__ __forceinline__ static T ld(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
    template <class T> __device__ __forceinline__ static void st(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, SCOPE); }
    // the slot of node v, entered if it is new
    __device__ __forceinline__ u32 slot_of(u32 v) const {
        if (GLOBAL) return v;
        u32 h = (v * 0x9E3779B1u) >> (32 - LOG_SLOTS);
        for (;;) {
            u32 k = ld(&key[h]);
            if (k == EMPTY) {
                u32 expect = EMPTY;
                if (__hip_atomic_compare_exchange_strong(&key[h], &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) return h;
                k = expect;
            }
            if ((k & IDMASK) == v) return h;
            h = (h + 1) & (SLOTS - 1);
        }
    }
    __device__ __forceinline__ u32 node_of(u32 slot) const { return GLOBAL ? slot : (ld(&key[slot]) & IDMASK); }
    __device__ __forceinline__ void clear(u32 n, int lane) const {
        for (u32 i = lane; i < n; i += 64) { st(&key[i], EMPTY); st(&dist[i], FAR); }
    }
};

// The window of source `src` (index inside its cell) and its vote.  All lanes of the wave call it with the same arguments; the
// table is empty before and after.  -> false if the window outgrew `cap` nodes (nothing is written then).
template <bool GLOBAL, class IX>
__device__ __forceinline__ bool skel_window(const WaveTab<GLOBAL, IX>& t, u32 cap, const u64* __restrict__ adj_begin, const u32* __restrict__ adj_nbr,
                                            const double* __restrict__ adj_w, u64 n_adj, u64 base, u32 n_cell, u32 src, double max_dist,
                                            const uint8_t* __restrict__ classes, int n_classes, int lane, u32& n_reached, int& vote, u64& n_steps) {
    typedef WaveTab<GLOBAL, IX> T;
    const u64 lt = (1ull << lane) - 1;
    const u32 s0 = t.slot_of(src);                                               // every lane: the same slot
    if (lane == 0) { T::st(&t.dist[s0], (u64)0); T::st(&t.key[s0], GLOBAL ? (EMPTY | INQ) : (src | INQ)); T::st(&t.list[0], (IX)s0); T::st(&t.queue[0], (IX)s0); }
    u32 n = 1, qh = 0, qn = 1;                                                   // reached nodes; queue head and length (the same in every lane)
    bool fits = true;
    while (qn && fits) {
        const u32 su = T::ld(&t.queue[qh]);
        qh = qh + 1 < t.slots ? qh + 1 : 0;
        --qn;
        const u32 u = t.node_of(su);
        if (lane == 0) T::st(&t.key[su], GLOBAL ? EMPTY : u);                    // no longer queued
        const double du = __longlong_as_double((long long)T::ld(&t.dist[su]));
        const u64 r1 = clamp_u64(adj_begin[base + u + 1], n_adj), r0 = clamp_u64(adj_begin[base + u], r1);
        for (u64 r = r0; r < r1 && fits; r += 64) {
            const u64 i = r + lane;
            bool first = false, push = false;
            u32 slot = 0;
            if (i < r1) {
                const u32 v = adj_nbr[i];
                const double nd = du + adj_w[i];
                if (v < n_cell && nd <= max_dist) {                              // networkx skips on > cutoff: equality stays in
                    const u64 nb = (u64)__double_as_longlong(nd);
                    slot = t.slot_of(v);
                    const u64 old = __hip_atomic_fetch_min(&t.dist[slot], nb, __ATOMIC_RELAXED, T::SCOPE);
                    if (nb < old) {
                        first = old == FAR;
                        push = !(__hip_atomic_fetch_or(&t.key[slot], INQ, __ATOMIC_RELAXED, T::SCOPE) & INQ);
                    }
                }
            }
            const u64 bf = __ballot(first), bp = __ballot(push);
            if (first) T::st(&t.list[n + (u32)__popcll(bf & lt)], (IX)slot);
            if (push) {
                u32 q = qh + qn + (u32)__popcll(bp & lt);                        // < 2 slots + 64
                if (q >= t.slots) q -= t.slots;
                if (q >= t.slots) q -= t.slots;
                T::st(&t.queue[q], (IX)slot);
            }
            n += (u32)__popcll(bf);
            qn += (u32)__popcll(bp);
            ++n_steps;
            fits = n <= cap;
        }
    }
    if (fits) {
        u32 cnt = 0;                                                             // lane c: nodes of class c in the window
        for (u32 i0 = 0; i0 < n; i0 += 64) {
            int cls = -1;
            if (i0 + lane < n) cls = classes[base + t.node_of(T::ld(&t.list[i0 + lane]))];
            for (int c = 0; c < n_classes; ++c) {
                const u64 b = __ballot(cls == c);
                if (lane == c) cnt += (u32)__popcll(b);
            }
        }
        u64 best = lane < n_classes ? ((u64)cnt << 6 | (u64)(63 - lane)) : 0;
        for (int msk = 32; msk; msk >>= 1) { const u64 o = __shfl_xor(best, msk); best = o > best ? o : best; }
        vote = 63 - (int)(best & 63);
        n_reached = n;
    }
    for (u32 i = lane; i < n; i += 64) {                                         // empty the table again
        const u32 slot = T::ld(&t.list[i]);
        T::st(&t.key[slot], EMPTY);
        T::st(&t.dist[slot], FAR);
    }
    return fits;
}

__global__ __launch_bounds__(256) void k_skel_vote_lds(const u64* __restrict__ adj_begin, const u32* __restrict__ adj_nbr, const double* __restrict__ adj_w, u64 n_adj,
                                                       const u64* __restrict__ node_begin, u64 n_cells, u64 n_nodes, const uint8_t* __restrict__ classes,
                                                       int n_classes, double max_dist, uint8_t* vote, u32* n_reached, uint8_t* redo, u64* counts) {
    __shared__ u64 s_dist[4][SLOTS];
    __shared__ u32 s_key[4][SLOTS];
    __shared__ unsigned short s_queue[4][SLOTS];
    __shared__ unsigned short s_list[4][LISTN];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 wave = grid_tid() >> 6, n_waves = grid_stride() >> 6;
    const WaveTab<false, unsigned short> t{s_dist[w], s_key[w], s_queue[w], s_list[w], SLOTS};
    t.clear(SLOTS, lane);
    u64 n_steps = 0, n_redo = 0;
    for (u64 g = wave; g < n_nodes; g += n_waves) {
        const u64 c = segment_of(node_begin, n_cells, g);
        const u64 n1 = clamp_u64(node_begin[c + 1], n_nodes), n0 = clamp_u64(node_begin[c], n1);
        if (g < n0 || g >= n1) { if (lane == 0) counts[7] = 1; continue; }       // offsets that do not cover the nodes
        u32 nr = 0;
        int v = 0;
        if (skel_window(t, CAP, adj_begin, adj_nbr, adj_w, n_adj, n0, (u32)(n1 - n0), (u32)(g - n0), max_dist, classes, n_classes, lane, nr, v, n_steps)) {
            if (lane == 0) { vote[g] = (uint8_t)v; if (n_reached) n_reached[g] = nr; }
        } else {
            if (lane == 0) redo[g] = 1;
            ++n_redo;
        }
    }
    if (lane == 0) {
        if (n_redo) atomicAdd(&counts[0], n_redo);
        if (n_steps) atomicAdd(&counts[1], n_steps);
    }
}

// the flagged sources again, over arrays of `m` entries per wave in the scratch (m >= 64, m >= the nodes of every cell)
__global__ __launch_bounds__(256) void k_skel_vote_glb(const u64* __restrict__ adj_begin, const u32* __restrict__ adj_nbr, const double* __restrict__ adj_w, u64 n_adj,
                                                       const u64* __restrict__ node_begin, u64 n_cells, u64 n_nodes, const uint8_t* __restrict__ classes,
                                                       int n_classes, double max_dist, uint8_t* vote, u32* n_reached, const uint8_t* __restrict__ redo,
                                                       u64* g_dist, u32* g_key, u32* g_queue, u32* g_list, u64 m, u64* counts) {
    const int lane = threadIdx.x & 63;
    const u64 wave = grid_tid() >> 6, n_waves = grid_stride() >> 6;
    const WaveTab<true, u32> t{g_dist + wave * m, g_key + wave * m, g_queue + wave * m, g_list + wave * m, (u32)m};
    bool ready = false;
    u64 n_steps = 0;
    for (u64 g = wave; g < n_nodes; g += n_waves) {
        if (!redo[g]) continue;
        const u64 c = segment_of(node_begin, n_cells, g);
        const u64 n1 = clamp_u64(node_begin[c + 1], n_nodes), n0 = clamp_u64(node_begin[c], n1);
        if (g < n0 || g >= n1 || n1 - n0 > m) { if (lane == 0) counts[7] = 1; continue; }
        if (!ready) { t.clear((u32)m, lane); ready = true; }
        u32 nr = 0;
        int v = 0;
        skel_window(t, (u32)m, adj_begin, adj_nbr, adj_w, n_adj, n0, (u32)(n1 - n0), (u32)(g - n0), max_dist, classes, n_classes, lane, nr, v, n_steps);
        if (lane == 0) { vote[g] = (uint8_t)v; if (n_reached) n_reached[g] = nr; }
    }
    if (lane == 0 && n_steps) atomicAdd(&counts[2], n_steps);
}

// ---- components -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cc_union(const long long* __restrict__ edges, const u64* __restrict__ edge_begin, const u64* __restrict__ node_begin,
                                                  u64 n_cells, u64 n_nodes, u64 n_edges, const uint8_t* __restrict__ classes, int soma, u32* parent, u64* counts) {
    for (u64 e = grid_tid(); e < n_edges; e += grid_stride()) {
        u64 ga = 0, gb = 0;
        if (!edge_rows(edges, edge_begin, node_begin, n_cells, n_nodes, e, ga, gb)) { counts[7] = 1; continue; }
        if ((int)classes[ga] == soma || (int)classes[gb] == soma) continue;
        uf_union(parent, (u32)ga, (u32)gb);
    }
}
__global__ __launch_bounds__(256) void k_cc_keys(const u32* __restrict__ parent, const uint8_t* __restrict__ classes, int soma, u64 n_nodes, u32* root, u64* key) {
    for (u64 g = grid_tid(); g < n_nodes; g += grid_stride()) {
        const int cls = classes[g];
        const u32 r = cls == soma ? (u32)n_nodes : uf_find(parent, (u32)g);
        root[g] = r;
        key[g] = (u64)r << 6 | (u64)(cls & 63);
    }
}
// at the first record of every (root, class) run: its length against the root's best (count, smallest class)
__global__ __launch_bounds__(256) void k_cc_best(const u64* __restrict__ skey, const u32* __restrict__ head, u64 n_nodes, u64* best) {
    for (u64 i = grid_tid(); i < n_nodes; i += grid_stride()) {
        const u64 k = skey[i], r = k >> 6;
        if (!head[i] || r >= n_nodes) continue;
        const u64 cnt = upper_bound(skey, n_nodes, k) - i;
        atomicMax(&best[r], cnt << 6 | (63 - (k & 63)));
    }
}
__global__ __launch_bounds__(256) void k_cc_write(const u64* __restrict__ skey, const u32* __restrict__ root, const u64* __restrict__ best,
                                                  const uint8_t* __restrict__ classes, int one, int zero, u64 n_nodes, uint8_t* out, u64* counts) {
    for (u64 g = grid_tid(); g < n_nodes; g += grid_stride()) {
        const u64 r = root[g];
        if (r >= n_nodes) { out[g] = classes[g]; continue; }                    // soma keeps its label
        const u64 b = best[r];
        int maj = 63 - (int)(b & 63);
        if (maj == one) {
            const u64 c1 = b >> 6, total = lower_bound(skey, n_nodes, (r + 1) << 6) - lower_bound(skey, n_nodes, r << 6);
            if (total >= (1ull << 24)) counts[6] = 1;                           // float32 shares: the reference's rule is pinned below 2^24
            if (50 * c1 < 33 * total) maj = zero;
        }
        out[g] = (uint8_t)maj;
    }
}

// ---- scratch ----------------------------------------------------------------------------------------------------------------------
struct CsrScratch { u64 *key, *skey; u32 *i0, *perm; PrimScratch prim; };
size_t layout(CsrScratch& w, void* base, size_t n_adj) {
    ScratchAlloc a(base);
    a.take_into(n_adj, w.key, w.skey);
    a.take_into(n_adj, w.i0, w.perm);
    w.prim = take_prim(a, n_adj);
    return a.used;
}
// waves of the second pass: as many as SD_SKEL_REDO_GRID blocks hold, fewer where their arrays would pass SD_SKEL_REDO_BYTES
struct VoteScratch { uint8_t* redo; u64* dist; u32 *key, *queue, *list; size_t m, blocks; };
size_t layout(VoteScratch& w, void* base, size_t n_nodes, size_t max_cell_nodes) {
    ScratchAlloc a(base);
    w.m = std::max<size_t>(max_cell_nodes, 64);
    w.blocks = std::min<size_t>(SD_SKEL_REDO_GRID, std::max<size_t>(1, (size_t)SD_SKEL_REDO_BYTES / (4 * 20 * w.m)));
    a.take_into(n_nodes, w.redo);
    a.take_into(4 * w.blocks * w.m, w.dist);
    a.take_into(4 * w.blocks * w.m, w.key, w.queue, w.list);
    return a.used;
}
struct CompScratch { u32 *parent, *root, *i0, *perm, *head; u64 *key, *skey, *best; PrimScratch prim; };
size_t layout(CompScratch& w, void* base, size_t n_nodes) {
    ScratchAlloc a(base);
    a.take_into(n_nodes, w.parent, w.root, w.i0, w.perm, w.head);
    a.take_into(n_nodes, w.key, w.skey, w.best);
    w.prim = take_prim(a, n_nodes);
    return a.used;
}

int check_tables(const char* who, size_t n_cells, size_t n_nodes, size_t n_edges) {
    if (n_cells >= LIM31 || n_nodes >= LIM31 - 1 || n_edges >= LIM31 / 2)
        return fail(who, ": cells, nodes and half edges < 2^31 per call");
    return SD_OK;
}

}  // namespace

extern "C" {

size_t sd_skel_csr_temp_bytes(size_t n_edges) {
    CsrScratch w;
    return layout(w, nullptr, n_edges ? 2 * n_edges : 1);
}

int sd_skel_csr(const int64_t* edges_dev, const uint64_t* edge_begin_dev, const uint64_t* node_begin_dev, size_t n_cells, size_t n_nodes,
                size_t n_edges, const double* weight_dev, uint64_t* adj_begin_dev, uint32_t* adj_nbr_dev, double* adj_w_dev, uint64_t* counts_dev,
                void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_skel_csr";
    if (!counts_dev) return fail(who, ": null counts");
    if (int rc = check_tables(who, n_cells, n_nodes, n_edges); rc != SD_OK) return rc;
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (n_cells == 0) {
        if (n_nodes || n_edges) return fail(who, ": nodes or edges without cells");
        return SD_OK;
    }
    if (!edge_begin_dev || !node_begin_dev || !adj_begin_dev || (n_edges && (!edges_dev || !weight_dev || !adj_nbr_dev || !adj_w_dev)))
        return fail(who, ": bad argument");
    if (n_edges)
        if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_skel_csr_temp_bytes(n_edges), "sd_skel_csr_temp_bytes(n_edges)"); rc != SD_OK) return rc;
    const u64 Cn = n_cells, N = n_nodes, E = n_edges;
    const u64* eb = reinterpret_cast<const u64*>(edge_begin_dev);
    const u64* nb = reinterpret_cast<const u64*>(node_begin_dev);
    const long long* edges = reinterpret_cast<const long long*>(edges_dev);
    u64* adj_begin = reinterpret_cast<u64*>(adj_begin_dev);
    launch_1d(k_check_offsets, Cn, SD_SKEL_NODE_GRID, s, nb, Cn, N, counts);
    launch_1d(k_check_offsets, Cn, SD_SKEL_NODE_GRID, s, eb, Cn, E, counts);
    CsrScratch w;
    layout(w, temp_dev, E ? 2 * E : 1);
    if (E) {
        launch_1d(k_csr_keys, 2 * E, SD_SKEL_EDGE_GRID, s, edges, eb, nb, Cn, N, E, w.key, counts);
        if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, 2 * n_edges, bits_for(N + 1), s); rc != SD_OK) return rc;
        launch_1d(k_csr_place, 2 * E, SD_SKEL_EDGE_GRID, s, edges, weight_dev, w.skey, w.perm, N, E, adj_nbr_dev, adj_w_dev, counts);
    }
    launch_1d(k_csr_rows, N + 1, SD_SKEL_NODE_GRID, s, w.skey, N, 2 * E, adj_begin);
    return launch_status("sd_skel_csr: launch failed");
}

size_t sd_skel_vote_temp_bytes(size_t n_nodes, size_t max_cell_nodes) {
    VoteScratch w;
    return layout(w, nullptr, n_nodes ? n_nodes : 1, max_cell_nodes);
}

int sd_skel_vote(const uint64_t* adj_begin_dev, const uint32_t* adj_nbr_dev, const double* adj_w_dev, size_t n_adj, const uint64_t* node_begin_dev,
                 size_t n_cells, size_t n_nodes, size_t max_cell_nodes, const uint8_t* classes_dev, int n_classes, double max_dist,
                 uint8_t* vote_dev, uint32_t* n_reached_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_skel_vote";
    if (!counts_dev) return fail(who, ": null counts");
    if (int rc = check_tables(who, n_cells, n_nodes, n_adj / 2); rc != SD_OK) return rc;
    if (n_classes < 1 || n_classes > SD_SKEL_MAX_CLASSES) return fail(who, ": 1 <= n_classes <= 64");
    if (!(max_dist >= 0.0)) return fail(who, ": max_dist >= 0");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (n_nodes == 0) return SD_OK;
    if (n_cells == 0) return fail(who, ": nodes without cells");
    if (!adj_begin_dev || !node_begin_dev || !classes_dev || !vote_dev || (n_adj && (!adj_nbr_dev || !adj_w_dev)))
        return fail(who, ": bad argument");
    if (max_cell_nodes < 1 || max_cell_nodes > n_nodes) return fail(who, ": 1 <= max_cell_nodes <= n_nodes");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_skel_vote_temp_bytes(n_nodes, max_cell_nodes), "sd_skel_vote_temp_bytes(n_nodes, max_cell_nodes)"); rc != SD_OK)
        return rc;
    VoteScratch w;
    layout(w, temp_dev, n_nodes, max_cell_nodes);
    if (hipMemsetAsync(w.redo, 0, n_nodes, s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    const u64* adj_begin = reinterpret_cast<const u64*>(adj_begin_dev);
    const u64* nb = reinterpret_cast<const u64*>(node_begin_dev);
    const u64 N = n_nodes, Cn = n_cells, A = n_adj;
    launch_1d(k_skel_vote_lds, 64 * N, SD_SKEL_VOTE_GRID, s, adj_begin, adj_nbr_dev, adj_w_dev, A, nb, Cn, N, classes_dev, n_classes, max_dist,
              vote_dev, n_reached_dev, w.redo, counts);
    hipLaunchKernelGGL(k_skel_vote_glb, dim3((unsigned)w.blocks), dim3(256), 0, s, adj_begin, adj_nbr_dev, adj_w_dev, A, nb, Cn, N, classes_dev, n_classes,
                       max_dist, vote_dev, n_reached_dev, w.redo, w.dist, w.key, w.queue, w.list, (u64)w.m, counts);
    return launch_status("sd_skel_vote: launch failed");
}

size_t sd_skel_components_temp_bytes(size_t n_nodes) {
    CompScratch w;
    return layout(w, nullptr, n_nodes ? n_nodes : 1);
}

int sd_skel_components(const int64_t* edges_dev, const uint64_t* edge_begin_dev, const uint64_t* node_begin_dev, size_t n_cells, size_t n_nodes,
                       size_t n_edges, const uint8_t* classes_dev, int soma_class, int one_class, int zero_class, uint8_t* out_dev,
                       uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_skel_components";
    if (!counts_dev) return fail(who, ": null counts");
    if (int rc = check_tables(who, n_cells, n_nodes, n_edges); rc != SD_OK) return rc;
    if (soma_class < -1 || soma_class >= SD_SKEL_MAX_CLASSES || one_class < -1 || one_class >= SD_SKEL_MAX_CLASSES || zero_class < 0 ||
        zero_class >= SD_SKEL_MAX_CLASSES)
        return fail(who, ": classes are below 64 (soma and one may be -1: absent)");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (n_nodes == 0) return SD_OK;
    if (n_cells == 0) return fail(who, ": nodes without cells");
    if (!edge_begin_dev || !node_begin_dev || !classes_dev || !out_dev || (n_edges && !edges_dev))
        return fail(who, ": bad argument");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_skel_components_temp_bytes(n_nodes), "sd_skel_components_temp_bytes(n_nodes)"); rc != SD_OK) return rc;
    CompScratch w;
    layout(w, temp_dev, n_nodes);
    const u64 Cn = n_cells, N = n_nodes, E = n_edges;
    const u64* eb = reinterpret_cast<const u64*>(edge_begin_dev);
    const u64* nb = reinterpret_cast<const u64*>(node_begin_dev);
    const long long* edges = reinterpret_cast<const long long*>(edges_dev);
    launch_1d(k_check_offsets, Cn, SD_SKEL_NODE_GRID, s, nb, Cn, N, counts);
    launch_1d(k_check_offsets, Cn, SD_SKEL_NODE_GRID, s, eb, Cn, E, counts);
    launch_1d(k_iota, N, SD_SKEL_NODE_GRID, s, w.parent, N);
    if (hipMemsetAsync(w.best, 0, n_nodes * sizeof(u64), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    if (E) launch_1d(k_cc_union, E, SD_SKEL_EDGE_GRID, s, edges, eb, nb, Cn, N, E, classes_dev, soma_class, w.parent, counts);
    launch_1d(k_cc_keys, N, SD_SKEL_NODE_GRID, s, w.parent, classes_dev, soma_class, N, w.root, w.key);
    if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, n_nodes, bits_for(N + 1) + 6, s); rc != SD_OK) return rc;
    launch_1d(k_heads, N, SD_SKEL_NODE_GRID, s, w.skey, (const u64*)nullptr, w.head, N);
    launch_1d(k_cc_best, N, SD_SKEL_NODE_GRID, s, w.skey, w.head, N, w.best);
    launch_1d(k_cc_write, N, SD_SKEL_NODE_GRID, s, w.skey, w.root, w.best, classes_dev, one_class, zero_class, N, out_dev, counts);
    return launch_status("sd_skel_components: launch failed");
}

}  // extern "C"
