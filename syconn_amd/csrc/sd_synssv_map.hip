// Organelles of the two partner cells mapped to every cell-level synapse: the array form of what the reference's
// extraction/cs_processing_steps.py does per cell in Python -- _map_objects_from_synssv_partners_thread (:888-1009: three cKDTrees per
// cell, query_ball_tree of the representative coordinates) and _map_objects_from_synssv (:1012-1052: one cKDTree per synapse, every
// second mesh vertex of every nearby organelle queried against every second voxel of the synapse).  One organelle type per call.
//
// A "side" is (synapse row, partner slot): side 2 i + p belongs to cell neuron_partners[i][p].
//
//   pairs    one wave per side.  The organelles arrive sorted by cell; the wave finds its cell's run by binary search, its lanes test
//            the representative coordinates (d^2 <= D^2, inclusive as query_ball_tree is), and a ballot with a prefix popcount keeps
//            the run's order.  The first call counts and scans (side_begin, the total); the second fills the caller's pair list.
//   voxels   the sampled voxels of all synapses (rows 0, f, 2 f, ... of every run) as float64 nm, synapse-major: the tile index of
//            sd_pointtiles.h with the synapses as segments, a coarse spatial key (boxes of 4 voxels, relative to the synapse's
//            corner) and one box per synapse next to the tile boxes.  Nothing of this depends on the organelle type.
//   query    every pair is split into work items of at most MAP_T sampled vertices (one scan over ceil(len / MAP_T)); one block of
//            256 threads per item.  A thread holds MAP_T / 256 vertices; vertices outside the synapse's box by R or more are dropped;
//            the block walks the synapse's tiles, skips a tile that no vertex of the block can profit from (__syncthreads_or),
//            stages the others through LDS and tests point by point.  Per block one 32-bit atomic add (vertices with a voxel
//            strictly inside R) and one 64-bit atomic min on the bit pattern of the smallest d^2 (non-negative doubles order like
//            their bits).
//
// The box tests carry the 1 + 1e-9 margin of SsvGeom (sd_syn_ssv.hip): they decide only what rounding cannot change, the point test
// (every product and sum rounded on its own) decides the rest.  No scalar memory writes, no inline assembly.
#include "../../include/syconn_dense.h"
#include "sd_sortseg.h"
#include "sd_pointtiles.h"

namespace {

constexpr int MAP_T = SD_SYNSSV_MAP_ITEM;                    // sampled vertices per work item
constexpr int MAP_VPT = MAP_T / 256;                         // per thread
constexpr int MAP_QUERY_GRID = 8192;                         // blocks of the query kernel (items beyond are reached by the stride)
constexpr u64 INF_BITS = 0x7ff0000000000000ull;
static_assert(MAP_T % 256 == 0 && MAP_VPT <= 32, "one flag bit per vertex of a thread");
static_assert(3 * TILE <= 256, "the block stages a tile through LDS with one coordinate per thread");

struct MapGeom { double s[3], r2, r2_hi; };                  // voxel size in nm, squared radius, r2 (1 + 1e-9)

// ---- pairs ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_map_pairs(const u64* __restrict__ side_cell, const int* __restrict__ syn_rep, u64 n_sides,
                                                   const u64* __restrict__ org_cell, const u32* __restrict__ org_row,
                                                   const int* __restrict__ org_rep, u64 m, MapGeom g, const u32* side_begin, u32* cnt,
                                                   u32* pair_obj, u64 pair_cap) {
    const int lane = threadIdx.x & 63;
    const u64 wave = grid_tid() >> 6, n_waves = grid_stride() >> 6;
    for (u64 side = wave; side < n_sides; side += n_waves) {
        const u64 c = side_cell[side];
        u32 base = 0;
        if (c != 0) {                                                            // 0 = no cell: organelles of cell 0 are unassigned
            const double r[3] = {(double)syn_rep[3 * (side >> 1)], (double)syn_rep[3 * (side >> 1) + 1], (double)syn_rep[3 * (side >> 1) + 2]};
            const u64 out0 = pair_obj ? side_begin[side] : 0;
            for (u64 j0 = lower_bound(org_cell, m, c); j0 < m && org_cell[j0] == c; j0 += 64) {
                const u64 j = j0 + lane;
                bool hit = false;
                if (j < m && org_cell[j] == c) {
#pragma clang fp contract(off)
                    double p[3], q[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) { p[a] = (double)org_rep[3 * j + a] * g.s[a]; q[a] = r[a] * g.s[a]; }
                    hit = sq_dist(p, q) <= g.r2;
                }
                const u64 mask = __ballot(hit);
                if (hit && pair_obj) {
                    const u64 at = out0 + base + __popcll(mask & ((1ull << lane) - 1));
                    if (at < pair_cap) pair_obj[at] = org_row[j];
                }
                base += (u32)__popcll(mask);
            }
        }
        if (!pair_obj && lane == 0) cnt[side] = base;
    }
}
__global__ __launch_bounds__(256) void k_map_side_begin(const u32* scan, u64 n, u32* side_begin, u64* counts) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        if (i == 0) side_begin[0] = 0;
        side_begin[i + 1] = scan[i];
        if (i == n - 1) counts[0] = scan[i];
    }
}

// ---- voxels -----------------------------------------------------------------------------------------------------------------------
// the sampled voxel k of synapse s is voxel row vb[s] + k f; rows are clamped so that a bad offset table (flagged in counts[7])
// cannot make a kernel read outside vox
__device__ __forceinline__ u64 vox_row(const u64* vb, const u64* svb, u64 s, u64 j, u32 f, u64 n_vox) {
    const u64 row = vb[s] + (j - svb[s]) * f;
    return row < n_vox ? row : n_vox - 1;
}
// one wave per synapse: the offsets are checked, the smallest voxel coordinates are the corner of the sort key
__global__ __launch_bounds__(256) void k_map_syn_corner(const u32* __restrict__ vox, const u64* __restrict__ vb, const u64* __restrict__ svb,
                                                        u64 n_syn, u64 n_vox, u64 n_sv, u32 f, u32* corner, u64* counts) {
    const int lane = threadIdx.x & 63;
    const u64 wave = grid_tid() >> 6, n_waves = grid_stride() >> 6;
    for (u64 s = wave; s < n_syn; s += n_waves) {
        const u64 b0 = vb[s], b1 = vb[s + 1], s0 = svb[s], s1 = svb[s + 1];
        const bool bad = b1 < b0 || b1 > n_vox || s1 < s0 || s1 > n_sv || s1 - s0 != (b1 - b0 + f - 1) / f || (s == 0 && s0 != 0) ||
                         (s == n_syn - 1 && s1 != n_sv);
        u32 lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
        if (!bad)
            for (u64 k = lane; k < s1 - s0; k += 64)
#pragma unroll
                for (int a = 0; a < 3; ++a) lo[a] = min(lo[a], vox[3 * (b0 + k * f) + a]);
#pragma unroll
        for (int a = 0; a < 3; ++a)
            for (int msk = 32; msk; msk >>= 1) lo[a] = min(lo[a], (u32)__shfl_xor((int)lo[a], msk));
        if (lane == 0) {
            if (bad) counts[7] = 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) corner[3 * s + a] = lo[a];
        }
    }
}
__global__ __launch_bounds__(256) void k_map_vox_keys(const u32* __restrict__ vox, const u64* __restrict__ vb, const u64* __restrict__ svb,
                                                      const u32* __restrict__ corner, u64 n_syn, u64 n_vox, u64 n_sv, u32 f, int b, u64* key) {
    for (u64 j = grid_tid(); j < n_sv; j += grid_stride()) {
        const u64 s = segment_of(svb, n_syn, j);
        const u64 row = vox_row(vb, svb, s, j, f, n_vox);
        u64 k = s;
#pragma unroll
        for (int a = 2; a >= 0; --a) {                                             // z is the slowest axis of the key
            const u32 c = (vox[3 * row + a] - corner[3 * s + a]) >> 2;
            k = (k << b) | (u64)min(c, (1u << b) - 1u);
        }
        key[j] = k;
    }
}
__global__ __launch_bounds__(256) void k_map_vox_place(const u32* __restrict__ vox, const u64* __restrict__ vb, const u64* __restrict__ svb,
                                                       const u64* __restrict__ skey, const u32* __restrict__ perm, u64 n_syn, u64 n_vox,
                                                       u64 n_sv, u32 f, int b, MapGeom g, double* pts) {
    for (u64 i = grid_tid(); i < n_sv; i += grid_stride()) {
        u64 s = skey[i] >> (3 * b);
        if (s >= n_syn) s = n_syn - 1;
        u64 j = perm[i];
        if (j >= n_sv) j = n_sv - 1;
        const u64 row = vox_row(vb, svb, s, j, f, n_vox);
#pragma unroll
        for (int a = 0; a < 3; ++a) pts[3 * i + a] = (double)vox[3 * row + a] * g.s[a];     // float64(voxel) * s, as numpy does it
    }
}

// ---- query ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_map_pair_init(const u32* __restrict__ pair_obj, const u64* __restrict__ vtb, u64 P, u64 n_org,
                                                       u64 n_vert, u32 f, u32* pair_len, u32* pair_close, u64* pair_min, u32* icnt, u64* counts) {
    const int lane = threadIdx.x & 63;
    for (u64 base = (u64)blockIdx.x * 256; base < P; base += grid_stride()) {
        const u64 p = base + threadIdx.x;
        u32 items = 0;
        if (p < P) {
            const u64 o = pair_obj[p];
            u64 len = 0;
            bool bad = o >= n_org;
            if (!bad) {
                const u64 v0 = vtb[o], v1 = vtb[o + 1];
                bad = v1 < v0 || v1 > n_vert;
                if (!bad) len = (v1 - v0 + f - 1) / f;
                if (len >> 32) { bad = true; len = 0; }
            }
            if (bad) counts[7] = 1;
            items = (u32)((len + MAP_T - 1) / MAP_T);
            pair_len[p] = (u32)len; pair_close[p] = 0; pair_min[p] = INF_BITS; icnt[p] = items;
            if (p == 0) counts[0] = P;
        }
        u64 sum = items;
        for (int msk = 32; msk; msk >>= 1) sum += __shfl_xor(sum, msk);
        if (lane == 0 && sum) atomicAdd(&counts[1], sum);
    }
}

__global__ __launch_bounds__(256) void k_map_query(const float* __restrict__ verts, const u64* __restrict__ vtb, u64 n_vert, const double* __restrict__ pts,
                                                   const u64* __restrict__ svb, u64 n_sv, const double* __restrict__ tbox, u64 n_slots,
                                                   const double* __restrict__ sbox, const u32* __restrict__ side_begin, u64 n_sides,
                                                   const u32* __restrict__ pair_obj, const u32* __restrict__ pair_len, const u32* __restrict__ icnt,
                                                   const u32* __restrict__ iscan, u64 P, u32 f, MapGeom g, u32* pair_close, u64* pair_min,
                                                   u64* counts) {
    __shared__ double tile[3 * TILE];
    __shared__ u32 w_close[4];
    __shared__ u64 w_min[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 n_items = counts[1];
    if (n_items >> 32) { if (tid == 0) counts[7] = 1; return; }                  // the scan of the item counts is 32 bits wide
    u64 n_reject = 0, n_tests = 0, n_skip = 0, n_stage = 0;
    for (u64 item = blockIdx.x; item < n_items; item += gridDim.x) {
        const u64 p = upper_bound(iscan, P, item);                               // pairs without vertices have no item
        if (p >= P) break;
        const u64 chunk = item - (u64)(iscan[p] - icnt[p]);
        const u64 syn = segment_of(side_begin, n_sides, p) >> 1;
        const u64 i0 = svb[syn], i1 = svb[syn + 1] < n_sv ? svb[syn + 1] : n_sv;
        const u64 n_tiles = i1 > i0 ? (i1 - i0 + TILE - 1) / TILE : 0, slot0 = tile_slot0(i0, syn);
        double sb[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) sb[a] = sbox[6 * syn + a];
        const u64 v0 = vtb[pair_obj[p]], len = pair_len[p];
        double vx[MAP_VPT][3], best[MAP_VPT];
        u32 alive = 0;
#pragma unroll
        for (int v = 0; v < MAP_VPT; ++v) {
            const u64 k = chunk * MAP_T + (u64)v * 256 + tid;
            best[v] = INFINITY;
            vx[v][0] = vx[v][1] = vx[v][2] = 0.0;
            if (k < len) {
                u64 row = v0 + k * f;
                if (row >= n_vert) row = n_vert - 1;
#pragma unroll
                for (int a = 0; a < 3; ++a) vx[v][a] = (double)verts[3 * row + a];
                if (n_tiles && box_dist2(vx[v], sb) < g.r2_hi) alive |= 1u << v; else ++n_reject;
            }
        }
        for (u64 t = 0; t < n_tiles; ++t) {
            const double* tb = tile_box(tbox, n_slots, slot0, t);
            double bx[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) bx[a] = tb[a];
            u32 want = 0;
#pragma unroll
            for (int v = 0; v < MAP_VPT; ++v)
                if ((alive >> v) & 1u) {
                    const double thr = fmin(g.r2_hi, best[v] * (1.0 + 1e-9));    // nothing in the tile can be inside R or beat the best
                    if (box_dist2(vx[v], bx) < thr) want |= 1u << v;
                }
            if (!__syncthreads_or((int)want)) { ++n_skip; continue; }
            ++n_stage;
            const u64 t0 = i0 + t * TILE;
            const int cnt = (int)(i1 - t0 < (u64)TILE ? i1 - t0 : (u64)TILE);
            if (tid < 3 * cnt) tile[tid] = pts[3 * t0 + tid];
            __syncthreads();
#pragma unroll
            for (int v = 0; v < MAP_VPT; ++v)
                if ((want >> v) & 1u) {
                    double b = best[v];
                    for (int q = 0; q < cnt; ++q) b = fmin(b, sq_dist(vx[v], &tile[3 * q]));
                    best[v] = b;
                    n_tests += (u64)cnt;
                }
            __syncthreads();
        }
        u32 c = 0;
        u64 mb = INF_BITS;
#pragma unroll
        for (int v = 0; v < MAP_VPT; ++v)
            if (((alive >> v) & 1u) && best[v] < g.r2) {                            // strict: cKDTree.query gives inf at exactly R
                ++c;
                const u64 bits = (u64)__double_as_longlong(best[v]);
                mb = bits < mb ? bits : mb;
            }
        for (int msk = 32; msk; msk >>= 1) {
            c += (u32)__shfl_xor((int)c, msk);
            const u64 o = __shfl_xor(mb, msk);
            mb = o < mb ? o : mb;
        }
        if (lane == 0) { w_close[wv] = c; w_min[wv] = mb; }
        __syncthreads();
        if (tid == 0) {
            u32 tc = 0;
            u64 tm = INF_BITS;
            for (int w = 0; w < 4; ++w) { tc += w_close[w]; tm = w_min[w] < tm ? w_min[w] : tm; }
            if (tc) { atomicAdd(&pair_close[p], tc); atomicMin(&pair_min[p], tm); }
        }
        __syncthreads();
    }
    for (int msk = 32; msk; msk >>= 1) { n_reject += __shfl_xor(n_reject, msk); n_tests += __shfl_xor(n_tests, msk); }
    if (lane == 0) {
        if (n_reject) atomicAdd(&counts[2], n_reject);
        if (n_tests) atomicAdd(&counts[5], n_tests);
    }
    if (tid == 0) {                                                              // tile decisions are the block's
        if (n_skip) atomicAdd(&counts[3], n_skip);
        if (n_stage) atomicAdd(&counts[4], n_stage);
    }
}

// ---- scratch ----------------------------------------------------------------------------------------------------------------------
struct MapPairScratch { u32 *cnt, *scan; PrimScratch prim; };
size_t layout(MapPairScratch& w, void* base, size_t n_sides) {
    ScratchAlloc a(base);
    a.take_into(n_sides, w.cnt, w.scan);
    w.prim = take_prim(a, n_sides);
    return a.used;
}
// the voxel part comes first and depends on (n_syn, n_sv) alone: it lasts from the voxel stage of one call to the query stage of the
// next over the same scratch, whatever the pair count of either
struct MapQueryScratch { double *pts, *tbox, *sbox; u32 *corner, *icnt, *iscan, *i0, *perm; u64 *key, *skey; size_t n_slots; PrimScratch prim; };
size_t layout(MapQueryScratch& w, void* base, size_t n_syn, size_t n_sv, size_t n_pairs) {
    ScratchAlloc a(base);
    w.n_slots = tile_slots(n_sv, n_syn);
    a.take_into(3 * n_sv, w.pts);
    a.take_into(6 * w.n_slots, w.tbox);
    a.take_into(6 * n_syn, w.sbox);
    a.take_into(3 * n_syn, w.corner);
    a.take_into(n_pairs, w.icnt, w.iscan);
    a.take_into(n_sv, w.i0, w.perm);
    a.take_into(n_sv, w.key, w.skey);
    w.prim = take_prim(a, std::max(n_sv, n_pairs));
    return a.used;
}

bool map_geom(const double* scale, double radius, MapGeom& g) {
    if (!scale || !(radius >= 0.0) || !std::isfinite(radius)) return false;
    for (int a = 0; a < 3; ++a) {
        if (!(scale[a] > 0.0)) return false;
        g.s[a] = scale[a];
    }
    g.r2 = radius * radius;
    g.r2_hi = g.r2 * (1.0 + 1e-9);
    return true;
}

}  // namespace

extern "C" {

size_t sd_synssv_map_pairs_temp_bytes(size_t n_sides) {
    MapPairScratch w;
    return layout(w, nullptr, n_sides ? n_sides : 1);
}

int sd_synssv_map_pairs(const uint64_t* side_cell_dev, const int32_t* syn_rep_dev, size_t n_sides, const uint64_t* org_cell_dev,
                        const uint32_t* org_row_dev, const int32_t* org_rep_dev, size_t n_org, const double* scale_host,
                        double max_rep_dist_nm, uint32_t* side_begin_dev, uint32_t* pair_obj_dev, size_t pair_cap, uint64_t* counts_dev,
                        void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_synssv_map_pairs";
    if (!counts_dev || !side_begin_dev) return fail(who, ": null counts or side_begin");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (n_sides >= LIM31 || (n_sides & 1) || n_org >= LIM31 || pair_cap >= LIM31)
        return fail(who, ": an even number of sides, sides, organelles and pairs < 2^31 per call");
    MapGeom g;
    if (!map_geom(scale_host, max_rep_dist_nm, g)) return fail(who, ": bad scale or distance");
    if (!pair_obj_dev) {
        if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
        if (hipMemsetAsync(side_begin_dev, 0, sizeof(u32), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    }
    if (n_sides == 0) return SD_OK;
    if (!side_cell_dev || !syn_rep_dev || (n_org && (!org_cell_dev || !org_row_dev || !org_rep_dev)))
        return fail(who, ": bad argument");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_synssv_map_pairs_temp_bytes(n_sides), "sd_synssv_map_pairs_temp_bytes(n_sides)"); rc != SD_OK) return rc;
    MapPairScratch w;
    layout(w, temp_dev, n_sides);
    const u64 n = n_sides;
    launch_1d(k_map_pairs, 64 * n, 4096, s, reinterpret_cast<const u64*>(side_cell_dev), syn_rep_dev, n, reinterpret_cast<const u64*>(org_cell_dev),
              org_row_dev, org_rep_dev, (u64)n_org, g, side_begin_dev, w.cnt, pair_obj_dev, (u64)pair_cap);
    if (!pair_obj_dev) {
        if (int rc = scan_u32(who, w.prim, w.cnt, w.scan, n_sides, s); rc != SD_OK) return rc;
        launch_1d(k_map_side_begin, n, 4096, s, w.scan, n, side_begin_dev, counts);
    }
    return launch_status("sd_synssv_map_pairs: launch failed");
}

size_t sd_synssv_map_query_temp_bytes(size_t n_syn, size_t n_sampled_vox, size_t n_pairs) {
    MapQueryScratch w;
    return layout(w, nullptr, n_syn ? n_syn : 1, n_sampled_vox ? n_sampled_vox : 1, n_pairs ? n_pairs : 1);
}

int sd_synssv_map_query(const uint32_t* vox_dev, const uint64_t* vox_begin_dev, const uint64_t* sampled_begin_dev, size_t n_syn, size_t n_vox,
                        size_t n_sampled_vox, const float* vert_dev, const uint64_t* vert_begin_dev, size_t n_org, size_t n_vert,
                        const uint32_t* side_begin_dev, const uint32_t* pair_obj_dev, size_t n_pairs, size_t scratch_pairs, int sample_fact,
                        const double* scale_host, double max_vert_dist_nm, int stages, size_t n_items_hint, uint32_t* pair_close_dev,
                        uint32_t* pair_len_dev, uint64_t* pair_min_d2_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes,
                        void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_synssv_map_query";
    if (!counts_dev) return fail(who, ": null counts");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (n_syn >= LIM31 / 2 || n_sampled_vox >= LIM31 || n_pairs >= LIM31 || n_org >= LIM31 || n_pairs > scratch_pairs || sample_fact < 1)
        return fail(who, ": synapses < 2^30, sampled voxels, organelles and pairs < 2^31 per call, "
                                           "sample_fact >= 1");
    MapGeom g;
    if (!map_geom(scale_host, max_vert_dist_nm, g)) return fail(who, ": bad scale or distance");
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (n_syn == 0 || !(stages & 3)) return SD_OK;
    if (!vox_begin_dev || !sampled_begin_dev || (n_sampled_vox && (!vox_dev || !n_vox)))
        return fail(who, ": bad argument");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_synssv_map_query_temp_bytes(n_syn, n_sampled_vox, scratch_pairs), "sd_synssv_map_query_temp_bytes(...)"); rc != SD_OK)
        return rc;
    MapQueryScratch w;
    layout(w, temp_dev, n_syn, n_sampled_vox ? n_sampled_vox : 1, scratch_pairs ? scratch_pairs : 1);
    const u64 S = n_syn, V = n_sampled_vox, P = n_pairs;
    const u32 f = (u32)sample_fact;
    const u64* vb = reinterpret_cast<const u64*>(vox_begin_dev);
    const u64* svb = reinterpret_cast<const u64*>(sampled_begin_dev);
    if (stages & 1) {
        const int sbits = bits_for(S), b = std::min(10, (64 - sbits) / 3);
        launch_1d(k_map_syn_corner, 64 * S, 4096, s, vox_dev, vb, svb, S, (u64)n_vox, V, f, w.corner, counts);
        if (V) {
            launch_1d(k_map_vox_keys, V, 4096, s, vox_dev, vb, svb, w.corner, S, (u64)n_vox, V, f, b, w.key);
            if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, n_sampled_vox, sbits + 3 * b, s); rc != SD_OK) return rc;
            launch_1d(k_map_vox_place, V, 4096, s, vox_dev, vb, svb, w.skey, w.perm, S, (u64)n_vox, V, f, b, g, w.pts);
        }
        launch_1d(k_tile_boxes<true>, 64 * S, 4096, s, w.pts, svb, S, V, (u64)w.n_slots, w.tbox, w.sbox);
    }
    if ((stages & 2) && P) {
        if (!vert_begin_dev || !side_begin_dev || !pair_obj_dev || !pair_close_dev || !pair_len_dev || !pair_min_d2_dev || !n_org ||
            (n_vert && !vert_dev))
            return fail(who, ": bad argument");
        const u64* vtb = reinterpret_cast<const u64*>(vert_begin_dev);
        u64* pmin = reinterpret_cast<u64*>(pair_min_d2_dev);
        launch_1d(k_map_pair_init, P, 4096, s, pair_obj_dev, vtb, P, (u64)n_org, (u64)n_vert, f, pair_len_dev, pair_close_dev, pmin, w.icnt, counts);
        if (int rc = scan_u32(who, w.prim, w.icnt, w.iscan, n_pairs, s); rc != SD_OK) return rc;
        const u64 want = n_items_hint ? n_items_hint : MAP_QUERY_GRID;
        const int grid = (int)std::min<u64>(want, MAP_QUERY_GRID);
        if (n_vert)
            hipLaunchKernelGGL(k_map_query, dim3(grid), dim3(256), 0, s, vert_dev, vtb, (u64)n_vert, w.pts, svb, V, w.tbox, (u64)w.n_slots, w.sbox,
                               side_begin_dev, 2 * S, pair_obj_dev, pair_len_dev, w.icnt, w.iscan, P, f, g, pair_close_dev, pmin, counts);
    }
    return launch_status("sd_synssv_map_query: launch failed");
}

}  // extern "C"
