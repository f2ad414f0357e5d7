// Rendering locations of ALL objects of a vertex table in one call: the array form of what the reference does per supervoxel in
// SegmentationObject.sample_locations (reps/segmentation.py:700-732), one open3d call or one cKDTree + one histogramdd each
// (batchjob_sample_location_caching.py).  Object s owns verts[begin[s] : begin[s + 1]], as MeshTable.vert_begin lays them out.
//
//   voxel    generate_rendering_locs (handler/multiviews.py:339-355): open3d's voxel_down_sample as open3d publishes it.  Per object in
//            float64: vmin = min - 0.5 ds per axis; a vertex falls into voxel floor((p - vmin) / ds) (one subtraction, one division, one
//            floor); a location is the sum of the voxel's vertices in ASCENDING VERTEX ORDER, starting from 0, divided by their number.
//            Locations ascend by voxel (ix, iy, iz), x most significant (open3d: the order of a hash map).
//   surface  surface_samples (reps/rep_helper.py:376-417) for float32 vertices.  Per object: off = min, c = fl32(v - off), mx = max c,
//            nb = max(1, ceil(mx / bin_size)); the bin of a vertex is numpy's histogramdd over float32 edges e_j = fl32(fl32(j) step),
//            step = fl32(mx / fl32(nb)), e_nb = mx: the number of edges <= c, minus one, c == mx in the last bin, one bin where mx == 0.
//            Every occupied bin in C order of (bx, by, bz): the centre (b + 0.5) bin_size in float64 (bin_size, not mx / nb: the
//            reference's quirk), the vertex p nearest to it in float64 (lowest vertex index among equidistant ones), the ball of all
//            vertices with ((dx dx) + dy dy) + dz dz <= r r around p, their float32 sum IN ASCENDING VERTEX ORDER, one float32
//            division by the count, + off in float32.
//
//   both     k_loc_boxes  one wave per object: min / max, non-finite vertices and the extent limit flagged (the offsets: k_check_offsets
//                         of sd_tables.h).
//            keys         voxel / bin of every vertex packed into 3 x 21 bits.  Two stable sorts (sd_sortseg.h): by that key, then by
//                         object.  Within a run of equal (object, key) the vertices then ascend by their index.
//            runs         head flags over (object, key) and their scan: a run is a location.  The objects keep their vertex ranges in
//                         the sorted order, so loc_begin[s] is the scan in front of begin[s]: no second scan, no count per object.
//   voxel    one LANE per run adds its vertices in order.  An in-order sum has no parallel form; a wave per run would only spread the
//            loads.  Not measured against that.
//   surface  one WAVE per run.  The tiles of sd_pointtiles.h (slot rule, k_tile_boxes, box_dist2, sq_dist as they are) are cut over the
//            vertices IN VERTEX ORDER, not in Morton order: marching-cubes vertices ascend by grid edge, so 64 consecutive ones are a
//            thin slab piece, and a walk over the tiles in ascending order meets the members of a ball in ascending vertex order.  The
//            float32 sum is then taken as the members appear: no emit, no segmented sort of the members, no second scan.  Morton tiles
//            would prune better and need exactly those three.  Which is faster has not been measured.  The nearest vertex is decided
//            by (d^2, index), a total order: the result depends neither on the tiling nor on the visit order.
//
// The grid constants rest on no measurement.  Every index read from device memory is clamped before it is used.  No float atomics, no
// inline assembly.
#include "../../include/syconn_dense.h"
#include "sd_sortseg.h"
#include "sd_pointtiles.h"

namespace {

constexpr int AX_BITS = 21;                                  // key bits per axis
constexpr u64 AX_MASK = ((u64)1 << AX_BITS) - 1;
constexpr u32 NO_IX = 0xffffffffu;
static_assert(((u64)1 << AX_BITS) == SD_LOCATIONS_MAX_CELLS, "the extent limit of the header is the key packing");
static_assert(TILE == 64, "one point of a tile per lane");

struct Bins { float bs[3]; };                                // bin sizes of the surface rule

__device__ __forceinline__ double ld_vert(const void* v, int f32, u64 i) {
    return f32 ? (double)reinterpret_cast<const float*>(v)[i] : reinterpret_cast<const double*>(v)[i];
}
__device__ __forceinline__ u64 pack3(u64 x, u64 y, u64 z) { return (x << (2 * AX_BITS)) | (y << AX_BITS) | z; }

// ---- the surface rule's histogram ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 n_bins(float mx, float bs) {
    const float q = ceilf(mx / bs);
    return q >= 1.f ? (q < (float)SD_LOCATIONS_MAX_CELLS ? (u32)q : (u32)SD_LOCATIONS_MAX_CELLS) : 1u;        // NaN -> 1
}
// histogramdd's bin of c in [0, mx]: edges ascend, so the number of edges <= c is a binary search
__device__ __forceinline__ u32 bin_of(float c, float mx, float bs) {
#pragma clang fp contract(off)
    if (!(mx > 0.f)) return 0;                               // edges -0.5 | 0.5
    const u32 nb = n_bins(mx, bs);
    const float step = mx / (float)nb;
    u32 lo = 0, hi = nb + 1;
    while (lo < hi) {
        const u32 mid = lo + (hi - lo) / 2;
        const float e = mid == nb ? mx : (float)mid * step;
        if (e <= c) lo = mid + 1; else hi = mid;
    }
    const u32 b = lo ? lo - 1 : 0;
    return b < nb ? b : nb - 1;                              // c == mx: the last bin
}

// ---- per object: ob[8 s + ...] = voxel: vmin[3] (= min - ds / 2); surface: off[3], mx[3] (float32 values) -----------------------------
template <bool SURFACE>
__global__ __launch_bounds__(256) void k_loc_boxes(const void* __restrict__ verts, int f32, const u64* __restrict__ begin, u64 n_obj, u64 n, double ds,
                                                   Bins B, double* ob, u64* counts) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const u64 wave = grid_tid() >> 6, n_waves = grid_stride() >> 6;
    for (u64 s = wave; s < n_obj; s += n_waves) {
        const u64 b1 = clamp_u64(begin[s + 1], n), b0 = clamp_u64(begin[s], b1);       // k_check_offsets has flagged a bad table
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        bool wild = false;
        for (u64 i = b0 + lane; i < b1; i += 64)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double v = ld_vert(verts, f32, 3 * i + a);
                    if (!(fabs(v) < INFINITY)) wild = true;
                    lo[a] = fmin(lo[a], v); hi[a] = fmax(hi[a], v);
                }
        wave_minmax3(lo, hi);
        wild = __ballot(wild) != 0;
        if (lane == 0) {
            const bool empty = b1 == b0;
            bool over = false;
            double o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (!empty && !wild)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if (SURFACE) {
                        const float off = (float)lo[a], mx = (float)hi[a] - off;           // = max fl32(v - off): rounding is monotonic
                        o[a] = off; o[3 + a] = mx;
                        if (!(mx / B.bs[a] <= (float)SD_LOCATIONS_MAX_CELLS)) over = true;
                    } else {
                        const double vmin = lo[a] - 0.5 * ds;
                        o[a] = vmin;
                        if (!(floor((hi[a] - vmin) / ds) < (double)SD_LOCATIONS_MAX_CELLS)) over = true;
                    }
                }
#pragma unroll
            for (int a = 0; a < 8; ++a) ob[8 * s + a] = o[a];
            if (wild) counts[5] = 1;
            if (over) counts[4] = 1;
        }
    }
}

template <bool SURFACE>
__global__ __launch_bounds__(256) void k_loc_keys(const void* __restrict__ verts, int f32, const u64* __restrict__ begin, const double* __restrict__ ob,
                                                  u64 n_obj, u64 n, double ds, Bins B, u64* key) {
#pragma clang fp contract(off)
    for (u64 j = grid_tid(); j < n; j += grid_stride()) {
        const u64 s = segment_of(begin, n_obj, j);
        u64 ix[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (SURFACE) {
                const float c = reinterpret_cast<const float*>(verts)[3 * j + a] - (float)ob[8 * s + a];
                ix[a] = bin_of(c, (float)ob[8 * s + 3 + a], B.bs[a]);
            } else {
                const double q = floor((ld_vert(verts, f32, 3 * j + a) - ob[8 * s + a]) / ds);
                ix[a] = q > 0.0 ? (q < (double)AX_MASK ? (u64)q : AX_MASK) : 0;             // NaN -> 0
            }
        }
        key[j] = pack3(ix[0], ix[1], ix[2]);
    }
}
__global__ __launch_bounds__(256) void k_loc_objkeys(const u32* __restrict__ perm, const u64* __restrict__ begin, u64 n_obj, u64 n, u64* okey) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) okey[i] = segment_of(begin, n_obj, clamp_u64(perm[i], n - 1));
}
__global__ __launch_bounds__(256) void k_loc_gather(const u64* __restrict__ key, const u32* __restrict__ perm, u64 n, u64* out) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) out[i] = key[clamp_u64(perm[i], n - 1)];
}
// loc_begin[s] = runs in front of begin[s]; counts[0] = all runs; counts[1]: the capacity of an emitting call is smaller
__global__ __launch_bounds__(256) void k_loc_begin(const u64* __restrict__ begin, const u32* __restrict__ seg, u64 n_obj, u64 n, u64 cap, int emit,
                                                   u64* loc_begin, u64* counts) {
    for (u64 s = grid_tid(); s <= n_obj; s += grid_stride()) {
        const u64 b = s == n_obj ? n : clamp_u64(begin[s], n);
        loc_begin[s] = b ? seg[b - 1] : 0;
        if (s == n_obj) {
            counts[0] = seg[n - 1];
            if (emit && seg[n - 1] > cap) counts[1] = 1;
        }
    }
}
__global__ __launch_bounds__(256) void k_loc_runs(const u32* __restrict__ head, const u32* __restrict__ seg, u64 n, u32* run_pos) {
    for (u64 i = grid_tid(); i < n; i += grid_stride())
        if (head[i]) run_pos[clamp_u64(seg[i] - 1, n - 1)] = (u32)i;
}

// ---- voxel rule: one lane per run ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_loc_voxel_emit(const void* __restrict__ verts, int f32, const u32* __restrict__ perm, const u32* __restrict__ head,
                                                        const u32* __restrict__ seg, u64 n, u64 cap, double* loc) {
#pragma clang fp contract(off)
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        if (!head[i]) continue;
        const u64 r = seg[i] - 1;
        if (r >= cap) continue;
        double sum[3] = {0.0, 0.0, 0.0};
        u64 k = 0, j = i;
        do {
            const u64 v = clamp_u64(perm[j], n - 1);
#pragma unroll
            for (int a = 0; a < 3; ++a) sum[a] += ld_vert(verts, f32, 3 * v + a);
            ++k; ++j;
        } while (j < n && !head[j]);
#pragma unroll
        for (int a = 0; a < 3; ++a) loc[3 * r + a] = sum[a] / (double)k;
    }
}

// ---- surface rule -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_loc_place(const float* __restrict__ verts, const u64* __restrict__ begin, const double* __restrict__ ob, u64 n_obj,
                                                   u64 n, double* spts) {
#pragma clang fp contract(off)
    for (u64 j = grid_tid(); j < n; j += grid_stride()) {
        const u64 s = segment_of(begin, n_obj, j);
#pragma unroll
        for (int a = 0; a < 3; ++a) spts[3 * j + a] = (double)(verts[3 * j + a] - (float)ob[8 * s + a]);       // float32 widens exactly
    }
}

__device__ __forceinline__ bool before(double d, u32 ix, double kd, u32 ki) { return d < kd || (d == kd && ix < ki); }

// the points of one tile (rows t0 .. t0 + 63 below i1) against the best so far; the result is the same in every lane
__device__ __forceinline__ void nearest_visit(const double* __restrict__ spts, u64 t0, u64 i1, const double* q, int lane, double& best, u32& bix) {
    const u64 i = t0 + lane;
    double d = INFINITY;
    u32 ix = NO_IX;
    if (i < i1) {
        const double p[3] = {spts[3 * i], spts[3 * i + 1], spts[3 * i + 2]};
        d = sq_dist(p, q);
        ix = (u32)i;
    }
    for (int msk = 32; msk; msk >>= 1) {
        const double od = __shfl_xor(d, msk);
        const u32 oi = (u32)__shfl_xor((int)ix, msk);
        if (before(od, oi, d, ix)) { d = od; ix = oi; }
    }
    if (before(d, ix, best, bix)) { best = d; bix = ix; }
}

__global__ __launch_bounds__(256) void k_loc_surface_emit(const double* __restrict__ spts, const u64* __restrict__ begin, u64 n_obj, u64 n,
                                                          const double* __restrict__ tbox, u64 n_slots, const double* __restrict__ ob,
                                                          const u64* __restrict__ okey, const u64* __restrict__ vkey, const u32* __restrict__ run_pos,
                                                          const u32* __restrict__ seg, Bins B, double r2, u64 cap, float* loc, u64* counts) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const u64 wave = grid_tid() >> 6, n_waves = grid_stride() >> 6;
    u64 n_visit = 0, n_skip = 0;
    const u64 n_runs = seg[n - 1] < cap ? seg[n - 1] : cap;                           // past the capacity nothing is written
    for (u64 r = wave; r < n_runs; r += n_waves) {
        const u64 i = clamp_u64(run_pos[r], n - 1), s = clamp_u64(okey[i], n_obj - 1), k = vkey[i];
        const u64 i1 = clamp_u64(begin[s + 1], n), i0 = clamp_u64(begin[s], i1);
        const u64 n_tiles = (i1 - i0 + TILE - 1) / TILE, slot0 = tile_slot0(i0, s);
        const double q[3] = {((double)((k >> (2 * AX_BITS)) & AX_MASK) + 0.5) * (double)B.bs[0], ((double)((k >> AX_BITS) & AX_MASK) + 0.5) * (double)B.bs[1],
                             ((double)(k & AX_MASK) + 0.5) * (double)B.bs[2]};
        // ---- the vertex nearest to the bin centre: the tile with the nearest box first, then every tile whose box is not farther
        double bd = INFINITY;
        u64 bt = 0;
        for (u64 t = lane; t < n_tiles; t += 64) {
            const double d = box_dist2(q, tile_box(tbox, n_slots, slot0, t));
            if (d < bd) { bd = d; bt = t; }
        }
        for (int msk = 32; msk; msk >>= 1) {
            const double od = __shfl_xor(bd, msk);
            const u64 ot = __shfl_xor(bt, msk);
            if (od < bd || (od == bd && ot < bt)) { bd = od; bt = ot; }
        }
        double best = INFINITY;
        u32 bix = NO_IX;
        if (n_tiles) { nearest_visit(spts, i0 + bt * TILE, i1, q, lane, best, bix); ++n_visit; }
        for (u64 t0 = 0; t0 < n_tiles; t0 += 64) {
            const u64 t = t0 + lane;
            const bool live = t < n_tiles && t != bt;
            double d = INFINITY;
            if (live) d = box_dist2(q, tile_box(tbox, n_slots, slot0, t));
            u64 m = __ballot(live && !(d > best));                                   // equal: a lower index may still be inside
            n_skip += (u64)__popcll(__ballot(live)) - (u64)__popcll(m);
            while (m) {
                const int b = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                if (__shfl(d, b) > best) { ++n_skip; continue; }
                nearest_visit(spts, i0 + (t0 + b) * TILE, i1, q, lane, best, bix);
                ++n_visit;
            }
        }
        if (bix == NO_IX) continue;                                                  // an object without vertices has no run
        const u64 pi = clamp_u64(bix, n - 1);
        const double p[3] = {spts[3 * pi], spts[3 * pi + 1], spts[3 * pi + 2]};
        // ---- the ball around p: tiles and their points in ascending order, the float32 sum as the members appear
        float sum[3] = {0.f, 0.f, 0.f};
        u32 cnt = 0;
        for (u64 t0 = 0; t0 < n_tiles; t0 += 64) {
            const u64 t = t0 + lane;
            double d = INFINITY;
            if (t < n_tiles) d = box_dist2(p, tile_box(tbox, n_slots, slot0, t));
            u64 m = __ballot(t < n_tiles && d <= r2);
            n_skip += (u64)__popcll(__ballot(t < n_tiles)) - (u64)__popcll(m);
            while (m) {
                const int b = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                ++n_visit;
                const u64 j = i0 + (t0 + b) * TILE + lane;
                float c[3] = {0.f, 0.f, 0.f};
                double d2 = INFINITY;
                if (j < i1) {
                    const double w[3] = {spts[3 * j], spts[3 * j + 1], spts[3 * j + 2]};
                    d2 = sq_dist(w, p);
                    c[0] = (float)w[0]; c[1] = (float)w[1]; c[2] = (float)w[2];
                }
                u64 mm = __ballot(j < i1 && d2 <= r2);
                while (mm) {                                                         // mm and the sums are the same in every lane
                    const int l = __ffsll((unsigned long long)mm) - 1;
                    mm &= mm - 1;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const float x = __shfl(c[a], l);
                        sum[a] = cnt ? sum[a] + x : x;
                    }
                    ++cnt;
                }
            }
        }
        if (lane < 3) {
            const float sa = lane == 0 ? sum[0] : (lane == 1 ? sum[1] : sum[2]);
            loc[3 * r + lane] = sa / (float)cnt + (float)ob[8 * s + lane];
        }
    }
    if (lane == 0) {
        if (n_visit) atomicAdd(&counts[2], n_visit);
        if (n_skip) atomicAdd(&counts[3], n_skip);
    }
}

// ---- scratch ------------------------------------------------------------------------------------------------------------------------
struct LocScratch { double *ob, *spts, *tbox; u64 *key, *skey, *okey, *sokey; u32 *i0, *perm, *perm2, *head, *seg, *run_pos; size_t n_slots; PrimScratch prim; };
size_t layout(LocScratch& w, void* base, size_t n, size_t n_obj, bool surface) {
    ScratchAlloc a(base);
    w.n_slots = tile_slots(n, n_obj);
    a.take_into(8 * n_obj, w.ob);
    a.take_into(n, w.key, w.skey, w.okey, w.sokey);
    a.take_into(n, w.i0, w.perm, w.perm2, w.head, w.seg, w.run_pos);
    w.spts = w.tbox = nullptr;
    if (surface) { a.take_into(3 * n, w.spts); a.take_into(6 * w.n_slots, w.tbox); }
    w.prim = take_prim(a, n);
    return a.used;
}

// what both rules share: the checks, the boxes, the keys, the two sorts, the runs and loc_begin.  *done: nothing is left to emit.
template <bool SURFACE>
int runs(const char* who, const void* verts_dev, int f32, const u64* begin, size_t n_obj, size_t n_verts, double ds, const Bins& B, u64* loc_begin,
         const void* loc_dev, size_t loc_cap, u64* counts, void* temp_dev, size_t temp_bytes, size_t need, const char* query, LocScratch& w, bool* done,
         hipStream_t s) {
    *done = true;
    if (!counts || !loc_begin) return fail(who, ": null counts or offsets");
    if (n_verts >= LIM31 || n_obj >= LIM31 || loc_cap >= LIM31) return fail(who, ": vertices, objects and locations < 2^31 per call");
    if (loc_cap && !loc_dev) return fail(who, ": bad argument");
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (hipMemsetAsync(loc_begin, 0, (n_obj + 1) * sizeof(u64), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    if (n_obj == 0) return n_verts ? fail(who, ": vertices without objects") : SD_OK;
    if (!begin || (n_verts && !verts_dev)) return fail(who, ": bad argument");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, need, query); rc != SD_OK) return rc;
    layout(w, temp_dev, n_verts ? n_verts : 1, n_obj, SURFACE);
    const u64 N = n_verts, Cn = n_obj;
    launch_1d(k_check_offsets, Cn, SD_LOCATIONS_GRID, s, begin, Cn, N, counts);
    launch_1d(k_loc_boxes<SURFACE>, 64 * Cn, SD_LOCATIONS_WAVE_GRID, s, verts_dev, f32, begin, Cn, N, ds, B, w.ob, counts);
    if (N == 0) return launch_status((std::string(who) + ": launch failed").c_str());
    launch_1d(k_loc_keys<SURFACE>, N, SD_LOCATIONS_GRID, s, verts_dev, f32, begin, w.ob, Cn, N, ds, B, w.key);
    if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, n_verts, 3 * AX_BITS, s); rc != SD_OK) return rc;
    launch_1d(k_loc_objkeys, N, SD_LOCATIONS_GRID, s, w.perm, begin, Cn, N, w.okey);
    if (int rc = sort_carry(who, w.prim, w.okey, w.sokey, w.perm, w.perm2, n_verts, std::max(bits_for(Cn), 1), s); rc != SD_OK) return rc;
    launch_1d(k_loc_gather, N, SD_LOCATIONS_GRID, s, w.key, w.perm2, N, w.skey);
    if (int rc = number_segments(who, w.prim, w.sokey, w.skey, w.head, w.seg, n_verts, s); rc != SD_OK) return rc;
    launch_1d(k_loc_begin, Cn + 1, SD_LOCATIONS_GRID, s, begin, w.seg, Cn, N, (u64)loc_cap, loc_cap ? 1 : 0, loc_begin, counts);
    *done = loc_cap == 0;
    return launch_status((std::string(who) + ": launch failed").c_str());
}

}  // namespace

extern "C" {

size_t sd_locations_voxel_temp_bytes(size_t n_verts, size_t n_obj) {
    LocScratch w;
    return layout(w, nullptr, n_verts ? n_verts : 1, n_obj ? n_obj : 1, false);
}
int sd_locations_voxel(const void* verts_dev, int verts_f32, const uint64_t* vert_begin_dev, size_t n_obj, size_t n_verts, double ds,
                       uint64_t* loc_begin_dev, double* loc_dev, size_t loc_cap, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_locations_voxel";
    if (!(ds > 0.0) || !(ds < INFINITY)) return fail(who, ": the voxel size must be positive and finite");
    LocScratch w;
    bool done;
    const int f32 = verts_f32 ? 1 : 0;
    if (int rc = runs<false>(who, verts_dev, f32, reinterpret_cast<const u64*>(vert_begin_dev), n_obj, n_verts, ds, Bins{{1.f, 1.f, 1.f}},
                             reinterpret_cast<u64*>(loc_begin_dev), loc_dev, loc_cap, reinterpret_cast<u64*>(counts_dev), temp_dev, temp_bytes,
                             sd_locations_voxel_temp_bytes(n_verts, n_obj), "sd_locations_voxel_temp_bytes(n_verts, n_obj)", w, &done, s);
        rc != SD_OK || done)
        return rc;
    launch_1d(k_loc_voxel_emit, n_verts, SD_LOCATIONS_GRID, s, verts_dev, f32, w.perm2, w.head, w.seg, (u64)n_verts, (u64)loc_cap, loc_dev);
    return launch_status("sd_locations_voxel: launch failed");
}

size_t sd_locations_surface_temp_bytes(size_t n_verts, size_t n_obj) {
    LocScratch w;
    return layout(w, nullptr, n_verts ? n_verts : 1, n_obj ? n_obj : 1, true);
}
int sd_locations_surface(const float* verts_dev, const uint64_t* vert_begin_dev, size_t n_obj, size_t n_verts, const float* bin_sizes3, double r,
                         uint64_t* loc_begin_dev, float* loc_dev, size_t loc_cap, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_locations_surface";
    if (!bin_sizes3) return fail(who, ": bad argument");
    Bins B;
    for (int a = 0; a < 3; ++a) {
        if (!(bin_sizes3[a] > 0.f) || !(bin_sizes3[a] < INFINITY)) return fail(who, ": the bin sizes must be positive and finite");
        B.bs[a] = bin_sizes3[a];
    }
    if (!(r >= 0.0) || !(r < INFINITY)) return fail(who, ": the radius must be finite and not negative");
    LocScratch w;
    bool done;
    const u64* begin = reinterpret_cast<const u64*>(vert_begin_dev);
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = runs<true>(who, verts_dev, 1, begin, n_obj, n_verts, 0.0, B, reinterpret_cast<u64*>(loc_begin_dev), loc_dev, loc_cap, counts, temp_dev,
                            temp_bytes, sd_locations_surface_temp_bytes(n_verts, n_obj), "sd_locations_surface_temp_bytes(n_verts, n_obj)", w, &done, s);
        rc != SD_OK || done)
        return rc;
    const u64 N = n_verts, Cn = n_obj;
    launch_1d(k_loc_runs, N, SD_LOCATIONS_GRID, s, w.head, w.seg, N, w.run_pos);
    launch_1d(k_loc_place, N, SD_LOCATIONS_GRID, s, verts_dev, begin, w.ob, Cn, N, w.spts);
    launch_1d(k_tile_boxes<false>, 64 * Cn, SD_LOCATIONS_WAVE_GRID, s, w.spts, begin, Cn, N, (u64)w.n_slots, w.tbox, (double*)nullptr);
    // one wave per run: at most min(n_verts, loc_cap) of them, the kernel reads their number from the scan
    launch_1d(k_loc_surface_emit, 64 * std::min<u64>(N, loc_cap), SD_LOCATIONS_WAVE_GRID, s, w.spts, begin, Cn, N, w.tbox, (u64)w.n_slots, w.ob, w.sokey,
              w.skey, w.run_pos, w.seg, B, r * r, (u64)loc_cap, loc_dev, counts);
    return launch_status("sd_locations_surface: launch failed");
}

}  // extern "C"
