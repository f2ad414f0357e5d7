// What the point queries over sorted tables share (sd_synssv_map.hip, sd_syn_props.hip): the float64 distances and the segmented tile
// index.  The searches they walk the tables with are those of sd_tables.h.
//   index     segment s owns points[begin[s] : begin[s + 1]].  A key per point holds the segment number in the high bits and a spatial
//             code below it; sort_by_key (sd_sortseg.h) orders the points and the caller places them in sorted order as float64.
//             Every TILE sorted points of a segment are a tile with one box (min | max); tile t of segment s is slot
//             begin[s] / TILE + s + t of a table of n_points / TILE + n_segments + 1 slots (a segment's first tile starts a new slot
//             whatever begin[s] % TILE is: one spare slot per segment, one for the clamp).  The key and place kernels and the walk
//             over the tiles differ per caller and stay with it; the slot rule is tile_slots / tile_slot0 / tile_box and nowhere else.
//   distances d^2 and the box distance^2 are summed in ONE order with nothing fused, so that a box test never contradicts the point
//             test behind it (see box_dist2).
#pragma once
#include "sd_sortseg.h"
#include <cmath>

namespace {

// ---- distances --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sq_dist(const double* p, const double* q) {
#pragma clang fp contract(off)                              // ((dx dx) + dy dy) + dz dz, no fused multiply-add: cKDTree's own sum
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return ((dx * dx) + dy * dy) + dz * dz;
}
// the same sum over the per-axis gaps to the box (bx = min | max): never above sq_dist of a point inside the box, rounding included
// (every gap is at most the point's |difference| on that axis, and products and sums of non-negative doubles round monotonically)
__device__ __forceinline__ double box_dist2(const double* p, const double* bx) {
#pragma clang fp contract(off)
    const double dx = fmax(0.0, fmax(bx[0] - p[0], p[0] - bx[3])), dy = fmax(0.0, fmax(bx[1] - p[1], p[1] - bx[4])),
                 dz = fmax(0.0, fmax(bx[2] - p[2], p[2] - bx[5]));
    return ((dx * dx) + dy * dy) + dz * dz;
}
// per axis the smallest lo and the largest hi of the wave, in every lane
__device__ __forceinline__ void wave_minmax3(double* lo, double* hi) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int msk = 32; msk; msk >>= 1) { lo[a] = fmin(lo[a], __shfl_xor(lo[a], msk)); hi[a] = fmax(hi[a], __shfl_xor(hi[a], msk)); }
}

// ---- tiles ------------------------------------------------------------------------------------------------------------------------
constexpr int TILE = 64;                                     // sorted points per tile = lanes of a wave

inline size_t tile_slots(size_t n_points, size_t n_segments) { return n_points / TILE + n_segments + 1; }
// slot of the first tile of the segment whose points start at sorted row i0
__device__ __forceinline__ u64 tile_slot0(u64 i0, u64 segment) { return i0 / TILE + segment; }
// the box of tile t of a segment; a slot beyond the table (bad offsets only) reads the last one
__device__ __forceinline__ const double* tile_box(const double* tbox, u64 n_slots, u64 slot0, u64 t) {
    const u64 slot = slot0 + t < n_slots ? slot0 + t : n_slots - 1;
    return tbox + 6 * slot;
}

// one wave per segment: the box of every tile of its sorted points and, with SEG_BOX, of the segment (an empty one: +inf | -inf)
template <bool SEG_BOX>
__global__ __launch_bounds__(256) void k_tile_boxes(const double* __restrict__ pts, const u64* __restrict__ begin, u64 n_segments, u64 n_points,
                                                    u64 n_slots, double* tbox, double* sbox) {
    const int lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * 256) >> 6;
    for (u64 s = wave; s < n_segments; s += n_waves) {
        const u64 i1 = begin[s + 1] < n_points ? begin[s + 1] : n_points, i0 = begin[s] < i1 ? begin[s] : i1;
        double slo[3] = {INFINITY, INFINITY, INFINITY}, shi[3] = {-INFINITY, -INFINITY, -INFINITY};
        u64 slot = tile_slot0(i0, s);
        for (u64 t0 = i0; t0 < i1; t0 += TILE, ++slot) {
            const u64 i = t0 + lane;
            double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            if (i < i1)
#pragma unroll
                for (int a = 0; a < 3; ++a) lo[a] = hi[a] = pts[3 * i + a];
            wave_minmax3(lo, hi);
            if (SEG_BOX)
#pragma unroll
                for (int a = 0; a < 3; ++a) { slo[a] = fmin(slo[a], lo[a]); shi[a] = fmax(shi[a], hi[a]); }
            if (lane == 0 && slot < n_slots)
#pragma unroll
                for (int a = 0; a < 3; ++a) { tbox[6 * slot + a] = lo[a]; tbox[6 * slot + 3 + a] = hi[a]; }
        }
        if (SEG_BOX && lane == 0)
#pragma unroll
            for (int a = 0; a < 3; ++a) { sbox[6 * s + a] = slo[a]; sbox[6 * s + 3 + a] = shi[a]; }
    }
}

}  // namespace
