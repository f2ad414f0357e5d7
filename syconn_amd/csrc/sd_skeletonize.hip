// Cell skeletons from a labelled chunk on the device: the TEASAR tracing that proc/skeleton.py:21-86 (kimimaro_skelgen) gets from
// kimimaro.skeletonize, restated by rule (kimimaro itself is not part of the reference tree, so nothing here is pinned
// against it -- the device equals the float64 / float32 CPU restatement of the same rules bit for bit).  The stages and their entries:
//     components of equal label, 26-connected, dust removed, numbered by first voxel      -> sd_skeletonize_components
//     exact squared anisotropic distance to the nearest voxel of another component, DBF   -> sd_skeletonize_d2
//     single-source float32 distance fields (DAF0 from the first voxel, DAF from the root) and the float64 penalised field: start state
//     and tiled relaxation to the fixed point                                             -> sd_skeletonize_field_start, sd_skeletonize_relax
//     per-component argmax with the smallest raster index on ties (root, DAF maximum, the round's target) -> sd_skeletonize_argmax
//     the penalty field p                                                                 -> sd_skeletonize_penalty
//     one round of tree growth: walk from the target to the tree, join the path, invalidate around the new nodes -> sd_skeletonize_round
//     nodes, edges, radii per component                                                   -> sd_skeletonize_emit
// All volumes are (X, Y, Z) with z fastest; the raster index of a voxel is (x Y + y) Z + z, below 2^31.
//
// Every loop is bounded.  Nothing here iterates "until nothing changes" across workgroups inside one launch: a relaxation sweep is ONE launch
// that relaxes every dirty tile to LOCAL convergence in LDS (at most SD_SKELETONIZE_TILE^3 + 1 Jacobi steps: a value that is final after k
// steps has a shortest path of k hops inside the tile), writes the tile's own voxels back and marks the neighbour tiles whose halo changed
// for the NEXT launch.  A tile writes only its own voxels and only reads its halo, so no read-modify-write on the field is needed (the halo loads
// and the stores are relaxed atomics of agent scope, which makes the concurrent access defined), and a halo value read
// while the neighbour stores is either the old or the new one: both are upper bounds, and the neighbour's mark makes this tile run again
// after the kernel boundary.  sd_skeletonize_relax enqueues the number of sweeps its caller asks for (a launch with no dirty tile returns
// at once) and reports the dirty tiles that remain; the caller continues from there (values only fall, so the warm start reaches the same
// fixed point) and stops at its own bound, foreground voxels + 1 sweeps.  No kernel waits for a flag that another workgroup sets.
// The walk of a round is one thread per component (a path is sequential) and at most `size of the component` steps long.
// Floating point: every operation rounded once, never fused (fp contract off), as sd_pointtiles.h / sd_spinehead.hip do.
// Unmeasured choices, stated as such: the tile edge 16 (46 KiB of float64 with the halo, 23 KiB of component numbers, which fits
// twice into the 160 KiB of a CU; whether two workgroups are resident was not checked), dirty FLAGS walked by every launch rather than a compacted work list, the argmax by 64-bit atomic maxima rather than a segmented
// reduction, and the invalidation as one clipped box fill per new node: three axis passes that keep a per-voxel maximum of r are exact for
// one component only, and here the boxes of different components overlap in one volume.
#include "../../include/syconn_dense.h"
#include "sd_sortseg.h"
#include <math.h>
#include <stdint.h>

namespace {

constexpr int T = SD_SKELETONIZE_TILE, TH = T + 2, TVOL = TH * TH * TH;
constexpr int VG = SD_SKELETONIZE_VOX_GRID, TG = SD_SKELETONIZE_TILE_GRID, CG = SD_SKELETONIZE_COMP_GRID, NG = SD_SKELETONIZE_NODE_GRID;
constexpr u64 INF64 = ~0ull;

struct Geo { int X, Y, Z, tx, ty, tz; };
struct Len { float v[27]; };        // len(o) by (ox + 1) * 9 + (oy + 1) * 3 + (oz + 1); the centre is unused
struct W3 { int v[3]; };

__device__ __forceinline__ void dec3(u64 i, int Y, int Z, int& x, int& y, int& z) {
    const unsigned u = (unsigned)i, r = u / (unsigned)Z, q = r / (unsigned)Y;
    z = (int)(u - r * (unsigned)Z); y = (int)(r - q * (unsigned)Y); x = (int)q;
}

// ---- a. components ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sk_cc_init(const uint64_t* __restrict__ seg, u64 nvox, int* __restrict__ L, u32* __restrict__ cnt) {
    for (u64 i = grid_tid(); i < nvox; i += grid_stride()) { L[i] = seg[i] ? (int)i : -1; cnt[i] = 0; }
}
// the 13 neighbours that precede a voxel in raster order; equal labels unite (two labels never do, whatever their contact)
__global__ __launch_bounds__(256) void k_sk_cc_union(const uint64_t* __restrict__ seg, int X, int Y, int Z, int* L) {
    const u64 nvox = (u64)X * Y * Z;
    for (u64 i = grid_tid(); i < nvox; i += grid_stride()) {
        const uint64_t l = seg[i];
        if (!l) continue;
        int x, y, z;
        dec3(i, Y, Z, x, y, z);
        for (int k = 0; k < 13; ++k) {
            const int ox = k / 9 - 1, oy = (k / 3) % 3 - 1, oz = k % 3 - 1;
            const int xx = x + ox, yy = y + oy, zz = z + oz;
            if (xx < 0 || yy < 0 || yy >= Y || zz < 0 || zz >= Z) continue;
            const u64 j = ((u64)xx * Y + yy) * Z + zz;
            if (seg[j] == l) uf_union(L, (int)i, (int)j);
        }
    }
}
__global__ __launch_bounds__(256) void k_sk_cc_flatten(u64 nvox, int* L, u32* cnt) {
    for (u64 i = grid_tid(); i < nvox; i += grid_stride()) {
        if (L[i] < 0) continue;
        const int r = uf_find(L, (int)i);
        atomicAdd(cnt + r, 1u);      // (L keeps its chains here: a store would race with the finds of other threads)
    }
}
__global__ __launch_bounds__(256) void k_sk_cc_flag(u64 nvox, const int* __restrict__ L, const u32* __restrict__ cnt, u64 dust, u32* __restrict__ flag) {
    for (u64 i = grid_tid(); i < nvox; i += grid_stride()) flag[i] = (L[i] == (int)i && (u64)cnt[i] >= dust) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_sk_cc_number(const uint64_t* __restrict__ seg, u64 nvox, const int* L, const u32* __restrict__ cnt,
                                                     const u32* __restrict__ flag, const u32* __restrict__ pos, u64 cap, int* __restrict__ comp,
                                                     uint64_t* __restrict__ sizes, uint64_t* __restrict__ labels, int* __restrict__ first, u64* counts) {
    for (u64 i = grid_tid(); i < nvox; i += grid_stride()) {
        if (i == nvox - 1) counts[0] = pos[i];
        int c = 0;
        if (L[i] >= 0) {
            const int r = uf_find(L, (int)i);
            if (flag[r] && (u64)pos[r] <= cap) c = (int)pos[r];
            if (flag[r] && (u64)pos[r] > cap) counts[7] = 1;
            if (c && r == (int)i) { sizes[c] = cnt[i]; labels[c] = seg[i]; first[c] = (int)i; }
        }
        comp[i] = c;
    }
}

// ---- b. distance to the boundary -------------------------------------------------------------------------------------------------------
// one axis pass: candidates are the voxels of the contiguous same-component run through v (their value of the pass before + the squared
// step) and the first voxel of another component beyond each end (the squared step alone); the array border is no boundary
__global__ __launch_bounds__(256) void k_sk_d2_axis(const int* __restrict__ comp, const u64* __restrict__ in, u64* __restrict__ out, int X, int Y, int Z,
                                                    int axis, u64 w2) {
    const u64 nvox = (u64)X * Y * Z;
    const int n = axis == 0 ? X : (axis == 1 ? Y : Z);
    const long long stride = axis == 0 ? (long long)Y * Z : (axis == 1 ? Z : 1);
    for (u64 i = grid_tid(); i < nvox; i += grid_stride()) {
        const int c = comp[i];
        if (c <= 0) { out[i] = 0; continue; }
        int co[3];
        dec3(i, Y, Z, co[0], co[1], co[2]);
        const int pos = co[axis];
        u64 best = in ? in[i] : INF64;
        for (int dir = -1; dir <= 1; dir += 2)
            for (int k = 1; k < n; ++k) {          // (bounded by the extent)
                const int q = pos + dir * k;
                if (q < 0 || q >= n) break;
                const u64 dd = w2 * (u64)k * (u64)k;
                if (dd >= best) break;             // every later candidate of this direction is at least dd
                const u64 j = (u64)((long long)i + (long long)dir * k * stride);
                if (comp[j] != c) { best = dd; break; }
                if (in) {
                    const u64 g = in[j];
                    if (g != INF64 && g + dd < best) best = g + dd;
                }
            }
        out[i] = best;
    }
}
__global__ __launch_bounds__(256) void k_sk_dbf(const int* __restrict__ comp, const u64* __restrict__ d2, u64 nvox, float* __restrict__ dbf, u32* dbf_max,
                                               u64* counts) {
    for (u64 i = grid_tid(); i < nvox; i += grid_stride()) {
        const int c = comp[i];
        float f = 0.0f;
        if (c > 0) {
            const u64 d = d2[i];
            if (d == INF64) { counts[1] = 1; f = __builtin_inff(); }
            else {
                f = (float)sqrt((double)d);
                if (__float_as_uint(f) > __hip_atomic_load(dbf_max + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dbf_max + c, __float_as_uint(f));
            }
        }
        dbf[i] = f;
    }
}

// ---- the relaxation state: dirty flags of the tiles, double buffered, and three rotating counters of set flags ---------------------------
// sweep s reads flags[s & 1] / cnt[s % 3], sets flags[(s + 1) & 1] / cnt[(s + 1) % 3] and clears cnt[(s + 2) % 3]; an entry runs a
// multiple of six sweeps, so every entry starts at buffer 0
struct Relax { int* flags[2]; u32* cnt; };

__device__ __forceinline__ void mark_tile(int* flags, u32* cnt, int t) {
    if (__hip_atomic_load(flags + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 && atomicExch(flags + t, 1) == 0) atomicAdd(cnt, 1u);
}
// the tile of voxel i and its up to 26 neighbours (a source on a tile face changes the halo of the tile beyond)
__device__ __forceinline__ void mark_around(const Geo& g, int* flags, u32* cnt, u64 i) {
    int x, y, z;
    dec3(i, g.Y, g.Z, x, y, z);
    const int ax = x / T, ay = y / T, az = z / T;
    for (int k = 0; k < 27; ++k) {
        const int bx = ax + k / 9 - 1, by = ay + (k / 3) % 3 - 1, bz = az + k % 3 - 1;
        if (bx < 0 || by < 0 || bz < 0 || bx >= g.tx || by >= g.ty || bz >= g.tz) continue;
        mark_tile(flags, cnt, (bx * g.ty + by) * g.tz + bz);
    }
}

template <class F> __device__ __forceinline__ F inf_of();
template <> __device__ __forceinline__ float inf_of<float>() { return __builtin_inff(); }
template <> __device__ __forceinline__ double inf_of<double>() { return __builtin_inf(); }

template <class F> __global__ __launch_bounds__(256) void k_sk_field_fill(const int* __restrict__ comp, u64 nvox, F* __restrict__ field) {
    for (u64 i = grid_tid(); i < nvox; i += grid_stride()) field[i] = inf_of<F>();
}
__global__ __launch_bounds__(256) void k_sk_relax_reset(Relax r, u64 ntiles) {
    for (u64 i = grid_tid(); i < ntiles; i += grid_stride()) { r.flags[0][i] = 0; r.flags[1][i] = 0; }
    if (grid_tid() < 4) r.cnt[grid_tid()] = 0;
}
template <class F> __global__ __launch_bounds__(256) void k_sk_field_sources(const int* __restrict__ src, u64 n_comp, u64 nvox, Geo g, F* __restrict__ field, Relax r) {
    for (u64 c = 1 + grid_tid(); c <= n_comp; c += grid_stride()) {
        const int s = src[c];
        if (s < 0 || (u64)s >= nvox) continue;
        field[s] = (F)0;
        mark_around(g, r.flags[0], r.cnt, (u64)s);
    }
}

// one sweep: every dirty tile to local convergence.  Thread t owns the z column (t / T, t % T) of the tile.
template <class F>
__global__ __launch_bounds__(256) void k_sk_relax(const int* __restrict__ comp, F* field, const double* __restrict__ pen, Len len, Geo g, Relax r, int sweep,
                                                  u64* counts) {
#pragma clang fp contract(off)
    __shared__ F sf[TVOL];
    __shared__ int sc[TVOL];
    __shared__ u32 s_nbr;
    int* cur = r.flags[sweep & 1];
    int* nxt = r.flags[(sweep + 1) & 1];
    u32 *ccur = r.cnt + sweep % 3, *cnxt = r.cnt + (sweep + 1) % 3;
    if (blockIdx.x == 0 && threadIdx.x == 0) r.cnt[(sweep + 2) % 3] = 0;
    if (__hip_atomic_load(ccur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;      // converged before this launch (nobody writes ccur in it)
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(counts + 4, 1ull);
    const int ntiles = g.tx * g.ty * g.tz;
    const int t = threadIdx.x, lx = t / T, ly = t % T;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {      // (uniform per workgroup: the barriers below need every thread)
        if (cur[tile] == 0) continue;
        __syncthreads();                                                 // the LDS of the tile before is done with
        if (t == 0) { cur[tile] = 0; s_nbr = 0; atomicAdd(counts + 5, 1ull); }
        const int bz = tile % g.tz, by = (tile / g.tz) % g.ty, bx = tile / (g.tz * g.ty);
        const int ox = bx * T - 1, oy = by * T - 1, oz = bz * T - 1;
        for (int k = t; k < TVOL; k += 256) {
            const int hz = k % TH, hy = (k / TH) % TH, hx = k / (TH * TH);
            const int x = ox + hx, y = oy + hy, z = oz + hz;
            int c = 0;
            F f = inf_of<F>();
            if (x >= 0 && y >= 0 && z >= 0 && x < g.X && y < g.Y && z < g.Z) {
                const u64 j = ((u64)x * g.Y + y) * g.Z + z;
                c = comp[j];
                if (c > 0) f = __hip_atomic_load(field + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (a neighbour tile may be storing it)
            }
            sc[k] = c; sf[k] = f;
        }
        __syncthreads();
        const int base = ((lx + 1) * TH + (ly + 1)) * TH + 1;            // local index of this thread's voxel z = 0
        const int gx = ox + 1 + lx, gy = oy + 1 + ly;
        const bool col_in = gx < g.X && gy < g.Y;
        F pv[T];
        if (pen) {
            for (int z = 0; z < T; ++z) {
                const int gz = oz + 1 + z;
                pv[z] = (col_in && gz < g.Z) ? (F)pen[((u64)gx * g.Y + gy) * g.Z + gz] : (F)0;
            }
        }
        bool over = true;
        for (int it = 0; it <= T * T * T; ++it) {                       // Jacobi steps: read all, barrier, write, barrier
            F nv[T];
            bool changed = false;
            for (int z = 0; z < T; ++z) {
                const int k = base + z, c = sc[k];
                F best = sf[k];
                if (c > 0) {
                    for (int o = 0; o < 27; ++o) {
                        if (o == 13) continue;
                        const int kk = k + ((o / 9 - 1) * TH + ((o / 3) % 3 - 1)) * TH + (o % 3 - 1);
                        if (sc[kk] != c) continue;
                        const F cand = pen ? sf[kk] + pv[z] : sf[kk] + (F)len.v[o];
                        if (cand < best) best = cand;
                    }
                    if (best < sf[k]) changed = true;
                }
                nv[z] = best;
            }
            __syncthreads();
            if (changed)
                for (int z = 0; z < T; ++z) sf[base + z] = nv[z];
            if (!__syncthreads_or(changed ? 1 : 0)) { over = false; break; }
        }
        if (over && t == 0) counts[6] = 1;
        // write back what fell, and collect the neighbour tiles that see it in their halo
        u32 nbr = 0;
        if (col_in)
            for (int z = 0; z < T; ++z) {
                const int gz = oz + 1 + z;
                if (gz >= g.Z) break;
                const int k = base + z;
                if (sc[k] <= 0) continue;
                const u64 j = ((u64)gx * g.Y + gy) * g.Z + gz;
                const F v = sf[k];
                if (v < field[j]) {      // (own voxel: nobody else writes it)
                    __hip_atomic_store(field + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    for (int o = 0; o < 27; ++o) {
                        if (o == 13) continue;
                        const int dx = o / 9 - 1, dy = (o / 3) % 3 - 1, dz = o % 3 - 1;
                        if ((dx == 0 || (dx < 0 ? lx == 0 : lx == T - 1)) && (dy == 0 || (dy < 0 ? ly == 0 : ly == T - 1)) &&
                            (dz == 0 || (dz < 0 ? z == 0 : z == T - 1)))
                            nbr |= 1u << o;
                    }
                }
            }
        if (nbr) atomicOr(&s_nbr, nbr);
        __syncthreads();
        if (t < 27 && t != 13 && ((s_nbr >> t) & 1u)) {
            const int nx = bx + t / 9 - 1, ny = by + (t / 3) % 3 - 1, nz = bz + t % 3 - 1;
            if (nx >= 0 && ny >= 0 && nz >= 0 && nx < g.tx && ny < g.ty && nz < g.tz) mark_tile(nxt, cnxt, (nx * g.ty + ny) * g.tz + nz);
        }
    }
}
__global__ __launch_bounds__(64) void k_sk_relax_report(Relax r, u64* counts) {
    if (threadIdx.x == 0) counts[3] = r.cnt[0];
}

// ---- c. argmax per component: key = value bits << 32 | ~raster index, so the largest key is the largest value at the smallest index -------
__global__ __launch_bounds__(256) void k_sk_zero64(u64* p, u64 n) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) p[i] = 0;
}
__global__ __launch_bounds__(256) void k_sk_argmax(const int* __restrict__ comp, const float* __restrict__ field, const uint8_t* __restrict__ valid, u64 nvox, u64* keys) {
    for (u64 i = grid_tid(); i < nvox; i += grid_stride()) {
        const int c = comp[i];
        if (c <= 0 || (valid && !valid[i])) continue;
        const float f = field[i];
        if (!(f >= 0.0f)) continue;      // (NaN or negative: no such value in a field of this file)
        const u64 key = ((u64)__float_as_uint(f) << 32) | (u64)(0xffffffffu - (u32)i);
        if (key > __hip_atomic_load(keys + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(keys + c, key);
    }
}
__global__ __launch_bounds__(256) void k_sk_argmax_out(const u64* __restrict__ keys, u64 n_comp, int* __restrict__ idx, float* __restrict__ val) {
    for (u64 c = grid_tid(); c <= n_comp; c += grid_stride()) {
        const u64 k = c ? keys[c] : 0;
        idx[c] = k ? (int)(0xffffffffu - (u32)(k & 0xffffffffull)) : -1;
        if (val) val[c] = k ? __uint_as_float((u32)(k >> 32)) : 0.0f;
    }
}

// ---- d. penalty ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sk_penalty(const int* __restrict__ comp, const float* __restrict__ dbf, const float* __restrict__ daf, u64 nvox,
                                                   const double* __restrict__ M, const float* __restrict__ daf_max, double scale, int e, double* __restrict__ p) {
#pragma clang fp contract(off)
    for (u64 i = grid_tid(); i < nvox; i += grid_stride()) {
        const int c = comp[i];
        double v = 0.0;
        if (c > 0) {
            const double b = 1.0 - (double)dbf[i] / M[c];
            double pw = b;
            for (int k = 1; k < e; ++k) pw = pw * b;
            const double dm = (double)daf_max[c];
            const double far = dm > 0.0 ? (double)daf[i] / dm : 0.0;      // a one-voxel component: DAF = DAFmax = 0
            v = scale * pw + far;
        }
        p[i] = v;
    }
}

// ---- e., f. one round ----------------------------------------------------------------------------------------------------------------
// one thread per component: from the target by parent steps to the first voxel with dist == 0; the walked voxels are appended to `list`
// (with the root in the first round) and get their parent; their dist is zeroed by the next kernel, after every walk has read the field
__global__ __launch_bounds__(256) void k_sk_walk(const int* __restrict__ comp, Geo g, const double* __restrict__ dist, int* __restrict__ parent,
                                                const int* __restrict__ target, const int* __restrict__ root, const uint64_t* __restrict__ sizes, u64 n_comp,
                                                int* __restrict__ voided, int* __restrict__ list, u32* n_list, u64* counts) {
    for (u64 c = 1 + grid_tid(); c <= n_comp; c += grid_stride()) {
        if (voided[c]) continue;
        if (root) { const int r = root[c]; if (r >= 0) { parent[r] = r; list[atomicAdd(n_list, 1u)] = r; } }
        int u = target[c];
        if (u < 0) continue;
        const u64 bound = sizes[c];
        u64 steps = 0;
        while (true) {
            const double du = dist[u];
            if (!(du > 0.0)) break;
            if (++steps > bound) { counts[1] = 1; voided[c] = 1; break; }
            int x, y, z;
            dec3((u64)u, g.Y, g.Z, x, y, z);
            double bd = __builtin_inf();
            int bn = -1;
            for (int o = 0; o < 27; ++o) {          // ascending raster index, strict <: the smallest index wins a tie
                if (o == 13) continue;
                const int xx = x + o / 9 - 1, yy = y + (o / 3) % 3 - 1, zz = z + o % 3 - 1;
                if (xx < 0 || yy < 0 || zz < 0 || xx >= g.X || yy >= g.Y || zz >= g.Z) continue;
                const u64 j = ((u64)xx * g.Y + yy) * g.Z + zz;
                if (comp[j] != (int)c) continue;
                const double dj = dist[j];
                if (dj < bd) { bd = dj; bn = (int)j; }
            }
            if (bn < 0 || !(bd < du)) { atomicAdd(counts + 2, 1ull); voided[c] = 1; break; }      // float64 absorption: the step does not descend
            parent[u] = bn;
            list[atomicAdd(n_list, 1u)] = u;
            u = bn;
        }
    }
}
// the new nodes become sources (dist 0, their tiles dirty) and clear the valid mask in their box, clipped to the array, own component only
__global__ __launch_bounds__(256) void k_sk_new_nodes(const int* __restrict__ comp, Geo g, const float* __restrict__ dbf, const int* __restrict__ list,
                                                     const u32* __restrict__ n_list, W3 w, float inv_scale, float inv_const, double* dist,
                                                     uint8_t* valid, Relax r) {
#pragma clang fp contract(off)
    const u32 n = *n_list;
    for (u32 k = blockIdx.x; k < n; k += gridDim.x) {
        const int v = list[k];
        const int c = comp[v];
        if (threadIdx.x == 0) { dist[v] = 0.0; mark_around(g, r.flags[0], r.cnt, (u64)v); }
        const float rv = inv_scale * dbf[v] + inv_const;
        int co[3], lo[3], n3[3];
        dec3((u64)v, g.Y, g.Z, co[0], co[1], co[2]);
        const int ext[3] = {g.X, g.Y, g.Z};
        bool empty = !(rv >= 0.0f);
        for (int a = 0; a < 3; ++a) {
            const double hd = floor((double)rv / (double)w.v[a]);
            const int h = hd > 4096.0 ? 4096 : (int)hd;      // (extents are at most 2048)
            lo[a] = max(co[a] - h, 0);
            n3[a] = min(co[a] + h, ext[a] - 1) - lo[a] + 1;
            if (h < 0) empty = true;
        }
        if (empty) continue;
        const u64 total = (u64)n3[0] * n3[1] * n3[2];
        for (u64 q = threadIdx.x; q < total; q += 256) {
            const u32 qq = (u32)q, rz = qq / (u32)n3[2], rx = rz / (u32)n3[1];
            const int z = lo[2] + (int)(qq - rz * (u32)n3[2]), y = lo[1] + (int)(rz - rx * (u32)n3[1]), x = lo[0] + (int)rx;
            const u64 j = ((u64)x * g.Y + y) * g.Z + z;
            if (comp[j] == c) valid[j] = 0;
        }
    }
}
__global__ __launch_bounds__(64) void k_sk_zero32(u32* p) { if (threadIdx.x == 0) *p = 0; }

// ---- g. emit ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sk_emit_flag(const int* __restrict__ comp, const int* __restrict__ parent, const int* __restrict__ voided, u64 nvox,
                                                     u32* __restrict__ flag) {
    for (u64 i = grid_tid(); i < nvox; i += grid_stride()) {
        const int c = comp[i];
        flag[i] = (c > 0 && parent[i] >= 0 && !voided[c]) ? 1u : 0u;
    }
}
__global__ __launch_bounds__(256) void k_sk_emit_keys(const int* __restrict__ comp, const u32* __restrict__ flag, const u32* __restrict__ pos, u64 nvox, u64 cap,
                                                     u64* __restrict__ keys, u64* counts) {
    for (u64 i = grid_tid(); i < nvox; i += grid_stride()) {
        if (i == nvox - 1) counts[0] = pos[i];
        if (!flag[i]) continue;
        const u64 p = (u64)pos[i] - 1;
        if (p < cap) keys[p] = ((u64)(u32)comp[i] << 32) | i;
    }
}
__global__ __launch_bounds__(256) void k_sk_emit_pad(const u32* __restrict__ pos, u64 nvox, u64 cap, u64* __restrict__ keys) {
    const u64 n = pos[nvox - 1];
    for (u64 i = grid_tid(); i < cap; i += grid_stride())
        if (i >= n) keys[i] = INF64;
}
// node_begin[c] for c = 0 .. n_comp + 1 (entry 0 and 1 are 0: component numbers start at 1); nodeidx[voxel] = its row
__global__ __launch_bounds__(256) void k_sk_emit_begin(const u64* __restrict__ skeys, u64 cap, u64 n_comp, u64* __restrict__ node_begin) {
    for (u64 c = grid_tid(); c <= n_comp + 1; c += grid_stride()) node_begin[c] = lower_bound(skeys, cap, c << 32);
}
// a component with nodes has one edge fewer than nodes: edge_begin[c] = node_begin[c] - (components with nodes before c), by a scan
__global__ __launch_bounds__(256) void k_sk_emit_nonempty(const u64* __restrict__ node_begin, u64 n_comp, u32* __restrict__ flag) {
    for (u64 c = grid_tid(); c <= n_comp + 1; c += grid_stride()) flag[c] = (c >= 1 && c <= n_comp && node_begin[c + 1] > node_begin[c]) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_sk_emit_edge_begin(const u64* __restrict__ node_begin, const u32* __restrict__ flag, const u32* __restrict__ pos, u64 n_comp,
                                                           u64* __restrict__ edge_begin) {
    for (u64 c = grid_tid(); c <= n_comp + 1; c += grid_stride()) edge_begin[c] = node_begin[c] - (u64)(pos[c] - flag[c]);
}
// (both kernels do nothing when the table is too small: the sorted keys are then only a part of the nodes)
__global__ __launch_bounds__(256) void k_sk_emit_nodes(const u32* __restrict__ pos, u64 nvox, const u64* __restrict__ skeys, u64 cap, Geo g, W3 w, const float* __restrict__ dbf, int* __restrict__ nodeidx,
                                                      int* __restrict__ node_voxel, float* __restrict__ vertices, float* __restrict__ radii) {
    if ((u64)pos[nvox - 1] > cap) return;
    for (u64 i = grid_tid(); i < cap; i += grid_stride()) {
        const u64 k = skeys[i];
        if (k == INF64) continue;
        const u64 v = k & 0xffffffffull;
        int co[3];
        dec3(v, g.Y, g.Z, co[0], co[1], co[2]);
        nodeidx[v] = (int)i;
        node_voxel[i] = (int)v;
        for (int a = 0; a < 3; ++a) vertices[3 * i + a] = (float)(co[a] * w.v[a]);
        radii[i] = dbf[v];
    }
}
__global__ __launch_bounds__(256) void k_sk_emit_edges(const u32* __restrict__ pos, u64 nvox, const u64* __restrict__ skeys, u64 cap, const int* __restrict__ parent, const int* __restrict__ root,
                                                      const int* __restrict__ nodeidx, const u64* __restrict__ node_begin, const u64* __restrict__ edge_begin,
                                                      int* __restrict__ edges) {
    if ((u64)pos[nvox - 1] > cap) return;
    for (u64 i = grid_tid(); i < cap; i += grid_stride()) {
        const u64 k = skeys[i];
        if (k == INF64) continue;
        const u64 v = k & 0xffffffffull, c = k >> 32;
        const int r = root[c];
        if ((int)v == r) continue;
        const u64 nb = node_begin[c], j = i - nb, jr = (u64)nodeidx[r] - nb;
        const u64 e = edge_begin[c] + (j < jr ? j : j - 1);
        edges[2 * e] = (int)j;
        edges[2 * e + 1] = (int)((u64)nodeidx[parent[v]] - nb);
    }
}

// ---- scratch ---------------------------------------------------------------------------------------------------------------------------
struct SkLayout { int *L, *list, *nodeidx; u32 *cnt, *flag, *pos, *cflag, *cpos, *scal; u64* tmp64; Relax relax; PrimScratch prim; size_t total; };
bool bad_dims(int X, int Y, int Z) {
    return X <= 0 || Y <= 0 || Z <= 0 || X > SD_SKELETONIZE_MAX_EXTENT || Y > SD_SKELETONIZE_MAX_EXTENT || Z > SD_SKELETONIZE_MAX_EXTENT ||
           (size_t)X * Y * Z >= LIM31;
}
Geo geo_of(int X, int Y, int Z) { return Geo{X, Y, Z, (X + T - 1) / T, (Y + T - 1) / T, (Z + T - 1) / T}; }
SkLayout layout(void* base, int X, int Y, int Z) {
    ScratchAlloc a(base);
    SkLayout l{};
    const size_t nvox = (size_t)X * Y * Z;
    const Geo g = geo_of(X, Y, Z);
    const size_t ntiles = (size_t)g.tx * g.ty * g.tz;
    a.take_into(nvox, l.L, l.list, l.nodeidx);
    a.take_into(nvox, l.cnt, l.flag, l.pos);
    l.tmp64 = a.take<u64>(nvox);
    a.take_into(nvox + 2, l.cflag, l.cpos);      // per component (at most one per voxel), entries 0 .. n_comp + 1
    a.take_into(ntiles, l.relax.flags[0], l.relax.flags[1]);
    l.relax.cnt = a.take<u32>(64);
    l.scal = a.take<u32>(64);
    l.prim = take_prim(a, nvox + 2);
    l.total = a.used;
    return l;
}
struct EmitLayout { u64 *keys, *skeys; u32 *iota, *perm; PrimScratch prim; size_t total; };
EmitLayout emit_layout(void* base, size_t cap) {
    ScratchAlloc a(base);
    EmitLayout l{};
    a.take_into(cap, l.keys, l.skeys);
    a.take_into(cap, l.iota, l.perm);
    l.prim = take_prim(a, cap);
    l.total = a.used;
    return l;
}
bool bad_w(const int32_t* w) { return !w || w[0] < 1 || w[1] < 1 || w[2] < 1 || w[0] > SD_SKELETONIZE_MAX_ANISOTROPY || w[1] > SD_SKELETONIZE_MAX_ANISOTROPY || w[2] > SD_SKELETONIZE_MAX_ANISOTROPY; }

}  // namespace

extern "C" {

size_t sd_skeletonize_temp_bytes(int X, int Y, int Z) {
    if (bad_dims(X, Y, Z)) return 0;
    return layout(nullptr, X, Y, Z).total;
}

int sd_skeletonize_components(const uint64_t* seg_dev, int X, int Y, int Z, uint64_t dust_threshold, int32_t* comp_dev, uint64_t* sizes_dev,
                              uint64_t* labels_dev, int32_t* first_dev, size_t max_comps, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes,
                              void* stream) {
    const char* who = "sd_skeletonize_components";
    if (!seg_dev || !comp_dev || !sizes_dev || !labels_dev || !first_dev || !counts_dev || max_comps < 1 || max_comps >= LIM31) return fail(who, ": bad argument");
    if (bad_dims(X, Y, Z)) return fail(who, ": extents must be 1 .. 2048 with fewer than 2^31 voxels");
    const SkLayout l = layout(temp_dev, X, Y, Z);
    if (check_scratch(who, temp_dev, temp_bytes, l.total, "sd_skeletonize_temp_bytes(X, Y, Z)") != SD_OK) return SD_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (zero_counts(counts_dev, 8, s) != SD_OK) return SD_ERR_HIP;
    const u64 nvox = (u64)X * Y * Z;
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    launch_1d(k_sk_cc_init, nvox, VG, s, seg_dev, nvox, l.L, l.cnt);
    launch_1d(k_sk_cc_union, nvox, VG, s, seg_dev, X, Y, Z, l.L);
    launch_1d(k_sk_cc_flatten, nvox, VG, s, nvox, l.L, l.cnt);
    launch_1d(k_sk_cc_flag, nvox, VG, s, nvox, (const int*)l.L, (const u32*)l.cnt, (u64)dust_threshold, l.flag);
    const int rc = scan_u32(who, l.prim, l.flag, l.pos, nvox, s);
    if (rc != SD_OK) return rc;
    launch_1d(k_sk_cc_number, nvox, VG, s, seg_dev, nvox, (const int*)l.L, (const u32*)l.cnt, (const u32*)l.flag, (const u32*)l.pos, (u64)max_comps, comp_dev,
              sizes_dev, labels_dev, first_dev, counts);
    return launch_status("sd_skeletonize_components: launch failed");
}

int sd_skeletonize_d2(const int32_t* comp_dev, int X, int Y, int Z, const int32_t* anisotropy_xyz, size_t n_comp, uint64_t* d2_dev, float* dbf_dev,
                      float* dbf_max_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    const char* who = "sd_skeletonize_d2";
    if (!comp_dev || !d2_dev || !dbf_dev || !dbf_max_dev || !counts_dev || n_comp >= LIM31) return fail(who, ": bad argument");
    if (bad_w(anisotropy_xyz)) return fail(who, ": the anisotropy must be three integers in 1 .. 32768");
    if (bad_dims(X, Y, Z)) return fail(who, ": extents must be 1 .. 2048 with fewer than 2^31 voxels");
    const SkLayout l = layout(temp_dev, X, Y, Z);
    if (check_scratch(who, temp_dev, temp_bytes, l.total, "sd_skeletonize_temp_bytes(X, Y, Z)") != SD_OK) return SD_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (zero_counts(counts_dev, 8, s) != SD_OK) return SD_ERR_HIP;
    if (hipMemsetAsync(dbf_max_dev, 0, (n_comp + 1) * sizeof(float), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "sd_skeletonize_d2: memset failed");
    const u64 nvox = (u64)X * Y * Z;
    u64 w2[3];
    for (int a = 0; a < 3; ++a) w2[a] = (u64)anisotropy_xyz[a] * (u64)anisotropy_xyz[a];
    u64* d2 = reinterpret_cast<u64*>(d2_dev);
    launch_1d(k_sk_d2_axis, nvox, VG, s, comp_dev, (const u64*)nullptr, d2, X, Y, Z, 0, w2[0]);
    launch_1d(k_sk_d2_axis, nvox, VG, s, comp_dev, (const u64*)d2, l.tmp64, X, Y, Z, 1, w2[1]);
    launch_1d(k_sk_d2_axis, nvox, VG, s, comp_dev, (const u64*)l.tmp64, d2, X, Y, Z, 2, w2[2]);
    launch_1d(k_sk_dbf, nvox, VG, s, comp_dev, (const u64*)d2, nvox, dbf_dev, reinterpret_cast<u32*>(dbf_max_dev), reinterpret_cast<u64*>(counts_dev));
    return launch_status("sd_skeletonize_d2: launch failed");
}

int sd_skeletonize_field_start(const int32_t* comp_dev, int X, int Y, int Z, const int32_t* source_dev, size_t n_comp, void* field_dev, int field_f64,
                               void* temp_dev, size_t temp_bytes, void* stream) {
    const char* who = "sd_skeletonize_field_start";
    if (!comp_dev || !source_dev || !field_dev || n_comp >= LIM31 || (field_f64 != 0 && field_f64 != 1)) return fail(who, ": bad argument");
    if (bad_dims(X, Y, Z)) return fail(who, ": extents must be 1 .. 2048 with fewer than 2^31 voxels");
    const SkLayout l = layout(temp_dev, X, Y, Z);
    if (check_scratch(who, temp_dev, temp_bytes, l.total, "sd_skeletonize_temp_bytes(X, Y, Z)") != SD_OK) return SD_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const u64 nvox = (u64)X * Y * Z;
    const Geo g = geo_of(X, Y, Z);
    const u64 ntiles = (u64)g.tx * g.ty * g.tz;
    launch_1d(k_sk_relax_reset, ntiles, TG, s, l.relax, ntiles);
    if (field_f64) {
        launch_1d(k_sk_field_fill<double>, nvox, VG, s, comp_dev, nvox, reinterpret_cast<double*>(field_dev));
        launch_1d(k_sk_field_sources<double>, n_comp, CG, s, source_dev, (u64)n_comp, nvox, g, reinterpret_cast<double*>(field_dev), l.relax);
    } else {
        launch_1d(k_sk_field_fill<float>, nvox, VG, s, comp_dev, nvox, reinterpret_cast<float*>(field_dev));
        launch_1d(k_sk_field_sources<float>, n_comp, CG, s, source_dev, (u64)n_comp, nvox, g, reinterpret_cast<float*>(field_dev), l.relax);
    }
    return launch_status("sd_skeletonize_field_start: launch failed");
}

int sd_skeletonize_relax(const int32_t* comp_dev, int X, int Y, int Z, const int32_t* anisotropy_xyz, void* field_dev, const double* penalty_dev,
                         int max_sweeps, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    const char* who = "sd_skeletonize_relax";
    if (!comp_dev || !field_dev || !counts_dev || max_sweeps < 1 || max_sweeps > SD_SKELETONIZE_MAX_SWEEPS) return fail(who, ": bad argument");
    if (bad_w(anisotropy_xyz)) return fail(who, ": the anisotropy must be three integers in 1 .. 32768");
    if (bad_dims(X, Y, Z)) return fail(who, ": extents must be 1 .. 2048 with fewer than 2^31 voxels");
    const SkLayout l = layout(temp_dev, X, Y, Z);
    if (check_scratch(who, temp_dev, temp_bytes, l.total, "sd_skeletonize_temp_bytes(X, Y, Z)") != SD_OK) return SD_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const Geo g = geo_of(X, Y, Z);
    const u64 ntiles = (u64)g.tx * g.ty * g.tz;
    Len len;
    for (int o = 0; o < 27; ++o) {      // float32(sqrt(double(sum (w_a o_a)^2))): one of 13 classes, the same for o and -o
        const long long dx = (long long)(o / 9 - 1) * anisotropy_xyz[0], dy = (long long)((o / 3) % 3 - 1) * anisotropy_xyz[1],
                        dz = (long long)(o % 3 - 1) * anisotropy_xyz[2];
        len.v[o] = (float)sqrt((double)(dx * dx + dy * dy + dz * dz));
    }
    const int sweeps = (max_sweeps + 5) / 6 * 6;
    const int grid = (int)(ntiles < (u64)TG ? ntiles : (u64)TG);
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    for (int k = 0; k < sweeps; ++k) {
        if (penalty_dev) hipLaunchKernelGGL(k_sk_relax<double>, dim3(grid), dim3(256), 0, s, comp_dev, reinterpret_cast<double*>(field_dev), penalty_dev, len, g, l.relax, k, counts);
        else hipLaunchKernelGGL(k_sk_relax<float>, dim3(grid), dim3(256), 0, s, comp_dev, reinterpret_cast<float*>(field_dev), (const double*)nullptr, len, g, l.relax, k, counts);
    }
    hipLaunchKernelGGL(k_sk_relax_report, dim3(1), dim3(64), 0, s, l.relax, counts);
    return launch_status("sd_skeletonize_relax: launch failed");
}

int sd_skeletonize_argmax(const int32_t* comp_dev, const float* field_dev, const uint8_t* valid_dev, size_t n_vox, size_t n_comp, int32_t* index_dev,
                          float* value_dev, uint64_t* keys_dev, void* stream) {
    if (!comp_dev || !field_dev || !index_dev || !keys_dev || n_vox < 1 || n_vox >= LIM31 || n_comp >= LIM31)
        return fail("sd_skeletonize_argmax", ": bad argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    u64* keys = reinterpret_cast<u64*>(keys_dev);
    launch_1d(k_sk_zero64, n_comp + 1, CG, s, keys, (u64)n_comp + 1);
    launch_1d(k_sk_argmax, n_vox, VG, s, comp_dev, field_dev, valid_dev, (u64)n_vox, keys);
    launch_1d(k_sk_argmax_out, n_comp + 1, CG, s, (const u64*)keys, (u64)n_comp, index_dev, value_dev);
    return launch_status("sd_skeletonize_argmax: launch failed");
}

int sd_skeletonize_penalty(const int32_t* comp_dev, const float* dbf_dev, const float* daf_dev, size_t n_vox, size_t n_comp, const double* m_dev,
                           const float* daf_max_dev, double pdrf_scale, int pdrf_exponent, double* penalty_dev, void* stream) {
    if (!comp_dev || !dbf_dev || !daf_dev || !m_dev || !daf_max_dev || !penalty_dev || n_vox < 1 || n_vox >= LIM31 || n_comp >= LIM31)
        return fail("sd_skeletonize_penalty", ": bad argument");
    if (pdrf_exponent < 1 || pdrf_exponent > SD_SKELETONIZE_MAX_EXPONENT) return fail("sd_skeletonize_penalty", ": the exponent must be an integer in 1 .. 64");
    if (!(pdrf_scale >= 0.0) || !(pdrf_scale <= 1.7976931348623157e308)) return fail("sd_skeletonize_penalty", ": pdrf_scale must be finite and not negative");
    launch_1d(k_sk_penalty, n_vox, VG, reinterpret_cast<hipStream_t>(stream), comp_dev, dbf_dev, daf_dev, (u64)n_vox, m_dev, daf_max_dev, pdrf_scale, pdrf_exponent,
              penalty_dev);
    return launch_status("sd_skeletonize_penalty: launch failed");
}

int sd_skeletonize_round(const int32_t* comp_dev, int X, int Y, int Z, const int32_t* anisotropy_xyz, const float* dbf_dev, double* dist_dev,
                         uint8_t* valid_dev, int32_t* parent_dev, const int32_t* target_dev, const int32_t* root_dev, const uint64_t* sizes_dev,
                         size_t n_comp, float inv_scale, float inv_const, int32_t* void_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes,
                         void* stream) {
    const char* who = "sd_skeletonize_round";
    if (!comp_dev || !dbf_dev || !dist_dev || !valid_dev || !parent_dev || !target_dev || !sizes_dev || !void_dev || !counts_dev || n_comp < 1 || n_comp >= LIM31)
        return fail(who, ": bad argument");
    if (!(inv_scale >= 0.0f) || !(inv_scale <= 3.0e38f) || !(inv_const >= -3.0e38f) || !(inv_const <= 3.0e38f)) return fail(who, ": scale and const must be finite, scale not negative");
    if (bad_w(anisotropy_xyz)) return fail(who, ": the anisotropy must be three integers in 1 .. 32768");
    if (bad_dims(X, Y, Z)) return fail(who, ": extents must be 1 .. 2048 with fewer than 2^31 voxels");
    const SkLayout l = layout(temp_dev, X, Y, Z);
    if (check_scratch(who, temp_dev, temp_bytes, l.total, "sd_skeletonize_temp_bytes(X, Y, Z)") != SD_OK) return SD_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const Geo g = geo_of(X, Y, Z);
    W3 w{{anisotropy_xyz[0], anisotropy_xyz[1], anisotropy_xyz[2]}};
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    hipLaunchKernelGGL(k_sk_zero32, dim3(1), dim3(64), 0, s, l.scal);
    launch_1d(k_sk_walk, n_comp, CG, s, comp_dev, g, (const double*)dist_dev, parent_dev, target_dev, root_dev, sizes_dev, (u64)n_comp, void_dev, l.list, l.scal, counts);
    hipLaunchKernelGGL(k_sk_new_nodes, dim3(NG), dim3(256), 0, s, comp_dev, g, dbf_dev, (const int*)l.list, (const u32*)l.scal, w, inv_scale, inv_const, dist_dev, valid_dev,
                       l.relax);
    return launch_status("sd_skeletonize_round: launch failed");
}

size_t sd_skeletonize_emit_temp_bytes(size_t max_nodes) {
    if (max_nodes < 1 || max_nodes >= LIM31) return 0;
    return emit_layout(nullptr, max_nodes).total;
}

int sd_skeletonize_emit(const int32_t* comp_dev, int X, int Y, int Z, const int32_t* anisotropy_xyz, const int32_t* parent_dev, const float* dbf_dev,
                        const int32_t* root_dev, const int32_t* void_dev, size_t n_comp, size_t max_nodes, uint64_t* node_begin_dev,
                        uint64_t* edge_begin_dev, int32_t* node_voxel_dev, float* vertices_dev, float* radii_dev, int32_t* edges_dev,
                        uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* emit_temp_dev, size_t emit_temp_bytes, void* stream) {
    const char* who = "sd_skeletonize_emit";
    if (!comp_dev || !parent_dev || !dbf_dev || !root_dev || !void_dev || !node_begin_dev || !edge_begin_dev || !node_voxel_dev || !vertices_dev || !radii_dev ||
        !edges_dev || !counts_dev || n_comp < 1 || n_comp >= LIM31 || max_nodes < 1 || max_nodes >= LIM31)
        return fail(who, ": bad argument");
    if (bad_w(anisotropy_xyz)) return fail(who, ": the anisotropy must be three integers in 1 .. 32768");
    if (bad_dims(X, Y, Z)) return fail(who, ": extents must be 1 .. 2048 with fewer than 2^31 voxels");
    const SkLayout l = layout(temp_dev, X, Y, Z);
    if (check_scratch(who, temp_dev, temp_bytes, l.total, "sd_skeletonize_temp_bytes(X, Y, Z)") != SD_OK) return SD_ERR_INVALID;
    const EmitLayout e = emit_layout(emit_temp_dev, max_nodes);
    if (check_scratch(who, emit_temp_dev, emit_temp_bytes, e.total, "sd_skeletonize_emit_temp_bytes(max_nodes)") != SD_OK) return SD_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (zero_counts(counts_dev, 8, s) != SD_OK) return SD_ERR_HIP;
    const u64 nvox = (u64)X * Y * Z, cap = max_nodes;
    const Geo g = geo_of(X, Y, Z);
    W3 w{{anisotropy_xyz[0], anisotropy_xyz[1], anisotropy_xyz[2]}};
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    launch_1d(k_sk_emit_flag, nvox, VG, s, comp_dev, parent_dev, void_dev, nvox, l.flag);
    int rc = scan_u32(who, l.prim, l.flag, l.pos, nvox, s);
    if (rc != SD_OK) return rc;
    launch_1d(k_sk_emit_keys, nvox, VG, s, comp_dev, (const u32*)l.flag, (const u32*)l.pos, nvox, cap, e.keys, counts);
    launch_1d(k_sk_emit_pad, cap, NG, s, (const u32*)l.pos, nvox, cap, e.keys);
    rc = sort_by_key(who, e.prim, (const u64*)e.keys, e.skeys, e.iota, e.perm, cap, 64, s);
    if (rc != SD_OK) return rc;
    launch_1d(k_sk_emit_begin, n_comp + 2, CG, s, (const u64*)e.skeys, cap, (u64)n_comp, reinterpret_cast<u64*>(node_begin_dev));
    if (n_comp + 2 > nvox + 2) return fail(who, ": more components than voxels");
    launch_1d(k_sk_emit_nonempty, n_comp + 2, CG, s, (const u64*)node_begin_dev, (u64)n_comp, l.cflag);
    rc = scan_u32(who, l.prim, l.cflag, l.cpos, n_comp + 2, s);
    if (rc != SD_OK) return rc;
    launch_1d(k_sk_emit_edge_begin, n_comp + 2, CG, s, (const u64*)node_begin_dev, (const u32*)l.cflag, (const u32*)l.cpos, (u64)n_comp, reinterpret_cast<u64*>(edge_begin_dev));
    launch_1d(k_sk_emit_nodes, cap, NG, s, (const u32*)l.pos, nvox, (const u64*)e.skeys, cap, g, w, dbf_dev, l.nodeidx, node_voxel_dev, vertices_dev, radii_dev);
    launch_1d(k_sk_emit_edges, cap, NG, s, (const u32*)l.pos, nvox, (const u64*)e.skeys, cap, parent_dev, root_dev, (const int*)l.nodeidx, (const u64*)node_begin_dev, (const u64*)edge_begin_dev,
              edges_dev);
    return launch_status("sd_skeletonize_emit: launch failed");
}

}  // extern "C"
