// Synapse agglomeration on the device: the array form of what extraction/cs_processing_steps.py does per cell
// pair in Python -- connected_cluster_kdtree (:552-602, a networkx graph with one node per voxel and one cKDTree per fragment and per
// pair of first-stage components) and the per-component half of _combine_and_split_syn_thread (:453-474: voxel share of every
// fragment, size, bounding box, the voxel nearest the scaled centre of mass, the size filter).  All cell pairs ("groups") of a dataset
// go through one set of launches.
//
// The partition is the connected components of the graph "scaled distance strictly below the gap" over the voxels of one group
// (DESIGN.md section 7 says when that is the reference's).  Voxels arrive in the reference's flat order (group-major, the fragments of
// a group in list order, every fragment's voxels in stored order) with the fragment number of every voxel.
//
//   cells    voxels are binned into boxes of (cx, cy, cz) voxels whose scaled diagonal is below the gap: the voxels of one group in
//            one box are connected without a test.  Key = (group | box coordinate relative to the group's corner); a stable radix
//            sort of the voxel permutation by key, head flags and a scan give the cell list; the first voxel of a cell in sorted
//            order is its smallest flat index.  Every cell gets its tight voxel box.
//   link     one wave per cell walks the lexicographically upper half of its neighbourhood (64 neighbours per trip, found by binary
//            search in the sorted cell keys).  From the two tight boxes: smallest possible distance >= gap -> nothing; largest
//            possible distance < gap -> union (both with a margin of 1e-9 for rounding, so that only point_d2 decides at the gap); otherwise, unless both are in one set already, the 64 lanes test voxel pairs and
//            stop at the first hit (ballot).  Union-find over the cells: uf_union of sd_tables.h (larger root under the smaller).
//   number   smallest flat index per root; a flag at that index, scanned over the flat order, numbers the components in ascending
//            order of their smallest flat index -- which is the reference's order, and group-major because the flat order is.
//   stats    stable sort of the voxels by component (flat order survives inside a component), head flags over (component,
//            fragment) give the voxel count of every contributing fragment; box and int64 coordinate sums by wave-reduced atomics;
//            the voxel nearest the mean in two passes (smallest float64 squared distance as ordered bits, then the smallest flat index
//            that attains it); a scan over the keep flags gathers the voxel runs of the components that pass the size filter.
//
// Distances are float64 of voxel * scale, compared as d^2 < gap^2: exact for integral scales.  No scalar memory writes, no inline
// assembly.
#include "../../include/syconn_dense.h"
#include "sd_sortseg.h"
#include "sd_tables.h"

namespace {

struct SsvGeom {
    double s[3], gap2;      // voxel size in nm, squared gap
    double gap2_lo, gap2_hi; // gap2 (1 -+ 1e-9): the box tests decide only what rounding cannot change; the rest is left to point_d2
    int c[3], b[3], r[3];   // cell dimension in voxels, key bits per axis, reach in cells per axis
};

// do all 64 lanes of the wave hold a valid item with the same key?  (called by every lane)
__device__ __forceinline__ bool wave_same(u32 key, bool active) {
    const u32 k0 = (u32)__shfl((int)key, 0);
    return __all(active && key == k0);
}

// ---- cells ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ssv_keys(const int* __restrict__ vox, const u32* __restrict__ vfrag, const u32* __restrict__ fgroup,
                                                  const int* __restrict__ gorg, u64 n, u64 n_frag, u64 n_group, SsvGeom g, u64* key, u64* counts) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        const u32 f = vfrag[i];
        u64 grp = f < n_frag ? fgroup[f] : n_group;
        bool bad = grp >= n_group;
        if (bad) grp = 0;
        u64 k = grp;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            long long c = ((long long)vox[3 * i + a] - gorg[3 * grp + a]) / g.c[a];
            if (vox[3 * i + a] < gorg[3 * grp + a] || c >= (1ll << g.b[a])) { bad = true; c = 0; }
            k = (k << g.b[a]) | (u64)c;
        }
        if (bad) counts[7] = 1;
        key[i] = k;
    }
}

// per cell: start in the sorted order, key, itself as union-find parent, an empty box; the sentinel start and the cell count
__global__ __launch_bounds__(256) void k_ssv_cells(const u64* skey, const u32* head, const u32* seg, u64 n, u32* cell_start, u64* cell_key,
                                                   u32* parent, u32* minflat, int* box, u64* counts) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        if (head[i]) {
            const u32 c = seg[i] - 1u;
            cell_start[c] = (u32)i; cell_key[c] = skey[i]; parent[c] = c; minflat[c] = 0xffffffffu;
#pragma unroll
            for (int a = 0; a < 3; ++a) { box[6 * (u64)c + a] = 0x7fffffff; box[6 * (u64)c + 3 + a] = (int)0x80000000; }
        }
        if (i == n - 1) { cell_start[seg[i]] = (u32)n; counts[1] = seg[i]; }
    }
}

// the voxel rows in sorted order and the tight box of every cell (one atomic per wave where the wave holds one cell)
__global__ __launch_bounds__(256) void k_ssv_cell_boxes(const int* __restrict__ vox, const u32* perm, const u32* seg, u64 n, int* svox, int* box) {
    const int lane = threadIdx.x & 63;
    for (u64 base = (u64)blockIdx.x * 256; base < n; base += grid_stride()) {
        const u64 i = base + threadIdx.x;
        const bool act = i < n;
        u32 c = 0; int v[3] = {0, 0, 0};
        if (act) {
            c = seg[i] - 1u;
            const u64 p = perm[i];
#pragma unroll
            for (int a = 0; a < 3; ++a) { v[a] = vox[3 * p + a]; svox[3 * i + a] = v[a]; }
        }
        if (wave_same(c, act)) {
            int lo[3] = {v[0], v[1], v[2]}, hi[3] = {v[0], v[1], v[2]};
#pragma unroll
            for (int a = 0; a < 3; ++a)
                for (int m = 32; m; m >>= 1) { lo[a] = min(lo[a], __shfl_xor(lo[a], m)); hi[a] = max(hi[a], __shfl_xor(hi[a], m)); }
            if (lane == 0)
#pragma unroll
                for (int a = 0; a < 3; ++a) { atomicMin(&box[6 * (u64)c + a], lo[a]); atomicMax(&box[6 * (u64)c + 3 + a], hi[a]); }
        } else if (act) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { atomicMin(&box[6 * (u64)c + a], v[a]); atomicMax(&box[6 * (u64)c + 3 + a], v[a]); }
        }
    }
}

// ---- link -------------------------------------------------------------------------------------------------------------------------
// squared scaled distance between a point and a box / the smallest and largest between two boxes (inclusive voxel boxes)
__device__ __forceinline__ double point_box_d2(const int* v, const int* bx, const SsvGeom& g) {
    double d2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int gapv = max(0, max(bx[a] - v[a], v[a] - bx[3 + a]));
        const double d = (double)gapv * g.s[a];
        d2 += d * d;
    }
    return d2;
}
__device__ __forceinline__ double point_d2(const int* p, const int* q, const SsvGeom& g) {
#pragma clang fp contract(off)                              // every product and sum rounded on its own, as numpy / cKDTree do
    double d2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double d = (double)p[a] * g.s[a] - (double)q[a] * g.s[a];
        d2 += d * d;
    }
    return d2;
}

// wave-cooperative: is any voxel of cell A within the gap of any voxel of cell B?  Lanes hold voxels of A (64 per trip, those
// that can reach B's box at all), the wave walks the voxels of B that can reach A's box.
__device__ bool pair_test(const int* __restrict__ svox, u32 a0, u32 a1, u32 b0, u32 b1, const int* boxA, const int* boxB, const SsvGeom& g, int lane) {
    for (u32 ta = a0; ta < a1; ta += 64) {
        const u32 ia = ta + lane;
        bool act = ia < a1;
        int p[3] = {0, 0, 0};
        if (act) {
            p[0] = svox[3 * (u64)ia]; p[1] = svox[3 * (u64)ia + 1]; p[2] = svox[3 * (u64)ia + 2];
            act = point_box_d2(p, boxB, g) < g.gap2_hi;
        }
        if (!__any(act)) continue;
        for (u32 ib = b0; ib < b1; ++ib) {
            const int q[3] = {svox[3 * (u64)ib], svox[3 * (u64)ib + 1], svox[3 * (u64)ib + 2]};
            if (!(point_box_d2(q, boxA, g) < g.gap2_hi)) continue;                  // uniform over the wave
            if (__any(act && point_d2(p, q, g) < g.gap2)) return true;
        }
    }
    return false;
}

__global__ __launch_bounds__(256) void k_ssv_link(const int* __restrict__ svox, const u32* cell_start, const u64* cell_key, const int* box,
                                                  u32* parent, SsvGeom g, u64* counts) {
    const int lane = threadIdx.x & 63;
    const u64 wave = grid_tid() >> 6, n_waves = grid_stride() >> 6;
    const u64 n_cells = counts[1];
    const int wy = 2 * g.r[1] + 1, wz = 2 * g.r[2] + 1;
    const int T = (2 * g.r[0] + 1) * wy * wz, M = (T - 1) / 2;                  // the upper half of the neighbourhood: t > T / 2
    u32 n_found = 0, n_far = 0, n_near = 0, n_joined = 0, n_tested = 0;          // statistics (lane 0's are added up)
    for (u64 c = wave; c < n_cells; c += n_waves) {
        const u64 key = cell_key[c];
        int cc[3]; u64 k = key;
#pragma unroll
        for (int a = 2; a >= 0; --a) { cc[a] = (int)(k & ((1ull << g.b[a]) - 1)); k >>= g.b[a]; }
        const u64 grp = k;
        int bA[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) bA[a] = box[6 * c + a];
        for (int m0 = 0; m0 < M; m0 += 64) {
            const int m = m0 + lane;
            long nb = -1;
            int cls = 0;                                                          // 1: union without looking, 2: needs a voxel test
            if (m < M) {
                const int t = T / 2 + 1 + m;
                const int d[3] = {t / (wy * wz) - g.r[0], (t / wz) % wy - g.r[1], t % wz - g.r[2]};
                u64 nk = grp; bool ok = true;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const long long q = (long long)cc[a] + d[a];
                    ok = ok && q >= 0 && q < (1ll << g.b[a]);
                    nk = (nk << g.b[a]) | (u64)(ok ? q : 0);
                }
                if (ok) nb = find_exact(cell_key, n_cells, nk);
                if (nb >= 0) {
                    double dmin = 0.0, dmax = 0.0;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const int lo = box[6 * nb + a], hi = box[6 * nb + 3 + a];
                        const double near = (double)max(0, max(lo - bA[3 + a], bA[a] - hi)) * g.s[a];
                        const double far = (double)max(hi - bA[a], bA[3 + a] - lo) * g.s[a];
                        dmin += near * near; dmax += far * far;
                    }
                    cls = !(dmin < g.gap2_hi) ? 0 : (dmax < g.gap2_lo ? 1 : 2);
                }
            }
            if (cls == 1) uf_union(parent, (u32)c, (u32)nb);
            n_found += __popcll(__ballot(nb >= 0)); n_near += __popcll(__ballot(cls == 1));
            n_far += __popcll(__ballot(nb >= 0 && cls == 0));
            u64 todo = __ballot(cls == 2);
            while (todo) {
                const int j = __builtin_ctzll(todo);
                todo &= todo - 1;
                const u32 other = (u32)__shfl((int)nb, j);
                const int same = __shfl((int)(uf_find(parent, (u32)c) == uf_find(parent, other)), 0);
                if (same) { ++n_joined; continue; }
                ++n_tested;
                int bB[6];
#pragma unroll
                for (int a = 0; a < 6; ++a) bB[a] = box[6 * (u64)other + a];
                if (pair_test(svox, cell_start[c], cell_start[c + 1], cell_start[other], cell_start[other + 1], bA, bB, g, lane) && lane == 0)
                    uf_union(parent, (u32)c, other);
            }
        }
    }
    if (lane == 0) {
        if (n_found) atomicAdd(&counts[2], (u64)n_found);
        if (n_far) atomicAdd(&counts[3], (u64)n_far);
        if (n_near) atomicAdd(&counts[4], (u64)n_near);
        if (n_joined) atomicAdd(&counts[5], (u64)n_joined);
        if (n_tested) atomicAdd(&counts[6], (u64)n_tested);
    }
}

__global__ __launch_bounds__(256) void k_ssv_compress(u32* parent, const u64* counts) {
    const u64 n_cells = counts[1];
    for (u64 c = grid_tid(); c < n_cells; c += grid_stride()) parent[c] = uf_find(parent, (u32)c);
}

// ---- number -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ssv_rootmin(const u32* parent, const u32* cell_start, const u32* perm, u32* minflat, const u64* counts) {
    const u64 n_cells = counts[1];
    for (u64 c = grid_tid(); c < n_cells; c += grid_stride())
        atomicMin(&minflat[parent[c]], perm[cell_start[c]]);                     // stable sort: the first voxel of a cell is its smallest
}
__global__ __launch_bounds__(256) void k_ssv_flag(const u32* parent, const u32* minflat, u32* flag, const u64* counts) {
    const u64 n_cells = counts[1];
    for (u64 c = grid_tid(); c < n_cells; c += grid_stride())
        if (parent[c] == (u32)c) flag[minflat[c]] = 1u;
}
__global__ __launch_bounds__(256) void k_ssv_labels(const u32* perm, const u32* seg, const u32* parent, const u32* minflat, const u32* fscan,
                                                    u64 n, int* labels, u64* counts) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        labels[perm[i]] = (int)(fscan[minflat[parent[seg[i] - 1u]]] - 1u);
        if (i == n - 1) counts[0] = fscan[n - 1];
    }
}

// ---- statistics -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ssv_compkeys(const int* labels, u64 n, u64 K, u64* key, u64* counts) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        const u64 k = (u64)(u32)labels[i];
        if (k >= K) counts[3] = 1;
        key[i] = k < K ? k : K - 1;
    }
}
__global__ __launch_bounds__(256) void k_ssv_stat_init(u64 K, int* bbox, u64* sums, u64* best, u32* rep) {
    for (u64 k = grid_tid(); k < K; k += grid_stride()) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { bbox[6 * k + a] = 0x7fffffff; bbox[6 * k + 3 + a] = (int)0x80000000; sums[3 * k + a] = 0; }
        best[k] = ~0ull; rep[k] = 0xffffffffu;
    }
}
// heads of the components and of the (component, fragment) runs in the sorted order
__global__ __launch_bounds__(256) void k_ssv_stat_heads(const u64* skey, const u32* sflat, const u32* vfrag, u64 n, u32* headp, u32* comp_begin) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        const bool hc = i == 0 || skey[i] != skey[i - 1];
        headp[i] = (hc || vfrag[sflat[i]] != vfrag[sflat[i - 1]]) ? 1u : 0u;
        if (hc) comp_begin[skey[i]] = (u32)i;
        if (i == n - 1) comp_begin[skey[i] + 1] = (u32)n;
    }
}
__global__ __launch_bounds__(256) void k_ssv_stat_pairs(const u64* skey, const u32* sflat, const u32* vfrag, const u32* headp, const u32* pscan,
                                                        u64 n, u32* pair_comp, u32* pair_frag, u32* pair_begin, u64* counts) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        if (headp[i]) {
            const u32 p = pscan[i] - 1u;
            pair_comp[p] = (u32)skey[i]; pair_frag[p] = vfrag[sflat[i]]; pair_begin[p] = (u32)i;
        }
        if (i == n - 1) { pair_begin[pscan[i]] = (u32)n; counts[0] = pscan[i]; }
    }
}
__global__ __launch_bounds__(256) void k_ssv_stat_reduce(const int* __restrict__ vox, const u64* skey, const u32* sflat, u64 n, int* bbox, u64* sums) {
    const int lane = threadIdx.x & 63;
    for (u64 base = (u64)blockIdx.x * 256; base < n; base += grid_stride()) {
        const u64 i = base + threadIdx.x;
        const bool act = i < n;
        u32 k = 0; int v[3] = {0, 0, 0};
        if (act) {
            k = (u32)skey[i];
            const u64 p = sflat[i];
            v[0] = vox[3 * p]; v[1] = vox[3 * p + 1]; v[2] = vox[3 * p + 2];
        }
        if (wave_same(k, act)) {
            int lo[3] = {v[0], v[1], v[2]}, hi[3] = {v[0], v[1], v[2]};
            long long sm[3] = {v[0], v[1], v[2]};
#pragma unroll
            for (int a = 0; a < 3; ++a)
                for (int m = 32; m; m >>= 1) {
                    lo[a] = min(lo[a], __shfl_xor(lo[a], m)); hi[a] = max(hi[a], __shfl_xor(hi[a], m)); sm[a] += __shfl_xor(sm[a], m);
                }
            if (lane == 0)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    atomicMin(&bbox[6 * (u64)k + a], lo[a]); atomicMax(&bbox[6 * (u64)k + 3 + a], hi[a]); atomicAdd(&sums[3 * (u64)k + a], (u64)sm[a]);
                }
        } else if (act) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicMin(&bbox[6 * (u64)k + a], v[a]); atomicMax(&bbox[6 * (u64)k + 3 + a], v[a]); atomicAdd(&sums[3 * (u64)k + a], (u64)(long long)v[a]);
            }
        }
    }
}
// squared distance of every voxel to its component's scaled mean, as ordered bits (a non-negative double orders like its bits), and
// the smallest per component
__global__ __launch_bounds__(256) void k_ssv_stat_dist(const int* __restrict__ vox, const u64* skey, const u32* sflat, const u32* comp_begin,
                                                       const u64* sums, u64 n, SsvGeom g, u64* d2bits, u64* best) {
    const int lane = threadIdx.x & 63;
    for (u64 base = (u64)blockIdx.x * 256; base < n; base += grid_stride()) {
        const u64 i = base + threadIdx.x;
        const bool act = i < n;
        u32 k = 0; u64 bits = ~0ull;
        if (act) {
            k = (u32)skey[i];
            const u64 p = sflat[i];
            const double size = (double)(comp_begin[k + 1] - comp_begin[k]);
            double d2 = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma clang fp contract(off)                              // no fused multiply-add: the rounding of numpy's mean and distances
                const double mean = ((double)(long long)sums[3 * (u64)k + a] * g.s[a]) / size;
                const double d = (double)vox[3 * p + a] * g.s[a] - mean;
                d2 += d * d;
            }
            bits = (u64)__double_as_longlong(d2);
            d2bits[i] = bits;
        }
        if (wave_same(k, act)) {
            for (int m = 32; m; m >>= 1) { const u64 o = __shfl_xor(bits, m); bits = o < bits ? o : bits; }
            if (lane == 0) atomicMin(&best[k], bits);
        } else if (act) {
            atomicMin(&best[k], bits);
        }
    }
}
__global__ __launch_bounds__(256) void k_ssv_stat_rep(const u64* skey, const u32* sflat, const u64* d2bits, const u64* best, u64 n, u32* rep) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        const u64 k = skey[i];
        if (d2bits[i] == best[k]) atomicMin(&rep[k], sflat[i]);
    }
}
__global__ __launch_bounds__(256) void k_ssv_stat_keep(const u64* skey, const u32* comp_begin, u64 n, u64 min_vx, u32* keep) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        const u64 k = skey[i];
        keep[i] = (u64)(comp_begin[k + 1] - comp_begin[k]) >= min_vx ? 1u : 0u;
    }
}
__global__ __launch_bounds__(256) void k_ssv_stat_gather(const int* __restrict__ vox, const u32* sflat, const u32* keep, const u32* kscan, u64 n,
                                                         u32* vox_out, u64* counts) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        if (keep[i]) {
            const u64 o = kscan[i] - 1u, p = sflat[i];
            vox_out[3 * o] = (u32)vox[3 * p]; vox_out[3 * o + 1] = (u32)vox[3 * p + 1]; vox_out[3 * o + 2] = (u32)vox[3 * p + 2];
        }
        if (i == n - 1) counts[1] = kscan[i];
    }
}

// scratch of the two entry points, laid over the same allocation of sd_syn_ssv_temp_bytes(n): sd_syn_ssv_stats writes every array
// before it reads it, and the staged calls of sd_syn_ssv_components need only their own layout to last from one to the next
struct SsvCompScratch { u64 *key, *skey, *cell_key; u32 *i0, *perm, *head, *seg, *cell_start, *parent, *minflat, *flag, *fscan; int *svox, *box; PrimScratch prim; };
size_t layout(SsvCompScratch& w, void* base, size_t n) {
    ScratchAlloc a(base);
    a.take_into(n, w.key, w.skey, w.cell_key, w.i0, w.perm, w.head, w.seg);
    a.take_into(n + 1, w.cell_start);                        // one start per cell and the sentinel
    a.take_into(n, w.parent, w.minflat, w.flag, w.fscan);
    a.take_into(3 * n, w.svox);
    a.take_into(6 * n, w.box);
    w.prim = take_prim(a, n);
    return a.used;
}
struct SsvStatScratch { u64 *key, *skey, *d2bits, *best, *sums; u32 *i0, *sflat, *headp, *pscan, *keep, *kscan; PrimScratch prim; };
size_t layout(SsvStatScratch& w, void* base, size_t n) {
    ScratchAlloc a(base);
    a.take_into(n, w.key, w.skey, w.d2bits, w.best);
    a.take_into(3 * n, w.sums);
    a.take_into(n, w.i0, w.sflat, w.headp, w.pscan, w.keep, w.kscan);
    w.prim = take_prim(a, n);
    return a.used;
}

bool ssv_geom(const double* scale, double gap, const int* cell, const int* bits, SsvGeom& g) {
    if (!scale || !(gap > 0.0)) return false;
    g.gap2 = gap * gap;
    g.gap2_lo = g.gap2 * (1.0 - 1e-9); g.gap2_hi = g.gap2 * (1.0 + 1e-9);
    double diag2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        if (!(scale[a] > 0.0)) return false;
        g.s[a] = scale[a];
        g.c[a] = cell ? cell[a] : 1; g.b[a] = bits ? bits[a] : 0;
        if (g.c[a] < 1 || g.b[a] < 0 || g.b[a] > 31) return false;
        const double d = (double)(g.c[a] - 1) * scale[a];
        diag2 += d * d;
        const double r = std::floor(gap / ((double)g.c[a] * scale[a])) + 1.0;
        if (r > 64.0) return false;
        g.r[a] = (int)r;
    }
    return diag2 < g.gap2;                                   // the voxels of one cell must be connected without a test
}

}  // namespace

extern "C" {

size_t sd_syn_ssv_temp_bytes(size_t n_vox) {
    const size_t n = n_vox ? n_vox : 1;
    SsvCompScratch c; SsvStatScratch t;
    return std::max(layout(c, nullptr, n), layout(t, nullptr, n));
}

int sd_syn_ssv_components(const int32_t* vox_dev, const uint32_t* vox_frag_dev, const uint32_t* frag_group_dev, const int32_t* group_origin_dev,
                          size_t n_vox, size_t n_frag, size_t n_group, const double* scale_host, double gap_nm, const int32_t* cell_host,
                          const int32_t* bits_host, int stages, int32_t* labels_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes,
                          void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_syn_ssv_components";
    if (!counts_dev) return fail(who, ": null counts");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (stages & 1)
        if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (n_vox == 0) return SD_OK;
    if (!vox_dev || !vox_frag_dev || !frag_group_dev || !group_origin_dev || !labels_dev || !n_frag || !n_group)
        return fail(who, ": bad argument");
    if (n_vox >= LIM31) return fail(who, ": < 2^31 voxel rows per call");
    SsvGeom g;
    if (!ssv_geom(scale_host, gap_nm, cell_host, bits_host, g))
        return fail(who, ": bad geometry (the scaled diagonal of a cell must be below the gap)");
    int gbits = 0;
    while (gbits < 64 && ((u64)(n_group - 1) >> gbits)) ++gbits;
    const int kbits = gbits + g.b[0] + g.b[1] + g.b[2];
    if (kbits > 63) return fail(who, ": group and cell coordinates need more than 63 key bits");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_syn_ssv_temp_bytes(n_vox), "sd_syn_ssv_temp_bytes(n_vox)"); rc != SD_OK) return rc;
    SsvCompScratch w;
    layout(w, temp_dev, n_vox);
    const u64 n = n_vox;
    if (stages & 1) {
        launch_1d(k_ssv_keys, n, 4096, s, vox_dev, vox_frag_dev, frag_group_dev, group_origin_dev, n, (u64)n_frag, (u64)n_group, g, w.key, counts);
        if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, n_vox, kbits > 0 ? kbits : 1, s); rc != SD_OK) return rc;
        if (int rc = number_segments(who, w.prim, w.skey, nullptr, w.head, w.seg, n_vox, s); rc != SD_OK) return rc;
        launch_1d(k_ssv_cells, n, 4096, s, w.skey, w.head, w.seg, n, w.cell_start, w.cell_key, w.parent, w.minflat, w.box, counts);
        launch_1d(k_ssv_cell_boxes, n, 4096, s, vox_dev, w.perm, w.seg, n, w.svox, w.box);
    }
    if (stages & 2) {
        launch_1d(k_ssv_link, 64 * n, 4096, s, w.svox, w.cell_start, w.cell_key, w.box, w.parent, g, counts);
        launch_1d(k_ssv_compress, n, 4096, s, w.parent, counts);
    }
    if (stages & 4) {
        if (hipMemsetAsync(w.flag, 0, n * sizeof(u32), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
        launch_1d(k_ssv_rootmin, n, 4096, s, w.parent, w.cell_start, w.perm, w.minflat, counts);
        launch_1d(k_ssv_flag, n, 4096, s, w.parent, w.minflat, w.flag, counts);
        if (int rc = scan_u32(who, w.prim, w.flag, w.fscan, n_vox, s); rc != SD_OK) return rc;
        launch_1d(k_ssv_labels, n, 4096, s, w.perm, w.seg, w.parent, w.minflat, w.fscan, n, labels_dev, counts);
    }
    return launch_status("sd_syn_ssv_components: launch failed");
}

int sd_syn_ssv_stats(const int32_t* vox_dev, const uint32_t* vox_frag_dev, const int32_t* labels_dev, size_t n_vox, size_t n_comp,
                     const double* scale_host, uint64_t min_obj_vx, uint32_t* comp_begin_dev, int32_t* bbox_dev, uint32_t* rep_flat_dev,
                     uint32_t* pair_comp_dev, uint32_t* pair_frag_dev, uint32_t* pair_begin_dev, uint32_t* vox_out_dev, uint64_t* counts_dev,
                     void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_syn_ssv_stats";
    if (!counts_dev) return fail(who, ": null counts");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 4, s); rc != SD_OK) return rc;
    if (n_vox == 0) return SD_OK;
    if (!vox_dev || !vox_frag_dev || !labels_dev || !n_comp || n_comp > n_vox || !comp_begin_dev || !bbox_dev || !rep_flat_dev || !pair_comp_dev ||
        !pair_frag_dev || !pair_begin_dev || !vox_out_dev)
        return fail(who, ": bad argument");
    if (n_vox >= LIM31) return fail(who, ": < 2^31 voxel rows per call");
    SsvGeom g{};
    if (!scale_host) return fail(who, ": null scale");
    for (int a = 0; a < 3; ++a) {
        if (!(scale_host[a] > 0.0)) return fail(who, ": bad scale");
        g.s[a] = scale_host[a];
    }
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_syn_ssv_temp_bytes(n_vox), "sd_syn_ssv_temp_bytes(n_vox)"); rc != SD_OK) return rc;
    SsvStatScratch w;
    layout(w, temp_dev, n_vox);
    const u64 n = n_vox, K = n_comp;
    launch_1d(k_ssv_compkeys, n, 4096, s, labels_dev, n, K, w.key, counts);
    if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.sflat, n_vox, 32, s); rc != SD_OK) return rc;
    launch_1d(k_ssv_stat_init, K, 4096, s, K, bbox_dev, w.sums, w.best, rep_flat_dev);
    launch_1d(k_ssv_stat_heads, n, 4096, s, w.skey, w.sflat, vox_frag_dev, n, w.headp, comp_begin_dev);
    if (int rc = scan_u32(who, w.prim, w.headp, w.pscan, n_vox, s); rc != SD_OK) return rc;
    launch_1d(k_ssv_stat_pairs, n, 4096, s, w.skey, w.sflat, vox_frag_dev, w.headp, w.pscan, n, pair_comp_dev, pair_frag_dev, pair_begin_dev, counts);
    launch_1d(k_ssv_stat_reduce, n, 4096, s, vox_dev, w.skey, w.sflat, n, bbox_dev, w.sums);
    launch_1d(k_ssv_stat_dist, n, 4096, s, vox_dev, w.skey, w.sflat, comp_begin_dev, w.sums, n, g, w.d2bits, w.best);
    launch_1d(k_ssv_stat_rep, n, 4096, s, w.skey, w.sflat, w.d2bits, w.best, n, rep_flat_dev);
    launch_1d(k_ssv_stat_keep, n, 4096, s, w.skey, comp_begin_dev, n, (u64)min_obj_vx, w.keep);
    if (int rc = scan_u32(who, w.prim, w.keep, w.kscan, n_vox, s); rc != SD_OK) return rc;
    launch_1d(k_ssv_stat_gather, n, 4096, s, vox_dev, w.sflat, w.keep, w.kscan, n, vox_out_dev, counts);
    return launch_status("sd_syn_ssv_stats: launch failed");
}

}  // extern "C"
