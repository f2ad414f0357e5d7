// Surface meshes of all labelled objects of a chunk in one pass, and the merge of per-chunk meshes (include/syconn_dense.h, "surface
// meshes"): the unsimplified marching-cubes surface of every "label == id" volume, over the table of tools/gen_mc_table.py.
//   volume     the padded / zoomed array is never made: padded[i, j, k] = vol[tx[i], ty[j], tz[k]] is read through the three tables.
//   records    a voxel v of the padded array owns the three grid edges that start at it (a vertex for either label of an edge whose
//              labels differ) and the cube whose lowest corner it is (per distinct non-zero corner label the triangles of its mask).
//              256 consecutive voxels are one item of the voxel kernels: a count pass, a scan over the items, and an emit pass that
//              repeats the count inside the block to place every record -- so records leave in voxel order, and ONE stable radix sort
//              by the label's rank (its index in the caller's ascending id list) makes them ascend by (object, key) / (object, cube,
//              table order).  No atomic decides a position; the two totals are counted with integer atomics.
//   indices    a triangle finds its three vertices by binary search in its object's ascending keys.
//   per object bounding box and area by one wave per object, lanes striding over its vertices / triangles, a fixed shuffle tree:
//              area is a fixed-order float64 sum.  No float atomics.
// Nothing is written past a given capacity: every record, vertex and triangle write is guarded by it, and counts[2] reports the loss.
#define SD_MC_TABLE_QUALIFIER __device__ const
#include "sd_mc_table.h"
#include "sd_sortseg.h"

namespace {

const int GRID = SD_MESH_GRID;

// Where a voxel sits: voxel i at coordinate i + MESH_HALF_VOXEL_SHIFT (in voxels of the padded array).  0 = voxel i at coordinate i; whether
// zmesh puts it at i + 0.5 has not been checked.  The ONE place that decides it.
__device__ const double MESH_HALF_VOXEL_SHIFT = 0.0;

struct Vol {
    const u64* lab;
    const int *tx, *ty, *tz;
    int X, Y, Z, NX, NY, NZ;
};

// source index of padded index i: -1 (scipy's constant, label 0) or [0, n_src); anything else is a bad table and reads as -1
__device__ __forceinline__ int src_index(const int* t, int i, int n_src) {
    const int s = t[i];
    return (s >= 0 && s < n_src) ? s : -1;
}
__device__ __forceinline__ u64 vol_at(const Vol& V, int sx, int sy, int sz) {
    if ((sx | sy | sz) < 0) return 0;
    return V.lab[((u64)sx * V.Y + sy) * V.Z + sz];
}

__global__ __launch_bounds__(256) void k_mesh_check_table(const int* __restrict__ t, u64 n, int n_src, u64* counts) {
    for (u64 i = grid_tid(); i < n; i += grid_stride())
        if (t[i] < -1 || t[i] >= n_src) counts[7] = 1;
}

// The records of voxel v: counted in (nv, nt) and, with EMIT, written at vbase + nv / tbase + nt.  A label that is not in ids raises
// counts[6] and has no records.
template <bool EMIT>
__device__ __forceinline__ void voxel_records(const Vol& V, u64 v, const u64* __restrict__ ids, u64 n_ids, u32& nv, u32& nt, u64 vbase, u64 tbase,
                                              u64 vcap, u64 tcap, u64* vrank, u64* vkey, u64* trank, u64* tpack, u64* counts) {
    nv = nt = 0;
    const int z = (int)(v % (u64)V.NZ), y = (int)((v / (u64)V.NZ) % (u64)V.NY), x = (int)(v / ((u64)V.NZ * V.NY));
    const bool h[3] = {x + 1 < V.NX, y + 1 < V.NY, z + 1 < V.NZ};
    const int sx[2] = {src_index(V.tx, x, V.X), h[0] ? src_index(V.tx, x + 1, V.X) : -1};
    const int sy[2] = {src_index(V.ty, y, V.Y), h[1] ? src_index(V.ty, y + 1, V.Y) : -1};
    const int sz[2] = {src_index(V.tz, z, V.Z), h[2] ? src_index(V.tz, z + 1, V.Z) : -1};
    u64 L[8];
    bool same = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
        L[c] = ((!dx || h[0]) && (!dy || h[1]) && (!dz || h[2])) ? vol_at(V, sx[dx], sy[dy], sz[dz]) : 0;
        same = same && L[c] == L[0];
    }
    if (same) return;                                        // the bulk: eight equal corners, no edge crosses and no triangle
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!h[a] || L[0] == L[1 << a]) continue;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const u64 lab = side ? L[1 << a] : L[0];
            if (!lab) continue;
            const long r = find_exact(ids, n_ids, lab);
            if (r < 0) { counts[6] = 1; continue; }
            if (EMIT) {
                const u64 pos = vbase + nv;
                if (pos < vcap) { vrank[pos] = (u64)r; vkey[pos] = v * 3 + a; }
            }
            ++nv;
        }
    }
    if (!(h[0] && h[1] && h[2])) return;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const u64 lab = L[c];
        if (!lab) continue;
        bool first = true;
        u32 mask = 0;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            if (L[d] == lab) { mask |= 1u << d; if (d < c) first = false; }
        }
        if (!first) continue;
        const u32 n = SD_MC_COUNT[mask];
        if (!n) continue;
        const long r = find_exact(ids, n_ids, lab);
        if (r < 0) { counts[6] = 1; continue; }
        if (EMIT) {
            for (u32 t = 0; t < n; ++t) {
                const u64 pos = tbase + nt + t;
                if (pos < tcap) { trank[pos] = (u64)r; tpack[pos] = v | ((u64)mask << 32) | ((u64)t << 40); }
            }
        }
        nt += n;
    }
}

// One item = 256 consecutive voxels.  Count pass: item_nv / item_nt (may be null: totals only) and the totals counts[0] / counts[1].
__global__ __launch_bounds__(256) void k_mesh_count(Vol V, u64 n_vox, u64 n_items, const u64* __restrict__ ids, u64 n_ids, u32* item_nv, u32* item_nt,
                                                    u64* counts) {
    __shared__ u32 sh[256];
    for (u64 it = blockIdx.x; it < n_items; it += gridDim.x) {
        const u64 v = it * 256 + threadIdx.x;
        u32 nv = 0, nt = 0;
        if (v < n_vox) voxel_records<false>(V, v, ids, n_ids, nv, nt, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, counts);
        sh[threadIdx.x] = nv | (nt << 16);                   // at most 6 and 40 per voxel: 256 of them fit 16 bits each
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const u32 tv = sh[0] & 0xffffu, tt = sh[0] >> 16;
            if (item_nv) { item_nv[it] = tv; item_nt[it] = tt; }
            if (tv) atomicAdd(&counts[0], (u64)tv);
            if (tt) atomicAdd(&counts[1], (u64)tt);
        }
        __syncthreads();
    }
}

// Emit pass: scan_nv / scan_nt are the inclusive scans of the item counts; inside an item a block scan of the per-voxel counts.
__global__ __launch_bounds__(256) void k_mesh_emit(Vol V, u64 n_vox, u64 n_items, const u64* __restrict__ ids, u64 n_ids, const u32* __restrict__ item_nv,
                                                   const u32* __restrict__ item_nt, const u32* __restrict__ scan_nv, const u32* __restrict__ scan_nt,
                                                   u64 vcap, u64 tcap, u64* vrank, u64* vkey, u64* trank, u64* tpack, u64* counts) {
    __shared__ u32 sh[256];
    for (u64 it = blockIdx.x; it < n_items; it += gridDim.x) {
        if (item_nv[it] == 0 && item_nt[it] == 0) continue;  // the same for the whole block
        const u64 v = it * 256 + threadIdx.x;
        u32 nv = 0, nt = 0;
        if (v < n_vox) voxel_records<false>(V, v, ids, n_ids, nv, nt, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, counts);
        const u32 own = nv | (nt << 16);
        sh[threadIdx.x] = own;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {                  // inclusive scan
            const u32 add = (int)threadIdx.x >= s ? sh[threadIdx.x - s] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        const u32 before = sh[threadIdx.x] - own;
        __syncthreads();
        if (own) {
            const u64 vbase = (u64)(scan_nv[it] - item_nv[it]) + (before & 0xffffu), tbase = (u64)(scan_nt[it] - item_nt[it]) + (before >> 16);
            voxel_records<true>(V, v, ids, n_ids, nv, nt, vbase, tbase, vcap, tcap, vrank, vkey, trank, tpack, counts);
        }
    }
}

__global__ __launch_bounds__(256) void k_mesh_fill(u64* a, u64 n, u64 value) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) a[i] = value;
}
__global__ __launch_bounds__(256) void k_mesh_gather(const u64* __restrict__ in, const u32* __restrict__ perm, u64 n, u64* out) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) out[i] = in[perm[i] < n ? perm[i] : 0];
}
// vert_begin / tri_begin [n_obj + 1] from the sorted ranks (records beyond the last object carry rank n_obj); counts[2]: records lost
__global__ __launch_bounds__(256) void k_mesh_begin(const u64* __restrict__ vrank_s, u64 vcap, const u64* __restrict__ trank_s, u64 tcap, u64 n_obj,
                                                    u64 vert_cap, u64 tri_cap, u64* vert_begin, u64* tri_begin, u64* counts) {
    for (u64 o = grid_tid(); o <= n_obj; o += grid_stride()) {
        vert_begin[o] = lower_bound(vrank_s, vcap, o);
        tri_begin[o] = lower_bound(trank_s, tcap, o);
        if (o == 0 && (counts[0] > vert_cap || counts[1] > tri_cap)) counts[2] = 1;
    }
}

#pragma clang fp contract(off)                              // every product and sum rounded on its own, as numpy does
__global__ __launch_bounds__(256) void k_mesh_verts(const u64* __restrict__ vrank_s, const u64* __restrict__ vkey_s, u64 vcap, u64 n_obj, int NY, int NZ,
                                                    double sx, double sy, double sz, double ox, double oy, double oz, float* verts) {
    const double s[3] = {sx, sy, sz}, o[3] = {ox, oy, oz};
    for (u64 i = grid_tid(); i < vcap; i += grid_stride()) {
        if (vrank_s[i] >= n_obj) continue;
        const u64 key = vkey_s[i], v = key / 3;
        const int a = (int)(key % 3);
        const double g[3] = {(double)(v / ((u64)NZ * NY)), (double)((v / (u64)NZ) % (u64)NY), (double)(v % (u64)NZ)};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double c = (g[k] + (k == a ? 0.5 : 0.0) + MESH_HALF_VOXEL_SHIFT) * s[k] + o[k];
            verts[i * 3 + k] = (float)(c < 0 ? 0.0 : c);
        }
    }
}

__global__ __launch_bounds__(256) void k_mesh_tris(const u64* __restrict__ trank_s, const u32* __restrict__ tperm, const u64* __restrict__ tpack, u64 tcap,
                                                   u64 n_obj, const u64* __restrict__ vert_begin, const u64* __restrict__ vkey_s, u64 vcap, int NY, int NZ,
                                                   u32* tris, u64* counts) {
    for (u64 i = grid_tid(); i < tcap; i += grid_stride()) {
        const u64 r = trank_s[i];
        if (r >= n_obj) continue;
        const u64 p = tpack[tperm[i] < tcap ? tperm[i] : 0];
        const u64 v = p & 0xffffffffull;
        const u32 mask = (u32)(p >> 32) & 0xffu, t = (u32)(p >> 40) & 7u;
        const u64 vb = clamp_u64(vert_begin[r], vcap), ve = clamp_u64(vert_begin[r + 1], vcap);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u32 e = SD_MC_EDGES[mask][(t * 3 + k) % 15] % 12, a = e >> 2, j = e & 3;
            const u32 c0 = a == 0 ? j * 2 : (a == 1 ? (j & 1) | ((j >> 1) << 2) : j);        // the j-th corner with coordinate 0 on axis a
            const u64 key = (v + (u64)(c0 & 1) * NY * NZ + (u64)((c0 >> 1) & 1) * NZ + (c0 >> 2)) * 3 + a;
            const long at = ve > vb ? find_exact(vkey_s + vb, ve - vb, key) : -1;
            if (at < 0) counts[5] = 1;                       // only after lost records (counts[2])
            tris[i * 3 + k] = at < 0 ? 0xffffffffu : (u32)at;
        }
    }
}

// One wave per object: the box of its vertices (zeros without vertices) and its area in um^2.  Lane l takes items l, l + 64, ..; the
// partial results meet in a fixed xor tree.  n_obj_dev (may be null) holds the number of objects where only the device knows it.
__global__ __launch_bounds__(256) void k_mesh_props(const u64* __restrict__ vert_begin, const u64* __restrict__ tri_begin, u64 n_obj, const u64* n_obj_dev,
                                                    const float* __restrict__ verts, u64 n_verts, const u32* __restrict__ tris, u64 n_tris, float* bb,
                                                    double* area) {
    const int lane = threadIdx.x & 63;
    if (n_obj_dev) n_obj = clamp_u64(*n_obj_dev, n_obj);
    for (u64 o = grid_tid() >> 6; o < n_obj; o += grid_stride() >> 6) {
        const u64 vb = clamp_u64(vert_begin[o], n_verts), ve = clamp_u64(vert_begin[o + 1], n_verts);
        const u64 tb = clamp_u64(tri_begin[o], n_tris), te = clamp_u64(tri_begin[o + 1], n_tris);
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (u64 i = vb + lane; i < ve; i += 64)
#pragma unroll
            for (int k = 0; k < 3; ++k) { const float c = verts[i * 3 + k]; lo[k] = fminf(lo[k], c); hi[k] = fmaxf(hi[k], c); }
        double sum = 0.0;
        for (u64 i = tb + lane; i < te; i += 64) {
            const u64 i0 = tris[i * 3], i1 = tris[i * 3 + 1], i2 = tris[i * 3 + 2], nv = ve > vb ? ve - vb : 0;
            if (i0 >= nv || i1 >= nv || i2 >= nv) continue;
            double p[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { p[0][k] = verts[(vb + i0) * 3 + k]; p[1][k] = verts[(vb + i1) * 3 + k]; p[2][k] = verts[(vb + i2) * 3 + k]; }
            const double ax = p[0][0] - p[1][0], ay = p[0][1] - p[1][1], az = p[0][2] - p[1][2];
            const double bx = p[0][0] - p[2][0], by = p[0][1] - p[2][1], bz = p[0][2] - p[2][2];
            const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            sum += __dsqrt_rn((cx * cx + cy * cy) + cz * cz);
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], m)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], m)); }
            sum += __shfl_xor(sum, m);
        }
        if (lane == 0) {
            const bool any = ve > vb;
#pragma unroll
            for (int k = 0; k < 3; ++k) { bb[o * 6 + k] = any ? lo[k] : 0.f; bb[o * 6 + 3 + k] = any ? hi[k] : 0.f; }
            area[o] = sum / 2.0 / 1e6;
        }
    }
}

// ---- the merge of per-chunk pieces ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_merge_sizes(const u32* __restrict__ perm, const u64* __restrict__ vb, const u64* __restrict__ tb, u64 n, u32* nv,
                                                     u32* nt) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        const u64 p = perm[i] < n ? perm[i] : 0;
        nv[i] = vb[p + 1] > vb[p] ? (u32)(vb[p + 1] - vb[p]) : 0u;
        nt[i] = tb[p + 1] > tb[p] ? (u32)(tb[p + 1] - tb[p]) : 0u;
    }
}
// per object (the head of its run of pieces): id and offsets; the last piece closes the tables and counts the objects
__global__ __launch_bounds__(256) void k_merge_objects(const u64* __restrict__ ids_s, const u32* __restrict__ head, const u32* __restrict__ seg,
                                                       const u32* __restrict__ nv, const u32* __restrict__ nt, const u32* __restrict__ sv,
                                                       const u32* __restrict__ st, u64 n, u64* obj_ids, u64* vert_begin, u64* tri_begin, u64* counts) {
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        if (head[i]) {
            const u64 o = seg[i] - 1;
            obj_ids[o] = ids_s[i];
            vert_begin[o] = sv[i] - nv[i];
            tri_begin[o] = st[i] - nt[i];
        }
        if (i == n - 1) { vert_begin[seg[i]] = sv[i]; tri_begin[seg[i]] = st[i]; counts[0] = seg[i]; }
    }
}
__global__ __launch_bounds__(256) void k_merge_verts(const u32* __restrict__ perm, const u64* __restrict__ vb, const u32* __restrict__ nv,
                                                     const u32* __restrict__ sv, u64 n_pieces, const float* __restrict__ verts, u64 n_verts, float* out) {
    for (u64 j = grid_tid(); j < n_verts; j += grid_stride()) {
        const u64 i = clamp_u64(upper_bound(sv, n_pieces, j), n_pieces - 1);
        const u64 src = vb[perm[i] < n_pieces ? perm[i] : 0] + (j - (u64)(sv[i] - nv[i]));
        if (src >= n_verts) continue;                        // only with a bad offset table (counts[7])
#pragma unroll
        for (int k = 0; k < 3; ++k) out[j * 3 + k] = verts[src * 3 + k];
    }
}
__global__ __launch_bounds__(256) void k_merge_tris(const u32* __restrict__ perm, const u64* __restrict__ tb, const u32* __restrict__ nt,
                                                    const u32* __restrict__ st, const u32* __restrict__ nv, const u32* __restrict__ sv,
                                                    const u32* __restrict__ seg, const u64* __restrict__ vert_begin, u64 n_pieces,
                                                    const u32* __restrict__ tris, u64 n_tris, u32* out) {
    for (u64 j = grid_tid(); j < n_tris; j += grid_stride()) {
        const u64 i = clamp_u64(upper_bound(st, n_pieces, j), n_pieces - 1);
        const u64 src = tb[perm[i] < n_pieces ? perm[i] : 0] + (j - (u64)(st[i] - nt[i]));
        if (src >= n_tris) continue;
        const u32 shift = (u32)((u64)(sv[i] - nv[i]) - vert_begin[seg[i] - 1]);                 // the piece's first vertex inside its object
#pragma unroll
        for (int k = 0; k < 3; ++k) out[j * 3 + k] = tris[src * 3 + k] + shift;
    }
}

struct BuildScratch {
    u32 *item_nv, *item_nt, *scan_nv, *scan_nt, *vi0, *vperm, *ti0, *tperm;
    u64 *vrank, *vrank_s, *vkey, *vkey_s, *trank, *trank_s, *tpack;
    PrimScratch prim;
};
size_t layout(BuildScratch& w, void* base, size_t n_items, size_t vcap, size_t tcap) {
    ScratchAlloc a(base);
    a.take_into(n_items, w.item_nv, w.item_nt, w.scan_nv, w.scan_nt);
    a.take_into(vcap, w.vi0, w.vperm);
    a.take_into(tcap, w.ti0, w.tperm);
    a.take_into(vcap, w.vrank, w.vrank_s, w.vkey, w.vkey_s);
    a.take_into(tcap, w.trank, w.trank_s, w.tpack);
    w.prim = take_prim(a, std::max(n_items, std::max(vcap, tcap)));
    return a.used;
}
struct MergeScratch {
    u64* ids_s;
    u32 *i0, *perm, *head, *seg, *nv, *nt, *sv, *st;
    PrimScratch prim;
};
size_t layout(MergeScratch& w, void* base, size_t n) {
    ScratchAlloc a(base);
    a.take_into(n, w.ids_s);
    a.take_into(n, w.i0, w.perm, w.head, w.seg, w.nv, w.nt, w.sv, w.st);
    w.prim = take_prim(a, n);
    return a.used;
}

// the checks both volume entries open with; fills V
int open_volume(const char* who, const uint64_t* labels_dev, int X, int Y, int Z, const int32_t* tx_dev, const int32_t* ty_dev, const int32_t* tz_dev, int NX,
                int NY, int NZ, const uint64_t* ids_dev, size_t n_ids, Vol& V, size_t& n_vox) {
    if (X < 1 || Y < 1 || Z < 1 || NX < 1 || NY < 1 || NZ < 1) return fail(who, ": extents must be positive");
    n_vox = (size_t)NX * (size_t)NY * (size_t)NZ;
    if (n_vox > LIM31 || n_ids >= LIM31) return fail(who, ": the padded volume holds at most 2^31 voxels, and ids < 2^31 per call");
    if (!labels_dev || !tx_dev || !ty_dev || !tz_dev || (n_ids && !ids_dev)) return fail(who, ": bad argument");
    V = Vol{reinterpret_cast<const u64*>(labels_dev), tx_dev, ty_dev, tz_dev, X, Y, Z, NX, NY, NZ};
    return SD_OK;
}
void check_tables(const Vol& V, const u64* ids, size_t n_ids, u64* counts, hipStream_t s) {
    launch_1d(k_mesh_check_table, V.NX, GRID, s, V.tx, (u64)V.NX, V.X, counts);
    launch_1d(k_mesh_check_table, V.NY, GRID, s, V.ty, (u64)V.NY, V.Y, counts);
    launch_1d(k_mesh_check_table, V.NZ, GRID, s, V.tz, (u64)V.NZ, V.Z, counts);
    if (n_ids) launch_1d(k_check_ascending, n_ids, GRID, s, ids, (u64)n_ids, counts);
}
inline int items_grid(size_t n_items) { return (int)std::min<size_t>(std::max<size_t>(n_items, 1), GRID); }

}  // namespace

extern "C" {

int sd_mesh_count(const uint64_t* labels_dev, int X, int Y, int Z, const int32_t* tx_dev, const int32_t* ty_dev, const int32_t* tz_dev, int NX, int NY, int NZ,
                  const uint64_t* ids_dev, size_t n_ids, uint64_t* counts_dev, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_mesh_count";
    if (!counts_dev) return fail(who, ": null counts");
    Vol V;
    size_t n_vox;
    if (int rc = open_volume(who, labels_dev, X, Y, Z, tx_dev, ty_dev, tz_dev, NX, NY, NZ, ids_dev, n_ids, V, n_vox); rc != SD_OK) return rc;
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    const u64* ids = reinterpret_cast<const u64*>(ids_dev);
    check_tables(V, ids, n_ids, counts, s);
    const size_t n_items = (n_vox + 255) / 256;
    hipLaunchKernelGGL(k_mesh_count, dim3(items_grid(n_items)), dim3(256), 0, s, V, (u64)n_vox, (u64)n_items, ids, (u64)n_ids, (u32*)nullptr, (u32*)nullptr,
                       counts);
    return launch_status("sd_mesh_count: launch failed");
}

size_t sd_mesh_build_temp_bytes(int NX, int NY, int NZ, size_t vert_cap, size_t tri_cap) {
    if (NX < 1 || NY < 1 || NZ < 1) return 0;
    const size_t n_vox = (size_t)NX * (size_t)NY * (size_t)NZ;
    if (n_vox > LIM31 || vert_cap >= LIM31 || tri_cap >= LIM31) return 0;
    BuildScratch w;
    return layout(w, nullptr, (n_vox + 255) / 256, std::max<size_t>(vert_cap, 1), std::max<size_t>(tri_cap, 1));
}

int sd_mesh_build(const uint64_t* labels_dev, int X, int Y, int Z, const int32_t* tx_dev, const int32_t* ty_dev, const int32_t* tz_dev, int NX, int NY, int NZ,
                  const uint64_t* ids_dev, size_t n_ids, const double* scale_xyz, const double* offset_xyz, size_t vert_cap, size_t tri_cap,
                  uint64_t* vert_begin_dev, uint64_t* tri_begin_dev, float* verts_dev, uint32_t* tris_dev, float* mesh_bb_dev, double* area_dev,
                  uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_mesh_build";
    if (!counts_dev) return fail(who, ": null counts");
    Vol V;
    size_t n_vox;
    if (int rc = open_volume(who, labels_dev, X, Y, Z, tx_dev, ty_dev, tz_dev, NX, NY, NZ, ids_dev, n_ids, V, n_vox); rc != SD_OK) return rc;
    if (vert_cap >= LIM31 || tri_cap >= LIM31) return fail(who, ": vertices and triangles < 2^31 per call");
    if (!scale_xyz || !offset_xyz || !vert_begin_dev || !tri_begin_dev || !verts_dev || !tris_dev || (n_ids && (!mesh_bb_dev || !area_dev)))
        return fail(who, ": bad argument");
    for (int k = 0; k < 3; ++k)
        if (!(scale_xyz[k] > 0) || offset_xyz[k] != offset_xyz[k]) return fail(who, ": scale must be positive and the offset a number");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    const size_t vcap = std::max<size_t>(vert_cap, 1), tcap = std::max<size_t>(tri_cap, 1), n_items = (n_vox + 255) / 256;
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_mesh_build_temp_bytes(NX, NY, NZ, vert_cap, tri_cap),
                               "sd_mesh_build_temp_bytes(NX, NY, NZ, vert_cap, tri_cap)"); rc != SD_OK) return rc;
    BuildScratch w;
    layout(w, temp_dev, n_items, vcap, tcap);
    const u64* ids = reinterpret_cast<const u64*>(ids_dev);
    const u64 N = n_ids;
    check_tables(V, ids, n_ids, counts, s);
    hipLaunchKernelGGL(k_mesh_count, dim3(items_grid(n_items)), dim3(256), 0, s, V, (u64)n_vox, (u64)n_items, ids, N, w.item_nv, w.item_nt, counts);
    if (int rc = scan_u32(who, w.prim, w.item_nv, w.scan_nv, n_items, s); rc != SD_OK) return rc;
    if (int rc = scan_u32(who, w.prim, w.item_nt, w.scan_nt, n_items, s); rc != SD_OK) return rc;
    launch_1d(k_mesh_fill, vcap, GRID, s, w.vrank, (u64)vcap, N);                              // records nobody writes sort behind every object
    launch_1d(k_mesh_fill, tcap, GRID, s, w.trank, (u64)tcap, N);
    // the scratch capacities are those of the caller's outputs, except that an output of 0 rows has one scratch row nobody may write
    hipLaunchKernelGGL(k_mesh_emit, dim3(items_grid(n_items)), dim3(256), 0, s, V, (u64)n_vox, (u64)n_items, ids, N, w.item_nv, w.item_nt, w.scan_nv,
                       w.scan_nt, (u64)vert_cap, (u64)tri_cap, w.vrank, w.vkey, w.trank, w.tpack, counts);
    const int bits = std::max(1, bits_for(N + 1));
    if (int rc = sort_by_key(who, w.prim, w.vrank, w.vrank_s, w.vi0, w.vperm, vcap, bits, s); rc != SD_OK) return rc;
    if (int rc = sort_by_key(who, w.prim, w.trank, w.trank_s, w.ti0, w.tperm, tcap, bits, s); rc != SD_OK) return rc;
    launch_1d(k_mesh_gather, vcap, GRID, s, w.vkey, w.vperm, (u64)vcap, w.vkey_s);
    u64 *vert_begin = reinterpret_cast<u64*>(vert_begin_dev), *tri_begin = reinterpret_cast<u64*>(tri_begin_dev);
    launch_1d(k_mesh_begin, N + 1, GRID, s, w.vrank_s, (u64)vcap, w.trank_s, (u64)tcap, N, (u64)vert_cap, (u64)tri_cap, vert_begin, tri_begin, counts);
    if (vert_cap)
        launch_1d(k_mesh_verts, vert_cap, GRID, s, w.vrank_s, w.vkey_s, (u64)vert_cap, N, NY, NZ, scale_xyz[0], scale_xyz[1], scale_xyz[2], offset_xyz[0],
                  offset_xyz[1], offset_xyz[2], verts_dev);
    if (tri_cap)
        launch_1d(k_mesh_tris, tri_cap, GRID, s, w.trank_s, w.tperm, w.tpack, (u64)tri_cap, N, vert_begin, w.vkey_s, (u64)vert_cap, NY, NZ, tris_dev, counts);
    if (N)
        launch_1d(k_mesh_props, N * 64, GRID, s, vert_begin, tri_begin, N, (const u64*)nullptr, verts_dev, (u64)vert_cap, tris_dev, (u64)tri_cap, mesh_bb_dev,
                  area_dev);
    return launch_status("sd_mesh_build: launch failed");
}

size_t sd_mesh_merge_temp_bytes(size_t n_pieces) {
    if (n_pieces >= LIM31) return 0;
    MergeScratch w;
    return layout(w, nullptr, std::max<size_t>(n_pieces, 1));
}

int sd_mesh_merge(const uint64_t* piece_ids_dev, const uint64_t* piece_vert_begin_dev, const uint64_t* piece_tri_begin_dev, size_t n_pieces,
                  const float* verts_dev, size_t n_verts, const uint32_t* tris_dev, size_t n_tris, uint64_t* obj_ids_dev, uint64_t* vert_begin_dev,
                  uint64_t* tri_begin_dev, float* verts_out_dev, uint32_t* tris_out_dev, float* mesh_bb_dev, double* area_dev, uint64_t* counts_dev,
                  void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_mesh_merge";
    if (!counts_dev || !vert_begin_dev || !tri_begin_dev) return fail(who, ": null counts or offsets");
    if (n_pieces >= LIM31 || n_verts >= LIM31 || n_tris >= LIM31) return fail(who, ": pieces, vertices and triangles < 2^31 per call");
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (int rc = zero_counts(counts, 8, s); rc != SD_OK) return rc;
    if (hipMemsetAsync(vert_begin_dev, 0, sizeof(u64), s) != hipSuccess || hipMemsetAsync(tri_begin_dev, 0, sizeof(u64), s) != hipSuccess)
        return sd_fail_msg(SD_ERR_HIP, "memset failed");
    if (n_pieces == 0) {
        if (n_verts || n_tris) return fail(who, ": vertices or triangles without pieces");
        return launch_status("sd_mesh_merge: launch failed");
    }
    if (!piece_ids_dev || !piece_vert_begin_dev || !piece_tri_begin_dev || !obj_ids_dev || !mesh_bb_dev || !area_dev ||
        (n_verts && (!verts_dev || !verts_out_dev)) || (n_tris && (!tris_dev || !tris_out_dev)))
        return fail(who, ": bad argument");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_mesh_merge_temp_bytes(n_pieces), "sd_mesh_merge_temp_bytes(n_pieces)"); rc != SD_OK) return rc;
    MergeScratch w;
    layout(w, temp_dev, n_pieces);
    const u64 P = n_pieces, NV = n_verts, NT = n_tris;
    const u64 *pid = reinterpret_cast<const u64*>(piece_ids_dev), *vb = reinterpret_cast<const u64*>(piece_vert_begin_dev),
              *tb = reinterpret_cast<const u64*>(piece_tri_begin_dev);
    u64 *vert_begin = reinterpret_cast<u64*>(vert_begin_dev), *tri_begin = reinterpret_cast<u64*>(tri_begin_dev);
    launch_1d(k_check_offsets, P, GRID, s, vb, P, NV, counts);
    launch_1d(k_check_offsets, P, GRID, s, tb, P, NT, counts);
    if (int rc = sort_by_key(who, w.prim, pid, w.ids_s, w.i0, w.perm, n_pieces, 64, s); rc != SD_OK) return rc;
    if (int rc = number_segments(who, w.prim, w.ids_s, nullptr, w.head, w.seg, n_pieces, s); rc != SD_OK) return rc;
    launch_1d(k_merge_sizes, P, GRID, s, w.perm, vb, tb, P, w.nv, w.nt);
    if (int rc = scan_u32(who, w.prim, w.nv, w.sv, n_pieces, s); rc != SD_OK) return rc;
    if (int rc = scan_u32(who, w.prim, w.nt, w.st, n_pieces, s); rc != SD_OK) return rc;
    launch_1d(k_merge_objects, P, GRID, s, w.ids_s, w.head, w.seg, w.nv, w.nt, w.sv, w.st, P, reinterpret_cast<u64*>(obj_ids_dev), vert_begin, tri_begin, counts);
    if (NV) launch_1d(k_merge_verts, NV, GRID, s, w.perm, vb, w.nv, w.sv, P, verts_dev, NV, verts_out_dev);
    if (NT) launch_1d(k_merge_tris, NT, GRID, s, w.perm, tb, w.nt, w.st, w.nv, w.sv, w.seg, vert_begin, P, tris_dev, NT, tris_out_dev);
    launch_1d(k_mesh_props, P * 64, GRID, s, vert_begin, tri_begin, P, counts, verts_out_dev, NV, tris_out_dev, NT, mesh_bb_dev, area_dev);
    return launch_status("sd_mesh_merge: launch failed");
}

}  // extern "C"
