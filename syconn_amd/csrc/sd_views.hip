// Multi-view depth and index images of a mesh, the view rotations and the pixel -> vertex vote: the compute form of what the reference
// renders with OpenGL -- proc/rendering_egl.py _render_mesh_coords (:611-681), multi_view_mesh_coords (:460-590) and screen_shot
// (:130-174), proc/meshes.py MeshObject (:69-175), calc_rot_matrices (:236-329) and flag_empty_spaces (:332-360) with
// extraction/in_bounding_boxC.pyx, proc/rendering.py render_sso_coords_index_views (:300-396), and reps/super_segmentation_helper.py
// semseg2mesh_counter (:1527-1551) with the decision of semseg2mesh (:1603-1615).
//
//   normalise   vn = fl32(fl32(v - center) / max_dist) wherever a vertex or a location is read (the division in float64 and rounded
//               once more, which is the correctly rounded float32 quotient); no normalised copy exists.
//   rotations   the float32 vertices (every stride-th) sorted by a 30-bit Morton code into tiles of 64 with one box each
//               (sd_pointtiles.h).  One wave per location walks the tile boxes and reads only tiles that meet the query box; the test
//               per point is in_bounding_box's own (float32 difference, strict on both sides).  Count and sum, then the centred
//               products, both reduced over the wave by one fixed butterfly; covariance / (n - 1); cyclic Jacobi in float64; rows by
//               descending eigenvalue; the component of largest magnitude of every row positive.
//   index       a uniform grid over the normalised triangles keyed by centroid cell: one sort, cell offsets by binary search.  The
//               header keeps the largest distance of any vertex to its triangle's centroid, and whether any normalised vertex is not 0.
//   candidates  per location the triangles of the cells that meet the sphere of radius 0.5 |E| + that distance: count, scan, emit,
//               one wave per location, ascending by cell and by triangle inside a cell.  One list serves all views.
//   raster      one workgroup per (location, view, window tile); the tile's depth buffer lives in LDS: 32-bit depths (depth views) or
//               64-bit keys (depth << 32 | triangle: index views).  A lane sets up one candidate (transform, snap, cull); a triangle
//               whose box is small is drawn by its lane, a large one by the whole wave.  Coverage is exact in integers, the depth in
//               float64 with every operation rounded on its own.  Depth views then go to bytes in place, through the two filter
//               passes (truncating) and the all-zero rule, still in LDS, and are stored once.
//   vote        32-bit counts per (vertex, label) by integer atomics, read modulo 256 as the reference's uint8 table wraps; first
//               maximum; a wrapped sum of 0 is "unpredicted".
//
// Every index read from device memory is checked before it is used; every output write is guarded by the capacity given.  No float
// atomics, no scalar memory writes, no inline assembly.
#include "../../include/syconn_dense.h"
#include "sd_pointtiles.h"

#pragma clang fp contract(off)

namespace {

constexpr int GRID = SD_VIEWS_GRID;
constexpr int MAXV = SD_VIEWS_MAX_VIEWS;
constexpr u32 BG_INDEX = 0xfffffffeu;                          // rgba2id_array of a cleared pixel: 256^4 - 2
constexpr long long SNAP_LIM = 1ll << 22;
// counts slots
enum { C_N = 0, C_LOST = 1, C_TOOBIG = 2, C_BADIDX = 3, C_BADLABEL = 4, C_OVER31 = 6, C_BADTABLE = 7 };
// header of the index (u64 words)
enum { H_G = 0, H_NTRI = 1, H_NONZERO = 2, H_HMAX = 3, H_MIN = 4, H_MAX = 7, H_LO = 10, H_CS = 13, H_WORDS = 16 };

struct Norm { float c[3]; float md; };

__device__ __forceinline__ float norm1(float v, float c, float md) { return (float)((double)(v - c) / (double)md); }
__device__ __forceinline__ void norm3(const float* v, const Norm& nm, double* out) {
    for (int a = 0; a < 3; ++a) out[a] = (double)norm1(v[a], nm.c[a], nm.md);
}
// doubles <-> u64 keys with the same order
__device__ __forceinline__ u64 key_of(double v) {
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : b | (1ull << 63);
}
__device__ __forceinline__ double value_of(u64 k) { return __longlong_as_double((long long)((k >> 63) ? k & ~(1ull << 63) : ~k)); }
__device__ __forceinline__ u64 wave_min_u64(u64 v) {
    for (int m = 32; m; m >>= 1) { const u64 o = __shfl_xor(v, m); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
    for (int m = 32; m; m >>= 1) { const u64 o = __shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
    for (int m = 32; m; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ u64 wave_id() { return ((u64)blockIdx.x * 256 + threadIdx.x) >> 6; }
__device__ __forceinline__ u64 wave_count() { return ((u64)gridDim.x * 256) >> 6; }

// =====================================================================================================================================
// rotations
__device__ __forceinline__ u32 spread10(u32 v) {
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__global__ __launch_bounds__(256) void k_vw_rot_keys(const float* __restrict__ verts, u64 m, u64 stride, Norm nm, u64* key) {
    for (u64 i = grid_tid(); i < m; i += grid_stride()) {
        u32 code = 0;
        for (int a = 0; a < 3; ++a) {
            const float v = norm1(verts[3 * i * stride + a], nm.c[a], nm.md);
            const float q = (v + 1.0f) * 512.0f;
            const u32 c = !(q > 0.0f) ? 0u : (q >= 1023.0f ? 1023u : (u32)q);
            code |= spread10(c) << a;
        }
        key[i] = code;
    }
}
__global__ __launch_bounds__(256) void k_vw_rot_place(const float* __restrict__ verts, const u32* __restrict__ perm, u64 m, u64 stride, Norm nm, double* pts,
                                                      u64* begin) {
    for (u64 i = grid_tid(); i < m; i += grid_stride()) {
        const u64 j = clamp_u64(perm[i], m - 1);
        for (int a = 0; a < 3; ++a) pts[3 * i + a] = (double)norm1(verts[3 * j * stride + a], nm.c[a], nm.md);
    }
    if (grid_tid() == 0) { begin[0] = 0; begin[1] = m; }
}
// eigenvectors of the symmetric a (6 entries: xx xy xz yy yz zz) by cyclic Jacobi; rows of `rows` by descending eigenvalue, signed
__device__ void eig3_rows(const double* c6, double rows[3][3]) {
    double A[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 16; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (off == 0.0) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
                const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {                                      // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {                                      // A <- J^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                A[p][q] = A[q][p] = 0.0;
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 2; ++i)                                                    // stable: equal eigenvalues keep their column order
        for (int j = 0; j < 2 - i; ++j)
            if (A[ord[j + 1]][ord[j + 1]] > A[ord[j]][ord[j]]) { const int t = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = t; }
    for (int i = 0; i < 3; ++i) {
        double v[3] = {V[0][ord[i]], V[1][ord[i]], V[2][ord[i]]};
        int big = 0;
        for (int a = 1; a < 3; ++a)
            if (fabs(v[a]) > fabs(v[big])) big = a;
        const double sg = v[big] < 0.0 ? -1.0 : 1.0;
        for (int a = 0; a < 3; ++a) rows[i][a] = sg * v[a];
    }
}
// one wave per location: the inliers of in_bounding_box among the tiled points, their PCA
__global__ __launch_bounds__(256) void k_vw_rot_solve(const double* __restrict__ pts, const double* __restrict__ tbox, u64 n_slots, u64 m,
                                                      const float* __restrict__ coords, u64 n_loc, Norm nm, float h, double* rot, uint8_t* empty) {
    const int lane = threadIdx.x & 63;
    const u64 n_tiles = (m + TILE - 1) / TILE;
    for (u64 loc = wave_id(); loc < n_loc; loc += wave_count()) {
        float c[3];
        for (int a = 0; a < 3; ++a) c[a] = norm1(coords[3 * loc + a], nm.c[a], nm.md);
        double qlo[3], qhi[3];                                                      // the query box, widened beyond the rounding of fl32(v - c)
        for (int a = 0; a < 3; ++a) {
            const double slack = ((double)h + fabs((double)c[a])) * 0x1p-20;
            qlo[a] = (double)c[a] - (double)h - slack;
            qhi[a] = (double)c[a] + (double)h + slack;
        }
        double mean[3] = {0, 0, 0}, cov[6] = {0, 0, 0, 0, 0, 0};
        double n = 0;
        for (int pass = 0; pass < 2; ++pass) {
            double acc[6] = {0, 0, 0, 0, 0, 0};
            double cnt = 0;
            for (u64 t = 0; t < n_tiles; ++t) {
                const double* bx = tile_box(tbox, n_slots, tile_slot0(0, 0), t);
                if (bx[0] > qhi[0] || bx[3] < qlo[0] || bx[1] > qhi[1] || bx[4] < qlo[1] || bx[2] > qhi[2] || bx[5] < qlo[2]) continue;
                const u64 i = t * TILE + lane;
                if (i >= m) continue;
                const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
                bool in = true;
                for (int a = 0; a < 3; ++a) {
                    const float d = (float)p[a] - c[a];
                    in = in && d > -h && d < h;
                }
                if (!in) continue;
                if (pass == 0) {
                    cnt += 1.0;
                    for (int a = 0; a < 3; ++a) acc[a] += p[a];
                } else {
                    const double d[3] = {p[0] - mean[0], p[1] - mean[1], p[2] - mean[2]};
                    acc[0] += d[0] * d[0]; acc[1] += d[0] * d[1]; acc[2] += d[0] * d[2];
                    acc[3] += d[1] * d[1]; acc[4] += d[1] * d[2]; acc[5] += d[2] * d[2];
                }
            }
            if (pass == 0) {
                n = wave_sum(cnt);
                for (int a = 0; a < 3; ++a) mean[a] = n > 0 ? wave_sum(acc[a]) / n : 0.0;
                if (n <= 2.0) break;
            } else {
                for (int k = 0; k < 6; ++k) cov[k] = wave_sum(acc[k]) / (n - 1.0);
            }
        }
        if (lane != 0) continue;
        if (empty) empty[loc] = n == 0.0 ? 1 : 0;
        if (!rot) continue;
        double* r = rot + 16 * loc;
        for (int k = 0; k < 16; ++k) r[k] = 0.0;
        if (n <= 2.0) continue;
        double rows[3][3];
        eig3_rows(cov, rows);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) r[i + 4 * j] = rows[i][j];
        r[15] = 1.0;
    }
}

struct RotScratch { u64 *key, *skey, *begin; u32 *i0, *perm; double *pts, *tbox; PrimScratch prim; };
size_t layout(RotScratch& w, void* base, size_t m) {
    ScratchAlloc a(base);
    const size_t mm = std::max<size_t>(m, 1);
    a.take_into(mm, w.key, w.skey);
    a.take_into(2, w.begin);
    a.take_into(mm, w.i0, w.perm);
    a.take_into(3 * mm, w.pts);
    a.take_into(6 * tile_slots(mm, 1), w.tbox);
    w.prim = take_prim(a, mm);
    return a.used;
}

// =====================================================================================================================================
// the triangle grid
inline u64 grid_cells_per_axis(size_t n_tris) {
    u64 g = 1;
    while (g < 128 && (g + 1) * (g + 1) * (g + 1) * 2 <= n_tris) ++g;
    return g;
}
struct IndexLayout { u64* hdr; u32 *cell_begin, *tri_sorted; };
size_t layout(IndexLayout& w, void* base, size_t n_tris) {
    ScratchAlloc a(base);
    const u64 g = grid_cells_per_axis(n_tris);
    w.hdr = a.take<u64>(H_WORDS);
    w.cell_begin = a.take<u32>(g * g * g + 1);
    w.tri_sorted = a.take<u32>(std::max<size_t>(n_tris, 1));
    return a.used;
}
struct IndexScratch { u64 *key, *skey; u32 *i0, *perm; PrimScratch prim; };
size_t layout(IndexScratch& w, void* base, size_t n_tris) {
    ScratchAlloc a(base);
    const size_t m = std::max<size_t>(n_tris, 1);
    a.take_into(m, w.key, w.skey);
    a.take_into(m, w.i0, w.perm);
    w.prim = take_prim(a, m);
    return a.used;
}

__global__ void k_vw_hdr_init(u64* hdr, u64 g, u64 n_tris) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int k = 0; k < H_WORDS; ++k) hdr[k] = 0;
    hdr[H_G] = g;
    hdr[H_NTRI] = n_tris;
    for (int a = 0; a < 3; ++a) hdr[H_MIN + a] = ~0ull;
}
__global__ __launch_bounds__(256) void k_vw_bounds(const float* __restrict__ verts, u64 n_verts, Norm nm, u64* hdr) {
    u64 lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0};
    u64 nz = 0;
    for (u64 i = grid_tid(); i < n_verts; i += grid_stride()) {
        double v[3];
        norm3(verts + 3 * i, nm, v);
        for (int a = 0; a < 3; ++a) {
            const u64 k = key_of(v[a]);
            lo[a] = k < lo[a] ? k : lo[a];
            hi[a] = k > hi[a] ? k : hi[a];
            if (v[a] != 0.0) nz = 1;
        }
    }
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min_u64(lo[a]); hi[a] = wave_max_u64(hi[a]); }
    nz = wave_max_u64(nz);
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; ++a) { atomicMin(&hdr[H_MIN + a], lo[a]); atomicMax(&hdr[H_MAX + a], hi[a]); }
        if (nz) atomicMax(&hdr[H_NONZERO], 1ull);
    }
}
__global__ void k_vw_hdr_final(u64* hdr) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double g = (double)hdr[H_G];
    for (int a = 0; a < 3; ++a) {
        const bool any = hdr[H_MIN + a] <= hdr[H_MAX + a];
        const double lo = any ? value_of(hdr[H_MIN + a]) : 0.0, hi = any ? value_of(hdr[H_MAX + a]) : 0.0;
        double cs = (hi - lo) / g;
        if (!(cs > 0.0) || !(cs < 1e300)) cs = 1.0;
        hdr[H_LO + a] = (u64)__double_as_longlong(lo);
        hdr[H_CS + a] = (u64)__double_as_longlong(cs);
    }
}
__device__ __forceinline__ long long cell_coord(double v, double lo, double cs, long long g) {
    const double q = floor((v - lo) / cs);
    return !(q > 0.0) ? 0 : (q >= (double)g ? g - 1 : (long long)q);
}
__global__ __launch_bounds__(256) void k_vw_trikeys(const float* __restrict__ verts, u64 n_verts, const u32* __restrict__ tris, u64 n_tris, Norm nm, u64* hdr,
                                                    u64* key, u64* counts) {
    const long long g = (long long)hdr[H_G];
    double lo[3], cs[3];
    for (int a = 0; a < 3; ++a) { lo[a] = __longlong_as_double((long long)hdr[H_LO + a]); cs[a] = __longlong_as_double((long long)hdr[H_CS + a]); }
    double hmax = 0.0;
    for (u64 t = grid_tid(); t < n_tris; t += grid_stride()) {
        const u64 i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
        if (i0 >= n_verts || i1 >= n_verts || i2 >= n_verts) { counts[C_BADIDX] = 1; key[t] = (u64)(g * g * g); continue; }
        double v[3][3];
        norm3(verts + 3 * i0, nm, v[0]); norm3(verts + 3 * i1, nm, v[1]); norm3(verts + 3 * i2, nm, v[2]);
        double cen[3];
        for (int a = 0; a < 3; ++a) cen[a] = ((v[0][a] + v[1][a]) + v[2][a]) / 3.0;
        for (int k = 0; k < 3; ++k) {
            const double d = __builtin_sqrt(sq_dist(v[k], cen));
            hmax = d > hmax ? d : hmax;
        }
        const long long cx = cell_coord(cen[0], lo[0], cs[0], g), cy = cell_coord(cen[1], lo[1], cs[1], g), cz = cell_coord(cen[2], lo[2], cs[2], g);
        key[t] = (u64)((cx * g + cy) * g + cz);
    }
    const u64 hk = wave_max_u64((u64)__double_as_longlong(hmax));                    // non-negative doubles order as their bits
    if ((threadIdx.x & 63) == 0) atomicMax(&hdr[H_HMAX], hk);
}
__global__ __launch_bounds__(256) void k_vw_cells(const u64* __restrict__ skey, const u32* __restrict__ perm, u64 n_tris, u64 n_cells, u32* cell_begin,
                                                  u32* tri_sorted) {
    for (u64 c = grid_tid(); c <= n_cells; c += grid_stride()) cell_begin[c] = (u32)lower_bound(skey, n_tris, c);
    for (u64 i = grid_tid(); i < n_tris; i += grid_stride()) tri_sorted[i] = perm[i];
}

// ---- candidates ----------------------------------------------------------------------------------------------------------------------
// one wave per location; EMIT = false: cnt[loc] = its candidates; EMIT = true: they are written from cand_begin[loc]
template <bool EMIT>
__global__ __launch_bounds__(256) void k_vw_cand(const u64* __restrict__ hdr, const u32* __restrict__ cell_begin, const u32* __restrict__ tri_sorted, u64 n_tris,
                                                 const float* __restrict__ coords, u64 n_loc, Norm nm, double half_diag, u32* cnt,
                                                 const u64* __restrict__ cand_begin, u32* cand, u64 cap, u64* counts) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)hdr[H_G];
    double lo[3], cs[3];
    for (int a = 0; a < 3; ++a) { lo[a] = __longlong_as_double((long long)hdr[H_LO + a]); cs[a] = __longlong_as_double((long long)hdr[H_CS + a]); }
    const double R = (half_diag + __longlong_as_double((long long)hdr[H_HMAX])) * (1.0 + 0x1p-30);
    const double R2 = R * R * (1.0 + 0x1p-30);
    for (u64 loc = wave_id(); loc < n_loc; loc += wave_count()) {
        double c[3];
        norm3(coords + 3 * loc, nm, c);
        long long a0[3], a1[3];
        bool none = false;
        for (int a = 0; a < 3; ++a) {
            a0[a] = cell_coord(c[a] - R, lo[a], cs[a], g);
            a1[a] = cell_coord(c[a] + R, lo[a], cs[a], g);
            if (!(c[a] == c[a])) none = true;
        }
        const u64 ny = (u64)(a1[1] - a0[1] + 1), nz = (u64)(a1[2] - a0[2] + 1);
        const u64 n_range = none ? 0 : (u64)(a1[0] - a0[0] + 1) * ny * nz;
        u64 running = 0;
        const u64 out0 = EMIT ? cand_begin[loc] : 0;
        for (u64 base = 0; base < n_range; base += 64) {
            const u64 k = base + lane;
            u32 b0 = 0, n = 0;
            if (k < n_range) {
                const long long cx = a0[0] + (long long)(k / (ny * nz)), cy = a0[1] + (long long)((k / nz) % ny), cz = a0[2] + (long long)(k % nz);
                const double bx[6] = {lo[0] + (double)cx * cs[0], lo[1] + (double)cy * cs[1], lo[2] + (double)cz * cs[2],
                                      lo[0] + (double)(cx + 1) * cs[0], lo[1] + (double)(cy + 1) * cs[1], lo[2] + (double)(cz + 1) * cs[2]};
                // the border cells also hold what the clamp of cell_coord put there: they reach to infinity
                double q[3] = {c[0], c[1], c[2]};
                const long long cc[3] = {cx, cy, cz};
                double bb[6];
                for (int a = 0; a < 3; ++a) {
                    bb[a] = cc[a] == 0 ? -INFINITY : bx[a] - cs[a] * 0x1p-20;
                    bb[3 + a] = cc[a] == g - 1 ? INFINITY : bx[3 + a] + cs[a] * 0x1p-20;
                }
                if (box_dist2(q, bb) <= R2) {
                    const u64 cell = (u64)((cx * g + cy) * g + cz);
                    b0 = cell_begin[cell];
                    const u32 b1 = cell_begin[cell + 1];
                    b0 = b0 < n_tris ? b0 : (u32)n_tris;
                    n = b1 > b0 ? (b1 < n_tris ? b1 : (u32)n_tris) - b0 : 0;
                }
            }
            u32 incl = n;
            for (int d = 1; d < 64; d <<= 1) { const u32 o = __shfl_up(incl, d); if (lane >= d) incl += o; }
            if (EMIT) {
                const u64 at = out0 + running + (incl - n);
                for (u32 j = 0; j < n; ++j) {
                    if (at + j < cap) cand[at + j] = tri_sorted[b0 + j];
                    else counts[C_LOST] = 1;
                }
            }
            running += __shfl(incl, 63);
        }
        if (!EMIT && lane == 0) {
            cnt[loc] = (u32)(running < 0xffffffffull ? running : 0xffffffffull);
            atomicAdd(&counts[C_N], running);
        }
    }
}
__global__ __launch_bounds__(256) void k_vw_cand_begin(const u32* __restrict__ incl, u64 n_loc, u64 cap, int emit, u64* cand_begin, u64* counts) {
    const bool over = counts[C_N] >= (1ull << 31);
    for (u64 i = grid_tid(); i < n_loc; i += grid_stride()) {
        cand_begin[i + 1] = over ? 0 : incl[i];
        if (i == 0) {
            cand_begin[0] = 0;
            if (over) counts[C_OVER31] = 1;
            if (emit && !over && counts[C_N] > cap) counts[C_LOST] = 1;
        }
    }
}

// =====================================================================================================================================
// the raster
struct RenderArgs {
    const float* verts; u64 n_verts;
    const u32* tris; u64 n_tris;
    const u64* hdr;
    const float* coords; u64 n_loc;
    const double* rot;
    const u64* cand_begin; const u32* cand; u64 cand_n;
    Norm nm;
    double E[3];
    double cs[MAXV], sn[MAXV];
    double gw[4];                                                                   // filter weights w[0 .. 3]: w[k] belongs to offsets -(3 - k) and 3 - k
    int n_views, W, H, tw, th, ntx, nty, halo;
    uint8_t* out8; u32* out32;
    u32* viewflag;
    u64* counts;
};
struct TriSetup {
    int x[3], y[3];
    int bias[3];
    double z0, dz1, dz2, area;
    u32 t;
    int c0, c1, r0, r1;                                                             // pixel box inside the region (view coordinates), inclusive
};
__device__ __forceinline__ int mirror(int i, int n) {
    while (i < 0 || i >= n) i = i < 0 ? -i - 1 : 2 * n - 1 - i;
    return i;
}
__device__ __forceinline__ long long snap(double v) {
    const double s = floor(v * 256.0 + 0.5);
    return !(s > -0x1p40) ? -(1ll << 40) : (s > 0x1p40 ? (1ll << 40) : (long long)s);
}
__device__ __forceinline__ long long floor_div256(long long v) { return v >> 8; }
__device__ __forceinline__ int edge_bias(int dx, int dy) { return (dy > 0 || (dy == 0 && dx < 0)) ? 0 : 1; }
__device__ __forceinline__ long long edge_fn(int ax, int ay, int bx, int by, int px, int py) {
    return (long long)(bx - ax) * (long long)(py - ay) - (long long)(by - ay) * (long long)(px - ax);
}
// candidate j of the location -> setup; false where nothing of it can be drawn in the region [rx0, rx1) x [ry0, ry1)
__device__ bool tri_setup(const RenderArgs& A, u32 t, const double* cn, const double* M, double cv, double sv, int rx0, int ry0, int rx1, int ry1,
                          bool count_here, TriSetup& S) {
    if (t >= A.n_tris) { A.counts[C_BADIDX] = 1; return false; }
    long long xs[3], ys[3];
    double zf[3];
    for (int k = 0; k < 3; ++k) {
        const u64 vi = A.tris[3 * (u64)t + k];
        if (vi >= A.n_verts) { A.counts[C_BADIDX] = 1; return false; }
        double vn[3];
        norm3(A.verts + 3 * vi, A.nm, vn);
        const double p0 = vn[0] - cn[0], p1 = vn[1] - cn[1], p2 = vn[2] - cn[2];
        double q[3];
        for (int i = 0; i < 3; ++i) q[i] = ((M[i] * p0) + M[i + 4] * p1) + M[i + 8] * p2;
        const double xe = q[0], ye = (cv * q[1]) - (sv * q[2]), ze = (sv * q[1]) + (cv * q[2]);
        const double X = (xe / A.E[0] + 0.5) * (double)A.W, Y = (ye / A.E[1] + 0.5) * (double)A.H;
        zf[k] = 0.5 - ze / A.E[2];
        xs[k] = snap(X);
        ys[k] = snap(Y);
    }
    const long long xmin = min(xs[0], min(xs[1], xs[2])), xmax = max(xs[0], max(xs[1], xs[2]));
    const long long ymin = min(ys[0], min(ys[1], ys[2])), ymax = max(ys[0], max(ys[1], ys[2]));
    // samples are at 256 c + 128: the columns c with xmin <= 256 c + 128 <= xmax
    long long c0 = floor_div256(xmin - 128 + 255), c1 = floor_div256(xmax - 128), r0 = floor_div256(ymin - 128 + 255), r1 = floor_div256(ymax - 128);
    if (c0 < 0) c0 = 0;
    if (r0 < 0) r0 = 0;
    if (c1 > A.W - 1) c1 = A.W - 1;
    if (r1 > A.H - 1) r1 = A.H - 1;
    if (c0 > c1 || r0 > r1) return false;                                            // the box misses the window
    bool big = false;
    for (int k = 0; k < 3; ++k) big = big || xs[k] >= SNAP_LIM || xs[k] <= -SNAP_LIM || ys[k] >= SNAP_LIM || ys[k] <= -SNAP_LIM;
    if (big) {
        if (count_here) atomicAdd(&A.counts[C_TOOBIG], 1ull);
        return false;
    }
    if (c0 < rx0) c0 = rx0;
    if (r0 < ry0) r0 = ry0;
    if (c1 > rx1 - 1) c1 = rx1 - 1;
    if (r1 > ry1 - 1) r1 = ry1 - 1;
    if (c0 > c1 || r0 > r1) return false;
    int k1 = 1, k2 = 2;
    long long area = edge_fn((int)xs[0], (int)ys[0], (int)xs[1], (int)ys[1], (int)xs[2], (int)ys[2]);
    if (area == 0) return false;
    if (area < 0) { k1 = 2; k2 = 1; area = -area; }
    S.x[0] = (int)xs[0]; S.y[0] = (int)ys[0];
    S.x[1] = (int)xs[k1]; S.y[1] = (int)ys[k1];
    S.x[2] = (int)xs[k2]; S.y[2] = (int)ys[k2];
    S.bias[0] = edge_bias(S.x[1] - S.x[0], S.y[1] - S.y[0]);                         // edge 0 -> 1
    S.bias[1] = edge_bias(S.x[2] - S.x[1], S.y[2] - S.y[1]);                         // edge 1 -> 2
    S.bias[2] = edge_bias(S.x[0] - S.x[2], S.y[0] - S.y[2]);                         // edge 2 -> 0
    S.z0 = zf[0];
    S.dz1 = zf[k1] - zf[0];
    S.dz2 = zf[k2] - zf[0];
    S.area = (double)area;
    S.t = t;
    S.c0 = (int)c0; S.c1 = (int)c1; S.r0 = (int)r0; S.r1 = (int)r1;
    return true;
}
// pixels first, first + step, ... of the setup's box
template <bool INDEX>
__device__ __forceinline__ void tri_draw(const TriSetup& S, int first, int step, int rx0, int ry0, int rw, void* lds) {
    const int bw = S.c1 - S.c0 + 1, n = bw * (S.r1 - S.r0 + 1);
    for (int k = first; k < n; k += step) {
        const int r = S.r0 + k / bw, c = S.c0 + k % bw;
        const int px = 256 * c + 128, py = 256 * r + 128;
        const long long e01 = edge_fn(S.x[0], S.y[0], S.x[1], S.y[1], px, py);
        const long long e12 = edge_fn(S.x[1], S.y[1], S.x[2], S.y[2], px, py);
        const long long e20 = edge_fn(S.x[2], S.y[2], S.x[0], S.y[0], px, py);
        if (e01 < S.bias[0] || e12 < S.bias[1] || e20 < S.bias[2]) continue;
        const double df = S.z0 + (((double)e20 * S.dz1) + ((double)e01 * S.dz2)) / S.area;
        const double dd = floor(df * 16777216.0);
        if (!(dd >= 0.0 && dd < 16777215.0)) continue;
        const u32 D = (u32)dd;
        const int at = (r - ry0) * rw + (c - rx0);
        if (INDEX) atomicMin(reinterpret_cast<u64*>(lds) + at, ((u64)D << 32) | S.t);
        else atomicMin(reinterpret_cast<u32*>(lds) + at, D);
    }
}

template <bool INDEX>
__global__ __launch_bounds__(1024) void k_vw_render(RenderArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_nonzero;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const u64 n_tiles = (u64)A.ntx * A.nty, total = A.n_loc * (u64)A.n_views * n_tiles;
    const bool mesh_zero = A.hdr[H_NONZERO] == 0;
    for (u64 item = blockIdx.x; item < total; item += gridDim.x) {
        const u64 tile = item % n_tiles, lv = item / n_tiles, view = lv % (u64)A.n_views, loc = lv / (u64)A.n_views;
        const int tx = (int)(tile % (u64)A.ntx), ty = (int)(tile / (u64)A.ntx);
        const int x0 = tx * A.tw, y0 = ty * A.th, x1 = min(A.W, x0 + A.tw), y1 = min(A.H, y0 + A.th);          // the core: what this block stores
        const int rx0 = max(0, x0 - A.halo), ry0 = max(0, y0 - A.halo), rx1 = min(A.W, x1 + A.halo), ry1 = min(A.H, y1 + A.halo);
        const int rw = rx1 - rx0, rh = ry1 - ry0, npx = rw * rh, cw = x1 - x0, ch = y1 - y0;
        const u64 out_base = lv * (u64)A.H * (u64)A.W;
        const double* M = A.rot + 16 * loc;
        bool skip = mesh_zero;
        if (!skip) {
            bool any = false;
            for (int k = 0; k < 16; ++k) any = any || M[k] != 0.0;
            skip = !any;
        }
        __syncthreads();                                                            // the previous item is done with the LDS
        if (skip) {
            for (int k = tid; k < cw * ch; k += nt) {
                const u64 o = out_base + (u64)(y0 + k / cw) * A.W + (x0 + k % cw);
                if (INDEX) A.out32[o] = BG_INDEX; else A.out8[o] = 255;
            }
            if (!INDEX && tid == 0 && n_tiles > 1) atomicOr(&A.viewflag[lv], 1u);
            continue;
        }
        if (INDEX) { u64* d = reinterpret_cast<u64*>(smem); for (int k = tid; k < npx; k += nt) d[k] = ~0ull; }
        else { u32* d = reinterpret_cast<u32*>(smem); for (int k = tid; k < npx; k += nt) d[k] = 0xffffffffu; }
        if (tid == 0) s_nonzero = 0;
        __syncthreads();
        double cn[3];
        norm3(A.coords + 3 * loc, A.nm, cn);
        const double cv = A.cs[view], sv = A.sn[view];
        const u64 ce = clamp_u64(A.cand_begin[loc + 1], A.cand_n), cb = clamp_u64(A.cand_begin[loc], ce);
        for (u64 base = cb; base < ce; base += (u64)nt) {                           // `base` is uniform over the block, so whole waves stay together
            const u64 j = base + (u64)tid;
            TriSetup S;
            bool ok = j < ce && tri_setup(A, A.cand[j], cn, M, cv, sv, rx0, ry0, rx1, ry1, tile == 0, S);
            const bool wide = ok && (S.c1 - S.c0 + 1) * (S.r1 - S.r0 + 1) > 64;
            if (ok && !wide) tri_draw<INDEX>(S, 0, 1, rx0, ry0, rw, smem);
            u64 mask = __ballot(wide);
            while (mask) {                                                          // a large box: all lanes of the wave draw it together
                const int src = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                TriSetup T;
                for (int k = 0; k < 3; ++k) { T.x[k] = __shfl(S.x[k], src); T.y[k] = __shfl(S.y[k], src); T.bias[k] = __shfl(S.bias[k], src); }
                T.z0 = __shfl(S.z0, src); T.dz1 = __shfl(S.dz1, src); T.dz2 = __shfl(S.dz2, src); T.area = __shfl(S.area, src);
                T.t = __shfl(S.t, src);
                T.c0 = __shfl(S.c0, src); T.c1 = __shfl(S.c1, src); T.r0 = __shfl(S.r0, src); T.r1 = __shfl(S.r1, src);
                tri_draw<INDEX>(T, lane, 64, rx0, ry0, rw, smem);
            }
        }
        __syncthreads();
        if (INDEX) {
            const u64* d = reinterpret_cast<const u64*>(smem);
            for (int k = tid; k < cw * ch; k += nt) {
                const int r = y0 + k / cw, c = x0 + k % cw;
                const u64 key = d[(r - ry0) * rw + (c - rx0)];
                const u64 t = key & 0xffffffffull;
                A.out32[out_base + (u64)r * A.W + c] = (key == ~0ull || t >= A.n_tris) ? BG_INDEX : A.tris[3 * t + 2];
            }
            continue;
        }
        // 32-bit depths -> bytes in place: chunk k's bytes land on words that chunks <= k have read already
        {
            const u32* d = reinterpret_cast<const u32*>(smem);
            uint8_t* b = reinterpret_cast<uint8_t*>(smem);
            for (int base = 0; base < npx; base += nt) {
                const int k = base + tid;
                const u32 v = k < npx ? d[k] : 0;
                __syncthreads();
                if (k < npx) b[k] = v == 0xffffffffu ? 255 : (uint8_t)(v >> 16);
            }
        }
        __syncthreads();
        uint8_t* bA = reinterpret_cast<uint8_t*>(smem);                              // [rh][rw] depth bytes
        uint8_t* bB = bA + npx;                                                     // [ch][rw] after the pass along axis 0
        uint8_t* bC = bB + npx;                                                     // [ch][cw] after the pass along axis 1
        for (int k = tid; k < ch * rw; k += nt) {
            const int r = y0 + k / rw, cc = k % rw;
            double tmp = (double)bA[(r - ry0) * rw + cc] * A.gw[3];
            for (int i = -3; i < 0; ++i) {
                const int ra = mirror(r + i, A.H) - ry0, rb = mirror(r - i, A.H) - ry0;
                tmp += ((double)bA[ra * rw + cc] + (double)bA[rb * rw + cc]) * A.gw[i + 3];
            }
            bB[k] = (uint8_t)(int)tmp;
        }
        __syncthreads();
        bool nonzero = false;
        for (int k = tid; k < ch * cw; k += nt) {
            const int rr = k / cw, c = x0 + k % cw;
            double tmp = (double)bB[rr * rw + (c - rx0)] * A.gw[3];
            for (int i = -3; i < 0; ++i) {
                const int ca = mirror(c + i, A.W) - rx0, cb2 = mirror(c - i, A.W) - rx0;
                tmp += ((double)bB[rr * rw + ca] + (double)bB[rr * rw + cb2]) * A.gw[i + 3];
            }
            const uint8_t v = (uint8_t)(int)tmp;
            bC[k] = v;
            nonzero = nonzero || v != 0;
        }
        if (nonzero) s_nonzero = 1;
        __syncthreads();
        const bool all255 = n_tiles == 1 && s_nonzero == 0;                          // an image whose sum is 0 becomes all 255
        for (int k = tid; k < ch * cw; k += nt) A.out8[out_base + (u64)(y0 + k / cw) * A.W + (x0 + k % cw)] = all255 ? 255 : bC[k];
        if (n_tiles > 1 && tid == 0 && s_nonzero) atomicOr(&A.viewflag[lv], 1u);
    }
}
// windows of more than one tile: the all-zero rule needs the whole view
__global__ __launch_bounds__(256) void k_vw_zero_rule(uint8_t* out, const u32* __restrict__ viewflag, u64 n_lv, u64 hw) {
    for (u64 lv = blockIdx.x; lv < n_lv; lv += gridDim.x) {
        if (viewflag[lv]) continue;
        for (u64 k = threadIdx.x; k < hw; k += 256) out[lv * hw + k] = 255;
    }
}

// =====================================================================================================================================
// the vote
__global__ __launch_bounds__(256) void k_vw_vote_count(const u32* __restrict__ idx, const uint8_t* __restrict__ lab, u64 n_px, u32 bg, u64 n_verts,
                                                       u32 n_labels, u32* cnt, u64* counts) {
    for (u64 i = grid_tid(); i < n_px; i += grid_stride()) {
        const u32 v = idx[i];
        if (v == bg) continue;
        if (v >= n_verts) { counts[C_BADIDX] = 1; continue; }
        const u32 l = lab[i];
        if (l >= n_labels) { counts[C_BADLABEL] = 1; continue; }
        atomicAdd(&cnt[(u64)v * n_labels + l], 1u);
    }
}
__global__ __launch_bounds__(256) void k_vw_vote_decide(const u32* __restrict__ cnt, u64 n_verts, u32 n_labels, u32 unpredicted, uint8_t* labels,
                                                        uint8_t* table, u64* counts) {
    u64 predicted = 0;
    for (u64 v = grid_tid(); v < n_verts; v += grid_stride()) {
        u32 best = 0, best_l = 0, sum = 0;
        for (u32 l = 0; l < n_labels; ++l) {
            const u32 c = cnt[v * n_labels + l] & 255u;                              // the reference's uint8 table wraps
            if (table) table[v * n_labels + l] = (uint8_t)c;
            sum += c;
            if (c > best) { best = c; best_l = l; }
        }
        labels[v] = (uint8_t)(sum == 0 ? unpredicted : best_l);
        predicted += sum != 0;
    }
    if (predicted) atomicAdd(&counts[C_N], predicted);
}

inline bool load_norm(const float* center3, float max_dist, Norm& nm) {
    if (!center3 || !(max_dist > 0.0f) || !(max_dist < INFINITY)) return false;
    for (int a = 0; a < 3; ++a) {
        if (!(fabsf(center3[a]) < INFINITY)) return false;
        nm.c[a] = center3[a];
    }
    nm.md = max_dist;
    return true;
}

int rotations(const char* who, const float* verts_dev, size_t n_verts, size_t stride, const float* coords_dev, size_t n_loc, const float* center3,
              float max_dist, float edge_length, double* rot_dev, uint8_t* empty_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!counts_dev) return fail(who, ": null counts");
    if (n_verts >= LIM31 || n_loc >= LIM31) return fail(who, ": vertices and locations < 2^31 per call");
    Norm nm;
    if (stride < 1 || !load_norm(center3, max_dist, nm) || !(edge_length >= 0.0f) || !(edge_length < INFINITY)) return fail(who, ": bad argument");
    if (int rc = zero_counts(counts_dev, 8, s); rc != SD_OK) return rc;
    if (n_loc == 0) return SD_OK;
    if (!coords_dev || (n_verts && !verts_dev) || (!rot_dev && !empty_dev)) return fail(who, ": bad argument");
    const size_t m = (n_verts + stride - 1) / stride;
    if (m == 0) {                                                                   // no point: no inlier anywhere
        if (rot_dev && hipMemsetAsync(rot_dev, 0, n_loc * 16 * sizeof(double), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
        if (empty_dev && hipMemsetAsync(empty_dev, 1, n_loc, s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
        return SD_OK;
    }
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_views_rotations_temp_bytes(n_verts, stride), "sd_views_rotations_temp_bytes(n_verts, stride)"); rc != SD_OK)
        return rc;
    RotScratch w;
    layout(w, temp_dev, m);
    const u64 Mn = m, N = n_loc, n_slots = tile_slots(m, 1);
    launch_1d(k_vw_rot_keys, Mn, GRID, s, verts_dev, Mn, (u64)stride, nm, w.key);
    if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, m, 30, s); rc != SD_OK) return rc;
    launch_1d(k_vw_rot_place, Mn, GRID, s, verts_dev, w.perm, Mn, (u64)stride, nm, w.pts, w.begin);
    launch_1d(k_tile_boxes<false>, 64, GRID, s, w.pts, w.begin, 1ull, Mn, n_slots, w.tbox, (double*)nullptr);
    launch_1d(k_vw_rot_solve, N * 64, GRID, s, w.pts, w.tbox, n_slots, Mn, coords_dev, N, nm, edge_length * 0.5f, rot_dev, empty_dev);
    return launch_status((std::string(who) + ": launch failed").c_str());
}

int render(const char* who, bool index, const float* verts_dev, size_t n_verts, const uint32_t* tris_dev, size_t n_tris, const void* index_dev,
           const float* coords_dev, size_t n_loc, const double* rot_dev, const float* center3, float max_dist, const double* edge3, const double* cos_v,
           const double* sin_v, int n_views, int W, int H, const double* weights7, const uint64_t* cand_begin_dev, const uint32_t* cand_dev, size_t cand_n,
           void* views_dev, size_t views_cap, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!counts_dev) return fail(who, ": null counts");
    if (n_verts >= LIM31 || n_tris >= LIM31 || n_loc >= LIM31 || cand_n >= LIM31) return fail(who, ": vertices, triangles, locations and candidates < 2^31 per call");
    RenderArgs A;
    if (!load_norm(center3, max_dist, A.nm) || !edge3 || !cos_v || !sin_v || n_views < 1 || n_views > MAXV || W < 1 || H < 1 || W > 8192 || H > 8192 ||
        (!index && !weights7))
        return fail(who, ": bad argument");
    for (int a = 0; a < 3; ++a) {
        if (!(edge3[a] > 0.0) || !(edge3[a] < INFINITY)) return fail(who, ": the edge lengths must be positive and finite");
        A.E[a] = edge3[a];
    }
    for (int v = 0; v < n_views; ++v) {
        if (!(fabs(cos_v[v]) <= 1.0) || !(fabs(sin_v[v]) <= 1.0)) return fail(who, ": cos / sin out of range");
        A.cs[v] = cos_v[v]; A.sn[v] = sin_v[v];
    }
    if (!index) for (int k = 0; k < 4; ++k) {
        if (!(weights7[k] >= 0.0) || !(weights7[k] <= 1.0) || weights7[k] != weights7[6 - k]) return fail(who, ": the filter weights must be symmetric and in [0, 1]");
        A.gw[k] = weights7[k];
    }
    const u64 hw = (u64)W * (u64)H, n_lv = (u64)n_loc * (u64)n_views;
    if (n_lv >= LIM31 || (n_lv && hw > ((u64)1 << 40) / n_lv)) return fail(who, ": too many views for one call");
    if (views_cap < n_lv * hw) return fail(who, ": views_cap is smaller than n_loc * n_views * H * W");
    if (int rc = zero_counts(counts_dev, 8, s); rc != SD_OK) return rc;
    if (n_loc == 0) return SD_OK;
    if (!index_dev || !coords_dev || !rot_dev || !cand_begin_dev || !views_dev || (n_verts && !verts_dev) || (n_tris && !tris_dev) || (cand_n && !cand_dev))
        return fail(who, ": bad argument");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_views_render_temp_bytes(n_loc, n_views), "sd_views_render_temp_bytes(n_loc, n_views)"); rc != SD_OK)
        return rc;
    const u64 tile_px = index ? SD_VIEWS_TILE_PX / 2 : SD_VIEWS_TILE_PX;
    A.halo = 0;
    if (hw <= tile_px) { A.tw = W; A.th = H; }
    else if (index) { A.tw = std::min(W, 128); A.th = std::min(H, 128); }
    else { A.halo = 3; A.tw = std::min(W, 256 - 6); A.th = std::min(H, 128 - 6); }
    A.ntx = (W + A.tw - 1) / A.tw;
    A.nty = (H + A.th - 1) / A.th;
    const u64 region = (u64)std::min(W, A.tw + 2 * A.halo) * (u64)std::min(H, A.th + 2 * A.halo);
    const size_t lds = (size_t)region * (index ? 8 : 4);
    A.verts = verts_dev; A.n_verts = n_verts; A.tris = tris_dev; A.n_tris = n_tris;
    A.hdr = reinterpret_cast<const u64*>(index_dev);
    A.coords = coords_dev; A.n_loc = n_loc; A.rot = rot_dev;
    A.cand_begin = reinterpret_cast<const u64*>(cand_begin_dev); A.cand = cand_dev; A.cand_n = cand_n;
    A.n_views = n_views; A.W = W; A.H = H;
    A.out8 = index ? nullptr : reinterpret_cast<uint8_t*>(views_dev);
    A.out32 = index ? reinterpret_cast<u32*>(views_dev) : nullptr;
    A.viewflag = reinterpret_cast<u32*>(temp_dev);
    A.counts = reinterpret_cast<u64*>(counts_dev);
    const bool tiled = (u64)A.ntx * A.nty > 1;
    if (tiled && !index && hipMemsetAsync(temp_dev, 0, n_lv * sizeof(u32), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    auto kern = index ? k_vw_render<true> : k_vw_render<false>;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(SD_VIEWS_TILE_PX * 4)) != hipSuccess)
        return sd_fail_msg(SD_ERR_HIP, (std::string(who) + ": the LDS request failed").c_str());
    const u64 items = n_lv * (u64)A.ntx * (u64)A.nty;
    const int blocks = (int)std::min<u64>(items, SD_VIEWS_RASTER_GRID), threads = region > 4096 ? 1024 : 256;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), lds, s, A);
    if (tiled && !index) hipLaunchKernelGGL(k_vw_zero_rule, dim3((int)std::min<u64>(n_lv, SD_VIEWS_RASTER_GRID)), dim3(256), 0, s, A.out8, A.viewflag, n_lv, hw);
    return launch_status((std::string(who) + ": launch failed").c_str());
}

}  // namespace

extern "C" {

size_t sd_views_rotations_temp_bytes(size_t n_verts, size_t stride) {
    RotScratch w;
    return layout(w, nullptr, stride ? (n_verts + stride - 1) / stride : n_verts);
}
int sd_views_rotations(const float* verts_dev, size_t n_verts, size_t stride, const float* coords_dev, size_t n_loc, const float* center3, float max_dist,
                       float edge_length, double* rot_dev, uint8_t* empty_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    if (!rot_dev && n_loc) return fail("sd_views_rotations", ": null output");
    return rotations("sd_views_rotations", verts_dev, n_verts, stride, coords_dev, n_loc, center3, max_dist, edge_length, rot_dev, empty_dev, counts_dev,
                     temp_dev, temp_bytes, stream);
}
int sd_views_flag_empty(const float* verts_dev, size_t n_verts, size_t stride, const float* coords_dev, size_t n_loc, const float* center3, float max_dist,
                        float edge_length, uint8_t* empty_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    if (!empty_dev && n_loc) return fail("sd_views_flag_empty", ": null output");
    return rotations("sd_views_flag_empty", verts_dev, n_verts, stride, coords_dev, n_loc, center3, max_dist, edge_length, nullptr, empty_dev, counts_dev,
                     temp_dev, temp_bytes, stream);
}

size_t sd_views_index_bytes(size_t n_tris) {
    IndexLayout w;
    return layout(w, nullptr, n_tris);
}
size_t sd_views_index_temp_bytes(size_t n_tris) {
    IndexScratch w;
    return layout(w, nullptr, n_tris);
}
int sd_views_index(const float* verts_dev, size_t n_verts, const uint32_t* tris_dev, size_t n_tris, const float* center3, float max_dist, void* index_dev,
                   size_t index_bytes, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_views_index";
    if (!counts_dev) return fail(who, ": null counts");
    if (n_verts >= LIM31 || n_tris >= LIM31) return fail(who, ": vertices and triangles < 2^31 per call");
    Norm nm;
    if (!load_norm(center3, max_dist, nm) || (n_verts && !verts_dev) || (n_tris && !tris_dev)) return fail(who, ": bad argument");
    if (!index_dev || index_bytes < sd_views_index_bytes(n_tris)) return fail(who, ": index smaller than sd_views_index_bytes(n_tris)");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_views_index_temp_bytes(n_tris), "sd_views_index_temp_bytes(n_tris)"); rc != SD_OK) return rc;
    if (int rc = zero_counts(counts_dev, 8, s); rc != SD_OK) return rc;
    IndexLayout ix;
    layout(ix, index_dev, n_tris);
    IndexScratch w;
    layout(w, temp_dev, n_tris);
    const u64 g = grid_cells_per_axis(n_tris), n_cells = g * g * g, T = n_tris, V = n_verts;
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    hipLaunchKernelGGL(k_vw_hdr_init, dim3(1), dim3(64), 0, s, ix.hdr, g, T);
    if (V) launch_1d(k_vw_bounds, V, GRID, s, verts_dev, V, nm, ix.hdr);
    hipLaunchKernelGGL(k_vw_hdr_final, dim3(1), dim3(64), 0, s, ix.hdr);
    if (T) {
        launch_1d(k_vw_trikeys, T, GRID, s, verts_dev, V, tris_dev, T, nm, ix.hdr, w.key, counts);
        if (int rc = sort_by_key(who, w.prim, w.key, w.skey, w.i0, w.perm, n_tris, bits_for(n_cells + 2), s); rc != SD_OK) return rc;
    }
    launch_1d(k_vw_cells, std::max(n_cells + 1, T), GRID, s, w.skey, w.perm, T, n_cells, ix.cell_begin, ix.tri_sorted);
    return launch_status("sd_views_index: launch failed");
}

size_t sd_views_candidates_temp_bytes(size_t n_loc) {
    ScratchAlloc a(nullptr);
    const size_t n = std::max<size_t>(n_loc, 1);
    a.take<u32>(n); a.take<u32>(n);
    take_prim(a, n);
    return a.used;
}
int sd_views_candidates(const void* index_dev, size_t n_tris, const float* coords_dev, size_t n_loc, const float* center3, float max_dist, const double* edge3,
                        uint64_t* cand_begin_dev, uint32_t* cand_dev, size_t cand_cap, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_views_candidates";
    if (!counts_dev || !cand_begin_dev) return fail(who, ": null counts or offsets");
    if (n_tris >= LIM31 || n_loc >= LIM31 || cand_cap >= LIM31) return fail(who, ": triangles, locations and candidates < 2^31 per call");
    Norm nm;
    if (!load_norm(center3, max_dist, nm) || !edge3 || !index_dev || (cand_cap && !cand_dev)) return fail(who, ": bad argument");
    double d2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        if (!(edge3[a] > 0.0) || !(edge3[a] < INFINITY)) return fail(who, ": the edge lengths must be positive and finite");
        d2 += edge3[a] * edge3[a];
    }
    if (int rc = zero_counts(counts_dev, 8, s); rc != SD_OK) return rc;
    if (hipMemsetAsync(cand_begin_dev, 0, sizeof(u64), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    if (n_loc == 0) return SD_OK;
    if (!coords_dev) return fail(who, ": bad argument");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_views_candidates_temp_bytes(n_loc), "sd_views_candidates_temp_bytes(n_loc)"); rc != SD_OK) return rc;
    ScratchAlloc a(temp_dev);
    u32 *cnt = a.take<u32>(n_loc), *incl = a.take<u32>(n_loc);
    const PrimScratch prim = take_prim(a, n_loc);
    IndexLayout ix;
    layout(ix, const_cast<void*>(index_dev), n_tris);
    const u64 N = n_loc, T = n_tris, cap = cand_cap;
    const double half_diag = 0.5 * std::sqrt(d2);
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    const u64* cb = reinterpret_cast<const u64*>(cand_begin_dev);
    launch_1d(k_vw_cand<false>, N * 64, GRID, s, ix.hdr, ix.cell_begin, ix.tri_sorted, T, coords_dev, N, nm, half_diag, cnt, cb, (u32*)nullptr, cap, counts);
    if (int rc = scan_u32(who, prim, cnt, incl, n_loc, s); rc != SD_OK) return rc;
    launch_1d(k_vw_cand_begin, N, GRID, s, incl, N, cap, cand_cap ? 1 : 0, reinterpret_cast<u64*>(cand_begin_dev), counts);
    if (cand_cap)
        launch_1d(k_vw_cand<true>, N * 64, GRID, s, ix.hdr, ix.cell_begin, ix.tri_sorted, T, coords_dev, N, nm, half_diag, cnt, cb, cand_dev, cap, counts);
    return launch_status("sd_views_candidates: launch failed");
}

size_t sd_views_render_temp_bytes(size_t n_loc, int n_views) { return up256(std::max<size_t>(n_loc, 1) * (size_t)std::max(n_views, 1) * sizeof(u32)); }
int sd_views_render(const float* verts_dev, size_t n_verts, const uint32_t* tris_dev, size_t n_tris, const void* index_dev, const float* coords_dev,
                    size_t n_loc, const double* rot_dev, const float* center3, float max_dist, const double* edge3, const double* cos_v, const double* sin_v,
                    int n_views, int W, int H, const double* weights7, const uint64_t* cand_begin_dev, const uint32_t* cand_dev, size_t cand_n,
                    uint8_t* views_dev, size_t views_cap, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    return render("sd_views_render", false, verts_dev, n_verts, tris_dev, n_tris, index_dev, coords_dev, n_loc, rot_dev, center3, max_dist, edge3, cos_v, sin_v,
                  n_views, W, H, weights7, cand_begin_dev, cand_dev, cand_n, views_dev, views_cap, counts_dev, temp_dev, temp_bytes, stream);
}
int sd_views_render_index(const float* verts_dev, size_t n_verts, const uint32_t* tris_dev, size_t n_tris, const void* index_dev, const float* coords_dev,
                          size_t n_loc, const double* rot_dev, const float* center3, float max_dist, const double* edge3, const double* cos_v,
                          const double* sin_v, int n_views, int W, int H, const uint64_t* cand_begin_dev, const uint32_t* cand_dev, size_t cand_n,
                          uint32_t* views_dev, size_t views_cap, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    return render("sd_views_render_index", true, verts_dev, n_verts, tris_dev, n_tris, index_dev, coords_dev, n_loc, rot_dev, center3, max_dist, edge3, cos_v,
                  sin_v, n_views, W, H, nullptr, cand_begin_dev, cand_dev, cand_n, views_dev, views_cap, counts_dev, temp_dev, temp_bytes, stream);
}

size_t sd_views_vote_temp_bytes(size_t n_verts, int n_labels) { return up256(std::max<size_t>(n_verts, 1) * (size_t)std::max(n_labels, 1) * sizeof(u32)); }
int sd_views_vote(const uint32_t* index_dev, const uint8_t* labels_dev, size_t n_px, uint32_t background_id, size_t n_verts, int n_labels, int unpredicted,
                  uint8_t* vertex_labels_dev, uint8_t* table_dev, uint64_t* counts_dev, void* temp_dev, size_t temp_bytes, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_views_vote";
    if (!counts_dev) return fail(who, ": null counts");
    if (n_px >= LIM31 || n_verts >= LIM31) return fail(who, ": pixels and vertices < 2^31 per call");
    if (n_labels < 1 || n_labels > 256 || unpredicted < 0 || unpredicted > 255) return fail(who, ": labels in [1, 256], the unpredicted label in [0, 255]");
    if ((u64)n_verts * (u64)n_labels >= LIM31) return fail(who, ": vertices x labels < 2^31 per call");
    if (int rc = zero_counts(counts_dev, 8, s); rc != SD_OK) return rc;
    if (n_verts == 0 && n_px == 0) return SD_OK;
    if ((n_px && (!index_dev || !labels_dev)) || (n_verts && !vertex_labels_dev)) return fail(who, ": bad argument");
    if (int rc = check_scratch(who, temp_dev, temp_bytes, sd_views_vote_temp_bytes(n_verts, n_labels), "sd_views_vote_temp_bytes(n_verts, n_labels)"); rc != SD_OK)
        return rc;
    u32* cnt = reinterpret_cast<u32*>(temp_dev);
    u64* counts = reinterpret_cast<u64*>(counts_dev);
    if (hipMemsetAsync(cnt, 0, std::max<size_t>(n_verts, 1) * (size_t)n_labels * sizeof(u32), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    const u64 P = n_px, V = n_verts;
    if (P) launch_1d(k_vw_vote_count, P, GRID, s, index_dev, labels_dev, P, background_id, V, (u32)n_labels, cnt, counts);
    if (V) launch_1d(k_vw_vote_decide, V, GRID, s, cnt, V, (u32)n_labels, (u32)unpredicted, vertex_labels_dev, table_dev, counts);
    return launch_status("sd_views_vote: launch failed");
}

}  // extern "C"
