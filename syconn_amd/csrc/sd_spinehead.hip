// Spine head volumes on the device: the per-window glue of extract_spinehead_volume_mesh
// (reps/super_segmentation_helper.py:2068-2198) around the entries that exist already.  Per synapse window:
//     :2135-2141  kd.load_seg + ndimage.zoom(order=0) + relabel_vol_nonexist2zero / (seg == sv)   -> sd_spinehead_window_mask
//     :2143       ndimage.binary_fill_holes                                                       -> sd_spinehead_fill_holes
//     :2161       ndimage.distance_transform_edt                                                  -> sd_edt_squared (sd_objseg.hip)
//     :2162       skimage peak_local_max(footprint 3x3x3, labels=seg)                             -> sd_spinehead_peaks
//     :2150-2160  in_bounding_box + the label rewrite 0 -> 9                                      -> sd_spinehead_box_vertices
//     :2165-2168  colorcode_vertices(maxima * ds, ...) scattered into local_maxi                  -> sd_spinehead_queries, sd_syn_props_knn,
//                                                                                                    sd_spinehead_markers
//     :2170       skimage watershed(-distance, local_maxi, mask=seg)                              -> sd_marker_flood (sd_objseg.hip)
//     :2171-2196  labels == 1, ndimage.label, the object next to the synapse, its voxel count     -> sd_spinehead_select
// All volumes are (X, Y, Z) with z fastest.  Every kernel walks its items with a grid stride of at most SD_SPINEHEAD_*_GRID blocks of
// 256 threads and indexes with size_t; volumes stay below 2^31 voxels (labels are int32, as in sd_objseg.hip).
// Hole filling labels the INVERTED mask with the run-based components of sd_objseg.hip (sd_object_segmentation without operations) and
// keeps the background components that own no voxel of the window border: no flood of its own.
#include "../../include/syconn_dense.h"
#include "sd_sortseg.h"
#include <stdint.h>

namespace {

constexpr int VG = SD_SPINEHEAD_VOX_GRID, PG = SD_SPINEHEAD_VERT_GRID, TG = SD_SPINEHEAD_ID_GRID;

__device__ __forceinline__ void dec3(size_t i, int n0, int n1, int& c0, int& c1, int& c2) {
    const unsigned u = (unsigned)i, r = u / (unsigned)n0, q = r / (unsigned)n1;
    c0 = (int)(u - r * (unsigned)n0); c1 = (int)(r - q * (unsigned)n1); c2 = (int)q;
}

struct I3 { long long v[3]; };
struct D3 { double v[3]; };
struct B6 { int lo[3], hi[3]; };

// mask[x][y][z] = seg[window offset + (tx[x], ty[y], tz[z])] is one of the cell's supervoxels; a table entry of -1 (scipy's constant 0
// beyond the last input sample) and every voxel outside the resident volume (kd.load_seg pads with zeros) give 0
__global__ __launch_bounds__(256) void k_sh_window_mask(const uint64_t* __restrict__ seg, int VX, int VY, int VZ, I3 rel, const int* __restrict__ tx,
                                                        const int* __restrict__ ty, const int* __restrict__ tz, int X, int Y, int Z,
                                                        const uint64_t* __restrict__ sv, long long n_sv, uint8_t* __restrict__ mask) {
    const size_t total = (size_t)X * Y * Z;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        int z, y, x;
        dec3(i, Z, Y, z, y, x);
        const int sx = tx[x], sy = ty[y], sz = tz[z];
        uint8_t m = 0;
        if (sx >= 0 && sy >= 0 && sz >= 0) {
            const long long gx = rel.v[0] + sx, gy = rel.v[1] + sy, gz = rel.v[2] + sz;      // relative to the resident volume
            if (gx >= 0 && gx < VX && gy >= 0 && gy < VY && gz >= 0 && gz < VZ) {
                const uint64_t id = seg[((size_t)gx * VY + (size_t)gy) * VZ + (size_t)gz];
                long long lo = 0, hi = n_sv;      // first entry >= id
                while (lo < hi) {
                    const long long mid = (lo + hi) >> 1;
                    if (sv[mid] < id) lo = mid + 1; else hi = mid;
                }
                m = (lo < n_sv && sv[lo] == id) ? 1 : 0;
            }
        }
        mask[i] = m;
    }
}

__global__ __launch_bounds__(256) void k_sh_invert(const uint8_t* __restrict__ in, size_t total, uint8_t* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) out[i] = in[i] ? 0 : 1;
}
__global__ __launch_bounds__(256) void k_sh_zero(int* p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0;
}
// open[c] = 1 for every background component c that owns a voxel of the window border
__global__ __launch_bounds__(256) void k_sh_border(const int* __restrict__ L, int X, int Y, int Z, int* __restrict__ open) {
    const size_t total = (size_t)X * Y * Z;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        int z, y, x;
        dec3(i, Z, Y, z, y, x);
        if (!(x == 0 || y == 0 || z == 0 || x == X - 1 || y == Y - 1 || z == Z - 1)) continue;
        const int c = L[i];
        if (c > 0 && open[c] == 0) open[c] = 1;      // (every writer stores the same value)
    }
}
__global__ __launch_bounds__(256) void k_sh_fill(const uint8_t* __restrict__ mask, const int* __restrict__ L, const int* __restrict__ open, size_t total,
                                                 uint8_t* __restrict__ filled, int* __restrict__ n_filled) {
    int local = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = L[i];
        const uint8_t f = (mask[i] || (c > 0 && !open[c])) ? 1 : 0;
        filled[i] = f;
        local += f;
    }
    if (local) atomicAdd(n_filled, local);
}

// ---- peaks -------------------------------------------------------------------------------------------------------------------------
// scal: [0..2] roi min, [3..5] roi max (inclusive), [6] mask voxels in roi, [7] of them equal to their neighbourhood maximum
__global__ __launch_bounds__(64) void k_shp_init(int* scal) {
    const int t = threadIdx.x;
    if (t < 3) scal[t] = 0x7fffffff;
    else if (t < 6) scal[t] = -1;
    else if (t < 16) scal[t] = 0;
}
__global__ __launch_bounds__(256) void k_shp_bbox(const uint8_t* __restrict__ mask, int X, int Y, int Z, int* scal) {
    const size_t total = (size_t)X * Y * Z;
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        if (!mask[i]) continue;
        int c[3];
        dec3(i, Z, Y, c[2], c[1], c[0]);
        if (c[0] < 1 || c[1] < 1 || c[2] < 1 || c[0] > X - 2 || c[1] > Y - 2 || c[2] > Z - 2) continue;      // exclude_border, width 1
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], c[a]); hi[a] = max(hi[a], c[a]); }
    }
    if (hi[0] >= 0)
        for (int a = 0; a < 3; ++a) { atomicMin(scal + a, lo[a]); atomicMax(scal + 3 + a, hi[a]); }
}
__global__ __launch_bounds__(256) void k_shp_flags(const uint8_t* __restrict__ mask, const int* __restrict__ d2, int X, int Y, int Z, int* scal,
                                                   uint32_t* __restrict__ flag) {
    const size_t total = (size_t)X * Y * Z;
    const int x0 = scal[0], y0 = scal[1], z0 = scal[2], x1 = scal[3], y1 = scal[4], z1 = scal[5];
    int n_roi = 0, n_eq = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        int z, y, x;
        dec3(i, Z, Y, z, y, x);
        uint32_t f = 0;
        if (mask[i] && x >= x0 && x <= x1 && y >= y0 && y <= y1 && z >= z0 && z <= z1) {
            const int v = d2[i];
            int m = v;
            for (int xx = max(x - 1, x0); xx <= min(x + 1, x1); ++xx)
                for (int yy = max(y - 1, y0); yy <= min(y + 1, y1); ++yy)
                    for (int zz = max(z - 1, z0); zz <= min(z + 1, z1); ++zz) {
                        const size_t j = ((size_t)xx * Y + yy) * Z + zz;
                        if (mask[j]) m = max(m, d2[j]);
                    }
            ++n_roi;
            if (m == v) { ++n_eq; f = v > 0 ? 1u : 0u; }
        }
        flag[i] = f;
    }
    if (n_roi) atomicAdd(scal + 6, n_roi);
    if (n_eq) atomicAdd(scal + 7, n_eq);
}
__global__ __launch_bounds__(256) void k_shp_compact(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, int X, int Y, int Z, const int* scal,
                                                     int* __restrict__ peaks, long long cap, int* __restrict__ n_peaks) {
    const size_t total = (size_t)X * Y * Z;
    const bool trivial = scal[6] == scal[7];      // image == image_max on the whole object: skimage returns no peak
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        if (i == total - 1) *n_peaks = trivial ? 0 : (int)pos[i];
        if (trivial || !flag[i]) continue;
        const long long p = (long long)pos[i] - 1;
        if (p >= cap) continue;
        int z, y, x;
        dec3(i, Z, Y, z, y, x);
        peaks[3 * p] = x; peaks[3 * p + 1] = y; peaks[3 * p + 2] = z;
    }
}

// ---- vertices ----------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_shv_flags(const T* __restrict__ verts, size_t n_verts, const long long* __restrict__ win_off, size_t n_win, D3 half,
                                                   D3 edge, uint32_t* __restrict__ flag) {
    const size_t total = n_verts * n_win;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t w = i / n_verts, v = i - w * n_verts;
        bool in = true;
        for (int a = 0; a < 3; ++a) {
            const double c = (double)verts[3 * v + a] - ((double)win_off[3 * w + a] + half.v[a]);
            in = in && c > -edge.v[a] && c < edge.v[a];
        }
        flag[i] = in ? 1u : 0u;
    }
}
// begin[w] = vertices in the windows before w; entries n_win and n_win + 1 (an empty segment for the padding queries) = all of them
__global__ __launch_bounds__(256) void k_shv_begin(const uint32_t* __restrict__ pos, size_t n_verts, size_t n_win, uint64_t* __restrict__ begin) {
    for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < n_win + 2; w += (size_t)gridDim.x * 256) {
        const size_t ww = w > n_win ? n_win : w;
        begin[w] = ww == 0 ? 0 : (uint64_t)pos[ww * n_verts - 1];
    }
}
template <typename T>
__global__ __launch_bounds__(256) void k_shv_scatter(const T* __restrict__ verts, const int* __restrict__ labels, size_t n_verts, const long long* __restrict__ win_off,
                                                     size_t n_win, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, size_t cap,
                                                     double* __restrict__ points, int* __restrict__ out_labels) {
    const size_t total = n_verts * n_win;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        if (!flag[i]) continue;
        const size_t p = (size_t)pos[i] - 1;
        if (p >= cap) continue;
        const size_t w = i / n_verts, v = i - w * n_verts;
        for (int a = 0; a < 3; ++a) points[3 * p + a] = (double)verts[3 * v + a] - (double)win_off[3 * w + a];
        const int l = labels[v];
        out_labels[p] = l == 0 ? 9 : l;
    }
}

// ---- queries and markers -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sh_queries(const int* __restrict__ peaks, const int* __restrict__ n_peaks, size_t n_win, size_t cap, size_t slots, D3 ds,
                                                    uint32_t* __restrict__ q_cell, double* __restrict__ q_xyz) {
    const size_t total = n_win * slots;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t w = i / slots, p = i - w * slots;
        const bool live = (long long)p < (long long)n_peaks[w];      // (slots <= cap: p indexes the window's peak list)
        q_cell[i] = live ? (uint32_t)w : (uint32_t)n_win;
        for (int a = 0; a < 3; ++a) q_xyz[3 * i + a] = live ? (double)peaks[3 * (w * cap + p) + a] * ds.v[a] : 0.0;
    }
}
__global__ __launch_bounds__(256) void k_sh_markers(const int* __restrict__ peaks, const int* __restrict__ n_peaks, const int* __restrict__ votes, size_t cap, int Y,
                                                    int Z, int* __restrict__ markers) {
    const size_t n = (size_t)min((long long)*n_peaks, (long long)cap);
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256)
        markers[((size_t)peaks[3 * p] * Y + peaks[3 * p + 1]) * Z + peaks[3 * p + 2]] = max(votes[p], 0);      // (-1: a window without vertices)
}

// ---- head selection ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_shs_head(const int* __restrict__ flood, size_t total, uint8_t* __restrict__ head) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) head[i] = flood[i] == 1 ? 1 : 0;
}
// sel: [0] smallest squared distance (bits of a double >= 0), [1] (count in the slice << 32) | ~id, [2] (id << 32) | raster index
__global__ __launch_bounds__(64) void k_shs_init(unsigned long long* sel) {
    if (threadIdx.x == 0) { sel[0] = ~0ull; sel[1] = 0ull; sel[2] = ~0ull; }
}
// squared distance of voxel (x, y, z) to c in the bits of cKDTree((coords + offset) * scaling).query([(c + offset) * scaling]) (:2189-2191): both
// points scaled, then subtracted (the window offset moves the rounding of the products), ((dx dx) + dy dy) + dz dz.  The one definition for
// k_shs_count and k_shs_nearest, which looks the minimum of the former up by equality: contraction is off HERE, so both get the same bits.
__device__ __forceinline__ double sh_dist2(int x, int y, int z, const I3& off, const I3& c, const D3& sc) {
#pragma clang fp contract(off)                              // every product and sum rounded on its own, as numpy / cKDTree do
    const double dx = (double)((long long)x + off.v[0]) * sc.v[0] - (double)(c.v[0] + off.v[0]) * sc.v[0];
    const double dy = (double)((long long)y + off.v[1]) * sc.v[1] - (double)(c.v[1] + off.v[1]) * sc.v[1];
    const double dz = (double)((long long)z + off.v[2]) * sc.v[2] - (double)(c.v[2] + off.v[2]) * sc.v[2];
    return ((dx * dx) + dy * dy) + dz * dz;
}
// voxels per object and per object inside the slice.  The voxels of an object are neighbours, so the lanes of a wave mostly hold one label:
// per distinct label of the wave one lane adds the wave's count (a ballot per label) instead of 64 atomics on one address.
__global__ __launch_bounds__(256) void k_shs_count(const int* __restrict__ L, int X, int Y, int Z, B6 box, I3 off, I3 c, D3 sc, int* __restrict__ cnt, int* __restrict__ cbox,
                                                   unsigned long long* sel) {
    const size_t total = (size_t)X * Y * Z;
    const int lane = threadIdx.x & 63;
    unsigned long long best = ~0ull;
    for (size_t base = (size_t)blockIdx.x * 256; base < total; base += (size_t)gridDim.x * 256) {      // (uniform per wave: the ballots need every lane)
        const size_t i = base + threadIdx.x;
        int l = 0;
        bool inb = false;
        if (i < total && (l = L[i]) > 0) {
            int z, y, x;
            dec3(i, Z, Y, z, y, x);
            inb = x >= box.lo[0] && x < box.hi[0] && y >= box.lo[1] && y < box.hi[1] && z >= box.lo[2] && z < box.hi[2];
            const unsigned long long b = (unsigned long long)__double_as_longlong(sh_dist2(x, y, z, off, c, sc));
            best = b < best ? b : best;
        } else {
            l = 0;
        }
        unsigned long long todo = __ballot(l > 0);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            const int l0 = __shfl(l, src, 64);
            const unsigned long long same = __ballot(l == l0), same_in = __ballot(l == l0 && inb);
            if (lane == src) {
                atomicAdd(cnt + l0, __popcll(same));
                if (same_in) atomicAdd(cbox + l0, __popcll(same_in));
            }
            todo &= ~same;
        }
    }
    if (best != ~0ull) atomicMin(sel, best);
}
__global__ __launch_bounds__(256) void k_shs_best(const int* __restrict__ cbox, const int* __restrict__ nb_obj, unsigned long long* sel) {
    const size_t n = (size_t)*nb_obj;
    for (size_t id = 1 + (size_t)blockIdx.x * 256 + threadIdx.x; id <= n; id += (size_t)gridDim.x * 256) {
        const int k = cbox[id];
        if (k > 0) atomicMax(sel + 1, ((unsigned long long)(unsigned)k << 32) | (unsigned long long)(0xffffffffu - (unsigned)id));
    }
}
__global__ __launch_bounds__(256) void k_shs_nearest(const int* __restrict__ L, int X, int Y, int Z, I3 off, I3 c, D3 sc, unsigned long long* sel) {
    const size_t total = (size_t)X * Y * Z;
    const unsigned long long want = sel[0];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int l = L[i];
        if (l <= 0) continue;
        int z, y, x;
        dec3(i, Z, Y, z, y, x);
        if ((unsigned long long)__double_as_longlong(sh_dist2(x, y, z, off, c, sc)) == want) atomicMin(sel + 2, ((unsigned long long)(unsigned)l << 32) | (unsigned long long)i);
    }
}
// result: [0] voxels of the chosen object, [1] the chosen id, [2] nb_obj
__global__ __launch_bounds__(64) void k_shs_final(const int* __restrict__ cnt, const int* __restrict__ nb_obj, const unsigned long long* sel, int* __restrict__ result) {
    if (threadIdx.x != 0) return;
    const int n = *nb_obj;
    int id = 1;
    if (n > 1) id = (sel[1] >> 32) ? (int)(0xffffffffu - (unsigned)(sel[1] & 0xffffffffull)) : (int)(sel[2] >> 32);
    result[0] = (n >= 1 && id >= 1 && id <= n) ? cnt[id] : 0;
    result[1] = id;
    result[2] = n;
}

// scratch of this file's entries: the labelling scratch of sd_objseg.hip, one uint8 and two int32 volumes, three id tables (a volume of
// n voxels has at most n / 2 + 1 six-connected components), scalars and the rocPRIM scan
struct ShScalars { int i[16]; unsigned long long sel[24]; };      // the 256-byte scalar block: nb_obj / the peaks' scal, then sel
static_assert(sizeof(ShScalars) == 256, "the scalar block keeps its size");
// flag, pos: the two int32 volumes as the peaks' scan sees them; lab: the first of them as labels (fill_holes, select)
struct ShLayout { char* cc; size_t cc_bytes, T; uint8_t* u8; uint32_t *flag, *pos; int *lab, *tab[3]; ShScalars* scal; PrimScratch prim; };
size_t layout(ShLayout& l, void* base, int X, int Y, int Z) {
    ScratchAlloc a(base);
    const size_t nvox = (size_t)X * Y * Z;
    l.T = nvox / 2 + 1026;
    l.cc_bytes = sd_objseg_workspace_bytes(X, Y, Z, 0);
    l.cc = a.take<char>(l.cc_bytes);
    l.u8 = a.take<uint8_t>(nvox);
    a.take_into(nvox, l.flag, l.pos);
    l.lab = reinterpret_cast<int*>(l.flag);
    a.take_into(l.T, l.tab[0], l.tab[1], l.tab[2]);
    l.scal = a.take<ShScalars>(1);
    l.prim = take_prim(a, nvox);
    return a.used;
}
bool bad_dims(int X, int Y, int Z) { return X <= 0 || Y <= 0 || Z <= 0 || (size_t)X * Y * Z >= (1ull << 31); }

struct VertLayout { uint32_t *flag, *pos; PrimScratch prim; size_t total; };
VertLayout vert_layout(void* base, size_t n_verts, size_t n_win) {
    ScratchAlloc a(base);
    VertLayout l{};
    const size_t n = n_verts * n_win;
    a.take_into(n ? n : 1, l.flag, l.pos);
    l.prim = take_prim(a, n ? n : 1);
    l.total = a.used;
    return l;
}

}  // namespace

extern "C" {

size_t sd_spinehead_workspace_bytes(int X, int Y, int Z) {
    if (bad_dims(X, Y, Z)) return 0;
    ShLayout l;
    return std::max(layout(l, nullptr, X, Y, Z), sd_objseg_watershed_workspace_bytes(X, Y, Z, 0));
}

int sd_spinehead_window_mask(const uint64_t* seg_dev, int VX, int VY, int VZ, const int64_t* vol_origin_xyz, const int64_t* win_offset_xyz,
                             const int32_t* tab_x_dev, const int32_t* tab_y_dev, const int32_t* tab_z_dev, int X, int Y, int Z,
                             const uint64_t* cell_sv_dev, size_t n_sv, uint8_t* mask_dev, void* stream) {
    if (!seg_dev || !vol_origin_xyz || !win_offset_xyz || !tab_x_dev || !tab_y_dev || !tab_z_dev || !cell_sv_dev || !mask_dev || VX <= 0 || VY <= 0 ||
        VZ <= 0 || n_sv < 1 || n_sv >= (1ull << 31) || bad_dims(X, Y, Z))
        return sd_fail_msg(SD_ERR_INVALID, "sd_spinehead_window_mask: bad argument");
    I3 rel;
    for (int a = 0; a < 3; ++a) rel.v[a] = (long long)win_offset_xyz[a] - (long long)vol_origin_xyz[a];
    hipLaunchKernelGGL(k_sh_window_mask, dim3(grid_for((size_t)X * Y * Z, VG)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), seg_dev, VX, VY, VZ, rel,
                       tab_x_dev, tab_y_dev, tab_z_dev, X, Y, Z, cell_sv_dev, (long long)n_sv, mask_dev);
    return launch_status("sd_spinehead_window_mask: launch failed");
}

int sd_spinehead_fill_holes(const uint8_t* mask_dev, int X, int Y, int Z, uint8_t* filled_dev, int32_t* n_filled_dev, void* ws, size_t ws_bytes,
                            void* stream) {
    if (!mask_dev || !filled_dev || !n_filled_dev || !ws || bad_dims(X, Y, Z)) return sd_fail_msg(SD_ERR_INVALID, "sd_spinehead_fill_holes: bad argument");
    ShLayout l;
    if (ws_bytes < layout(l, ws, X, Y, Z)) return sd_fail_msg(SD_ERR_NOMEM, "sd_spinehead_fill_holes: workspace too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t* inv = l.u8;
    int *L = l.lab, *open = l.tab[0], *scal = l.scal->i;
    const size_t nvox = (size_t)X * Y * Z;
    hipLaunchKernelGGL(k_sh_invert, dim3(grid_for(nvox, VG)), dim3(256), 0, s, mask_dev, nvox, inv);
    const int rc = sd_object_segmentation(inv, X, Y, Z, 0.0, nullptr, nullptr, 0, nullptr, 0, 0, 0, L, scal, nullptr, l.cc, l.cc_bytes, stream);
    if (rc != SD_OK) return rc;
    hipLaunchKernelGGL(k_sh_zero, dim3(grid_for(l.T, TG)), dim3(256), 0, s, open, l.T);
    hipLaunchKernelGGL(k_sh_zero, dim3(1), dim3(256), 0, s, n_filled_dev, (size_t)1);
    hipLaunchKernelGGL(k_sh_border, dim3(grid_for(nvox, VG)), dim3(256), 0, s, L, X, Y, Z, open);
    hipLaunchKernelGGL(k_sh_fill, dim3(grid_for(nvox, VG)), dim3(256), 0, s, mask_dev, L, open, nvox, filled_dev, n_filled_dev);
    return launch_status("sd_spinehead_fill_holes: launch failed");
}

int sd_spinehead_peaks(const uint8_t* mask_dev, const int32_t* d2_dev, int X, int Y, int Z, int32_t* peaks_dev, size_t max_peaks, int32_t* n_peaks_dev,
                       void* ws, size_t ws_bytes, void* stream) {
    if (!mask_dev || !d2_dev || !peaks_dev || !n_peaks_dev || !ws || max_peaks < 1 || max_peaks >= (1ull << 31) || bad_dims(X, Y, Z))
        return sd_fail_msg(SD_ERR_INVALID, "sd_spinehead_peaks: bad argument");
    ShLayout l;
    if (ws_bytes < layout(l, ws, X, Y, Z)) return sd_fail_msg(SD_ERR_NOMEM, "sd_spinehead_peaks: workspace too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint32_t *flag = l.flag, *pos = l.pos;
    int* scal = l.scal->i;
    const size_t nvox = (size_t)X * Y * Z;
    const int g = grid_for(nvox, VG);
    hipLaunchKernelGGL(k_shp_init, dim3(1), dim3(64), 0, s, scal);
    hipLaunchKernelGGL(k_shp_bbox, dim3(g), dim3(256), 0, s, mask_dev, X, Y, Z, scal);
    hipLaunchKernelGGL(k_shp_flags, dim3(g), dim3(256), 0, s, mask_dev, d2_dev, X, Y, Z, scal, flag);
    const int rc = scan_u32("sd_spinehead_peaks", l.prim, flag, pos, nvox, s);
    if (rc != SD_OK) return rc;
    hipLaunchKernelGGL(k_shp_compact, dim3(g), dim3(256), 0, s, flag, pos, X, Y, Z, scal, peaks_dev, (long long)max_peaks, n_peaks_dev);
    return launch_status("sd_spinehead_peaks: launch failed");
}

size_t sd_spinehead_box_vertices_temp_bytes(size_t n_verts, size_t n_win) {
    if (n_verts * n_win >= (1ull << 31)) return 0;
    return vert_layout(nullptr, n_verts, n_win).total;
}

int sd_spinehead_box_vertices(const void* verts_dev, int verts_f32, const int32_t* labels_dev, size_t n_verts, const int64_t* win_offset_dev, size_t n_win,
                              const int32_t* win_size_xyz, int stages, uint64_t* begin_dev, double* points_dev, int32_t* point_labels_dev,
                              size_t max_points, void* temp_dev, size_t temp_bytes, void* stream) {
    if (!verts_dev || !labels_dev || !win_offset_dev || !win_size_xyz || !begin_dev || !temp_dev || n_verts < 1 || n_win < 1 ||
        n_verts * n_win >= (1ull << 31) || !(stages & 3) || ((stages & 2) && (!points_dev || !point_labels_dev || max_points < 1)))
        return sd_fail_msg(SD_ERR_INVALID, "sd_spinehead_box_vertices: bad argument");
    const VertLayout l = vert_layout(temp_dev, n_verts, n_win);
    if (temp_bytes < l.total) return sd_fail_msg(SD_ERR_NOMEM, "sd_spinehead_box_vertices: scratch too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t n = n_verts * n_win;
    const long long* off = reinterpret_cast<const long long*>(win_offset_dev);
    if (stages & 1) {
        D3 half, edge;
        for (int a = 0; a < 3; ++a) {
            if (win_size_xyz[a] < 1) return sd_fail_msg(SD_ERR_INVALID, "sd_spinehead_box_vertices: bad window size");
            half.v[a] = (double)win_size_xyz[a] / 2;                    // offset + size / 2 (float64 in the reference)
            edge.v[a] = (double)(float)((double)win_size_xyz[a] / 2);   // the half edges are C floats (in_bounding_boxC.pyx)
        }
        if (verts_f32) hipLaunchKernelGGL(k_shv_flags<float>, dim3(grid_for(n, PG)), dim3(256), 0, s, reinterpret_cast<const float*>(verts_dev), n_verts, off, n_win, half, edge, l.flag);
        else hipLaunchKernelGGL(k_shv_flags<double>, dim3(grid_for(n, PG)), dim3(256), 0, s, reinterpret_cast<const double*>(verts_dev), n_verts, off, n_win, half, edge, l.flag);
        const int rc = scan_u32("sd_spinehead_box_vertices", l.prim, l.flag, l.pos, n, s);
        if (rc != SD_OK) return rc;
        hipLaunchKernelGGL(k_shv_begin, dim3(grid_for(n_win + 2, PG)), dim3(256), 0, s, l.pos, n_verts, n_win, begin_dev);
    }
    if (stages & 2) {
        if (verts_f32) hipLaunchKernelGGL(k_shv_scatter<float>, dim3(grid_for(n, PG)), dim3(256), 0, s, reinterpret_cast<const float*>(verts_dev), labels_dev, n_verts, off, n_win, l.flag, l.pos, max_points, points_dev, point_labels_dev);
        else hipLaunchKernelGGL(k_shv_scatter<double>, dim3(grid_for(n, PG)), dim3(256), 0, s, reinterpret_cast<const double*>(verts_dev), labels_dev, n_verts, off, n_win, l.flag, l.pos, max_points, points_dev, point_labels_dev);
    }
    return launch_status("sd_spinehead_box_vertices: launch failed");
}

int sd_spinehead_queries(const int32_t* peaks_dev, const int32_t* n_peaks_dev, size_t n_win, size_t max_peaks, size_t q_slots, const double* ds_xyz,
                         uint32_t* q_cell_dev, double* q_xyz_dev, void* stream) {
    if (!peaks_dev || !n_peaks_dev || !ds_xyz || !q_cell_dev || !q_xyz_dev || n_win < 1 || q_slots < 1 || q_slots > max_peaks || max_peaks >= (1ull << 31) ||
        n_win >= (1ull << 31) || n_win * q_slots >= (1ull << 31))
        return sd_fail_msg(SD_ERR_INVALID, "sd_spinehead_queries: bad argument");
    D3 ds;
    for (int a = 0; a < 3; ++a) ds.v[a] = ds_xyz[a];
    hipLaunchKernelGGL(k_sh_queries, dim3(grid_for(n_win * q_slots, VG)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), peaks_dev, n_peaks_dev, n_win,
                       max_peaks, q_slots, ds, q_cell_dev, q_xyz_dev);
    return launch_status("sd_spinehead_queries: launch failed");
}

int sd_spinehead_markers(const int32_t* peaks_dev, const int32_t* n_peaks_dev, const int32_t* votes_dev, size_t max_peaks, int X, int Y, int Z,
                         int32_t* markers_dev, void* stream) {
    if (!peaks_dev || !n_peaks_dev || !votes_dev || !markers_dev || max_peaks < 1 || max_peaks >= (1ull << 31) || bad_dims(X, Y, Z))
        return sd_fail_msg(SD_ERR_INVALID, "sd_spinehead_markers: bad argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(markers_dev, 0, (size_t)X * Y * Z * sizeof(int), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "sd_spinehead_markers: memset failed");
    hipLaunchKernelGGL(k_sh_markers, dim3(grid_for(max_peaks, VG)), dim3(256), 0, s, peaks_dev, n_peaks_dev, votes_dev, max_peaks, Y, Z, markers_dev);
    return launch_status("sd_spinehead_markers: launch failed");
}

int sd_spinehead_select(const int32_t* flood_dev, int X, int Y, int Z, const int64_t* c_xyz, const int64_t* win_offset_xyz, const double* scaling_xyz,
                        int32_t* objects_dev, int32_t* result_dev, void* ws, size_t ws_bytes, void* stream) {
    if (!flood_dev || !c_xyz || !win_offset_xyz || !scaling_xyz || !result_dev || !ws || bad_dims(X, Y, Z)) return sd_fail_msg(SD_ERR_INVALID, "sd_spinehead_select: bad argument");
    ShLayout l;
    if (ws_bytes < layout(l, ws, X, Y, Z)) return sd_fail_msg(SD_ERR_NOMEM, "sd_spinehead_select: workspace too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t* head = l.u8;
    int* L = objects_dev ? objects_dev : l.lab;
    int *cnt = l.tab[0], *cbox = l.tab[1], *nb = l.scal->i;
    unsigned long long* sel = l.scal->sel;
    const size_t nvox = (size_t)X * Y * Z;
    const int g = grid_for(nvox, VG);
    const int ext[3] = {X, Y, Z};
    B6 box;
    I3 off, c;
    D3 sc;
    for (int a = 0; a < 3; ++a) {      // labels[c - 10 : c + 11] with numpy's slice rules: a negative bound wraps once, then both clip to the extent
        long long lo = (long long)c_xyz[a] - 10, hi = (long long)c_xyz[a] + 11;
        const long long n = ext[a];
        if (lo < 0) lo += n;
        if (hi < 0) hi += n;
        lo = lo < 0 ? 0 : (lo > n ? n : lo);
        hi = hi < 0 ? 0 : (hi > n ? n : hi);
        box.lo[a] = (int)lo; box.hi[a] = (int)hi;
        c.v[a] = (long long)c_xyz[a];
        off.v[a] = (long long)win_offset_xyz[a];
        sc.v[a] = scaling_xyz[a];
    }
    hipLaunchKernelGGL(k_shs_head, dim3(g), dim3(256), 0, s, flood_dev, nvox, head);
    const int rc = sd_object_segmentation(head, X, Y, Z, 0.0, nullptr, nullptr, 0, nullptr, 0, 0, 0, L, nb, nullptr, l.cc, l.cc_bytes, stream);
    if (rc != SD_OK) return rc;
    hipLaunchKernelGGL(k_sh_zero, dim3(grid_for(l.T, TG)), dim3(256), 0, s, cnt, l.T);
    hipLaunchKernelGGL(k_sh_zero, dim3(grid_for(l.T, TG)), dim3(256), 0, s, cbox, l.T);
    hipLaunchKernelGGL(k_shs_init, dim3(1), dim3(64), 0, s, sel);
    hipLaunchKernelGGL(k_shs_count, dim3(g), dim3(256), 0, s, L, X, Y, Z, box, off, c, sc, cnt, cbox, sel);
    hipLaunchKernelGGL(k_shs_best, dim3(grid_for(l.T, TG)), dim3(256), 0, s, cbox, nb, sel);
    hipLaunchKernelGGL(k_shs_nearest, dim3(g), dim3(256), 0, s, L, X, Y, Z, off, c, sc, sel);
    hipLaunchKernelGGL(k_shs_final, dim3(1), dim3(64), 0, s, cnt, nb, sel, result_dev);
    return launch_status("sd_spinehead_select: launch failed");
}

}  // extern "C"
