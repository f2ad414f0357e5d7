// Contact-site extraction: the stencil of block_processing_C.pyx and the per-site closing of
// _contact_site_extraction_thread on the MI355X.  Volumes are (X,Y,Z) with z fastest; every call is asynchronous on `stream`.
#include "../../include/syconn_dense.h"
#include "sd_host_util.h"
#include <stdint.h>

namespace {

constexpr int CP_TX = 8, CP_TY = 8, CP_TZ = 16;        // output voxels per workgroup of the partner stencil
constexpr int CP_NOUT = CP_TX * CP_TY * CP_TZ;
constexpr int CP_SLOTS = 8;                              // distinct ids a lane counts in registers before the exact fallback
constexpr int CP_LDS_MAX = 64 * 1024;
constexpr int CP_WIN_MAX = 4096;                         // window voxels the exact fallback stages in LDS
constexpr uint64_t CP_OVF = ~0ull;                       // "table overflowed": never a packed pair (the high half is < 2^32 - 1)

__global__ __launch_bounds__(256) void k_seg_boundaries(const uint32_t* __restrict__ seg, int X, int Y, int Z,
                                                        uint8_t* __restrict__ out) {
    const size_t n = (size_t)X * Y * Z, sX = (size_t)Y * Z;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int z = (int)(i % Z), y = (int)((i / Z) % Y), x = (int)(i / sX);
        const uint32_t c = seg[i];
        bool b = false;
        if (c) {
            b |= x > 0 && seg[i - sX] != c;
            b |= x + 1 < X && seg[i + sX] != c;
            b |= y > 0 && seg[i - Z] != c;
            b |= y + 1 < Y && seg[i + Z] != c;
            b |= z > 0 && seg[i - 1] != c;
            b |= z + 1 < Z && seg[i + 1] != c;
        }
        out[i] = b ? 1 : 0;
    }
}

__device__ inline uint64_t pack_pair(uint32_t c, uint32_t k) {
    return c > k ? ((uint64_t)k << 32) | c : ((uint64_t)c << 32) | k;
}

// One workgroup = an 8 x 8 x 16 block of outputs.  The uint32 input block plus its (sx-1, sy-1, sz-1) halo sits in LDS; the
// boundary centres of the block are listed in LDS so that every lane works on one (the mask is sparse).  A lane counts the ids of
// its window in CP_SLOTS register slots; a window with more distinct ids stores CP_OVF, which k_contact_partners_exact resolves.
__global__ __launch_bounds__(256) void k_contact_partners(const uint8_t* __restrict__ edges, const uint32_t* __restrict__ seg,
                                                          int X, int Y, int Z, int sx, int sy, int sz, uint64_t* __restrict__ out,
                                                          int OX, int OY, int OZ, unsigned* __restrict__ n_ovf) {
    extern __shared__ uint32_t tile[];
    __shared__ uint16_t list[CP_NOUT];
    __shared__ int n_list, ovf_block;
    const int LX = CP_TX + sx - 1, LY = CP_TY + sy - 1, LZ = CP_TZ + sz - 1;
    const int ox0 = blockIdx.x * CP_TX, oy0 = blockIdx.y * CP_TY, oz0 = blockIdx.z * CP_TZ;
    const int hx = sx / 2, hy = sy / 2, hz = sz / 2;
    if (threadIdx.x == 0) { n_list = 0; ovf_block = 0; }
    for (int i = threadIdx.x; i < LX * LY * LZ; i += blockDim.x) {
        const int lz = i % LZ, ly = (i / LZ) % LY, lx = i / (LY * LZ);
        const int gx = ox0 + lx, gy = oy0 + ly, gz = oz0 + lz;
        tile[i] = (gx < X && gy < Y && gz < Z) ? seg[((size_t)gx * Y + gy) * Z + gz] : 0u;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < CP_NOUT; o += blockDim.x) {
        const int tz = o % CP_TZ, ty = (o / CP_TZ) % CP_TY, tx = o / (CP_TY * CP_TZ);
        const int x = ox0 + tx, y = oy0 + ty, z = oz0 + tz;
        if (x >= OX || y >= OY || z >= OZ) continue;
        if (edges[((size_t)(x + hx) * Y + (y + hy)) * Z + (z + hz)]) list[atomicAdd(&n_list, 1)] = (uint16_t)o;
        else out[((size_t)x * OY + y) * OZ + z] = 0;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n_list; k += blockDim.x) {
        const int o = list[k];
        const int tz = o % CP_TZ, ty = (o / CP_TZ) % CP_TY, tx = o / (CP_TY * CP_TZ);
        const uint32_t c = tile[((tx + hx) * LY + (ty + hy)) * LZ + tz + hz];
        uint32_t ids[CP_SLOTS];
        int cnt[CP_SLOTS];
#pragma unroll
        for (int s = 0; s < CP_SLOTS; ++s) { ids[s] = 0; cnt[s] = 0; }
        bool ovf = false;
        for (int i = 0; i < sx && !ovf; ++i)
            for (int j = 0; j < sy; ++j) {
                const uint32_t* row = tile + ((tx + i) * LY + ty + j) * LZ + tz;
                for (int l = 0; l < sz; ++l) {
                    const uint32_t v = row[l];
                    if (v == 0 || v == c) continue;
                    bool done = false;
#pragma unroll
                    for (int s = 0; s < CP_SLOTS; ++s) {
                        if (!done && cnt[s] == 0) { ids[s] = v; cnt[s] = 1; done = true; }
                        else if (!done && ids[s] == v) { ++cnt[s]; done = true; }
                    }
                    ovf |= !done;
                }
            }
        uint64_t res = CP_OVF;
        if (!ovf) {
            int best = 0;
            uint32_t key = 0;
#pragma unroll
            for (int s = 0; s < CP_SLOTS; ++s)      // std::map order with a strict '>': the smallest id of the highest count
                if (cnt[s] > best || (cnt[s] == best && best > 0 && ids[s] < key)) { best = cnt[s]; key = ids[s]; }
            res = best > 0 ? pack_pair(c, key) : 0;
        } else {
            ovf_block = 1;
        }
        out[((size_t)(ox0 + tx) * OY + oy0 + ty) * OZ + oz0 + tz] = res;
    }
    __syncthreads();
    if (threadIdx.x == 0 && ovf_block) atomicAdd(n_ovf, 1u);
}

// Exact count for the windows that overflowed the register slots: the workgroup stages the window in LDS, every lane takes
// positions p and counts how often win[p] occurs (O(W^2 / 256) per window), and a reduction keeps (highest count, smallest id).
// Returns at once when no workgroup of k_contact_partners overflowed; otherwise scans the output for CP_OVF.
__global__ __launch_bounds__(256) void k_contact_partners_exact(const uint32_t* __restrict__ seg, int X, int Y, int Z, int sx,
                                                                int sy, int sz, uint64_t* __restrict__ out, int OX, int OY, int OZ,
                                                                const unsigned* __restrict__ n_ovf) {
    if (*n_ovf == 0) return;
    __shared__ uint32_t win[CP_WIN_MAX];
    __shared__ uint32_t flagged[256];
    __shared__ int n_flag;
    __shared__ int r_cnt[256];
    __shared__ uint32_t r_id[256];
    const int W = sx * sy * sz;
    const size_t n = (size_t)OX * OY * OZ;
    for (size_t base = blockIdx.x * (size_t)256; base < n; base += (size_t)gridDim.x * 256) {
        if (threadIdx.x == 0) n_flag = 0;
        __syncthreads();
        const size_t i = base + threadIdx.x;
        if (i < n && out[i] == CP_OVF) flagged[atomicAdd(&n_flag, 1)] = threadIdx.x;
        __syncthreads();
        const int nf = n_flag;
        for (int f = 0; f < nf; ++f) {
            const size_t o = base + flagged[f];
            const int z = (int)(o % OZ), y = (int)((o / OZ) % OY), x = (int)(o / ((size_t)OY * OZ));
            for (int p = threadIdx.x; p < W; p += 256) {
                const int l = p % sz, j = (p / sz) % sy, q = p / (sy * sz);
                win[p] = seg[((size_t)(x + q) * Y + y + j) * Z + z + l];
            }
            __syncthreads();
            const uint32_t c = seg[((size_t)(x + sx / 2) * Y + y + sy / 2) * Z + z + sz / 2];
            int best = 0;
            uint32_t key = 0;
            for (int p = threadIdx.x; p < W; p += 256) {
                const uint32_t v = win[p];
                if (v == 0 || v == c || (best > 0 && v == key)) continue;
                int m = 0;
                for (int q = 0; q < W; ++q) m += win[q] == v;
                if (m > best || (m == best && v < key)) { best = m; key = v; }
            }
            r_cnt[threadIdx.x] = best;
            r_id[threadIdx.x] = key;
            __syncthreads();
            for (int h = 128; h > 0; h >>= 1) {
                if (threadIdx.x < h) {
                    const int cb = r_cnt[threadIdx.x + h];
                    const uint32_t ib = r_id[threadIdx.x + h];
                    if (cb > r_cnt[threadIdx.x] || (cb == r_cnt[threadIdx.x] && cb > 0 && ib < r_id[threadIdx.x])) {
                        r_cnt[threadIdx.x] = cb;
                        r_id[threadIdx.x] = ib;
                    }
                }
                __syncthreads();
            }
            if (threadIdx.x == 0) out[o] = r_cnt[0] > 0 ? pack_pair(c, r_id[0]) : 0;
            __syncthreads();
        }
        __syncthreads();                                         // n_flag is reset for the next piece
    }
}

// ---- per-site closing + dilation (cs_extraction_steps.py:437-461) ----------------------------------------------------------------
// Object table rows (int64[8]): id, box origin (x, y, z), box extent (x, y, z), offset of the box in the two uint8 workspace
// planes.  Rows are in ascending offset order; a voxel finds its row by binary search.
struct CdArgs {
    const int64_t* tab; int64_t n_obj, tot;
    const uint64_t* c0; int X, Y, Z;
    const uint8_t* in; uint8_t* dst;
    int axis, win, cap;
    int src;            // 0: set = (c0 == id); 1: set = (in <= thr); 2: set = (in > thr); 3: in holds distances
    int thr;
    int outside_in_set; // the erosion: everything outside the box is background of the eroded set, i.e. inside its complement
};

__device__ inline int64_t find_row(const int64_t* tab, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (tab[mid * 8 + 7] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One 1D pass of a truncated L1 distance transform inside every box of the batch: dst = min(cap, min_j src(v + j e_axis) + |j|).
__global__ __launch_bounds__(256) void k_box_dt_pass(CdArgs a) {
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < a.tot; v += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = find_row(a.tab, a.n_obj, v);
        const int64_t* row = a.tab + r * 8;
        const int ex = (int)row[4], ey = (int)row[5], ez = (int)row[6];
        const int64_t loc = v - row[7];
        const int lz = (int)(loc % ez), ly = (int)((loc / ez) % ey), lx = (int)(loc / ((int64_t)ey * ez));
        const int ext = a.axis == 0 ? ex : a.axis == 1 ? ey : ez;
        const int pos = a.axis == 0 ? lx : a.axis == 1 ? ly : lz;
        const int64_t lstride = a.axis == 0 ? (int64_t)ey * ez : a.axis == 1 ? ez : 1;
        const int64_t gstride = a.axis == 0 ? (int64_t)a.Y * a.Z : a.axis == 1 ? a.Z : 1;
        const int64_t g = ((int64_t)(row[1] + lx) * a.Y + row[2] + ly) * a.Z + row[3] + lz;
        const uint64_t id = (uint64_t)row[0];
        int best = a.cap;
        for (int j = -a.win; j <= a.win; ++j) {
            const int p = pos + j, dj = j < 0 ? -j : j;
            int val;
            if (p < 0 || p >= ext) {
                if (!a.outside_in_set) continue;
                val = 0;
            } else if (a.src == 0) {
                val = a.c0[g + j * gstride] == id ? 0 : a.cap;
            } else {
                const int d = a.in[v + j * lstride];
                val = a.src == 1 ? (d <= a.thr ? 0 : a.cap) : a.src == 2 ? (d > a.thr ? 0 : a.cap) : d;
            }
            best = min(best, val + dj);
        }
        a.dst[v] = (uint8_t)min(best, a.cap);
    }
}

// res(v) = (in <= thr) [src 1] or (in > thr) [src 2] or (c0 == id) [src 0]: background voxels of c0 take the smallest claiming id.
__global__ __launch_bounds__(256) void k_box_claim(CdArgs a, uint64_t* __restrict__ out) {
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < a.tot; v += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = find_row(a.tab, a.n_obj, v);
        const int64_t* row = a.tab + r * 8;
        const int ey = (int)row[5], ez = (int)row[6];
        const int64_t loc = v - row[7];
        const int lz = (int)(loc % ez), ly = (int)((loc / ez) % ey), lx = (int)(loc / ((int64_t)ey * ez));
        const int64_t g = ((int64_t)(row[1] + lx) * a.Y + row[2] + ly) * a.Z + row[3] + lz;
        if (a.c0[g] != 0) continue;
        const bool res = a.src == 1 ? a.in[v] <= a.thr : a.src == 2 ? a.in[v] > a.thr : false;
        if (res) atomicMin(reinterpret_cast<unsigned long long*>(out + g), (unsigned long long)row[0]);
    }
}

__global__ __launch_bounds__(256) void k_claim_init(const uint64_t* __restrict__ c0, size_t n, uint64_t* __restrict__ out) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = c0[i] ? c0[i] : ~0ull;
}

__global__ __launch_bounds__(256) void k_claim_finish(uint64_t* __restrict__ out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        if (out[i] == ~0ull) out[i] = 0;
}

}  // namespace

int sd_seg_boundaries(const uint32_t* seg_dev, int X, int Y, int Z, uint8_t* mask_dev, void* stream) {
    if (!seg_dev || !mask_dev || X <= 0 || Y <= 0 || Z <= 0) return sd_fail_msg(SD_ERR_INVALID, "sd_seg_boundaries: bad argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_seg_boundaries, dim3(grid_for((int64_t)X * Y * Z, 256 * 64)), dim3(256), 0, s, seg_dev, X, Y, Z, mask_dev);
    return launch_status("sd_seg_boundaries: launch failed");
}

size_t sd_contact_partners_workspace_bytes(void) { return 256; }

int sd_contact_partners(const uint8_t* edges_dev, const uint32_t* seg_dev, int X, int Y, int Z, int sx, int sy, int sz,
                        uint64_t* out_dev, void* workspace_dev, size_t ws_bytes, void* stream) {
    if (!edges_dev || !seg_dev || !out_dev || !workspace_dev || X <= 0 || Y <= 0 || Z <= 0)
        return sd_fail_msg(SD_ERR_INVALID, "sd_contact_partners: bad argument");
    if (sx <= 0 || sy <= 0 || sz <= 0 || !(sx & 1) || !(sy & 1) || !(sz & 1))
        return sd_fail_msg(SD_ERR_INVALID, "sd_contact_partners: the stencil must be odd along every axis");
    const int OX = X - sx + 1, OY = Y - sy + 1, OZ = Z - sz + 1;
    if (OX <= 0 || OY <= 0 || OZ <= 0) return SD_OK;                     // empty valid convolution
    const size_t lds = (size_t)(CP_TX + sx - 1) * (CP_TY + sy - 1) * (CP_TZ + sz - 1) * sizeof(uint32_t);
    if (lds > (size_t)CP_LDS_MAX || sx * sy * sz > CP_WIN_MAX)
        return sd_fail_msg(SD_ERR_INVALID, "sd_contact_partners: stencil too large for the LDS tile");
    if (ws_bytes < sd_contact_partners_workspace_bytes()) return sd_fail_msg(SD_ERR_NOMEM, "sd_contact_partners: workspace too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned* n_ovf = reinterpret_cast<unsigned*>(workspace_dev);
    if (hipMemsetAsync(n_ovf, 0, sizeof(unsigned), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    const dim3 grid((OX + CP_TX - 1) / CP_TX, (OY + CP_TY - 1) / CP_TY, (OZ + CP_TZ - 1) / CP_TZ);
    hipLaunchKernelGGL(k_contact_partners, grid, dim3(256), lds, s, edges_dev, seg_dev, X, Y, Z, sx, sy, sz, out_dev, OX, OY, OZ,
                       n_ovf);
    hipLaunchKernelGGL(k_contact_partners_exact, dim3(grid_for((int64_t)OX * OY * OZ, 2048)), dim3(256), 0, s, seg_dev, X, Y, Z,
                       sx, sy, sz, out_dev, OX, OY, OZ, n_ovf);
    return launch_status("sd_contact_partners: launch failed");
}

int sd_cs_close_dilate(const uint64_t* c0_dev, int X, int Y, int Z, const int64_t* table_dev, int64_t n_obj, int64_t tot_vox,
                       int n_close, int n_dilate, int flags, uint64_t* out_dev, void* workspace_dev, size_t ws_bytes, void* stream) {
    if (!c0_dev || !out_dev || X <= 0 || Y <= 0 || Z <= 0 || n_close < 0 || n_dilate < 0 || n_close > 100 || n_dilate > 100 ||
        n_obj < 0 || tot_vox < 0 || (n_obj > 0 && (!table_dev || !workspace_dev)))
        return sd_fail_msg(SD_ERR_INVALID, "sd_cs_close_dilate: bad argument");
    if (n_obj > 0 && ws_bytes < 2 * (size_t)tot_vox) return sd_fail_msg(SD_ERR_NOMEM, "sd_cs_close_dilate: workspace too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t n = (size_t)X * Y * Z;
    if (flags & SD_CS_FIRST) hipLaunchKernelGGL(k_claim_init, dim3(grid_for(n, 256 * 64)), dim3(256), 0, s, c0_dev, n, out_dev);
    if (n_obj > 0 && tot_vox > 0) {
        uint8_t* A = reinterpret_cast<uint8_t*>(workspace_dev);
        uint8_t* B = A + tot_vox;
        CdArgs a{table_dev, n_obj, tot_vox, c0_dev, X, Y, Z, nullptr, nullptr, 0, 0, 0, 0, 0, 0};
        const dim3 g(grid_for(tot_vox, 256 * 64)), b(256);
        // one truncated L1 distance transform (three 1D passes) of the set given by (src, thr) on `from`; result in the returned plane
        auto dt = [&](int src, int thr, const uint8_t* from, int win, int outside) -> uint8_t* {
            uint8_t* bufs[2] = {A, B};
            int w = (from == A) ? 1 : 0;
            const uint8_t* cur = from;
            for (int axis = 0; axis < 3; ++axis) {
                a.axis = axis; a.win = win; a.cap = win + 1; a.outside_in_set = outside;
                a.src = axis == 0 ? src : 3; a.thr = thr; a.in = cur; a.dst = bufs[w];
                hipLaunchKernelGGL(k_box_dt_pass, g, b, 0, s, a);
                cur = bufs[w];
                w ^= 1;
            }
            return const_cast<uint8_t*>(cur);
        };
        // res = dilate^k(close^n(c0 == id)) in the box: L1 dilation by n, erosion by n (outside = background), dilation by k
        int src = 0, thr = 0;
        const uint8_t* cur = nullptr;
        if (n_close > 0) {
            uint8_t* d1 = dt(0, 0, nullptr, n_close, 0);          // distance to the site
            uint8_t* d2 = dt(2, n_close, d1, n_close, 1);         // distance to the complement of its n-dilation (or the box border)
            cur = d2; src = 2; thr = n_close;                     // closed = d2 > n
        }
        if (n_dilate > 0) {
            uint8_t* d3 = dt(src, thr, cur, n_dilate, 0);
            cur = d3; src = 1; thr = n_dilate;                    // res = d3 <= k
        }
        if (src != 0) {                                           // n = k = 0: res is the site itself, nothing to claim
            a.src = src; a.thr = thr; a.in = cur;
            hipLaunchKernelGGL(k_box_claim, g, b, 0, s, a, out_dev);
        }
    }
    if (flags & SD_CS_LAST) hipLaunchKernelGGL(k_claim_finish, dim3(grid_for(n, 256 * 64)), dim3(256), 0, s, out_dev, n);
    return launch_status("sd_cs_close_dilate: launch failed");
}
