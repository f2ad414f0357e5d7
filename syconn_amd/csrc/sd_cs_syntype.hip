// Synapse statistics of contact sites on the device: the gfx950 counterpart of extract_cs_syntype
// (/root/reference/syconn/extraction/block_processing_C.pyx:78-158), which scans a chunk once on one core and keeps its results in
// std::unordered_maps, and the type masks of _contact_site_extraction_thread (cs_extraction_steps.py:411-433).
//
// Step 1 (k_cst_scan) is one streaming pass over a window of the four volumes, as k_segstats_scan (sd_segstats.hip): one update per
// run of equal labels (and, for the syn record, of equal syn flags) with order-independent atomics into an open-addressing table that
// holds per site its cs record, its syn record and the two type counters -- the result does not depend on the schedule.  Steps 2-3
// order the sites by id and lay out the dense records.  Step 4 (k_cst_voxels) lists each site's syn voxels in scan order: one
// workgroup walks the site's syn bounding box in raster order with a running block prefix count, so the order is exactly the
// reference's and no sort is needed.
#include "../../include/syconn_dense.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sd_hash.h"

namespace {

// Table of `cap` slots, structure of arrays in one buffer:
//   keys | cs_first | cs_size | syn_first | syn_size | asym | sym   (u64[cap] each; first = smallest raster index in the window)
//   bb i32[12][cap]: cs min x, y, z, cs max x, y, z, syn min x, y, z, syn max x, y, z (max = last + 1)
struct CstTable {
    u64 *keys, *cs_first, *cs_size, *syn_first, *syn_size, *asym, *sym;
    int* bb;
    u64 cap;
};
constexpr size_t CST_SLOT_BYTES = 7 * 8 + 12 * 4;
__host__ __device__ inline CstTable cst_table(void* base, u64 cap) {
    CstTable t;
    t.keys = reinterpret_cast<u64*>(base);
    t.cs_first = t.keys + cap; t.cs_size = t.cs_first + cap; t.syn_first = t.cs_size + cap; t.syn_size = t.syn_first + cap;
    t.asym = t.syn_size + cap; t.sym = t.asym + cap;
    t.bb = reinterpret_cast<int*>(t.sym + cap);
    t.cap = cap;
    return t;
}

__global__ __launch_bounds__(256) void k_cst_init(CstTable t) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < t.cap; i += (u64)gridDim.x * 256) {
        t.keys[i] = EMPTY; t.cs_first[i] = ~0ull; t.cs_size[i] = 0; t.syn_first[i] = ~0ull; t.syn_size[i] = 0;
        t.asym[i] = 0; t.sym[i] = 0;
#pragma unroll
        for (int r = 0; r < 12; ++r) t.bb[r * t.cap + i] = (r % 6) < 3 ? 0x7fffffff : 0;
    }
}

struct CstParams {
    const void* cs; const uint8_t* syn; const uint8_t* asym; const uint8_t* sym;
    int X, Y, Z;                        // shape of the four volumes (z fastest)
    int ox, oy, oz, nx, ny, nz;         // the window the pass reads
    CstTable t;
    void* cs_out; void* syn_out;        // optional (nx, ny, nz) copies of the window: the keys, the keys where syn != 0
    int* status;
};

__device__ __forceinline__ void rec_update(const CstTable& t, long s, int rec, u64 lin, int x, int y, int z, int len) {
    u64* first = rec ? t.syn_first : t.cs_first;
    u64* size = rec ? t.syn_size : t.cs_size;
    int* bb = t.bb + 6 * rec * t.cap;
    atomicMin(&first[s], lin);
    atomicAdd(&size[s], (u64)len);
    atomicMin(&bb[0 * t.cap + s], x); atomicMin(&bb[1 * t.cap + s], y); atomicMin(&bb[2 * t.cap + s], z);
    atomicMax(&bb[3 * t.cap + s], x + 1); atomicMax(&bb[4 * t.cap + s], y + 1); atomicMax(&bb[5 * t.cap + s], z + len);
}

// one wave = 64 consecutive voxels of the flattened window; a run head is the wave's first lane, the first voxel of a z-row or a
// change of the key (cs runs) or of the key or syn flag (syn runs).  The type masks are read only where the voxel is syn.
template <typename L>
__global__ __launch_bounds__(256) void k_cst_scan(const CstParams p) {
    const int lane = threadIdx.x & 63;
    const u64 nvox = (u64)p.nx * p.ny * p.nz;
    const u64 nwaves = (nvox + 63) / 64;
    const L* cs = reinterpret_cast<const L*>(p.cs);
    for (u64 w = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); w < nwaves; w += (u64)gridDim.x * 4) {
        const u64 base = w * 64, lin = base + lane;
        const int nvalid = (int)((nvox - base) < 64 ? (nvox - base) : 64);
        const bool valid = lane < nvalid;
        const u64 li = valid ? lin : (nvox - 1);
        int z, y, x;
        if (nvox < (1ull << 32)) {
            const unsigned u = (unsigned)li, r = u / (unsigned)p.nz, q = r / (unsigned)p.ny;
            z = (int)(u - r * (unsigned)p.nz); y = (int)(r - q * (unsigned)p.ny); x = (int)q;
        } else {
            z = (int)(li % p.nz); y = (int)((li / p.nz) % p.ny); x = (int)(li / ((u64)p.nz * p.ny));
        }
        const u64 g = ((u64)(p.ox + x) * p.Y + (u64)(p.oy + y)) * p.Z + (u64)(p.oz + z);
        u64 key = 0;
        unsigned sv = 0, av = 0, yv = 0;
        if (valid) { key = (u64)cs[g]; sv = p.syn[g]; }
        const bool sflag = valid && key != 0 && sv != 0;
        if (sflag) { av = p.asym[g]; yv = p.sym[g]; }
        if (valid && p.cs_out) reinterpret_cast<L*>(p.cs_out)[lin] = (L)key;
        if (valid && p.syn_out) reinterpret_cast<L*>(p.syn_out)[lin] = sv ? (L)key : (L)0;
        const u64 prevk = __shfl_up(key, 1, 64);
        const int prevs = __shfl_up((int)sflag, 1, 64);
        const bool row_start = (lane == 0) || (z == 0);
        const bool chead = valid && (row_start || key != prevk);
        const int clen = run_length(chead, lane, nvalid);
        const bool shead = valid && (chead || (int)sflag != prevs);
        const int slen = run_length(shead, lane, nvalid);
        const u64 am = __ballot(sflag && av == 1), ym = __ballot(sflag && yv == 1);
        if (chead && key != 0) {
            const long s = find_or_insert(p.t.keys, p.t.cap, key);
            if (s < 0) atomicExch(&p.status[0], 1);
            else rec_update(p.t, s, 0, lin, x, y, z, clen);
        }
        if (shead && sflag) {
            const long s = find_or_insert(p.t.keys, p.t.cap, key);
            if (s < 0) { atomicExch(&p.status[0], 1); continue; }
            rec_update(p.t, s, 1, lin, x, y, z, slen);
            const u64 run = (slen >= 64 ? ~0ull : ((1ull << slen) - 1ull)) << lane;
            const int na = __popcll(am & run), ny = __popcll(ym & run);
            if (na) atomicAdd(&p.t.asym[s], (u64)na);
            if (ny) atomicAdd(&p.t.sym[s], (u64)ny);
        }
    }
}

__global__ __launch_bounds__(256) void k_cst_compact(CstTable t, u64* ids, int* slots, u64* count, u64 max_out) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < t.cap; i += (u64)gridDim.x * 256) {
        const u64 k = t.keys[i];
        if (k == EMPTY || t.cs_size[i] == 0) continue;
        const u64 o = atomicAdd(count, 1ull);
        if (o >= max_out) continue;
        ids[o] = k; slots[o] = (int)i;
    }
}

// dense records (SD_CST_COLS int64 per site, in the order of `slots`; layout in include/syconn_dense.h), column 23 left for the scan
__global__ __launch_bounds__(256) void k_cst_gather(CstTable t, const int* slots, long n, int nx, int ny, int nz, int64_t* rec) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const u64 s = (u64)slots[i];
        int64_t* r = rec + i * SD_CST_COLS;
        r[0] = (int64_t)t.keys[s];
        for (int rc = 0; rc < 2; ++rc) {
            const u64 f = rc ? t.syn_first[s] : t.cs_first[s], sz = rc ? t.syn_size[s] : t.cs_size[s];
            int64_t* q = r + 1 + 10 * rc;
            const int* bb = t.bb + 6 * rc * t.cap;
            if (sz) {
                q[0] = (int64_t)(f / ((u64)ny * nz)); q[1] = (int64_t)((f / nz) % ny); q[2] = (int64_t)(f % nz);
            } else {
                q[0] = q[1] = q[2] = 0;
            }
            q[3] = (int64_t)sz;
            for (int a = 0; a < 6; ++a) q[4 + a] = sz ? bb[a * t.cap + s] : 0;
        }
        r[21] = (int64_t)t.asym[s]; r[22] = (int64_t)t.sym[s];
    }
}

// column 23 = exclusive prefix sum of the syn sizes (column 14) in record order; *total = their sum.  One workgroup.
__global__ __launch_bounds__(256) void k_cst_offsets(int64_t* rec, long n, int64_t* total) {
    __shared__ int64_t wsum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int64_t run = 0;
    for (long b = 0; b < n; b += 256) {
        const long i = b + threadIdx.x;
        const int64_t v = i < n ? rec[i * SD_CST_COLS + 14] : 0;
        int64_t inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        int64_t before = run;
        for (int k = 0; k < wv; ++k) before += wsum[k];
        if (i < n) rec[i * SD_CST_COLS + 23] = before + inc - v;
        run += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = run;
}

// one workgroup per site: its syn voxels in raster order of its syn box, at rec[23] + rank, as [x + off_x, y + off_y, z + off_z]
template <typename L>
__global__ __launch_bounds__(256) void k_cst_voxels(const L* __restrict__ cs, const uint8_t* __restrict__ syn, int Y, int Z, int ox,
                                                    int oy, int oz, const int64_t* __restrict__ rec, int64_t n_syn, int64_t offx,
                                                    int64_t offy, int64_t offz, int64_t* __restrict__ vox, int* status) {
    __shared__ int wcnt[4];
    const int64_t* r = rec + (long)blockIdx.x * SD_CST_COLS;
    const int64_t cnt = r[14], start = r[23];
    if (cnt == 0) return;
    const u64 key = (u64)r[0];
    const int x0 = (int)r[15], y0 = (int)r[16], z0 = (int)r[17];
    const u64 bx = (u64)(r[18] - x0), by = (u64)(r[19] - y0), bz = (u64)(r[20] - z0), tot = bx * by * bz;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int64_t done = 0;
    for (u64 b = 0; b < tot && done < cnt; b += 256) {
        const u64 i = b + threadIdx.x;
        int x = 0, y = 0, z = 0;
        bool f = false;
        if (i < tot) {
            z = (int)(i % bz); y = (int)((i / bz) % by); x = (int)(i / (bz * by));
            x += x0; y += y0; z += z0;
            const u64 g = ((u64)(ox + x) * Y + (u64)(oy + y)) * Z + (u64)(oz + z);
            f = (u64)cs[g] == key && syn[g] != 0;
        }
        const u64 m = __ballot(f);
        if (lane == 0) wcnt[wv] = __popcll(m);
        __syncthreads();
        int64_t pos = done + __popcll(m & ((1ull << lane) - 1ull));
        for (int k = 0; k < wv; ++k) pos += wcnt[k];
        if (f) {
            if (pos < cnt && start + pos < n_syn) {
                int64_t* v = vox + 3 * (start + pos);
                v[0] = x + offx; v[1] = y + offy; v[2] = z + offz;
            } else {
                atomicExch(status, 1);
            }
        }
        done += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (threadIdx.x == 0 && done != cnt) atomicExch(status, 1);
}

// type masks: uint8 raw data -> v >= 123; uint64 labels -> v == label (cs_extraction_steps.py:411-430)
template <typename V>
__global__ __launch_bounds__(256) void k_syntype_masks(const V* __restrict__ vol, u64 n, u64 la, u64 lb, uint8_t* __restrict__ a,
                                                       uint8_t* __restrict__ b, int raw) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        const u64 v = (u64)vol[i];
        if (raw) {
            a[i] = v >= 123 ? 1 : 0;
        } else {
            a[i] = v == la ? 1 : 0;
            if (b) b[i] = v == lb ? 1 : 0;
        }
    }
}

}  // namespace

extern "C" {

size_t sd_cs_syntype_table_bytes(size_t capacity) { return capacity * CST_SLOT_BYTES; }

int sd_cs_syntype_scan(const void* cs_dev, int dtype, const uint8_t* syn_dev, const uint8_t* asym_dev, const uint8_t* sym_dev, int X,
                       int Y, int Z, int ox, int oy, int oz, int nx, int ny, int nz, void* table_dev, size_t cap, void* cs_out_dev,
                       void* syn_out_dev, int32_t* status_dev, void* stream) {
    if (!cs_dev || !syn_dev || !asym_dev || !sym_dev || !table_dev || !status_dev || X <= 0 || Y <= 0 || Z <= 0)
        return sd_fail_msg(SD_ERR_INVALID, "sd_cs_syntype_scan: bad argument");
    if (dtype != SD_U32 && dtype != SD_U64) return sd_fail_msg(SD_ERR_INVALID, "sd_cs_syntype_scan: dtype must be SD_U32 or SD_U64");
    if (ox < 0 || oy < 0 || oz < 0 || nx < 0 || ny < 0 || nz < 0 || (long)ox + nx > X || (long)oy + ny > Y || (long)oz + nz > Z)
        return sd_fail_msg(SD_ERR_INVALID, "sd_cs_syntype_scan: window outside the volume");
    if (!pow2(cap) || cap > (1ull << 31)) return sd_fail_msg(SD_ERR_INVALID, "sd_cs_syntype_scan: capacity must be a power of two <= 2^31");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(status_dev, 0, sizeof(int32_t), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    CstParams p{};
    p.cs = cs_dev; p.syn = syn_dev; p.asym = asym_dev; p.sym = sym_dev;
    p.X = X; p.Y = Y; p.Z = Z; p.ox = ox; p.oy = oy; p.oz = oz; p.nx = nx; p.ny = ny; p.nz = nz;
    p.t = cst_table(table_dev, cap); p.cs_out = cs_out_dev; p.syn_out = syn_out_dev; p.status = status_dev;
    hipLaunchKernelGGL(k_cst_init, dim3(grid_for(cap)), dim3(256), 0, s, p.t);
    const u64 nwaves = ((u64)nx * ny * nz + 63) / 64;
    if (nwaves) {
        const int grid = (int)((nwaves + 3) / 4 < 8192 ? (nwaves + 3) / 4 : 8192);
        if (dtype == SD_U64) hipLaunchKernelGGL(k_cst_scan<uint64_t>, dim3(grid), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(k_cst_scan<uint32_t>, dim3(grid), dim3(256), 0, s, p);
    }
    return launch_status("sd_cs_syntype_scan: launch failed");
}

int sd_cs_syntype_compact(const void* table_dev, size_t cap, uint64_t* ids_dev, int32_t* slots_dev, size_t max_out,
                          uint64_t* count_dev, void* stream) {
    if (!table_dev || !pow2(cap) || !ids_dev || !slots_dev || !count_dev)
        return sd_fail_msg(SD_ERR_INVALID, "sd_cs_syntype_compact: bad argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(count_dev, 0, sizeof(uint64_t), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    hipLaunchKernelGGL(k_cst_compact, dim3(grid_for(cap)), dim3(256), 0, s, cst_table(const_cast<void*>(table_dev), cap),
                       reinterpret_cast<u64*>(ids_dev), slots_dev, reinterpret_cast<u64*>(count_dev), (u64)max_out);
    return launch_status("sd_cs_syntype_compact: launch failed");
}

int sd_cs_syntype_records(const void* table_dev, size_t cap, const int32_t* slots_dev, int64_t n, int nx, int ny, int nz,
                          int64_t* rec_dev, int64_t* n_syn_dev, void* stream) {
    if (!table_dev || !pow2(cap) || n < 0 || (n && (!slots_dev || !rec_dev)) || !n_syn_dev || nx < 0 || ny < 0 || nz < 0)
        return sd_fail_msg(SD_ERR_INVALID, "sd_cs_syntype_records: bad argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n) hipLaunchKernelGGL(k_cst_gather, dim3(grid_for((u64)n)), dim3(256), 0, s, cst_table(const_cast<void*>(table_dev), cap),
                              slots_dev, (long)n, nx, ny, nz, rec_dev);
    hipLaunchKernelGGL(k_cst_offsets, dim3(1), dim3(256), 0, s, rec_dev, (long)n, n_syn_dev);
    return launch_status("sd_cs_syntype_records: launch failed");
}

int sd_cs_syntype_voxels(const void* cs_dev, int dtype, const uint8_t* syn_dev, int X, int Y, int Z, int ox, int oy, int oz,
                         const int64_t* rec_dev, int64_t n, int64_t n_syn, const int64_t* offset_host, int64_t* vox_dev,
                         int32_t* status_dev, void* stream) {
    if (!cs_dev || !syn_dev || X <= 0 || Y <= 0 || Z <= 0 || ox < 0 || oy < 0 || oz < 0 || n < 0 || n_syn < 0 || !offset_host ||
        !status_dev || (n && !rec_dev) || (n_syn && !vox_dev))
        return sd_fail_msg(SD_ERR_INVALID, "sd_cs_syntype_voxels: bad argument");
    if (dtype != SD_U32 && dtype != SD_U64) return sd_fail_msg(SD_ERR_INVALID, "sd_cs_syntype_voxels: dtype must be SD_U32 or SD_U64");
    if (n > 0x7fffffffll) return sd_fail_msg(SD_ERR_INVALID, "sd_cs_syntype_voxels: too many sites");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(status_dev, 0, sizeof(int32_t), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    if (n == 0 || n_syn == 0) return SD_OK;
    const int64_t ofx = offset_host[0], ofy = offset_host[1], ofz = offset_host[2];
    if (dtype == SD_U64)
        hipLaunchKernelGGL(k_cst_voxels<uint64_t>, dim3((unsigned)n), dim3(256), 0, s, reinterpret_cast<const uint64_t*>(cs_dev), syn_dev,
                           Y, Z, ox, oy, oz, rec_dev, n_syn, ofx, ofy, ofz, vox_dev, status_dev);
    else
        hipLaunchKernelGGL(k_cst_voxels<uint32_t>, dim3((unsigned)n), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(cs_dev), syn_dev,
                           Y, Z, ox, oy, oz, rec_dev, n_syn, ofx, ofy, ofz, vox_dev, status_dev);
    return launch_status("sd_cs_syntype_voxels: launch failed");
}

int sd_syntype_masks(const void* vol_dev, int dtype, size_t n, uint64_t label_a, uint64_t label_b, uint8_t* out_a_dev,
                     uint8_t* out_b_dev, void* stream) {
    if (!vol_dev || !out_a_dev || (dtype != SD_U8 && dtype != SD_U64) || (dtype == SD_U8 && out_b_dev))
        return sd_fail_msg(SD_ERR_INVALID, "sd_syntype_masks: bad argument");
    if (n == 0) return SD_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == SD_U8)
        hipLaunchKernelGGL(k_syntype_masks<uint8_t>, dim3(grid_for(n)), dim3(256), 0, s, reinterpret_cast<const uint8_t*>(vol_dev),
                           (u64)n, (u64)label_a, (u64)label_b, out_a_dev, out_b_dev, 1);
    else
        hipLaunchKernelGGL(k_syntype_masks<uint64_t>, dim3(grid_for(n)), dim3(256), 0, s, reinterpret_cast<const uint64_t*>(vol_dev),
                           (u64)n, (u64)label_a, (u64)label_b, out_a_dev, out_b_dev, 0);
    return launch_status("sd_syntype_masks: launch failed");
}

}  // extern "C"
