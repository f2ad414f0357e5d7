// The FCN semantic-segmentation network of the compartment step on gfx950: 3 x 3 same-padded convolutions (+ bias + ReLU, the last of
// a block with its 2 x 2 max-pool fused), stride-2 transposed convolutions as four output-parity sub-convolutions (+ bias + ReLU +
// eval BatchNorm + skip addition), a 1 x 1 classifier with the argmax, and the C ABI around them.  The plan, the packed layouts and
// the tap tables: sd_fcn.h.
//
// MFMA core (fcn_mma).  A workgroup of 4 waves computes 8 x 32 positions of one plane for NT <= 4 tiles of 16 output channels; the
// workgroups of the other channel groups are neighbours in the grid and read the same input.  The input channels pass through LDS in
// chunks of 32: a halo tile [10][34][32 channels] (pixel stride 40 elements) is filled with 16-byte copies, positions outside the
// plane and channels beyond cin_p are written as zeros -- the zero padding of the convolution and the zero row / column one past the
// high edge of the transposed convolution come from there, the MFMA loop has no branch.  The first layer fills the tile from the
// renderer's planar uint8 tensor (n_loc, C, nb_views, H, W) in place (plane p = location p / nb_views, view p % nb_views): the integers
// 0 ... 255 are exact in fp16 and bf16, the 1 / 255 is applied in the fp32 epilogue.  One K step = one tap over one chunk: the A
// operand of lane l is the 8 channels 8 (l >> 4) ... of its pixel shifted by the tap, the B operand comes from the packed fragments.
// Wave w owns four 16-row MFMA tiles.  With the fused pool a tile is 2 rows x 8 columns ordered so that rows 4 g ... 4 g + 3 are the
// window of one pooled pixel -- the four accumulator registers of lane group g (C/D map: col = lane & 15, row = 4 (lane >> 4) + reg)
// --, so the pool is a maximum in registers and the pre-pool tensor is never written.  Otherwise a tile is 16 pixels of one row.
// Epilogues run in fp32 and round once: relu(acc [/ 255] + b), or scale relu(acc + b) + shift [+ skip].
//
// Small deep layers (x4 is 8 x 16 and x5 4 x 8 at 128 x 256) fill a fraction of an 8 x 32 tile; an M tile is NOT run over several planes
// there: their time is set by the serial K loop of few workgroups, not by the empty tile slots (tools/semseg_probe.py).
#include "sd_planar_mma.h"
#include "sd_netrt.h"
#include "sd_fcn.h"

#include <algorithm>

using namespace sdfcn;

namespace {

struct MmaArgs {
    const void* in;          // first layer: uint8 views; else T[planes][H][W][cin_p]
    void* out;               // T[planes][Ho][Wo][cout_p]
    const void* skip;        // transposed convolution: T[planes][Ho][Wo][cout_p] or null
    const void* wfrag;
    const float* bias;
    const float* scale;
    const float* shift;
    int32_t* flags;
    int H, W, Ho, Wo;        // input and stored output extents
    int cin, cin_p, cout_p;
    int n_chunks, n_taps, NTtot, groups;
    int tiles_x, tiles_y;
    int org;                 // plane coordinate of LDS tile row / column 0 relative to the tile origin: -1 convolution, 0 transposed
    int py, px;              // transposed convolution: output parity
    int tap_off[9];          // element offset of every tap inside the LDS tile
    long long plane0;        // first layer: the first plane of this launch set in the views tensor
    int nb_views;
    float in_scale;
};

// The LDS-staged implicit GEMM of one workgroup: acc[i][nt] += sum over chunks and taps.  pix[i]: the lane's A row of its i-th tile.
template <typename T, int NT, bool FIRST>
__device__ __forceinline__ void fcn_mma(const MmaArgs& a, T* tile, long long plane, int y0, int x0, int grp, const int (&pix)[4], f32x4 (&acc)[4][NT]) {
    using V8 = typename Act<T>::v8;
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[i][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < a.n_chunks; ++ch) {
        __syncthreads();      // the previous chunk's reads are done
        if constexpr (FIRST) {
            const U8Plane<T> u8(a.in, a.plane0 + plane, a.nb_views, a.cin, a.H, a.W);
            for (int p = tid; p < HALO_H * HALO_W; p += 256) {
                const int ly = p / HALO_W, lx = p - ly * HALO_W, gy = y0 + a.org + ly, gx = x0 + a.org + lx;
                const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
                V8 val;
#pragma unroll
                for (int c = 0; c < 8; ++c) val[c] = c < 4 ? u8.at(c, gy, gx, in) : (T)0.f;
                *reinterpret_cast<V8*>(tile + p * CKP) = val;
#pragma unroll
                for (int vv = 1; vv < 4; ++vv) *reinterpret_cast<uint4*>(tile + p * CKP + vv * 8) = uint4{0u, 0u, 0u, 0u};
            }
        } else {
            const T* base = reinterpret_cast<const T*>(a.in) + (size_t)plane * a.H * a.W * a.cin_p;
            for (int i = tid; i < HALO_H * HALO_W * 4; i += 256) {
                const int p = i >> 2, vv = i & 3, ly = p / HALO_W, lx = p - ly * HALO_W, gy = y0 + a.org + ly, gx = x0 + a.org + lx;
                const int c = ch * CK + vv * 8;
                uint4 val = {0u, 0u, 0u, 0u};
                if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && c < a.cin_p)
                    val = *reinterpret_cast<const uint4*>(base + ((size_t)gy * a.W + gx) * a.cin_p + c);
                *reinterpret_cast<uint4*>(tile + p * CKP + vv * 8) = val;
            }
        }
        __syncthreads();
        for (int t = 0; t < a.n_taps; ++t) {
            const V8* wf = reinterpret_cast<const V8*>(a.wfrag) + (((size_t)ch * a.n_taps + t) * a.NTtot + (size_t)grp * NT) * 64 + lane;
            V8 b[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = wf[nt * 64];
            const int off = a.tap_off[t] + 8 * g;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const V8 af = *reinterpret_cast<const V8*>(tile + pix[i] + off);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[i][nt] = mma16(af, b[nt], acc[i][nt]);
            }
        }
    }
}

__device__ __forceinline__ void block_coords(const MmaArgs& a, long long& plane, int& y0, int& x0, int& grp) {
    const long long t = (long long)blockIdx.x / a.groups;
    grp = (int)((long long)blockIdx.x - t * a.groups);
    const int tiles_pp = a.tiles_x * a.tiles_y;
    plane = t / tiles_pp;
    const int tt = (int)(t - plane * tiles_pp);
    y0 = (tt / a.tiles_x) * TILE_H, x0 = (tt % a.tiles_x) * TILE_W;
}

// 3 x 3 same-padded convolution + bias + ReLU (+ 2 x 2 max-pool)
template <typename T, int NT, bool FIRST, bool POOL>
__global__ __launch_bounds__(256) void k_fcn_conv(const MmaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fcn_smem[];
    T* tile = reinterpret_cast<T*>(fcn_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long plane;
    int y0, x0, grp;
    block_coords(a, plane, y0, x0, grp);
    int pix[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int cy, cx;
        lane_pos(wave, i, lane & 15, POOL, cy, cx);
        pix[i] = (cy * HALO_W + cx) * CKP;
    }
    f32x4 acc[4][NT];
    fcn_mma<T, NT, FIRST>(a, tile, plane, y0, x0, grp, pix, acc);
    T* out = reinterpret_cast<T*>(a.out) + (size_t)plane * a.Ho * a.Wo * a.cout_p;
    bool ovf = false;
    auto finish = [&](float v, int n, int py, int px) {
        v = FIRST ? fmaf(v, a.in_scale, a.bias[n]) : v + a.bias[n];
        v = fmaxf(v, 0.f);
        ovf |= stores_inf<T>(v);
        out[((size_t)py * a.Wo + px) * a.cout_p + n] = (T)v;
    };
    const int m = lane & 15, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int mt = wave * 4 + i;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = 16 * (grp * NT + nt) + m;
            if (n >= a.cout_p) continue;
            const f32x4 c = acc[i][nt];
            if (POOL) {
                const int py = (y0 >> 1) + (mt >> 2), px = (x0 >> 1) + 4 * (mt & 3) + g;
                if (py < a.Ho && px < a.Wo) finish(fmaxf(fmaxf(c[0], c[1]), fmaxf(c[2], c[3])), n, py, px);
            } else {
                const int py = y0 + (mt >> 1);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int px = x0 + 16 * (mt & 1) + 4 * g + r;
                    if (py < a.Ho && px < a.Wo) finish(c[r], n, py, px);
                }
            }
        }
    }
    if (ovf) a.flags[0] = 1;     // (every writer stores the same value: the race between blocks is harmless)
}

// One output parity of ConvTranspose2d(k = 3, stride = 2, padding = 1, output_padding = 1) + bias + ReLU + BatchNorm (+ skip)
template <typename T, int NT>
__global__ __launch_bounds__(256) void k_fcn_deconv(const MmaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fcn_smem[];
    T* tile = reinterpret_cast<T*>(fcn_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, g = lane >> 4;
    long long plane;
    int y0, x0, grp;
    block_coords(a, plane, y0, x0, grp);
    int pix[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int cy, cx;
        lane_pos(wave, i, m, false, cy, cx);
        pix[i] = (cy * HALO_W + cx) * CKP;
    }
    f32x4 acc[4][NT];
    fcn_mma<T, NT, false>(a, tile, plane, y0, x0, grp, pix, acc);
    const size_t pbase = (size_t)plane * a.Ho * a.Wo * a.cout_p;
    T* out = reinterpret_cast<T*>(a.out) + pbase;
    const T* skip = a.skip ? reinterpret_cast<const T*>(a.skip) + pbase : nullptr;
    bool ovf = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int mt = wave * 4 + i, iy = y0 + (mt >> 1);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = 16 * (grp * NT + nt) + m;
            if (n >= a.cout_p || iy >= a.H) continue;
            const float b = a.bias[n], sc = a.scale[n], sh = a.shift[n];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ix = x0 + 16 * (mt & 1) + 4 * g + r;
                if (ix >= a.W) continue;
                const size_t o = ((size_t)(2 * iy + a.py) * a.Wo + (2 * ix + a.px)) * a.cout_p + n;
                float v = fmaf(sc, fmaxf(acc[i][nt][r] + b, 0.f), sh);
                if (skip) v += (float)skip[o];
                ovf |= stores_inf<T>(v);
                out[o] = (T)v;
            }
        }
    }
    if (ovf) a.flags[0] = 1;
}

struct ClsArgs {
    const void* in;          // T[n_px][cp]
    const float* w;          // [n_class][cin]
    const float* b;
    float* logits;           // [planes][n_class][HW] or null
    uint8_t* labels;         // [planes][HW]
    long long n_px;
    int HW, cin, cp, n_class;
};

// 1 x 1 convolution in fp32 + argmax; one thread per pixel, every logit one FMA chain over the channels in order
template <typename T>
__global__ __launch_bounds__(256) void k_fcn_classify(const ClsArgs a) {
    using V8 = typename Act<T>::v8;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n_px) return;
    const T* x = reinterpret_cast<const T*>(a.in) + (size_t)idx * a.cp;
    float s[MAX_CLASS];
#pragma unroll
    for (int k = 0; k < MAX_CLASS; ++k) s[k] = k < a.n_class ? a.b[k] : 0.f;
    for (int c0 = 0; c0 < a.cin; c0 += 8) {
        const V8 xv = *reinterpret_cast<const V8*>(x + c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (c0 + j >= a.cin) break;
            const float xf = (float)xv[j];
#pragma unroll
            for (int k = 0; k < MAX_CLASS; ++k)
                if (k < a.n_class) s[k] = fmaf(a.w[k * a.cin + c0 + j], xf, s[k]);
        }
    }
    int best = 0;
    float top = s[0];
#pragma unroll
    for (int k = 1; k < MAX_CLASS; ++k)
        if (k < a.n_class && s[k] > top) top = s[k], best = k;      // strict: the lowest index wins a tie
    a.labels[idx] = (uint8_t)best;
    if (a.logits) {
        const long long plane = idx / a.HW, r = idx - plane * a.HW;
#pragma unroll
        for (int k = 0; k < MAX_CLASS; ++k)
            if (k < a.n_class) a.logits[((size_t)plane * a.n_class + k) * a.HW + r] = s[k];
    }
}

template <typename T, int NT>
void launch_conv_nt(bool first, bool pool, unsigned grid, hipStream_t s, const MmaArgs& a) {
    if (first && pool) hipLaunchKernelGGL((k_fcn_conv<T, NT, true, true>), dim3(grid), dim3(256), LDS_BYTES, s, a);
    else if (first) hipLaunchKernelGGL((k_fcn_conv<T, NT, true, false>), dim3(grid), dim3(256), LDS_BYTES, s, a);
    else if (pool) hipLaunchKernelGGL((k_fcn_conv<T, NT, false, true>), dim3(grid), dim3(256), LDS_BYTES, s, a);
    else hipLaunchKernelGGL((k_fcn_conv<T, NT, false, false>), dim3(grid), dim3(256), LDS_BYTES, s, a);
}
template <typename T>
void launch_mma(const Op& op, unsigned grid, hipStream_t s, const MmaArgs& a) {
    if (op.kind == OP_DECONV) {
        switch (op.NT) {
        case 1: hipLaunchKernelGGL((k_fcn_deconv<T, 1>), dim3(grid), dim3(256), LDS_BYTES, s, a); break;
        case 2: hipLaunchKernelGGL((k_fcn_deconv<T, 2>), dim3(grid), dim3(256), LDS_BYTES, s, a); break;
        case 3: hipLaunchKernelGGL((k_fcn_deconv<T, 3>), dim3(grid), dim3(256), LDS_BYTES, s, a); break;
        default: hipLaunchKernelGGL((k_fcn_deconv<T, 4>), dim3(grid), dim3(256), LDS_BYTES, s, a); break;
        }
        return;
    }
    switch (op.NT) {
    case 1: launch_conv_nt<T, 1>(op.first, op.pool, grid, s, a); break;
    case 2: launch_conv_nt<T, 2>(op.first, op.pool, grid, s, a); break;
    case 3: launch_conv_nt<T, 3>(op.first, op.pool, grid, s, a); break;
    default: launch_conv_nt<T, 4>(op.first, op.pool, grid, s, a); break;
    }
}

}  // namespace

struct sd_fcn : Net<Plan> {};

extern "C" {

int sd_fcn_create(int in_channels, const int32_t* blocks, const int32_t* block_len, int dec_last, int n_class, const float* weights, size_t n_floats,
                  int act_dtype, sd_fcn** out) {
    return create_net(out, "sd_fcn_create", [&](Plan& plan, std::string& err) {
        return build_plan(in_channels, blocks, block_len, dec_last, n_class, weights, n_floats, act_dtype, plan, err);
    });
}

void sd_fcn_destroy(sd_fcn* m) { delete m; }

size_t sd_fcn_workspace_bytes(sd_fcn* m, size_t n_planes, int H, int W) {
    if (!m) return 0;
    Workspace ws;
    std::string err;
    if (workspace(m->plan, n_planes, H, W, ws, err) != SD_OK) {
        fail(err);
        return 0;
    }
    return ws.total;
}

int sd_fcn_num_ops(sd_fcn* m) { return m ? (int)m->plan.ops.size() : 0; }

// ev (or null): n_ops + 1 events, recorded in front of the first launch and behind the launches of every op
static int fcn_forward(sd_fcn* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W, size_t plane0, size_t n_planes,
                       uint8_t* labels_dev, float* logits_dev, void* workspace_dev, size_t ws_bytes, int32_t* flags_dev, void* stream, hipEvent_t* ev) {
    if (!m || !views_dev || !labels_dev || !workspace_dev || !flags_dev) return fail("sd_fcn_forward: null argument");
    const Plan& p = m->plan;
    if (nb_views < 1 || n_planes_total < 1 || n_planes_total % (size_t)nb_views != 0 || n_planes_total > ((size_t)1 << 31) - 1)
        return fail("sd_fcn_forward: n_planes_total must be a multiple of nb_views below 2^31");
    Workspace ws;
    std::vector<Dims> dims;
    std::string err;
    if (workspace(p, n_planes, H, W, ws, err) != SD_OK || infer_shapes(p, H, W, dims, err) != SD_OK) return fail(err);
    if (plane0 >= n_planes_total || n_planes > n_planes_total - plane0) return fail("sd_fcn_forward: planes [plane0, plane0 + n_planes) are outside the views");
    if (ws_bytes < ws.total) return fail("sd_fcn_forward: workspace smaller than sd_fcn_workspace_bytes(m, n_planes, H, W)");
    if ((reinterpret_cast<uintptr_t>(workspace_dev) & 15) != 0) return fail("sd_fcn_forward: workspace must be 16-byte aligned");
    // every launch's block count, before anything is launched
    for (const Op& op : p.ops) {
        const long long h = H >> op.in_shift, w = W >> op.in_shift;
        const long long blocks = op.kind == OP_CLASSIFY ? ((long long)n_planes * H * W + 255) / 256
                                                        : (long long)n_planes * ((h + TILE_H - 1) / TILE_H) * ((w + TILE_W - 1) / TILE_W) * op.groups;
        if (blocks > 0x7fffffffLL) return fail("sd_fcn_forward: too many planes for one launch (use fewer planes per call)");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(flags_dev, 0, sizeof(int32_t), s) != hipSuccess) return fail("sd_fcn_forward: memset failed", SD_ERR_HIP);
    if (ev) (void)hipEventRecord(ev[0], s);
    char* wsb = reinterpret_cast<char*>(workspace_dev);
    for (size_t i = 0; i < p.ops.size(); ++i) {
        const Op& op = p.ops[i];
        const void* in = op.in_buf < 0 ? (const void*)views_dev : (const void*)(wsb + ws.off[op.in_buf]);
        const int h = H >> op.in_shift, w = W >> op.in_shift;
        if (op.kind == OP_CLASSIFY) {
            ClsArgs c{};
            c.in = in, c.w = reinterpret_cast<const float*>(m->dev_blob + op.bias_off), c.b = reinterpret_cast<const float*>(m->dev_blob + op.scale_off);
            c.logits = logits_dev, c.labels = labels_dev;
            c.HW = H * W, c.n_px = (long long)n_planes * c.HW, c.cin = op.cin, c.cp = rup(op.cin, 8), c.n_class = op.cout;
            const unsigned grid = (unsigned)((c.n_px + 255) / 256);
            if (p.act_dtype == SD_F16) hipLaunchKernelGGL(k_fcn_classify<f16_t>, dim3(grid), dim3(256), 0, s, c);
            else hipLaunchKernelGGL(k_fcn_classify<bf16_t>, dim3(grid), dim3(256), 0, s, c);
        } else {
            MmaArgs a{};
            a.in = in, a.out = wsb + ws.off[op.out_buf], a.skip = op.skip_buf >= 0 ? wsb + ws.off[op.skip_buf] : nullptr;
            a.bias = reinterpret_cast<const float*>(m->dev_blob + op.bias_off);
            a.scale = reinterpret_cast<const float*>(m->dev_blob + op.scale_off);
            a.shift = reinterpret_cast<const float*>(m->dev_blob + op.shift_off);
            a.flags = flags_dev;
            a.H = h, a.W = w, a.Ho = dims[i].h, a.Wo = dims[i].w;
            a.cin = op.cin, a.cin_p = op.cin_p, a.cout_p = op.cout_p;
            a.n_chunks = op.n_chunks, a.NTtot = op.NT * op.groups, a.groups = op.groups;
            a.tiles_y = (h + TILE_H - 1) / TILE_H, a.tiles_x = (w + TILE_W - 1) / TILE_W;
            a.org = op.kind == OP_CONV ? -1 : 0;
            a.plane0 = (long long)plane0, a.nb_views = nb_views, a.in_scale = 1.f / 255.f;
            const unsigned grid = (unsigned)((long long)n_planes * a.tiles_x * a.tiles_y * op.groups);
            const int n_par = op.kind == OP_DECONV ? 4 : 1;
            for (int par = 0; par < n_par; ++par) {
                Tap taps[9];
                a.n_taps = taps_of(op.kind, par, taps);
                for (int t = 0; t < a.n_taps; ++t) a.tap_off[t] = (taps[t].dy * HALO_W + taps[t].dx) * CKP;
                a.py = par >> 1, a.px = par & 1;
                a.wfrag = m->dev_blob + op.wfrag_off[par];
                if (p.act_dtype == SD_F16) launch_mma<f16_t>(op, grid, s, a);
                else launch_mma<bf16_t>(op, grid, s, a);
            }
        }
        if (ev) (void)hipEventRecord(ev[i + 1], s);
    }
    return hipGetLastError() == hipSuccess ? SD_OK : fail("sd_fcn_forward: launch failed", SD_ERR_HIP);
}

int sd_fcn_forward(sd_fcn* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W, size_t plane0, size_t n_planes,
                   uint8_t* labels_dev, float* logits_dev, void* workspace_dev, size_t ws_bytes, int32_t* flags_dev, void* stream) {
    return fcn_forward(m, views_dev, n_planes_total, nb_views, H, W, plane0, n_planes, labels_dev, logits_dev, workspace_dev, ws_bytes, flags_dev, stream,
                       nullptr);
}

int sd_fcn_forward_timed(sd_fcn* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W, size_t plane0, size_t n_planes,
                         uint8_t* labels_dev, float* logits_dev, void* workspace_dev, size_t ws_bytes, int32_t* flags_dev, void* stream, float* ms_out) {
    if (!m || !ms_out) return fail("sd_fcn_forward_timed: null argument");
    return timed(m->plan.ops.size() + 1, stream, ms_out, "sd_fcn_forward_timed", [&](hipEvent_t* ev) {
        return fcn_forward(m, views_dev, n_planes_total, nb_views, H, W, plane0, n_planes, labels_dev, logits_dev, workspace_dev, ws_bytes, flags_dev, stream,
                           ev);
    });
}

int sd_fcn_overflow(sd_fcn* m, const int32_t* flags_dev, void* stream, int32_t* flags_out) {
    return read_flags(m, flags_dev, 1, stream, flags_out, "sd_fcn_overflow");
}

int sd_fcn_read_buffer(sd_fcn* m, int index, const void* workspace_dev, const float* logits_dev, size_t n_planes, int H, int W, float* out_host,
                       int32_t* dims_out, void* stream) {
    if (!m || !workspace_dev || !dims_out) return fail("sd_fcn_read_buffer: null argument");
    const Plan& p = m->plan;
    const int n_ops = (int)p.ops.size();
    if (index < 0 || index >= n_ops) return fail("sd_fcn_read_buffer: index out of range");
    Workspace ws;
    std::vector<Dims> dims;
    std::string err;
    if (workspace(p, n_planes, H, W, ws, err) != SD_OK || infer_shapes(p, H, W, dims, err) != SD_OK) return fail(err);
    const Dims& d = dims[index];
    if (index == n_ops - 1) {
        dims_out[0] = (int32_t)n_planes, dims_out[1] = d.c, dims_out[2] = d.h, dims_out[3] = d.w;
        if (!out_host) return SD_OK;
        if (!logits_dev) return fail("sd_fcn_read_buffer: the logits were not kept (logits_dev is null)");
        return copy_out(out_host, logits_dev, n_planes * d.c * d.h * d.w * sizeof(float), stream, "sd_fcn_read_buffer");
    }
    dims_out[0] = (int32_t)n_planes, dims_out[1] = d.h, dims_out[2] = d.w, dims_out[3] = d.c;
    if (!out_host) return SD_OK;
    return read_stored(reinterpret_cast<const char*>(workspace_dev) + ws.off[index], n_planes * d.h * d.w, d.c, d.cp, p.act_dtype, out_host, stream,
                       "sd_fcn_read_buffer");
}

}  // extern "C"
