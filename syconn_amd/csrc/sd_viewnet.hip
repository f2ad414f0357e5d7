// The multi-view network of the cell type step on gfx950: one kernel per planar layer (valid k x k convolution + bias + (1, p, p)
// floor max-pool + activation + rounding + store, an implicit GEMM on v_mfma_f32_16x16x32), one kernel for the head (flatten, append
// the scalars, the Linear chain in fp32), and the C ABI around them.  The plan, the packed layouts and the lane maps: sd_viewnet.h.
//
// Layer kernel.  A workgroup of 4 waves computes 8 x 32 convolution outputs of one plane from a halo tile
// [8 + k - 1][32 + k - 1][cin_p] that it first brings into LDS: the first layer converts the renderer's planar uint8 planes (found
// through the sample table) to the storage type on the way -- the integers 0 ... 255 are exact in fp16 and bf16 --, the other layers
// copy 16 bytes per thread.  Positions beyond the plane are zero; they only feed outputs that are never stored.  Wave w owns output
// rows 2 w, 2 w + 1.  With a 2 x 2 pool a 16-row MFMA tile is 2 rows x 8 columns ordered so that rows 4 g ... 4 g + 3 are the window of
// one pooled pixel -- the accumulator rows of lane group g (C/D map: col = lane & 15, row = 4 (lane >> 4) + reg) --, so the pool is the
// maximum of a lane's four registers and rows / columns that the floor pool drops are never part of a stored window.  Without a pool
// a tile is 16 pixels of one row.  The epilogue runs in fp32: max, + bias (first layer: acc / 255 + (b - 0.5 sum w), a rising map,
// so it commutes with the maximum), activation, range guard, round to nearest even, 2-byte store (16 lanes = 32 contiguous bytes).
#include "sd_planar_mma.h"
#include "sd_netrt.h"
#include "sd_viewnet.h"

#include <algorithm>

using namespace sdvn;

namespace {

struct ConvArgs {
    const void* in;          // first layer: uint8 views; else T[planes][H][W][cin_p]
    const int32_t* table;    // first layer: source plane of every output plane
    void* out;               // T[planes][Ho][Wo][cout_p]
    const void* wfrag;
    const int32_t* aoff;
    const float* bias;
    int32_t* flags;
    int H, W, Ho, Wo;
    int k, pool, cin, cin_p, cout_p, nks;
    int tiles_x, tiles_y;
    long long n_tiles;
    long long n_planes_src;  // first layer: n_loc * nb_views
    int nb_views;
    float scale, slope;
};

template <typename T, int NT, bool FIRST>
__global__ __launch_bounds__(256) void k_vn_conv(const ConvArgs a) {
    using V8 = typename Act<T>::v8;
    using V4 = typename Act<T>::v4;
    extern __shared__ __attribute__((aligned(16))) unsigned char vn_smem[];
    T* tile = reinterpret_cast<T*>(vn_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int thin = TILE_H + a.k - 1, twin = TILE_W + a.k - 1;
    const int tiles_pp = a.tiles_x * a.tiles_y;
    const int m = lane & 15, g = lane >> 4;
    // this lane's A rows: the output pixel (inside the tile) of row m of each of the wave's four MFMA row tiles
    int pix[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int cy, cx;
        lane_pos(wave, i, m, a.pool == 2, cy, cx);
        pix[i] = (cy * twin + cx) * a.cin_p;
    }
    for (long long t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const long long plane = t / tiles_pp;
        const int tt = (int)(t - plane * tiles_pp);
        const int y0 = (tt / a.tiles_x) * TILE_H, x0 = (tt % a.tiles_x) * TILE_W;
        __syncthreads();      // the previous tile's reads are done
        if constexpr (FIRST) {
            const long long src = a.table[plane];
            if (src < 0 || src >= a.n_planes_src) {      // the same for all threads of the block: nothing is read
                if (tid == 0) a.flags[1] = 1;      // (every writer stores the same value: the race between blocks is harmless)
                continue;
            }
            const U8Plane<T> u8(a.in, src, a.nb_views, a.cin, a.H, a.W);
            for (int i = tid; i < thin * twin; i += 256) {
                const int iy = i / twin, ix = i - iy * twin, gy = y0 + iy, gx = x0 + ix;
                V4 val;
#pragma unroll
                for (int c = 0; c < 4; ++c) val[c] = u8.at(c, gy, gx, gy < a.H && gx < a.W);
                *reinterpret_cast<V4*>(tile + i * 4) = val;
            }
        } else {
            const T* base = reinterpret_cast<const T*>(a.in) + (size_t)plane * a.H * a.W * a.cin_p;
            const int vpp = a.cin_p >> 3, n = thin * twin * vpp;
            for (int i = tid; i < n; i += 256) {
                const int p = i / vpp, vv = i - p * vpp, iy = p / twin, ix = p - iy * twin, gy = y0 + iy, gx = x0 + ix;
                uint4 val = {0u, 0u, 0u, 0u};
                if (gy < a.H && gx < a.W) val = *reinterpret_cast<const uint4*>(base + ((size_t)gy * a.W + gx) * a.cin_p + vv * 8);
                *reinterpret_cast<uint4*>(tile + p * a.cin_p + vv * 8) = val;
            }
        }
        __syncthreads();
        f32x4 acc[4][NT];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[i][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < a.nks; ++ks) {
            const int2 off = reinterpret_cast<const int2*>(a.aoff)[ks * 4 + g];
            V8 b[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = reinterpret_cast<const V8*>(a.wfrag)[((size_t)ks * NT + nt) * 64 + lane];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                V8 af;
                if constexpr (FIRST) {
                    const V4 lo = *reinterpret_cast<const V4*>(tile + pix[i] + off.x), hi = *reinterpret_cast<const V4*>(tile + pix[i] + off.y);
                    af = V8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                } else {
                    af = *reinterpret_cast<const V8*>(tile + pix[i] + off.x);
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[i][nt] = mma16(af, b[nt], acc[i][nt]);
            }
        }
        // epilogue
        T* out = reinterpret_cast<T*>(a.out) + (size_t)plane * a.Ho * a.Wo * a.cout_p;
        bool ovf = false;
        auto finish = [&](float v, int n, int py, int px) {
            v = FIRST ? fmaf(v, a.scale, a.bias[n]) : v + a.bias[n];
            v = v < 0.f ? fmaf(v, a.slope, 0.f) : v;      // (a NaN stays a NaN; slope 0 gives +0)
            ovf |= stores_inf<T>(v);
            if (py < a.Ho && px < a.Wo) out[((size_t)py * a.Wo + px) * a.cout_p + n] = (T)v;
        };
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mt = wave * 4 + i;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int n = 16 * nt + m;
                if (n >= a.cout_p) continue;
                const f32x4 c = acc[i][nt];
                if (a.pool == 2) {
                    const int py = (y0 >> 1) + (mt >> 2), px = (x0 >> 1) + 4 * (mt & 3) + g;
                    // windows beyond the stored output hold zeros or partial sums: computed, never stored, not range-checked
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
        if (ovf) a.flags[0] = 1;
    }
}

struct HeadArgs {
    const void* feat;        // T[n_samples][S][cp]
    const float* scal;       // [n_samples][n_scalar]
    const float* w[MAX_FC];
    const float* b[MAX_FC];
    float* h[MAX_FC];        // [n_samples][nout]; the last one is the logits
    int nin[MAX_FC], nout[MAX_FC];
    int n_fc, n_scalar, C, cp, S, maxlen;
    long long n_samples;
    float slope;
};

// One block per sample.  x = [features in the order c S + s of x.view(N, -1) | scalars]; every output of a Linear is one wave's
// strided fp32 FMA chain over the inputs and a butterfly sum of the 64 partial sums.
template <typename T>
__global__ __launch_bounds__(256) void k_vn_head(const HeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vn_smem[];
    float* x = reinterpret_cast<float*>(vn_smem);
    float* y = x + a.maxlen;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int flat = a.C * a.S;
    for (long long s = blockIdx.x; s < a.n_samples; s += gridDim.x) {
        __syncthreads();
        const T* f = reinterpret_cast<const T*>(a.feat) + (size_t)s * a.S * a.cp;
        for (int i = tid; i < flat; i += 256) {
            const int c = i / a.S, sp = i - c * a.S;
            x[i] = (float)f[(size_t)sp * a.cp + c];
        }
        for (int i = tid; i < a.n_scalar; i += 256) x[flat + i] = a.scal[(size_t)s * a.n_scalar + i];
        __syncthreads();
        float* xin = x;
        float* xout = y;
        for (int l = 0; l < a.n_fc; ++l) {
            const int nin = a.nin[l], nout = a.nout[l];
            for (int j = wave; j < nout; j += 4) {
                const float* w = a.w[l] + (size_t)j * nin;
                float sum = 0.f;
                for (int i = lane; i < nin; i += 64) sum = fmaf(w[i], xin[i], sum);
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
                if (lane == 0) {
                    float v = sum + a.b[l][j];
                    if (l + 1 < a.n_fc) v = v < 0.f ? fmaf(v, a.slope, 0.f) : v;
                    xout[j] = v;
                    a.h[l][(size_t)s * nout + j] = v;
                }
            }
            __syncthreads();
            float* tmp = xin;
            xin = xout, xout = tmp;
        }
    }
}

// TS consecutive samples per block (the embedding call: one sample per rendering location, thousands of them, each a single plane of
// convolution work).  x = [TS][nin of the first Linear] in LDS, filled once per tile in k_vn_head's order; every output row j of a
// Linear belongs to one wave, whose lanes load w[j][i] once for i = lane, lane + 64, ... and feed TS accumulators from it -- per sample
// the FMA chain, the butterfly, the bias add and the activation of k_vn_head, in its order, so every sample has k_vn_head's bits; only
// the weight traffic differs (once per tile, not once per sample).  Lanes of a wave read consecutive floats of one LDS row: no bank
// conflict.  After the butterfly every lane holds every sum, so lane t stores sample t.  A partial last tile stages, accumulates and
// stores its real samples only.  The hidden tiles are [TS][hmax], hmax = the widest Linear output.
template <typename T, int TS>
__global__ __launch_bounds__(HEAD_TILE_THREADS) void k_vn_head_tile(const HeadArgs a, const int hmax) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vn_smem[];
    float* x = reinterpret_cast<float*>(vn_smem);
    float* y0 = x + (size_t)TS * a.nin[0];
    float* y1 = y0 + (size_t)TS * hmax;
    constexpr int NW = HEAD_TILE_THREADS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int flat = a.C * a.S, nin0 = a.nin[0];
    const long long n_tiles = (a.n_samples + TS - 1) / TS;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long s0 = tile * TS;
        const int nt = (int)(a.n_samples - s0 < TS ? a.n_samples - s0 : TS);      // real samples of this tile
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            const T* f = reinterpret_cast<const T*>(a.feat) + (size_t)(s0 + t) * a.S * a.cp;
            float* xt = x + (size_t)t * nin0;
            for (int i = tid; i < flat; i += HEAD_TILE_THREADS) {
                const int c = i / a.S, sp = i - c * a.S;
                xt[i] = (float)f[(size_t)sp * a.cp + c];
            }
            for (int i = tid; i < a.n_scalar; i += HEAD_TILE_THREADS) xt[flat + i] = a.scal[(size_t)(s0 + t) * a.n_scalar + i];
        }
        __syncthreads();
        const float* xin = x;
        int xs = nin0;
        float* xout = y0;
        for (int l = 0; l < a.n_fc; ++l) {
            const int nin = a.nin[l], nout = a.nout[l];
            for (int j = wave; j < nout; j += NW) {
                const float* w = a.w[l] + (size_t)j * nin;
                float sum[TS];
#pragma unroll
                for (int t = 0; t < TS; ++t) sum[t] = 0.f;
                if (nt == TS) {
                    for (int i = lane; i < nin; i += 64) {
                        const float wv = w[i];
#pragma unroll
                        for (int t = 0; t < TS; ++t) sum[t] = fmaf(wv, xin[t * xs + i], sum[t]);
                    }
                } else {
                    for (int i = lane; i < nin; i += 64) {
                        const float wv = w[i];
#pragma unroll
                        for (int t = 0; t < TS; ++t)
                            if (t < nt) sum[t] = fmaf(wv, xin[t * xs + i], sum[t]);      // rows t >= nt were never staged
                    }
                }
#pragma unroll
                for (int t = 0; t < TS; ++t)
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) sum[t] += __shfl_xor(sum[t], d);
                float mine = sum[0];
#pragma unroll
                for (int t = 1; t < TS; ++t) mine = lane == t ? sum[t] : mine;
                if (lane < nt) {
                    float v = mine + a.b[l][j];
                    if (l + 1 < a.n_fc) v = v < 0.f ? fmaf(v, a.slope, 0.f) : v;
                    xout[lane * hmax + j] = v;
                    a.h[l][(size_t)(s0 + lane) * nout + j] = v;
                }
            }
            __syncthreads();
            xin = xout, xs = hmax;
            xout = xout == y0 ? y1 : y0;
        }
    }
}

template <typename T, int TS>
hipError_t launch_head_tile(int grid, size_t lds, hipStream_t s, const HeadArgs& a, int hmax) {
    if (lds > 65536) {      // beyond the default limit of dynamic LDS: ask for it
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vn_head_tile<T, TS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_vn_head_tile<T, TS>), dim3(grid), dim3(HEAD_TILE_THREADS), lds, s, a, hmax);
    return hipSuccess;
}
template <typename T>
hipError_t launch_head_tile_ts(int TS, int grid, size_t lds, hipStream_t s, const HeadArgs& a, int hmax) {
    switch (TS) {
    case 8: return launch_head_tile<T, 8>(grid, lds, s, a, hmax);
    case 4: return launch_head_tile<T, 4>(grid, lds, s, a, hmax);
    case 2: return launch_head_tile<T, 2>(grid, lds, s, a, hmax);
    default: return launch_head_tile<T, 1>(grid, lds, s, a, hmax);
    }
}

template <typename T, bool FIRST>
void launch_conv_nt(int NT, int grid, size_t lds, hipStream_t s, const ConvArgs& a) {
    switch (NT) {
    case 1: hipLaunchKernelGGL((k_vn_conv<T, 1, FIRST>), dim3(grid), dim3(256), lds, s, a); break;
    case 2: hipLaunchKernelGGL((k_vn_conv<T, 2, FIRST>), dim3(grid), dim3(256), lds, s, a); break;
    case 3: hipLaunchKernelGGL((k_vn_conv<T, 3, FIRST>), dim3(grid), dim3(256), lds, s, a); break;
    case 4: hipLaunchKernelGGL((k_vn_conv<T, 4, FIRST>), dim3(grid), dim3(256), lds, s, a); break;
    default: hipLaunchKernelGGL((k_vn_conv<T, 5, FIRST>), dim3(grid), dim3(256), lds, s, a); break;
    }
}
template <typename T>
void launch_conv(bool first, int NT, int grid, size_t lds, hipStream_t s, const ConvArgs& a) {
    if (first) launch_conv_nt<T, true>(NT, grid, lds, s, a);
    else launch_conv_nt<T, false>(NT, grid, lds, s, a);
}

}  // namespace

struct sd_viewnet : Net<Plan> {};

extern "C" {

int sd_viewnet_create(const sd_viewnet_layer_desc* layers, int n_layers, const int32_t* fc, int n_fc, int in_channels, int n_scalar, int act,
                      const float* weights, size_t n_floats, int act_dtype, sd_viewnet** out) {
    return create_net(out, "sd_viewnet_create", [&](Plan& plan, std::string& err) {
        return build_plan(layers, n_layers, fc, n_fc, in_channels, n_scalar, act, weights, n_floats, act_dtype, plan, err);
    });
}

void sd_viewnet_destroy(sd_viewnet* m) { delete m; }

size_t sd_viewnet_workspace_bytes(sd_viewnet* m, size_t n_samples, int D, int H, int W) {
    if (!m) return 0;
    Workspace ws;
    std::string err;
    if (workspace(m->plan, n_samples, D, H, W, ws, err) != SD_OK) {
        fail(err);
        return 0;
    }
    return ws.total;
}

int sd_viewnet_num_ops(sd_viewnet* m) { return m ? (int)(m->plan.layers.size() + m->plan.fc.size()) : 0; }

// ev (or null): n_layers + 2 events, recorded in front of the first launch and behind every launch
static int vn_forward(sd_viewnet* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W, const int32_t* sample_table_dev,
                      size_t n_samples, int D, const float* scalars_dev, float* logits_dev, void* workspace_dev, size_t ws_bytes,
                      int32_t* flags_dev, void* stream, hipEvent_t* ev, bool tiled_head = false) {
    const std::string who = tiled_head ? "sd_viewnet_embed" : "sd_viewnet_forward";
    if (!m || !views_dev || !sample_table_dev || !logits_dev || !workspace_dev || !flags_dev) return fail(who + ": null argument");
    const Plan& p = m->plan;
    if (p.n_scalar > 0 && !scalars_dev) return fail(who + ": the model takes scalars, scalars_dev is null");
    if (nb_views < 1 || n_planes_total < 1 || n_planes_total % (size_t)nb_views != 0 || n_planes_total > ((size_t)1 << 31) - 1)
        return fail(who + ": n_planes_total must be a multiple of nb_views below 2^31");
    Workspace ws;
    std::vector<Dims> dims;
    std::string err;
    if (workspace(p, n_samples, D, H, W, ws, err) != SD_OK || infer_shapes(p, D, H, W, dims, err) != SD_OK) return fail(err);
    if (ws_bytes < ws.total) return fail(who + ": workspace smaller than sd_viewnet_workspace_bytes(m, n_samples, D, H, W)");
    if ((reinterpret_cast<uintptr_t>(workspace_dev) & 15) != 0) return fail(who + ": workspace must be 16-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(flags_dev, 0, 2 * sizeof(int32_t), s) != hipSuccess) return fail(who + ": memset failed", SD_ERR_HIP);
    if (ev) (void)hipEventRecord(ev[0], s);
    char* wsb = reinterpret_cast<char*>(workspace_dev);
    const long long planes = (long long)n_samples * D;
    const void* in = views_dev;
    int h = H, w = W;
    for (size_t i = 0; i < p.layers.size(); ++i) {
        const Layer& L = p.layers[i];
        ConvArgs a{};
        a.in = in, a.table = sample_table_dev, a.out = wsb + ws.layer_off[i];
        a.wfrag = m->dev_blob + L.wfrag_off;
        a.aoff = reinterpret_cast<const int32_t*>(m->dev_blob + L.aoff_off);
        a.bias = reinterpret_cast<const float*>(m->dev_blob + L.bias_off);
        a.flags = flags_dev;
        a.H = h, a.W = w, a.Ho = dims[i].h, a.Wo = dims[i].w;
        a.k = L.k, a.pool = L.pool, a.cin = L.cin, a.cin_p = L.cin_p, a.cout_p = L.cout_p, a.nks = L.nks;
        a.tiles_y = (dims[i].h * L.pool + TILE_H - 1) / TILE_H, a.tiles_x = (dims[i].w * L.pool + TILE_W - 1) / TILE_W;
        a.n_tiles = planes * a.tiles_x * a.tiles_y;
        a.n_planes_src = (long long)n_planes_total, a.nb_views = nb_views;
        a.scale = 1.f / 255.f;
        a.slope = p.act == ACT_LEAKY ? LEAKY_SLOPE : 0.f;
        const int grid = (int)std::min<long long>(a.n_tiles, SD_VIEWNET_GRID);
        if (p.act_dtype == SD_F16) launch_conv<f16_t>(i == 0, L.NT, grid, L.lds_bytes, s, a);
        else launch_conv<bf16_t>(i == 0, L.NT, grid, L.lds_bytes, s, a);
        if (ev) (void)hipEventRecord(ev[i + 1], s);
        in = a.out, h = dims[i].h, w = dims[i].w;
    }
    HeadArgs ha{};
    ha.feat = in, ha.scal = scalars_dev;
    ha.n_fc = (int)p.fc.size(), ha.n_scalar = p.n_scalar, ha.C = p.layers.back().cout, ha.cp = p.layers.back().cout_p, ha.S = D * h * w;
    ha.n_samples = (long long)n_samples;
    ha.slope = p.act == ACT_LEAKY ? LEAKY_SLOPE : 0.f;
    for (int j = 0; j < ha.n_fc; ++j) {
        ha.w[j] = reinterpret_cast<const float*>(m->dev_blob + p.fc[j].w_off);
        ha.b[j] = reinterpret_cast<const float*>(m->dev_blob + p.fc[j].b_off);
        ha.nin[j] = p.fc[j].nin, ha.nout[j] = p.fc[j].nout;
        ha.h[j] = j + 1 < ha.n_fc ? reinterpret_cast<float*>(wsb + ws.hidden_off[j]) : logits_dev;
        ha.maxlen = std::max(ha.maxlen, std::max(ha.nin[j], ha.nout[j]));
    }
    if (tiled_head) {
        const int TS = head_tile_samples(p), hmax = head_tile_hmax(p);
        const long long tiles = (ha.n_samples + TS - 1) / TS;
        const int hgrid = (int)std::min<long long>(tiles, SD_VIEWNET_HEAD_TILE_GRID);
        const size_t hlds = head_tile_lds(p, TS);
        const hipError_t e = p.act_dtype == SD_F16 ? launch_head_tile_ts<f16_t>(TS, hgrid, hlds, s, ha, hmax) : launch_head_tile_ts<bf16_t>(TS, hgrid, hlds, s, ha, hmax);
        if (e != hipSuccess) return fail(who + ": the head's LDS request was refused", SD_ERR_HIP);
    } else {
        const int hgrid = (int)std::min<long long>(ha.n_samples, SD_VIEWNET_HEAD_GRID);
        const size_t hlds = 2 * sizeof(float) * (size_t)ha.maxlen;
        if (p.act_dtype == SD_F16) hipLaunchKernelGGL(k_vn_head<f16_t>, dim3(hgrid), dim3(256), hlds, s, ha);
        else hipLaunchKernelGGL(k_vn_head<bf16_t>, dim3(hgrid), dim3(256), hlds, s, ha);
    }
    if (ev) (void)hipEventRecord(ev[p.layers.size() + 1], s);
    return hipGetLastError() == hipSuccess ? SD_OK : fail(who + ": launch failed", SD_ERR_HIP);
}

int sd_viewnet_forward(sd_viewnet* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W, const int32_t* sample_table_dev,
                       size_t n_samples, int D, const float* scalars_dev, float* logits_dev, void* workspace_dev, size_t ws_bytes,
                       int32_t* flags_dev, void* stream) {
    return vn_forward(m, views_dev, n_planes_total, nb_views, H, W, sample_table_dev, n_samples, D, scalars_dev, logits_dev, workspace_dev, ws_bytes,
                      flags_dev, stream, nullptr);
}

static int vn_forward_timed(sd_viewnet* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W,
                            const int32_t* sample_table_dev, size_t n_samples, int D, const float* scalars_dev, float* logits_dev,
                            void* workspace_dev, size_t ws_bytes, int32_t* flags_dev, void* stream, float* ms_out, bool tiled_head) {
    const std::string who = tiled_head ? "sd_viewnet_embed_timed" : "sd_viewnet_forward_timed";
    if (!m || !ms_out) return fail(who + ": null argument");
    return timed(m->plan.layers.size() + 2, stream, ms_out, who, [&](hipEvent_t* ev) {
        return vn_forward(m, views_dev, n_planes_total, nb_views, H, W, sample_table_dev, n_samples, D, scalars_dev, logits_dev, workspace_dev, ws_bytes,
                          flags_dev, stream, ev, tiled_head);
    });
}

int sd_viewnet_forward_timed(sd_viewnet* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W,
                             const int32_t* sample_table_dev, size_t n_samples, int D, const float* scalars_dev, float* logits_dev,
                             void* workspace_dev, size_t ws_bytes, int32_t* flags_dev, void* stream, float* ms_out) {
    return vn_forward_timed(m, views_dev, n_planes_total, nb_views, H, W, sample_table_dev, n_samples, D, scalars_dev, logits_dev, workspace_dev,
                            ws_bytes, flags_dev, stream, ms_out, false);
}

int sd_viewnet_embed(sd_viewnet* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W, const int32_t* sample_table_dev,
                     size_t n_samples, int D, const float* scalars_dev, float* logits_dev, void* workspace_dev, size_t ws_bytes,
                     int32_t* flags_dev, void* stream) {
    return vn_forward(m, views_dev, n_planes_total, nb_views, H, W, sample_table_dev, n_samples, D, scalars_dev, logits_dev, workspace_dev, ws_bytes,
                      flags_dev, stream, nullptr, true);
}

int sd_viewnet_embed_timed(sd_viewnet* m, const uint8_t* views_dev, size_t n_planes_total, int nb_views, int H, int W,
                           const int32_t* sample_table_dev, size_t n_samples, int D, const float* scalars_dev, float* logits_dev,
                           void* workspace_dev, size_t ws_bytes, int32_t* flags_dev, void* stream, float* ms_out) {
    return vn_forward_timed(m, views_dev, n_planes_total, nb_views, H, W, sample_table_dev, n_samples, D, scalars_dev, logits_dev, workspace_dev,
                            ws_bytes, flags_dev, stream, ms_out, true);
}

int sd_viewnet_embed_tile_samples(sd_viewnet* m) { return m ? head_tile_samples(m->plan) : 0; }

int sd_viewnet_overflow(sd_viewnet* m, const int32_t* flags_dev, void* stream, int32_t* flags_out) {
    return read_flags(m, flags_dev, 2, stream, flags_out, "sd_viewnet_overflow");
}

int sd_viewnet_read_buffer(sd_viewnet* m, int index, const void* workspace_dev, const float* logits_dev, size_t n_samples, int D, int H, int W,
                           float* out_host, int32_t* dims_out, void* stream) {
    if (!m || !workspace_dev || !logits_dev || !dims_out) return fail("sd_viewnet_read_buffer: null argument");
    const Plan& p = m->plan;
    const int nl = (int)p.layers.size(), nf = (int)p.fc.size();
    if (index < 0 || index >= nl + nf) return fail("sd_viewnet_read_buffer: index out of range");
    Workspace ws;
    std::vector<Dims> dims;
    std::string err;
    if (workspace(p, n_samples, D, H, W, ws, err) != SD_OK || infer_shapes(p, D, H, W, dims, err) != SD_OK) return fail(err);
    const char* wsb = reinterpret_cast<const char*>(workspace_dev);
    if (index >= nl) {
        const int j = index - nl, nout = p.fc[j].nout;
        dims_out[0] = (int32_t)n_samples, dims_out[1] = 1, dims_out[2] = 1, dims_out[3] = nout;
        if (!out_host) return SD_OK;
        const void* src = j + 1 < nf ? (const void*)(wsb + ws.hidden_off[j]) : (const void*)logits_dev;
        return copy_out(out_host, src, n_samples * nout * sizeof(float), stream, "sd_viewnet_read_buffer");
    }
    const Layer& L = p.layers[index];
    const size_t px = n_samples * D * dims[index].h * dims[index].w;
    dims_out[0] = (int32_t)(n_samples * D), dims_out[1] = dims[index].h, dims_out[2] = dims[index].w, dims_out[3] = L.cout;
    if (!out_host) return SD_OK;
    return read_stored(wsb + ws.layer_off[index], px, L.cout, L.cout_p, p.act_dtype, out_host, stream, "sd_viewnet_read_buffer");
}

}  // extern "C"
