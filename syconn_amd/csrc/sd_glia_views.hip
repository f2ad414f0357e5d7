// The two device steps between the glia view network's logits and glia_pred, and the view filter in front of the network:
//
//   sd_glia_view_probas         softmax over the two logits of every sample (/root/reference/syconn/handler/prediction.py:978-982: the
//                               InferenceModel's output is thresholded as a probability, segmentation.py:799-814).  One thread per sample:
//                               both float32 logits widened to float64, the larger one subtracted, exp, one division, ONE rounding to
//                               float32.  A logit that is NaN or infinite raises flag_dev[0].
//   sd_views_center_component   single_conn_comp_img (proc/image.py:125-144) for a batch of planes: keep the 4-connected component of
//                               pixel != background that holds the centre pixel (H / 2, W / 2), everything else becomes background.
//                               Only that one component matters, so nothing is labelled: one workgroup per plane floods from the centre.
//                               The foreground mask and the reached mask are bit planes in LDS, 32 pixels of a row per word (bit b of word
//                               wx is x = 32 wx + b; bits at x >= W are never foreground).  A round gives every word
//                                   fg & (reached | reached << 1 | reached >> 1 | carry of the left word | carry of the right word | up | down)
//                               -- the carries join neighbouring words of ONE row, never two rows -- and then fills the runs of foreground
//                               bits inside the word that a reached bit touches (five doubling steps per direction).  Words are updated in
//                               place: a word has one writer, every value another thread reads is a state the mask has had, and the mask
//                               only grows, so the fixed point -- the component -- does not depend on the order.
//                               Termination: a round that changes a word adds at least one pixel, so there are at most (foreground
//                               pixels of the component) + 1 <= H W + 1 rounds; the loop ends with the first round that changes nothing.
//                               The "changed" flags are three LDS words used in turn, so that one barrier per round suffices: the flag of
//                               round k is cleared behind the barrier of round k - 2 and read behind the barrier of round k.
//
// Every index is derived from the arguments (nothing is read from device memory to address with); the plane loop, the word loops and the
// pixel writes are bounded by n_planes, H ceil(W / 32) and W.  No float atomics, no scalar memory writes, no inline assembly.
#include "../../include/syconn_dense.h"
#include "sd_tables.h"

namespace {

constexpr int GRID = SD_GLIA_VIEWS_GRID;

__global__ __launch_bounds__(256) void k_gv_probas(const float2* __restrict__ logits, u64 n, float2* __restrict__ probas, int* flag) {
#pragma clang fp contract(off)
    for (u64 i = grid_tid(); i < n; i += grid_stride()) {
        const float2 l = logits[i];
        const double a = (double)l.x, b = (double)l.y;
        if (!(__builtin_isfinite(a) && __builtin_isfinite(b))) atomicOr(flag, 1);
        const double m = a > b ? a : b;
        const double ea = exp(a - m), eb = exp(b - m);
        const double s = ea + eb;
        probas[i] = make_float2((float)(ea / s), (float)(eb / s));
    }
}

// the runs of 1-bits of `f` that a bit of `x` (a subset of f) touches
__device__ __forceinline__ u32 fill_runs(u32 x, u32 f) {
    u32 m = f, y = x;
    y |= m & (y << 1); m &= m << 1;
    y |= m & (y << 2); m &= m << 2;
    y |= m & (y << 4); m &= m << 4;
    y |= m & (y << 8); m &= m << 8;
    y |= m & (y << 16);
    m = f;
    y |= m & (y >> 1); m &= m >> 1;
    y |= m & (y >> 2); m &= m >> 2;
    y |= m & (y >> 4); m &= m >> 4;
    y |= m & (y >> 8); m &= m >> 8;
    y |= m & (y >> 16);
    return y;
}

// WIDE: W is a multiple of 32 and both pointers are 16-byte aligned, so a word's 32 pixels are two aligned 16-byte vectors
template <bool WIDE>
__global__ __launch_bounds__(256) void k_gv_center(const uint8_t* in, u64 n_planes, int H, int W, u32 bg, uint8_t* out) {
    extern __shared__ __attribute__((aligned(16))) u32 gv_smem[];
    const int WW = (W + 31) >> 5, NW = H * WW;
    u32* fg = gv_smem;
    u32* reached = gv_smem + NW;
    u32* changed = gv_smem + 2 * NW;                                              // three flags, used in turn
    const int tid = threadIdx.x;
    const u32 bg4 = bg * 0x01010101u;
    for (u64 plane = blockIdx.x; plane < n_planes; plane += gridDim.x) {
        const uint8_t* src = in + plane * (u64)H * (u64)W;
        uint8_t* dst = out + plane * (u64)H * (u64)W;
        __syncthreads();                                                         // the previous plane's masks are done with
        for (int w = tid; w < NW; w += 256) {
            const int y = w / WW, wx = w - y * WW;
            const u64 row = (u64)y * (u64)W + 32u * (u32)wx;
            u32 f = 0;
            if (WIDE) {
                const uint4 v0 = *reinterpret_cast<const uint4*>(src + row), v1 = *reinterpret_cast<const uint4*>(src + row + 16);
                const u32 q[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const u32 d = q[k] ^ bg4;                                    // a byte is 0 where the pixel is background
#pragma unroll
                    for (int j = 0; j < 4; ++j) f |= ((d >> (8 * j)) & 0xffu) ? 1u << (4 * k + j) : 0u;
                }
            } else {
                const int nb = W - 32 * wx < 32 ? W - 32 * wx : 32;
                for (int b = 0; b < nb; ++b) f |= (u32)src[row + b] != bg ? 1u << b : 0u;
            }
            fg[w] = f;
            reached[w] = 0;
        }
        if (tid < 3) changed[tid] = 0;
        __syncthreads();
        if (tid == 0) {
            const int cy = H / 2, cx = W / 2;
            const int w = cy * WW + (cx >> 5);
            reached[w] = fg[w] & (1u << (cx & 31));
        }
        __syncthreads();
        for (int round = 0;; ++round) {
            const int p = round % 3;
            bool any = false;
            for (int w = tid; w < NW; w += 256) {
                const u32 f = fg[w];
                if (!f) continue;
                const int y = w / WW, wx = w - y * WW;
                const u32 r = reached[w];
                u32 nb = r | (r << 1) | (r >> 1);
                if (wx > 0) nb |= reached[w - 1] >> 31;
                if (wx + 1 < WW) nb |= reached[w + 1] << 31;
                if (y > 0) nb |= reached[w - WW];
                if (y + 1 < H) nb |= reached[w + WW];
                const u32 x = fill_runs(f & nb, f);
                if (x != r) { reached[w] = x; any = true; }
            }
            if (any) changed[p] = 1;
            __syncthreads();
            const u32 c = changed[p];
            if (tid == 0) changed[(p + 2) % 3] = 0;                              // round + 2's flag: last read behind the previous barrier
            if (!c) break;
        }
        for (int w = tid; w < NW; w += 256) {
            const int y = w / WW, wx = w - y * WW;
            const u64 row = (u64)y * (u64)W + 32u * (u32)wx;
            const u32 r = reached[w];
            if (WIDE) {
                const uint4 v0 = *reinterpret_cast<const uint4*>(src + row), v1 = *reinterpret_cast<const uint4*>(src + row + 16);
                u32 q[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    u32 keep = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) keep |= ((r >> (4 * k + j)) & 1u) ? 0xffu << (8 * j) : 0u;
                    q[k] = (q[k] & keep) | (bg4 & ~keep);
                }
                *reinterpret_cast<uint4*>(dst + row) = make_uint4(q[0], q[1], q[2], q[3]);
                *reinterpret_cast<uint4*>(dst + row + 16) = make_uint4(q[4], q[5], q[6], q[7]);
            } else {
                const int nb = W - 32 * wx < 32 ? W - 32 * wx : 32;
                for (int b = 0; b < nb; ++b) dst[row + b] = ((r >> b) & 1u) ? src[row + b] : (uint8_t)bg;
            }
        }
    }
}

template <bool WIDE>
int launch_center(const uint8_t* in, size_t n_planes, int H, int W, int bg, uint8_t* out, size_t lds, hipStream_t s) {
    if (lds > 65536 &&      // beyond the default limit of dynamic LDS: ask for it
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gv_center<WIDE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return sd_fail_msg(SD_ERR_HIP, "sd_views_center_component: the LDS request was refused");
    const int grid = (int)(n_planes < (size_t)GRID ? n_planes : (size_t)GRID);
    hipLaunchKernelGGL(k_gv_center<WIDE>, dim3(grid), dim3(256), lds, s, in, (u64)n_planes, H, W, (u32)bg, out);
    return launch_status("sd_views_center_component: launch failed");
}

}  // namespace

extern "C" {

int sd_glia_view_probas(const float* logits_dev, size_t n, float* probas_dev, int32_t* flag_dev, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_glia_view_probas";
    if (!flag_dev) return fail(who, ": null flag");
    if (n >= LIM31) return fail(who, ": samples < 2^31 per call");
    if (hipMemsetAsync(flag_dev, 0, sizeof(int32_t), s) != hipSuccess) return sd_fail_msg(SD_ERR_HIP, "memset failed");
    if (n == 0) return SD_OK;
    if (!logits_dev || !probas_dev) return fail(who, ": bad argument");
    if ((reinterpret_cast<uintptr_t>(logits_dev) | reinterpret_cast<uintptr_t>(probas_dev)) & 7) return fail(who, ": logits and probabilities must be 8-byte aligned");
    launch_1d(k_gv_probas, n, GRID, s, reinterpret_cast<const float2*>(logits_dev), (u64)n, reinterpret_cast<float2*>(probas_dev), flag_dev);
    return launch_status("sd_glia_view_probas: launch failed");
}

int sd_views_center_component(const uint8_t* in_dev, size_t n_planes, int H, int W, int background, uint8_t* out_dev, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* who = "sd_views_center_component";
    if (H < 1 || W < 1) return fail(who, ": H and W must be positive");
    if (background < 0 || background > 255) return fail(who, ": background must be a uint8 value");
    if (n_planes >= LIM31) return fail(who, ": planes < 2^31 per call");
    const size_t words = (size_t)H * (((size_t)W + 31) / 32);
    const size_t lds = 8 * words + 16;                                            // two masks and the flags
    if (lds > SD_GLIA_VIEWS_LDS_BYTES) return fail(who, ": the plane's two bit masks (8 H ceil(W / 32) + 16 bytes) do not fit the LDS of one workgroup");
    if (n_planes == 0) return SD_OK;
    if (!in_dev || !out_dev) return fail(who, ": bad argument");
    const bool wide = W % 32 == 0 && !((reinterpret_cast<uintptr_t>(in_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 15);
    return wide ? launch_center<true>(in_dev, n_planes, H, W, background, out_dev, lds, s) : launch_center<false>(in_dev, n_planes, H, W, background, out_dev, lds, s);
}

}  // extern "C"
