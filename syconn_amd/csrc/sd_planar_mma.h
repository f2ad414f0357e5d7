// The planar MFMA layer core of the 2D view networks (sd_viewnet.hip, sd_fcn.hip): a workgroup of 4 waves computes TILE_H x TILE_W =
// 8 x 32 positions of one plane as an implicit GEMM on v_mfma_f32_16x16x32, every wave four 16-row MFMA tiles.  Here: the MFMA
// wrapper, the lane -> position map of a tile, the renderer's uint8 planes as the first layer's source, and the fp16 range test.  The
// LDS layouts, the K loops and the epilogues stay with the kernels.
#pragma once
#include "sd_device.h"
#include "sd_netplan.h"

namespace sdnet {

constexpr int WAVES = 4, WAVE_MT = 4;      // waves of a workgroup, MFMA row tiles of a wave
static_assert(WAVES * WAVE_MT * 16 == TILE_H * TILE_W, "the row tiles cover the workgroup's tile");

// Mma16: c + a b on one 16 x 16 x 32 MFMA, for either storage type
__device__ __forceinline__ f32x4 mma16(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// The position (cy, cx) inside the workgroup's tile of A row m (= lane & 15) of the i-th row tile of `wave`.  With a 2 x 2 pool a
// row tile is 2 rows x 8 columns ordered so that rows 4 g ... 4 g + 3 are the window of one pooled pixel -- the accumulator rows of
// lane group g (C/D map: col = lane & 15, row = 4 (lane >> 4) + reg) --; without a pool it is 16 pixels of one row.
__device__ __forceinline__ void lane_pos(int wave, int i, int m, bool pool, int& cy, int& cx) {
    const int mt = wave * WAVE_MT + i;
    if (pool) {
        cy = 2 * (mt >> 2) + ((m & 3) >> 1);
        cx = 8 * (mt & 3) + 2 * (m >> 2) + (m & 1);
    } else {
        cy = mt >> 1;
        cx = 16 * (mt & 1) + m;
    }
}

// The epilogue's walk over a lane's accumulators (for i, for nt: the maximum of the four registers at the pooled pixel, or four
// pixels of a row) is written out in k_vn_conv and k_fcn_conv: as a function taking the epilogue body hipcc (ROCm 7.2) allots the
// callers other registers and the view net's layers measure 1.5 to 3.5 % slower (profiles/viewnets_walk_ab.txt).

// Plane `src` of the renderer's planar uint8 tensor (n_loc, cin, nb_views, H, W): location src / nb_views, view src % nb_views.
// at(c, gy, gx, inside): channel c at (gy, gx) in the storage type -- the integers 0 ... 255 are exact in fp16 and bf16 --, zero for a
// channel the tensor does not have or where the caller found the position outside the plane.
template <typename T> struct U8Plane {
    const uint8_t* base;
    size_t cs;      // channel stride
    int cin, W;
    __device__ __forceinline__ U8Plane(const void* in, long long src, int nb_views, int cin_, int H, int W_) : cin(cin_), W(W_) {
        const long long loc = src / nb_views, v = src - loc * nb_views;
        const size_t hw = (size_t)H * W;
        cs = hw * nb_views;
        base = reinterpret_cast<const uint8_t*>(in) + ((size_t)loc * cin * nb_views + v) * hw;
    }
    __device__ __forceinline__ T at(int c, int gy, int gx, bool inside) const {
        float u = 0.f;
        if (c < cin && inside) u = (float)base[c * cs + (size_t)gy * W + gx];
        return (T)u;
    }
};

// does v round to an infinity of the storage type?  (only fp16 can: bf16 has fp32's exponent range)
template <typename T> __device__ __forceinline__ bool stores_inf(float v) {
    if constexpr (std::is_same<T, f16_t>::value) return !(fabsf(v) < 65520.f);      // 65520 is the first value that rounds to inf
    return false;
}

}  // namespace sdnet
