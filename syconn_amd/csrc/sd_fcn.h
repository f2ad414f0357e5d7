// Everything about an FCN semantic-segmentation network (sd_fcn.hip) that needs no device: the validated plan with its packed weight
// blob, the shapes of every stored tensor for an input geometry and the workspace layout.  Host-only like sd_viewnet.h: no HIP
// include, so tools/fcn_plan_dump.cpp and the CPU tests link sd_fcn_plan.cpp alone.
//
// Layout.  Activations are channels-last in the storage type T (fp16 / bf16): [plane][y][x][cp] with cp = channels rounded up to 8,
// the pad channels hold zero.  One plane = one (location, view) pair.  Every MFMA op (3 x 3 convolution, one output parity of a
// transposed convolution) is an implicit GEMM on v_mfma_f32_16x16x32: M = 8 x 32 positions of a workgroup's tile, N = cout in tiles of
// 16 (at most MAX_NT per workgroup, the groups go into the grid), K = input channels in chunks of CK = 32 staged through LDS, times
// the taps of the op; one K step of 32 = the 32 channels of one chunk under one tap.
//   wfrag  T[n_chunks][n_taps][NTtot][64 lanes][8]   B operand: element j of lane l = W[c = 32 chunk + 8 (l >> 4) + j][tap][n = 16 nt +
//                                    (l & 15)], zero where c or n is padding.  NTtot = groups x NT.  Convolution: tap = 3 ky + kx, reads
//                                    the input at (y + ky - 1, x + kx - 1).  Transposed convolution (oy = 2 iy - 1 + ky): parity
//                                    (py, px) of the output has the row taps py = 0: (ky 1, dy 0); py = 1: (ky 2, dy 0), (ky 0, dy 1)
//                                    and the same along x; tap order is row-major over (row tap, column tap); one wfrag per parity
//   bias   float[16 NTtot]         b (zero for pad channels)
//   scale, shift float[16 NTtot]   eval BatchNorm behind a transposed convolution: scale = gamma / sqrt(var + eps), shift = beta -
//                                    mean scale, computed in double and rounded to fp32 once; zero for pad channels
//   cls    float[n_class][dec_last] then float[n_class]: the classifier in fp32
#pragma once
#include "sd_netplan.h"      // the tile (TILE_H x TILE_W positions of one workgroup), rup, to_storage / from_storage

namespace sdfcn {

using namespace sdnet;

constexpr int CK = 32;                      // input channels per LDS chunk = one K step
constexpr int CKP = 40;                     // element stride of a pixel inside the LDS tile (80 bytes: 16-byte aligned, spreads the banks)
constexpr int HALO_H = TILE_H + 2, HALO_W = TILE_W + 2;
constexpr size_t LDS_BYTES = (size_t)HALO_H * HALO_W * CKP * 2;      // 27200
constexpr int MAX_NT = 4;                   // N tiles of one workgroup (64 output channels)
constexpr int MAX_C = 512, MAX_CLASS = 16, N_BLOCKS = 5, MAX_BLOCK_CONVS = 3;
constexpr double BN_EPS = 1e-5;
enum { OP_CONV = 0, OP_DECONV = 1, OP_CLASSIFY = 2 };

struct Op {
    int kind = OP_CONV;
    int cin = 0, cout = 0, cin_p = 0, cout_p = 0;
    bool first = false, pool = false;      // convolution: reads the uint8 views / its 2 x 2 pool is fused
    int in_shift = 0, out_shift = 0;       // the input / stored output is (H >> shift) x (W >> shift)
    int in_buf = -1, out_buf = -1, skip_buf = -1;      // indices of stored tensors (ops); in_buf -1: the views
    int n_chunks = 0, NT = 0, groups = 0;  // K chunks, N tiles per workgroup, workgroups along N
    size_t wfrag_off[4] = {0, 0, 0, 0};    // convolution: [0]; transposed convolution: parity 2 py + px
    size_t bias_off = 0, scale_off = 0, shift_off = 0;      // classifier: bias_off = weights, scale_off = bias
    double macs_per_in_px = 0;             // real multiply-adds per input pixel (convolution: = per pre-pool output pixel)
};
struct Plan {
    int act_dtype = SD_F16, in_channels = 0, n_class = 0, dec_last = 0;
    std::vector<Op> ops;      // encoder convolutions, five transposed convolutions, the classifier
    std::vector<char> blob;
};
struct Dims { int c = 0, cp = 0, h = 0, w = 0; };      // a stored tensor

// blocks: the output channels of all encoder convolutions, block after block; block_len[5]: convolutions per block.
// weights: float32 in registration order (encoder w[cout][cin][3][3], b; per decoder step w[cin][cout][3][3], b, gamma, beta, mean, var;
// classifier w[n_class][dec_last], b).  SD_OK, or SD_ERR_INVALID with the reason in `err`.
int build_plan(int in_channels, const int32_t* blocks, const int32_t* block_len, int dec_last, int n_class, const float* W, size_t n_floats,
               int act_dtype, Plan& plan, std::string& err);
// H, W multiples of 32; the stored tensor of every op (the classifier's: the float32 logits, cp = c)
int infer_shapes(const Plan& p, int H, int W, std::vector<Dims>& dims, std::string& err);
// every stored tensor has its own range (the skip tensors live until their addition and every tensor stays readable); the last op has none
struct Workspace { std::vector<size_t> off; size_t total = 0; };
int workspace(const Plan& p, size_t n_planes, int H, int W, Workspace& ws, std::string& err);
double macs_per_view(const Plan& p, int H, int W);
// taps of an op: (dy, dx) inside the LDS tile relative to the position, and (ky, kx) of the weight.  parity only for OP_DECONV.
struct Tap { int dy, dx, ky, kx; };
int taps_of(int kind, int parity, Tap taps[9]);

}  // namespace sdfcn
