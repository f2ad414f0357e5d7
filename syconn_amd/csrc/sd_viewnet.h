// Everything about a multi-view network (sd_viewnet.hip) that needs no device: the validated plan with its packed weight blob, the
// shapes of every layer for an input geometry and the workspace layout.  Host-only like sd_plan.h: no HIP include, so
// tools/viewnet_plan_dump.cpp and the CPU tests link sd_viewnet_plan.cpp alone.
//
// Layout.  Activations are channels-last in the storage type T (fp16 / bf16): [plane][y][x][cp] with cp = channels rounded up to 8,
// the pad channels hold act(0) = 0.  plane = sample * D + slot.  A layer is an implicit GEMM on v_mfma_f32_16x16x32: M = the 8 x 32
// convolution outputs of a workgroup's tile (rows of one 16-row MFMA tile = the 2 x 2 windows of four pooled pixels, so the pool is a
// maximum over the four accumulator registers of a lane), N = cout in tiles of 16, K = taps x cp in steps of 32.
//   wfrag  T[nks][NT][64 lanes][8]   B operand: element j of lane l = W[k = 32 ks + 8 (l >> 4) + j][n = 16 nt + (l & 15)], zero where
//                                    k or n is padding;  k = tap * cin_p + c, tap = ky * k + kx
//   aoff   int32[nks][4][2]          A operand: element offset, inside the workgroup's LDS halo tile [8 + k - 1][32 + k - 1][cin_p],
//                                    of the 8 consecutive k of lane group l >> 4 relative to the lane's output pixel; the first layer
//                                    (cin_p = 4) reads two taps of 4 channels, hence two offsets; padding k point at offset 0
//   bias   float[16 NT]              b, for the first layer b - 0.5 sum(stored w): conv(u / 255 - 0.5) = acc(u) / 255 - 0.5 sum(w) + b
#pragma once
#include "sd_netplan.h"      // the tile (TILE_H x TILE_W convolution outputs of one workgroup), rup, to_storage / from_storage

namespace sdvn {

using namespace sdnet;

constexpr int MAX_NT = 5;                   // cout <= 80
constexpr int MAX_FC = 4;
constexpr size_t MAX_LDS = 65536;           // halo tile of a layer / the two vectors of the head
constexpr int ACT_RELU = 0, ACT_LEAKY = 1;
constexpr float LEAKY_SLOPE = 0.01f;        // torch.nn.LeakyReLU()

struct Layer {
    int cin = 0, cout = 0, k = 0, pool = 0;
    int cin_p = 0, cout_p = 0;      // channel strides of the input and the output tensor
    int NT = 0, K = 0, nks = 0;     // N tiles, padded K, K steps of 32
    size_t wfrag_off = 0, aoff_off = 0, bias_off = 0;      // byte offsets into the blob
    size_t lds_bytes = 0;
    double macs_per_out = 0;        // k k cin cout: real multiply-adds per convolution output pixel
};
struct Fc { int nin = 0, nout = 0; size_t w_off = 0, b_off = 0; };
struct Plan {
    int act_dtype = SD_F16, act = ACT_RELU, in_channels = 0, n_scalar = 0;
    std::vector<Layer> layers;
    std::vector<Fc> fc;
    std::vector<char> blob;
};
struct Dims { int h = 0, w = 0; };      // the stored (pooled) output of a layer

// Validates the description against the weights and packs the blob.  SD_OK, or SD_ERR_INVALID with the reason in `err`.
int build_plan(const sd_viewnet_layer_desc* layers, int n_layers, const int32_t* fc, int n_fc, int in_channels, int n_scalar, int act,
               const float* W, size_t n_floats, int act_dtype, Plan& plan, std::string& err);
// valid convolution, floor pool; refuses an empty output and a flattened size that the first Linear does not take
int infer_shapes(const Plan& p, int D, int H, int W, std::vector<Dims>& dims, std::string& err);
struct Workspace { std::vector<size_t> layer_off, hidden_off; size_t total = 0; };      // hidden_off: outputs of all Linear layers but the last
int workspace(const Plan& p, size_t n_samples, int D, int H, int W, Workspace& ws, std::string& err);
// multiply-adds of one sample, convolutions (real channels, computed pixels only) + head
double macs_per_sample(const Plan& p, int D, int H, int W);
// The sample-tiled head (k_vn_head_tile): TS samples of a workgroup share one pass over the weights.  LDS: the input tile [TS][nin of
// the first Linear] and two hidden tiles [TS][hmax], float; TS = the largest of 8, 4, 2, 1 that fits the 160 KiB a gfx950 workgroup can
// have (TS = 1 always fits: three vectors of at most 8192 values).
constexpr size_t HEAD_TILE_LDS = 160 * 1024;
constexpr int HEAD_TILE_THREADS = 512;      // 8 waves, one output row of a Linear each
inline int head_tile_hmax(const Plan& p) {
    int h = 0;
    for (const Fc& f : p.fc) h = f.nout > h ? f.nout : h;
    return h;
}
inline size_t head_tile_lds(const Plan& p, int TS) { return sizeof(float) * (size_t)TS * ((size_t)p.fc[0].nin + 2 * (size_t)head_tile_hmax(p)); }
inline int head_tile_samples(const Plan& p) {
    for (int ts = 8; ts > 1; ts >>= 1)
        if (head_tile_lds(p, ts) <= HEAD_TILE_LDS) return ts;
    return 1;
}

}  // namespace sdvn
