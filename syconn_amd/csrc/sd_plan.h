// Everything about a U-Net model that needs no device: the validated plan with its packed weight blob (build_plan), the shapes
// and the workspace layout of a tile, and which sub-box every op computes for an output box of interest.  Host-only: no HIP
// include, so tools/plan_dump.cpp and the CPU tests link it alone.  The launch side is sd_api.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/syconn_dense.h"

constexpr int SD_CHUNK = 16;      // channels per chunk plane = one MFMA k-step (layout: sd_internal.h)
// workspace scratch (first 64 KiB of a tile's workspace): [0, SD_GN_SCALE_OFF) GroupNorm sums (2 * C doubles, zero between ops),
// [SD_GN_SCALE_OFF, 64 KiB) scale / shift of a GroupNorm whose apply is not deferred (2 * C floats)
#define SD_GN_SCALE_OFF ((size_t)40960)

// true when launch_upconv (sd_kernels.hip) runs this shape with the row-coalescing kernel (activations of all chunks in
// registers): the form into which a deferred GroupNorm apply folds for less than the separate apply pass costs (the generic MFMA
// kernel pays more for it than the pass it replaces: 192 -> 96 channels 80 -> 108 us vs a 10 us pass)
bool upconv_rows_kernel(int nchunk, int Cd);

namespace sdplan {

constexpr size_t WS_SCRATCH = 65536;  // GroupNorm sums (double[2*C]) + scale/shift (float[2*C]) at workspace start

inline int rup(int v, int m) { return (v + m - 1) / m * m; }
inline size_t rup_sz(size_t v, size_t m) { return (v + m - 1) / m * m; }

struct Dims { int d = 0, h = 0, w = 0; };
struct Box { int lo[3], hi[3]; bool any; };      // z,y,x; hi exclusive; any == false: "the whole tensor" / "nothing yet" by context
// sd_model_set_roi: the part of the network output the caller keeps -- decoder ops then compute only what that box depends on
struct Roi { bool set = false; int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}; };

struct Op {
    sd_op_desc d{};
    // device pointers (into the model's weight blob)
    size_t wpack_off = 0, bias_off = 0, aux_off = 0;   // byte offsets
    size_t w3_off = 0;     // first conv, planar, bf16 / fp16 plans: three-way bf16 split of the weights / 255 for uint8 input (0: none)
    int NT = 1, NB = 1;
    bool first = false;    // conv reading the network input (cin = 1)
    int fuse_pool = -1;    // index of the MaxPool op computed in this conv's epilogue
    int fuse_final = -1;   // index of the final 1x1x1 op computed in this conv's epilogue
    int fuse_first = -1;   // conv: index of the first (cin = 1) convolution whose output (this conv's src0) it computes itself
    int fuse_gn = -1;      // conv: index of the GroupNorm op whose statistics this conv's epilogue accumulates
    int fuse_pool_raw = -1;   // conv with fuse_gn: index of the MaxPool op (behind that GroupNorm) whose RAW pooling this conv's epilogue does
    size_t pooldir_off = 0;   //   its per-channel direction masks (gamma < 0: minimum) in the blob
    bool stats_done = false;   // groupnorm: statistics come from the producing conv
    int gn_pool = -1;          // groupnorm: index of the MaxPool op fused into the apply pass
    bool pool_in_conv = false;   // groupnorm (deferred, with gn_pool): the producing conv pools the RAW tensor, its readers apply the table
    bool gn_defer = false;       // groupnorm: statistics -> scale / shift only; every consumer of the buffer applies them itself
    size_t fwfrag_off = 0;             // fused final 1x1x1: hi/lo MFMA weight fragments
    float oscale = 1.f;                // split-fp16 plan: 2^-k, undoes the power of two the packed weights / bias of this layer carry
    float final_oscale = 1.f;          //   ... and the one of the fused final layer's fragments
    bool skipped = false;  // op is executed inside its producer
    // up-convolution heading a fused level-0 decoder (sd_dec0.hip): indices of the merge conv and the second conv (whose
    // fuse_final names the final layer); those ops are `skipped` and their output buffers are never materialised
    int dec0_c1 = -1, dec0_c2 = -1;
    bool in_dec0 = false;
};

// The environment switches that shape a plan, read in one place.
struct PlanSwitches {
    // read once per model (read_plan_switches)
    bool keep_all = false;        // SD_KEEP_ALL: also store activations that only feed a fused consumer (tests)
    bool no_fuse = false;         // SD_NO_FUSE: every layer a separate launch, for layer-wise debugging
    bool no_ws_reuse = false;     // SD_NO_WS_REUSE
    bool no_first_fuse = false, no_gn_fuse = false, no_gn_defer = false, no_gn_pool_raw = false, split_no_final_fuse = false,
         gn_skip_not_deferred = false, no_dec0 = false;      // SD_NO_FIRST_FUSE ... SD_NO_DEC0
};
PlanSwitches read_plan_switches();
struct ProcessSwitches { bool no_nt3, roi_no_dec0, roi_no_encoder, no_upconv_wl; };      // SD_NO_NT3, SD_ROI_NO_DEC0, SD_ROI_NO_ENCODER, SD_NO_UPCONV_WL
const ProcessSwitches& process_switches();      // read once per process, at the first call

struct Plan {
    int act_dtype = SD_BF16;
    bool split = false;            // act_dtype == SD_F16X2 (sd_split.hip): every buffer holds 2 * Cp / 16 fp16 chunk planes [hi | lo]
    std::vector<Op> ops;
    int nbuf = 0;
    std::vector<int> bufC;    // real channels per buffer id
    std::vector<int> bufCp;   // padded channel stride
    // deferred GroupNorm apply: buffer b holds the RAW tensor, its consumers apply scale / shift (+ReLU) on the fly from a
    // per-tile [2*Cp] float table that lives in the workspace at gn_tab_off[b] (buf_gn[b] = index of the GroupNorm op)
    std::vector<int> buf_gn;
    std::vector<size_t> gn_tab_off;
    size_t ws_base = WS_SCRATCH;  // first byte of the activation buffers (behind the scratch and the tables)
    int final_cout = 0;
    bool keep_all = false;   // SD_KEEP_ALL=1
    bool ws_reuse = true;    // activation buffers with disjoint lifetimes share workspace memory
    std::vector<char> blob;  // host image of the packed weights (the model drops it after the upload)
};

// Validates the plan, folds BatchNorm, packs every weight layout into plan.blob and decides every fusion.  SD_OK, or
// SD_ERR_INVALID with the reason in `err`.
int build_plan(const sd_op_desc* ops, int n_ops, const float* W, size_t n_floats, int act_dtype, const PlanSwitches& sw, Plan& plan,
               std::string& err);

// shape inference for an input tile; fills dims[] per buffer (OpT: anything with an sd_op_desc `d`)
template <class OpT>
int infer_shapes(const std::vector<OpT>& ops, int nbuf, int D, int H, int W, std::vector<Dims>& dims, std::string& err) {
    dims.assign(nbuf, Dims{});
    dims[0] = {D, H, W};
    for (const OpT& op : ops) {
        const sd_op_desc& d = op.d;
        switch (d.kind) {
        case SD_OP_CONV: {
            const Dims a = dims[d.src0];
            Dims o = a;
            if (d.src1 >= 0) {
                o = dims[d.src1];
                if (a.d < o.d || a.h < o.h || a.w < o.w) { err = "merge conv: src0 smaller than src1"; return SD_ERR_INVALID; }
            }
            if (o.d <= 0) { err = "conv input not produced yet"; return SD_ERR_INVALID; }
            dims[d.dst] = o;
            break;
        }
        case SD_OP_POOL: {
            const Dims a = dims[d.src0];
            dims[d.dst] = {d.kz == 2 ? (a.d + 1) / 2 : a.d, (a.h + 1) / 2, (a.w + 1) / 2};
            break;
        }
        case SD_OP_UPCONV: {
            const Dims a = dims[d.src0];
            dims[d.dst] = {a.d * d.kz, a.h * 2, a.w * 2};
            break;
        }
        case SD_OP_GROUPNORM:
        case SD_OP_FINAL: break;
        default: err = "unknown op kind"; return SD_ERR_INVALID;
        }
    }
    return SD_OK;
}

bool dec0_shape_ok(const Dims& o);
Box dec0_view(const Roi& roi, const Dims& o);
bool use_dec0(const Roi& roi, const Dims& o);

// First-fit placement behind `base`: buffer b lives from op first[b] to op last[b] (last < 0: never used) and takes bytes[b];
// buffers whose lifetimes do not overlap share memory.  `reuse == false` gives every buffer its own range, in id order.  Returns
// the end of the highest range.
size_t place_buffers(const std::vector<int>& first, const std::vector<int>& last, const std::vector<size_t>& bytes, size_t base,
                     bool reuse, std::vector<size_t>& off);
// op index of the first write and the last use of every buffer (nops / -1: none), as the launches of a tile really happen
void plan_lifetimes(const Plan& p, bool dec0, std::vector<int>& first, std::vector<int>& last);
size_t plan_workspace(const Plan& p, const std::vector<Dims>& dims, const Roi& roi, std::vector<size_t>& off);
// the sub-box every op computes for the output box of interest (any == false: the whole tensor)
std::vector<Box> plan_views(const Plan& p, const std::vector<Dims>& dims, const Roi& roi, bool dec0);

}  // namespace sdplan
