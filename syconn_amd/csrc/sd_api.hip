// Host side of libsyconn_dense_hip.so: the C ABI of include/syconn_dense.h.  Uploads the plan that sd_plan.cpp builds (BatchNorm
// folded, weights packed in MFMA fragment order, fusions decided, workspace planned) and enqueues the gfx950 kernels.
#include "sd_internal.h"
#include "../../include/syconn_dense.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <string>
#include <vector>

using namespace sdplan;

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess)                                                                               \
            return fail(_e == hipErrorOutOfMemory ? SD_ERR_NOMEM : SD_ERR_HIP,                              \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                                 \
    } while (0)

}  // namespace

thread_local const char* sd_tls_kernel = nullptr;      // (sd_internal.h)
int sd_fail_msg(int code, const char* msg) { return fail(code, msg); }   // for the other translation units

struct sd_model {
    int device = 0;
    Plan plan;                // (SD_F32: only the op descriptions, act_dtype and final_cout)
    sd_f32_model* f32 = nullptr;   // act_dtype == SD_F32: the reference-precision plan (sd_f32.hip) serves every call
    Roi roi;                  // sd_model_set_roi (z,y,x; hi exclusive)
    char* dev_blob = nullptr; // packed weights
    size_t blob_bytes = 0;
    void* dev_zero = nullptr;
    int* dev_ovf = nullptr;   // fp16 range-guard flag (set by the final-layer kernels, read and cleared by sd_model_overflow)
    // last forward
    std::vector<Dims> dims;
    std::vector<size_t> buf_off;
    std::vector<const char*> op_kernel;   // kernel symbol each op's launch used (static strings; nullptr: no launch of its own)
    std::vector<int> op_exec;             // index of the op whose launch computed this op (itself, or the op it is fused into); -1: not run
    int last_launches = 0;             // ops that ran as their own launch
    int profile_slots = 0;             // 0 = off; else ring of event sets, one per sd_forward
    long n_forward = 0;
    std::vector<hipEvent_t> events;    // [slot][n_ops + 1]
    unsigned long long* dev_clk = nullptr;   // [slot][n_ops][4] clock stamps of the convolution launches (ConvParams::clk)
    std::vector<char> ev_recorded;     // [slot][n_ops + 1]: event was recorded by the forward that used the slot (ops that run inside
                                       // another op's launch record none: every record is a packet between two kernels)
    size_t n_ops() const { return plan.ops.size(); }
    // the event set, the recorded flags and the clock stamps of the forward about to run (nullptr: profiling is off)
    struct ProfileSlot { hipEvent_t* ev = nullptr; char* rec = nullptr; unsigned long long* clk = nullptr; };
    ProfileSlot profile_slot() {
        ProfileSlot p;
        if (profile_slots <= 0) return p;
        const size_t slot = (size_t)(n_forward % profile_slots);
        p.ev = events.data() + slot * (n_ops() + 1);
        p.rec = ev_recorded.data() + slot * (n_ops() + 1);
        if (dev_clk) p.clk = dev_clk + slot * n_ops() * 4;
        return p;
    }
};

namespace {

// sub-box launches keep the tensor's strides and shift the base pointers: voxel (z, y, x) of a tensor of y / x extents (H, W)
template <class T>
T* at_voxel(T* p, size_t z, size_t y, size_t x, int H, int W, size_t esz) {
    return reinterpret_cast<T*>(reinterpret_cast<char*>(const_cast<void*>(static_cast<const void*>(p))) + ((z * H + y) * W + x) * esz);
}
constexpr size_t VOX_BYTES = SD_CHUNK * 2;      // bytes per voxel of a chunk plane (bf16 / fp16 storage)

// What the launches of one forward pass share.
struct Forward {
    sd_model* m;
    const Plan& P;
    const void* in; int in_dtype;
    void* out; int out_kind; const LabelArgs* lab;
    int N, D, H, W;
    char* wsb;                // workspace of tile 0
    // tile t of a batch uses [t*tstride, t*tstride + need) of the workspace, its input / output follow tile 0's
    size_t tstride, in_tstride, out_tstride;
    hipStream_t s;
    bool dec0;                // the fused level-0 decoder serves this tile shape
    bool no_first_u8;         // SD_NO_FIRST_U8, an A/B switch read per forward: uint8 input through the exact-f32 MFMA chain
    std::vector<Box> view;    // per op: the sub-box its launch computes (plan_views)
    unsigned long long* clk;  // profiling: clock stamps of this forward's slot, 4 per op (or nullptr)
    const char* err = nullptr;   // set by a launch function that refuses: the reason

    void* bufp(int b) const { return wsb + m->buf_off[b]; }
    const char* blob(size_t off) const { return m->dev_blob + off; }
    const float* blobf(size_t off) const { return reinterpret_cast<const float*>(m->dev_blob + off); }
    size_t out_esz() const { return out_kind == SD_OUT_PROBS_U8 || out_kind == SD_OUT_LABELS_U8 ? 1 : 4; }
    bool whole_tile(const Dims& o) const { return o.d == D && o.h == H && o.w == W; }
    // voxels of all tiles that op k's launch computes (its sub-box, if it has one): what the launchers choose the kernel form by
    long launch_vox(size_t k) const {
        const Dims o = m->dims[P.ops[k].d.dst];
        const Box& v = view[k];
        return (v.any ? (long)(v.hi[0] - v.lo[0]) * (v.hi[1] - v.lo[1]) * (v.hi[2] - v.lo[2]) : (long)o.d * o.h * o.w) * N;
    }
    // does convolution k compute the first convolution (its src0) itself?  Decided per launch: only some kernel forms can
    bool computes_first(size_t k) const {
        const Op& c = P.ops[k];
        if (c.fuse_first < 0 || P.keep_all) return false;
        const int nst = (P.bufCp[c.d.src0] / SD_CHUNK) * c.d.kz * (P.split ? 3 : 1);
        return P.split ? conv_can_fuse_first_split(c.d.kz, c.NT, c.NB, launch_vox(k), nst, c.fuse_final >= 0)
                       : conv_can_fuse_first(c.d.kz, c.NT, c.NB, launch_vox(k), nst, c.fuse_final >= 0);
    }
    // the scale / shift table of a deferred GroupNorm apply of buffer b (untouched if b is final)
    void gn_table(int b, const float*& tab, int& relu) const {
        if (b > 0 && P.buf_gn[b] >= 0) {
            tab = reinterpret_cast<const float*>(wsb + P.gn_tab_off[b]);
            relu = P.ops[P.buf_gn[b]].d.relu;
        }
    }

    int launch_first_op(size_t i) {
        const Op& op = P.ops[i];
        const sd_op_desc& d = op.d;
        const Dims o = m->dims[d.dst];
        const int BZ = sd_bz(d.kz), BY = sd_by(d.kz);
        FirstParams p{};
        p.in = in; p.D = o.d; p.H = o.h; p.W = o.w;
        p.dst = bufp(d.dst); p.Cd = P.bufCp[d.dst];
        p.wpack = blobf(op.wpack_off);
        p.wpack3 = (op.w3_off && !no_first_u8) ? blob(op.w3_off) : nullptr;
        p.bias = blobf(op.bias_off);
        p.relu = d.relu;
        p.batch = N; p.tstride = tstride; p.in_tstride = in_tstride; p.ovf = m->dev_ovf;
        p.nbx = (o.w + SD_BX - 1) / SD_BX; p.nby = (o.h + BY - 1) / BY; p.nbz = (o.d + BZ - 1) / BZ;
        return launch_first(p, P.act_dtype, in_dtype, d.kz, s);
    }

    // a deferred-GroupNorm convolution keeps the scale / shift of all its tiles in LDS (128 B per 16 channels and tile): launch
    // the tiles in groups that fit beside the halo / weight buffers (24 KiB are always free)
    int launch_conv_tile_groups(const ConvParams& p, const Op& op) const {
        const size_t per_tile = conv_gn_lds_per_tile(p.nchunk0 + p.nchunk1);
        const int group = (int)std::max<size_t>(1, std::min<size_t>((size_t)N, (24 * 1024) / per_tile));
        int rc = SD_OK;
        for (int t0 = 0; t0 < N && rc == SD_OK; t0 += group) {
            ConvParams q = p;
            q.batch = std::min(group, N - t0);
            q.batch_total = N;      // the kernel form is chosen for the whole launch set, not per tile group
            auto adv = [&](const void* ptr) { return ptr ? reinterpret_cast<const char*>(ptr) + (size_t)t0 * tstride : nullptr; };
            q.src0 = adv(p.src0); q.src1 = adv(p.src1);
            q.dst = const_cast<char*>(adv(p.dst));
            q.pool_dst = const_cast<char*>(adv(p.pool_dst));
            q.gn_sums = reinterpret_cast<double*>(const_cast<char*>(adv(p.gn_sums)));
            q.gn0 = reinterpret_cast<const float*>(adv(p.gn0)); q.gn1 = reinterpret_cast<const float*>(adv(p.gn1));
            q.final_out = p.final_out ? reinterpret_cast<char*>(p.final_out) + (size_t)t0 * out_tstride : nullptr;
            rc = launch_conv(q, P.act_dtype, op.d.kz, op.NT, op.NB, s);
        }
        return rc;
    }

    int launch_conv_op(size_t i) {
        const Op& op = P.ops[i];
        const sd_op_desc& d = op.d;
        const Dims o = m->dims[d.dst], a = m->dims[d.src0];
        const int BZ = sd_bz(d.kz), BY = sd_by(d.kz);
        ConvParams p{};
        p.src0 = bufp(d.src0); p.C0 = P.bufCp[d.src0]; p.H0 = a.h; p.W0 = a.w; p.P0 = (size_t)a.d * a.h * a.w;
        const int vmul = P.split ? 3 : 1;      // split-fp16 plan: virtual chunks [hi | hi | lo]
        p.nchunk0 = p.C0 / SD_CHUNK * vmul;
        p.oscale = op.oscale;
        if (d.src1 >= 0) {
            const Dims b = m->dims[d.src1];
            p.src1 = bufp(d.src1); p.C1 = P.bufCp[d.src1]; p.H1 = b.h; p.W1 = b.w; p.P1 = (size_t)b.d * b.h * b.w;
            p.nchunk1 = p.C1 / SD_CHUNK * vmul;
        }
        p.dst = bufp(d.dst); p.Cd = P.bufCp[d.dst];
        p.D = o.d; p.H = o.h; p.W = o.w; p.Pd = (size_t)o.d * o.h * o.w;
        p.Hd = o.h; p.Wd = o.w; p.final_nvox = (long)o.d * o.h * o.w;
        p.wpack = blob(op.wpack_off);
        p.bias = blobf(op.bias_off);
        p.relu = d.relu; p.zero = m->dev_zero;
        p.store_main = 1; p.ovf = m->dev_ovf;
        p.batch = N; p.tstride = tstride; p.out_tstride = out_tstride;
        if (clk) p.clk = clk + i * 4;
    #ifdef SD_TIMING
        p.dbg = (getenv("SD_TIMING_OP") && atoi(getenv("SD_TIMING_OP")) == (int)i) ? reinterpret_cast<long long*>(wsb + m->buf_off[1]) : nullptr;
    #endif
        const int pooled = op.fuse_pool >= 0 ? op.fuse_pool : op.fuse_pool_raw;
        if (pooled >= 0) {
            const sd_op_desc& pd = P.ops[pooled].d;
            p.pool_dst = bufp(pd.dst); p.pH = m->dims[pd.dst].h; p.pW = m->dims[pd.dst].w;
            p.Pp = (size_t)m->dims[pd.dst].d * p.pH * p.pW;
            if (op.fuse_pool_raw >= 0) p.pool_dir = reinterpret_cast<const unsigned*>(blob(op.pooldir_off));
        }
        if (op.fuse_final >= 0) {
            const Op& fo = P.ops[op.fuse_final];
            if (!whole_tile(o)) { err = "final layer shape != input shape"; return SD_ERR_INVALID; }
            p.final_wfrag = blob(op.fwfrag_off);
            p.final_b = blobf(fo.bias_off);
            p.final_cout = fo.d.cout; p.final_kind = out_kind; p.final_out = out;
            p.final_oscale = op.final_oscale;
            if (lab) p.lab = *lab;
            p.store_main = P.keep_all ? 1 : 0;
        }
        if (computes_first(i)) {
            const Op& fo = P.ops[op.fuse_first];
            p.first_in = in; p.first_in_tstride = in_tstride; p.first_in_f32 = in_dtype == SD_F32 ? 1 : 0;
            p.first_w = blobf(fo.wpack_off);
            p.first_bias = blobf(fo.bias_off);
            p.first_w3 = (fo.w3_off && in_dtype == SD_U8 && !no_first_u8) ? blob(fo.w3_off) : nullptr;
            p.first_relu = fo.d.relu;
        }
        if (op.fuse_gn >= 0) {      // (scratch is zero: see the start of the forward pass and k_gn_finalize)
            p.gn_sums = reinterpret_cast<double*>(wsb); p.gn_C = p.Cd;
        }
        p.nbx = (o.w + SD_BX - 1) / SD_BX; p.nby = (o.h + BY - 1) / BY; p.nbz = (o.d + BZ - 1) / BZ;
        if (view[i].any) {      // sub-box launch: same strides, shifted bases, the box as the extent
            const Box& v = view[i];
            p.src0 = at_voxel(p.src0, v.lo[0], v.lo[1], v.lo[2], p.H0, p.W0, VOX_BYTES);
            if (p.src1) p.src1 = at_voxel(p.src1, v.lo[0], v.lo[1], v.lo[2], p.H1, p.W1, VOX_BYTES);
            p.dst = at_voxel(p.dst, v.lo[0], v.lo[1], v.lo[2], o.h, o.w, VOX_BYTES);
            if (p.final_out) p.final_out = at_voxel(p.final_out, v.lo[0], v.lo[1], v.lo[2], o.h, o.w, out_esz());
            if (p.pool_dst)      // (only z-ranges reach a convolution with fused pooling: lo[1] = lo[2] = 0)
                p.pool_dst = at_voxel(p.pool_dst, v.lo[0] / (d.kz == 3 ? 2 : 1), 0, 0, p.pH, p.pW, VOX_BYTES);
            if (p.first_in) p.first_in = at_voxel(p.first_in, v.lo[0], 0, 0, o.h, o.w, in_dtype == SD_U8 ? 1 : 4);
            p.D = v.hi[0] - v.lo[0]; p.H = v.hi[1] - v.lo[1]; p.W = v.hi[2] - v.lo[2];
        }
        gn_table(d.src0, p.gn0, p.gn_relu0);
        if (d.src1 >= 0) gn_table(d.src1, p.gn1, p.gn_relu1);
        if (p.gn0 || p.gn1) return launch_conv_tile_groups(p, op);
        return launch_conv(p, P.act_dtype, d.kz, op.NT, op.NB, s);
    }

    int launch_dec0_op(size_t i) {
        const Op& op = P.ops[i];
        const Op& c1 = P.ops[op.dec0_c1];
        const Op& c2 = P.ops[op.dec0_c2];
        const Op& fo = P.ops[c2.fuse_final];
        const Dims a = m->dims[op.d.src0], o = m->dims[c1.d.src1];
        if (!whole_tile(o) || a.d != D) { err = "final layer shape != input shape"; return SD_ERR_INVALID; }
        Dec0Params p{};
        p.l1 = bufp(op.d.src0); p.skip = bufp(c1.d.src1);
        p.D = o.d; p.H = o.h; p.W = o.w; p.H1 = a.h; p.W1 = a.w; p.Ps = (size_t)o.d * o.h * o.w;
        p.wup = blob(op.wpack_off); p.bup = blobf(op.bias_off);
        p.w1 = blob(c1.wpack_off); p.b1 = blobf(c1.bias_off);
        p.w2 = blob(c2.wpack_off); p.b2 = blobf(c2.bias_off);
        p.fw = blob(c2.fwfrag_off); p.fb = blobf(fo.bias_off);
        p.final_cout = fo.d.cout; p.final_kind = out_kind; p.final_out = out;
        if (lab) p.lab = *lab;
        p.zero = m->dev_zero; p.ovf = m->dev_ovf;
        p.batch = N; p.tstride = tstride; p.out_tstride = out_tstride;
        if (view[i].any) {      // sub-box launch: the tensors' extents as strides, shifted bases, the box as the extent
            const Box& v = view[i];
            p.sH = o.h; p.sW = o.w; p.sH1 = a.h; p.sW1 = a.w;
            p.Pl1 = (size_t)a.d * a.h * a.w; p.out_nvox = (long)o.d * o.h * o.w;
            p.skip = at_voxel(p.skip, v.lo[0], v.lo[1], v.lo[2], o.h, o.w, VOX_BYTES);
            p.l1 = at_voxel(p.l1, v.lo[0], v.lo[1] / 2, v.lo[2] / 2, a.h, a.w, VOX_BYTES);
            p.final_out = at_voxel(p.final_out, v.lo[0], v.lo[1], v.lo[2], o.h, o.w, out_esz());
            p.D = v.hi[0] - v.lo[0]; p.H = v.hi[1] - v.lo[1]; p.W = v.hi[2] - v.lo[2];
            p.H1 = (v.hi[1] + 1) / 2 - v.lo[1] / 2; p.W1 = (v.hi[2] + 1) / 2 - v.lo[2] / 2;
        }
        p.dbg = getenv("SD_DEC0_DBG") ? reinterpret_cast<long long*>(wsb) : nullptr;      // (timing builds) GroupNorm scratch
        return launch_dec0(p, P.act_dtype, s);
    }

    int launch_upconv_op(size_t i) {
        const Op& op = P.ops[i];
        const sd_op_desc& d = op.d;
        UpconvParams p{};
        const Dims a = m->dims[d.src0], o = m->dims[d.dst];
        p.src = bufp(d.src0); p.Cs = P.bufCp[d.src0]; p.nchunk = p.Cs / SD_CHUNK * (P.split ? 3 : 1);
        p.oscale = op.oscale;
        p.D = a.d; p.H = a.h; p.W = a.w;
        p.Ps = (size_t)a.d * a.h * a.w; p.Hs = a.h; p.Ws = a.w; p.Hd = o.h; p.Wd = o.w;
        p.dst = bufp(d.dst); p.Cd = P.bufCp[d.dst]; p.kz = d.kz;
        p.Pd = (size_t)o.d * o.h * o.w;
        if (view[i].any) {      // sub-box of the source voxels (and the 2x box of the output they produce)
            const Box& v = view[i];
            p.src = at_voxel(p.src, v.lo[0], v.lo[1], v.lo[2], a.h, a.w, VOX_BYTES);
            p.dst = at_voxel(p.dst, (size_t)v.lo[0] * d.kz, 2 * v.lo[1], 2 * v.lo[2], p.Hd, p.Wd, VOX_BYTES);
            p.D = v.hi[0] - v.lo[0]; p.H = v.hi[1] - v.lo[1]; p.W = v.hi[2] - v.lo[2];
        }
        p.wpack = blob(op.wpack_off);
        p.bias = blobf(op.bias_off);
        p.relu = d.relu; p.ntot = d.kz * 4 * p.Cd; p.ovf = m->dev_ovf;
        p.batch = N; p.tstride = tstride;
        gn_table(d.src0, p.gn, p.gn_relu);
        return launch_upconv(p, P.act_dtype, op.NB, s);
    }

    int launch_pool_op(size_t i) {
        const sd_op_desc& d = P.ops[i].d;
        PoolParams p{};
        const Dims a = m->dims[d.src0], o = m->dims[d.dst];
        p.src = bufp(d.src0); p.dst = bufp(d.dst); p.C = P.bufCp[d.src0];
        p.D = a.d; p.H = a.h; p.W = a.w; p.Do = o.d; p.Ho = o.h; p.Wo = o.w; p.kz = d.kz;
        p.Ps = (size_t)a.d * a.h * a.w; p.Pd = (size_t)o.d * o.h * o.w;
        p.batch = N; p.tstride = tstride;
        return launch_pool(p, P.act_dtype, s);
    }

    int launch_groupnorm_op(size_t i) {
        const Op& op = P.ops[i];
        const sd_op_desc& d = op.d;
        GnParams p{};
        const Dims a = m->dims[d.src0];
        const Dims r = d.src1 >= 0 ? m->dims[d.src1] : a;
        p.buf = bufp(d.src0); p.C = P.bufCp[d.src0];
        p.D = r.d; p.H = r.h; p.W = r.w; p.Hs = a.h; p.Ws = a.w; p.P = (size_t)a.d * a.h * a.w;
        p.groups = d.groups; p.cout = P.bufC[d.src0]; p.eps = d.eps;
        p.gamma = blobf(op.aux_off);
        p.beta = p.gamma + p.C;
        p.sums = reinterpret_cast<double*>(wsb);
        // (not deferred: a fixed place behind the statistics scratch -- the scratch itself must stay zero between GroupNorm ops)
        p.scale_shift = reinterpret_cast<float*>(op.gn_defer ? wsb + P.gn_tab_off[d.src0] : wsb + SD_GN_SCALE_OFF);
        p.relu = d.relu;
        p.batch = N; p.tstride = tstride; p.skip_stats = op.stats_done ? 1 : 0;
        p.skip_apply = (op.gn_defer && (op.gn_pool < 0 || op.pool_in_conv)) ? 1 : 0;
        p.no_inplace = op.gn_defer ? 1 : 0;
        if (op.gn_pool >= 0 && !op.pool_in_conv) {
            const sd_op_desc& pd = P.ops[op.gn_pool].d;
            const Dims po = m->dims[pd.dst];
            p.pool_dst = bufp(pd.dst); p.pkz = pd.kz; p.pD = po.d; p.pH = po.h; p.pW = po.w;
        }
        return launch_groupnorm(p, P.act_dtype, s);
    }

    int launch_final_op(size_t i) {
        const Op& op = P.ops[i];
        const sd_op_desc& d = op.d;
        FinalParams p{};
        const Dims a = m->dims[d.src0];
        p.src = bufp(d.src0); p.Cs = P.bufCp[d.src0]; p.cin = d.cin0;
        p.w = blobf(op.wpack_off);
        p.bias = blobf(op.bias_off);
        p.wfrag = blob(op.aux_off);
        p.cout = d.cout; p.out = out; p.out_kind = out_kind; p.ovf = m->dev_ovf;
        p.nvox = (long)a.d * a.h * a.w;
        p.batch = N; p.tstride = tstride; p.out_tstride = out_tstride;
        if (lab) p.lab = *lab;
        gn_table(d.src0, p.gn_scale_shift, p.gn_relu);      // deferred GroupNorm apply of the input
        if (!whole_tile(a)) { err = "final layer shape != input shape"; return SD_ERR_INVALID; }
        return launch_final(p, P.act_dtype, s);
    }

    int launch_op(size_t i) {
        const Op& op = P.ops[i];
        switch (op.d.kind) {
        case SD_OP_CONV: return op.first ? launch_first_op(i) : launch_conv_op(i);
        case SD_OP_POOL: return launch_pool_op(i);
        case SD_OP_UPCONV: return (op.dec0_c1 >= 0 && dec0) ? launch_dec0_op(i) : launch_upconv_op(i);
        case SD_OP_GROUPNORM: return launch_groupnorm_op(i);
        case SD_OP_FINAL: return launch_final_op(i);
        default: return SD_ERR_INVALID;
        }
    }
};

}  // namespace

extern "C" {

const char* sd_last_error(void) { return g_err.c_str(); }
const char* sd_version(void) { return "syconn_dense_hip 0.1 (gfx950)"; }

int sd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sd_init(int device_ordinal) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(SD_ERR_NODEVICE, "no HIP device visible; libsyconn_dense_hip has no CPU fallback");
    if (device_ordinal < 0 || device_ordinal >= n) return fail(SD_ERR_INVALID, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device_ordinal));
    return SD_OK;
}

int sd_model_num_ops(const sd_model* m) { return m ? (int)m->n_ops() : 0; }
int sd_debug_last_launch_count(const sd_model* m) { return m ? m->last_launches : 0; }
int sd_debug_op_kernel(const sd_model* m, int op, char* buf, int n) {
    if (!m) return -1;
    if (op < 0 || op >= (int)m->n_ops()) return -1;
    if (m->f32) {      // (the fp32 FMA plan keeps its own op list: every op launches its own k32_* kernel)
        if (buf && n > 0) snprintf(buf, (size_t)n, "%s", f32_op_kernel(m->f32, op));
        return op;
    }
    const int e = op < (int)m->op_exec.size() ? m->op_exec[op] : -1;
    if (buf && n > 0) {
        const char* name = (e >= 0 && e < (int)m->op_kernel.size() && m->op_kernel[e]) ? m->op_kernel[e] : "";
        snprintf(buf, (size_t)n, "%s", name);
    }
    return e;
}

int sd_model_create(const sd_op_desc* ops, int n_ops, const float* W, size_t n_floats, int act_dtype,
                    sd_model** out) {
    if (!ops || n_ops <= 0 || !W || !out) return fail(SD_ERR_INVALID, "null argument");
    if (act_dtype != SD_BF16 && act_dtype != SD_F16 && act_dtype != SD_F32 && act_dtype != SD_F16X2)
        return fail(SD_ERR_INVALID, "act_dtype must be SD_BF16, SD_F16, SD_F16X2 or SD_F32");
    sd_model* m = new sd_model();
    m->plan.act_dtype = act_dtype;
    if (hipGetDevice(&m->device) != hipSuccess) { delete m; return fail(SD_ERR_NODEVICE, "no current HIP device"); }
    if (act_dtype == SD_F32) {       // reference-precision mode: its own plan, weights and kernels
        const int rc32 = f32_model_create(ops, n_ops, W, n_floats, &m->f32);
        if (rc32 != SD_OK) { delete m; return rc32; }
        for (int i = 0; i < n_ops; ++i) { Op op; op.d = ops[i]; m->plan.ops.push_back(op); }
        m->plan.final_cout = f32_final_cout(m->f32);
        *out = m;
        return SD_OK;
    }
    std::string err;
    int rc = build_plan(ops, n_ops, W, n_floats, act_dtype, read_plan_switches(), m->plan, err);
    if (rc == SD_OK) {
        std::vector<char>& blob = m->plan.blob;
        m->blob_bytes = rup_sz(blob.size(), 256);
        hipError_t e = hipMalloc((void**)&m->dev_blob, m->blob_bytes + 1024 + 512);
        if (e == hipSuccess) e = hipMemset(m->dev_blob + m->blob_bytes + 1024, 0, 512);
        m->dev_zero = m->dev_blob + m->blob_bytes + 1024;
        m->dev_ovf = reinterpret_cast<int*>(m->dev_blob + m->blob_bytes + 1024 + 256);
        if (e == hipSuccess) e = hipMemcpy(m->dev_blob, blob.data(), blob.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            err = std::string("weight upload: ") + hipGetErrorString(e);
            rc = e == hipErrorOutOfMemory ? SD_ERR_NOMEM : SD_ERR_HIP;
        }
        std::vector<char>().swap(blob);      // (the host image is not needed again)
    }
    if (rc != SD_OK) {
        sd_model_destroy(m);
        return fail(rc, err);
    }
    *out = m;
    return SD_OK;
}

void sd_model_destroy(sd_model* m) {
    if (!m) return;
    for (hipEvent_t e : m->events) (void)hipEventDestroy(e);
    if (m->dev_blob) (void)hipFree(m->dev_blob);
    if (m->dev_clk) (void)hipFree(m->dev_clk);
    f32_model_destroy(m->f32);
    delete m;
}

size_t sd_workspace_bytes(const sd_model* m, int D, int H, int W) {
    if (!m || D <= 0 || H <= 0 || W <= 0) { fail(SD_ERR_INVALID, "bad tile shape"); return 0; }
    if (m->f32) return f32_workspace_bytes(m->f32, D, H, W);
    std::vector<Dims> dims;
    std::vector<size_t> off;
    std::string err;
    if (infer_shapes(m->plan.ops, m->plan.nbuf, D, H, W, dims, err) != SD_OK) { fail(SD_ERR_INVALID, err); return 0; }
    return rup_sz(plan_workspace(m->plan, dims, m->roi, off), 256);
}

int sd_model_set_roi(sd_model* m, const int32_t* lo_zyx, const int32_t* hi_zyx) {
    if (!m || ((lo_zyx == nullptr) != (hi_zyx == nullptr))) return fail(SD_ERR_INVALID, "sd_model_set_roi: bad argument");
    m->roi.set = lo_zyx != nullptr;
    for (int a = 0; a < 3; ++a) { m->roi.lo[a] = lo_zyx ? lo_zyx[a] : 0; m->roi.hi[a] = hi_zyx ? hi_zyx[a] : 0; }
    if (m->roi.set)
        for (int a = 0; a < 3; ++a)
            if (m->roi.lo[a] < 0 || m->roi.hi[a] <= m->roi.lo[a]) { m->roi.set = false; return fail(SD_ERR_INVALID, "sd_model_set_roi: empty box"); }
    return SD_OK;
}

int sd_memcpy2d_async(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width_bytes, size_t height, int kind,
                      void* stream) {
    if (!dst || !src || width_bytes > dst_pitch || width_bytes > src_pitch || kind < 0 || kind > 2)
        return fail(SD_ERR_INVALID, "sd_memcpy2d_async: bad argument");
    if (width_bytes == 0 || height == 0) return SD_OK;
    const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIP_TRY(hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, width_bytes, height, k, reinterpret_cast<hipStream_t>(stream)));
    return SD_OK;
}

int sd_profile_enable(sd_model* m, int n_slots) {
    if (!m || n_slots < 0) return fail(SD_ERR_INVALID, "sd_profile_enable: bad argument");
    for (hipEvent_t e : m->events) (void)hipEventDestroy(e);
    m->events.clear();
    m->profile_slots = n_slots;
    m->n_forward = 0;
    m->ev_recorded.assign((size_t)std::max(n_slots, 0) * (m->n_ops() + 1), 0);
    if (m->dev_clk) { (void)hipFree(m->dev_clk); m->dev_clk = nullptr; }
    if (n_slots > 0) {
        m->events.resize((size_t)n_slots * (m->n_ops() + 1));
        for (auto& e : m->events) HIP_TRY(hipEventCreate(&e));
        const size_t nb = (size_t)n_slots * m->n_ops() * 4 * sizeof(unsigned long long);
        HIP_TRY(hipMalloc(&m->dev_clk, nb));
        HIP_TRY(hipMemset(m->dev_clk, 0, nb));
    }
    return SD_OK;
}

int sd_profile_read_clocks(sd_model* m, int slot, uint64_t* stamps, int n_ops) {
    if (!m || !stamps || m->profile_slots <= 0 || slot < 0 || slot >= m->profile_slots || !m->dev_clk)
        return fail(SD_ERR_INVALID, "sd_profile_read_clocks: profiling not enabled or bad slot");
    const int n = std::min<int>(n_ops, (int)m->n_ops());
    HIP_TRY(hipMemcpy(stamps, m->dev_clk + (size_t)slot * m->n_ops() * 4, (size_t)n * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_profile_read(sd_model* m, int slot, float* ms, int n_ops) {
    if (!m || !ms || m->profile_slots <= 0 || slot < 0 || slot >= m->profile_slots)
        return fail(SD_ERR_INVALID, "sd_profile_read: profiling not enabled or bad slot");
    const int n = std::min<int>(n_ops, (int)m->n_ops()), nall = (int)m->n_ops();
    const hipEvent_t* ev = m->events.data() + (size_t)slot * (m->n_ops() + 1);
    const char* rec = m->ev_recorded.data() + (size_t)slot * (m->n_ops() + 1);
    for (int i = 0; i < n; ++i) {
        ms[i] = 0.f;
        if (!rec[i]) continue;                       // ran inside another op's launch
        int j = i + 1;
        while (j < nall && !rec[j]) ++j;             // next op that launched (or the end-of-forward event)
        if (!rec[j]) return fail(SD_ERR_INVALID, "sd_profile_read: slot holds no complete forward");
        HIP_TRY(hipEventElapsedTime(&ms[i], ev[i], ev[j]));
    }
    return SD_OK;
}

int sd_model_overflow(sd_model* m, void* stream, int* flag_out) {
    if (!m || !flag_out) return fail(SD_ERR_INVALID, "null argument");
    *flag_out = 0;
    if (m->f32 || (m->plan.act_dtype != SD_F16 && m->plan.act_dtype != SD_F16X2) || !m->dev_ovf) return SD_OK;       // only fp16 storage can overflow
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(flag_out, m->dev_ovf, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (*flag_out) HIP_TRY(hipMemsetAsync(m->dev_ovf, 0, sizeof(int), s));
    return SD_OK;
}

int sd_forward(sd_model* m, const void* in_dev, int in_dtype, int D, int H, int W, void* out_dev, int out_kind,
               void* ws, size_t ws_bytes, void* stream) {
    return sd_forward_batch(m, in_dev, in_dtype, 1, D, H, W, out_dev, out_kind, ws, ws_bytes, stream);
}

static bool make_label_args(int C, const int32_t* ids, const double* thresholds, int n_ids, LabelArgs& a) {
    if (!ids || !thresholds || n_ids <= 0 || n_ids > 16) return false;
    a.n = n_ids;
    for (int i = 0; i < n_ids; ++i) {
        if (ids[i] < 0 || ids[i] >= C) return false;
        a.ids[i] = ids[i];
        const double t = thresholds[i];
        if (t != t) return false;
        // (uint8 p > t) <=> p >= floor(t) + 1, exact for any real t
        const double c = std::floor(t) + 1.0;
        a.cuts[i] = c < 0.0 ? 0 : (c > 256.0 ? 256 : (int)c);
    }
    return true;
}

static int forward_impl(sd_model* m, const void* in_dev, int in_dtype, int N, int D, int H, int W, void* out_dev,
                        int out_kind, const LabelArgs* lab, void* ws, size_t ws_bytes, void* stream);

int sd_forward_batch(sd_model* m, const void* in_dev, int in_dtype, int N, int D, int H, int W, void* out_dev,
                     int out_kind, void* ws, size_t ws_bytes, void* stream) {
    if (out_kind < 0 || out_kind > 2) return fail(SD_ERR_INVALID, "bad out_kind");
    return forward_impl(m, in_dev, in_dtype, N, D, H, W, out_dev, out_kind, nullptr, ws, ws_bytes, stream);
}

int sd_forward_labels_batch(sd_model* m, const void* in_dev, int in_dtype, int N, int D, int H, int W,
                            const int32_t* ids, const double* thresholds, int n_ids, uint8_t* out_dev, void* ws,
                            size_t ws_bytes, void* stream) {
    if (!m) return fail(SD_ERR_INVALID, "null argument");
    LabelArgs a{};
    if (!make_label_args(m->plan.final_cout, ids, thresholds, n_ids, a))
        return fail(SD_ERR_INVALID, "sd_forward_labels_batch: bad label arguments");
    return forward_impl(m, in_dev, in_dtype, N, D, H, W, out_dev, SD_OUT_LABELS_U8, &a, ws, ws_bytes, stream);
}

static int forward_impl(sd_model* m, const void* in_dev, int in_dtype, int N, int D, int H, int W, void* out_dev,
                        int out_kind, const LabelArgs* lab, void* ws, size_t ws_bytes, void* stream) {
    if (!m || !in_dev || !out_dev || !ws) return fail(SD_ERR_INVALID, "null argument");
    if (N <= 0 || N > 65535) return fail(SD_ERR_INVALID, "bad batch size");
    if (in_dtype != SD_U8 && in_dtype != SD_F32) return fail(SD_ERR_INVALID, "in_dtype must be SD_U8 or SD_F32");
    if (D <= 0 || H <= 0 || W <= 0) return fail(SD_ERR_INVALID, "bad tile shape");
    if ((long)D * H * W >= (1l << 31)) return fail(SD_ERR_INVALID, "tile has 2^31 or more voxels");
    if (m->f32) {
        const sd_model::ProfileSlot prof = m->profile_slot();
        if (prof.rec) std::fill(prof.rec, prof.rec + m->n_ops() + 1, 1);      // (the fp32 plan launches every op)
        ++m->n_forward;
        m->last_launches = (int)m->n_ops();
        return f32_forward(m->f32, in_dev, in_dtype, N, D, H, W, out_dev, out_kind, lab, ws, ws_bytes,
                           reinterpret_cast<hipStream_t>(stream), prof.ev);
    }
    const Plan& P = m->plan;
    std::string err;
    int rc = infer_shapes(P.ops, P.nbuf, D, H, W, m->dims, err);
    if (rc != SD_OK) return fail(rc, err);
    const size_t tstride = rup_sz(plan_workspace(P, m->dims, m->roi, m->buf_off), 256);
    if ((size_t)N * tstride > ws_bytes) return fail(SD_ERR_NOMEM, "workspace too small");
    const size_t nvox = (size_t)D * H * W;
    const size_t out_tstride = out_kind == SD_OUT_LABELS_U8 ? nvox : (size_t)P.final_cout * nvox * (out_kind == SD_OUT_PROBS_U8 ? 1 : 4);
    const bool dec0 = use_dec0(m->roi, m->dims[0]);
    if (m->roi.set)
        for (int a = 0; a < 3; ++a) {
            const int n = a == 0 ? D : a == 1 ? H : W;
            if (m->roi.lo[a] < 0 || m->roi.hi[a] > n || m->roi.lo[a] >= m->roi.hi[a]) return fail(SD_ERR_INVALID, "sd_model_set_roi: box outside the tile");
        }
    const sd_model::ProfileSlot prof = m->profile_slot();
    Forward F{m, P, in_dev, in_dtype, out_dev, out_kind, lab, N, D, H, W, reinterpret_cast<char*>(ws), tstride,
              nvox * (in_dtype == SD_U8 ? 1 : 4), out_tstride, reinterpret_cast<hipStream_t>(stream), dec0,
              getenv("SD_NO_FIRST_U8") != nullptr, plan_views(P, m->dims, m->roi, dec0), prof.clk};
    const size_t nops = m->n_ops();
    if (prof.rec) std::fill(prof.rec, prof.rec + nops + 1, 0);
    ++m->n_forward;
    m->last_launches = 0;
    m->op_kernel.assign(nops, nullptr);
    m->op_exec.assign(nops, -1);
    {
        // GroupNorm statistics scratch (sum and sum of squares per channel, doubles, at the start of every tile's workspace): zeroed
        // ONCE per forward pass; every k_gn_finalize leaves it zeroed for the next GroupNorm op
        int maxc = 0;
        for (const Op& op : P.ops)
            if (op.d.kind == SD_OP_GROUPNORM) maxc = std::max(maxc, P.bufCp[op.d.src0]);
        if ((size_t)2 * maxc * sizeof(double) > SD_GN_SCALE_OFF || SD_GN_SCALE_OFF + (size_t)2 * maxc * sizeof(float) > WS_SCRATCH)
            return fail(SD_ERR_INVALID, "GroupNorm: more channels than the statistics scratch holds");
        if (maxc > 0) {
            const int rc0 = launch_zero_scratch(F.wsb, tstride, 2 * maxc * (int)sizeof(double), N, F.s);
            if (rc0 != SD_OK) return fail(rc0, "zeroing the GroupNorm scratch failed");
        }
    }
    for (size_t i = 0; i < nops; ++i) {
        const Op& op = P.ops[i];
        if (op.skipped || (op.in_dec0 && dec0)) continue;
        ++m->last_launches;
        // (a first convolution that runs inside its consumer launches nothing: no event either)
        if (op.first && i + 1 < nops && P.ops[i + 1].fuse_first == (int)i && F.computes_first(i + 1)) { m->op_exec[i] = (int)i + 1; continue; }
        if (prof.ev) { HIP_TRY(hipEventRecord(prof.ev[i], F.s)); prof.rec[i] = 1; }
        sd_tls_kernel = nullptr;
        rc = F.launch_op(i);
        if (rc != SD_OK) {
            if (F.err) return fail(rc, F.err);
            char msg[128];
            snprintf(msg, sizeof msg, "launch of op %zu (kind %d) failed: %s", i, op.d.kind, hipGetErrorString(hipGetLastError()));
            return fail(rc, msg);
        }
        // what ran: this op by the kernel its launcher noted, and inside that launch the ops fused into it
        m->op_kernel[i] = sd_tls_kernel;
        if (m->op_exec[i] < 0) m->op_exec[i] = (int)i;
        auto own = [&](int j) { if (j >= 0 && j < (int)nops) m->op_exec[j] = (int)i; };
        own(op.fuse_pool); own(op.fuse_final); own(op.fuse_pool_raw); own(op.gn_pool);
        if (op.d.kind == SD_OP_UPCONV && op.dec0_c1 >= 0 && dec0) {
            own(op.dec0_c1); own(op.dec0_c2); own(P.ops[op.dec0_c2].fuse_final);
        }
    }
    if (prof.ev) { HIP_TRY(hipEventRecord(prof.ev[nops], F.s)); prof.rec[nops] = 1; }
    return SD_OK;
}

int sd_tile_gather(const void* vol, int dtype, int VD, int VH, int VW, int oz, int oy, int ox, void* tile, int TD, int TH,
                   int TW, void* stream) {
    if (!vol || !tile || (dtype != SD_U8 && dtype != SD_F32)) return fail(SD_ERR_INVALID, "sd_tile_gather: bad argument");
    int rc = launch_tile_gather(vol, dtype == SD_U8 ? 1 : 4, VD, VH, VW, oz, oy, ox, tile, TD, TH, TW,
                                reinterpret_cast<hipStream_t>(stream));
    return rc == SD_OK ? rc : fail(rc, "sd_tile_gather launch failed");
}

int sd_tile_scatter(const void* tile, int dtype, int C, int TD, int TH, int TW, int cz, int cy, int cx, int KD, int KH,
                    int KW, void* vol, int VD, int VH, int VW, int oz, int oy, int ox, void* stream) {
    if (!vol || !tile || (dtype != SD_U8 && dtype != SD_F32)) return fail(SD_ERR_INVALID, "sd_tile_scatter: bad argument");
    if (cz < 0 || cy < 0 || cx < 0 || cz + KD > TD || cy + KH > TH || cx + KW > TW || oz < 0 || oy < 0 || ox < 0)
        return fail(SD_ERR_INVALID, "sd_tile_scatter: crop outside tile");
    int rc = launch_tile_scatter(tile, dtype == SD_U8 ? 1 : 4, C, TD, TH, TW, cz, cy, cx, KD, KH, KW, vol, VD, VH, VW,
                                 oz, oy, ox, reinterpret_cast<hipStream_t>(stream));
    return rc == SD_OK ? rc : fail(rc, "sd_tile_scatter launch failed");
}

int sd_downsample2(const void* src, int dtype, int D, int H, int W, void* dst, void* stream) {
    if (!src || !dst || D <= 0 || H <= 0 || W <= 0 || (dtype != SD_U8 && dtype != SD_U64))
        return fail(SD_ERR_INVALID, "sd_downsample2: bad argument");
    int rc = launch_downsample2(src, dtype == SD_U8 ? 1 : 8, D, H, W, dst, reinterpret_cast<hipStream_t>(stream));
    return rc == SD_OK ? rc : fail(rc, "sd_downsample2 launch failed");
}

int sd_box_majority(const uint8_t* vol, int D, int H, int W, const int32_t* origins_zyx, size_t n, int ez, int ey, int ex,
                    double thresh_proba, double thresh_majority, uint8_t* out, void* stream) {
    if (!vol || (!origins_zyx && n) || (!out && n) || D <= 0 || H <= 0 || W <= 0 || ez <= 0 || ey <= 0 || ex <= 0)
        return fail(SD_ERR_INVALID, "sd_box_majority: bad argument");
    if (thresh_proba != thresh_proba) return fail(SD_ERR_INVALID, "sd_box_majority: NaN threshold");
    // (uint8 p > t) <=> p >= floor(t) + 1, exact for any real t
    const double c = std::floor(thresh_proba) + 1.0;
    const int cut = c < 0.0 ? 0 : (c > 256.0 ? 256 : (int)c);
    int rc = launch_box_majority(vol, D, H, W, origins_zyx, (long)n, ez, ey, ex, cut, thresh_majority, out,
                                 reinterpret_cast<hipStream_t>(stream));
    return rc == SD_OK ? rc : fail(rc, "sd_box_majority launch failed");
}

int sd_postproc_labels(const uint8_t* probs, int C, size_t nvox, const int32_t* ids, const double* thresholds, int n_ids,
                       void* out, int out_dtype, void* stream) {
    if (!probs || !ids || !thresholds || !out || n_ids <= 0 || n_ids > 16)
        return fail(SD_ERR_INVALID, "sd_postproc_labels: bad argument");
    if (out_dtype != SD_U8 && out_dtype != SD_U64) return fail(SD_ERR_INVALID, "sd_postproc_labels: out_dtype");
    LabelArgs a{};      // one threshold -> cut rule for the fused and the separate path (NaN rejected, cuts in [0, 256])
    if (!make_label_args(C, ids, thresholds, n_ids, a))
        return fail(SD_ERR_INVALID, "sd_postproc_labels: id out of range or NaN threshold");
    int rc = launch_labels(probs, nvox, a, out, out_dtype == SD_U64, reinterpret_cast<hipStream_t>(stream));
    return rc == SD_OK ? rc : fail(rc, "sd_postproc_labels launch failed");
}

int sd_debug_read_buffer(sd_model* m, int buf, const void* ws, float* out, int32_t* dims4, void* stream) {
    if (m && m->f32) return f32_read_buffer(m->f32, buf, ws, out, dims4, reinterpret_cast<hipStream_t>(stream));
    if (!m || buf <= 0 || buf >= m->plan.nbuf || m->dims.empty()) return fail(SD_ERR_INVALID, "sd_debug_read_buffer: bad argument");
    const Dims a = m->dims[buf];
    if (dims4) { dims4[0] = m->plan.bufC[buf]; dims4[1] = a.d; dims4[2] = a.h; dims4[3] = a.w; }
    if (!out) return SD_OK;
    int rc = launch_read_buffer(reinterpret_cast<const char*>(ws) + m->buf_off[buf], m->plan.act_dtype, m->plan.bufC[buf],
                                m->plan.bufCp[buf], a.d, a.h, a.w, out, reinterpret_cast<hipStream_t>(stream));
    return rc == SD_OK ? rc : fail(rc, "sd_debug_read_buffer launch failed");
}

}  // extern "C"
