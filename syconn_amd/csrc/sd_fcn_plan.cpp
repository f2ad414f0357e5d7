// The host-only plan builder of the FCN semantic-segmentation network (sd_fcn.h): validation, weight rounding, the MFMA fragment order
// of the convolutions and of the four output parities of the transposed convolutions, the BatchNorm constants, shapes and the
// workspace layout.
#include "sd_fcn.h"

#include <cmath>
#include <cstring>

namespace sdfcn {

int taps_of(int kind, int parity, Tap taps[9]) {
    if (kind == OP_CONV) {
        for (int t = 0; t < 9; ++t) taps[t] = {t / 3, t % 3, t / 3, t % 3};
        return 9;
    }
    // oy = 2 iy - 1 + ky: an even output row reads ky = 1 of its own input row, an odd one ky = 2 of its own and ky = 0 of the next
    static const int d_even[1] = {0}, k_even[1] = {1}, d_odd[2] = {0, 1}, k_odd[2] = {2, 0};
    const int py = parity >> 1, px = parity & 1, ny = py ? 2 : 1, nx = px ? 2 : 1;
    int n = 0;
    for (int a = 0; a < ny; ++a)
        for (int b = 0; b < nx; ++b)
            taps[n++] = {py ? d_odd[a] : d_even[a], px ? d_odd[b] : d_even[b], py ? k_odd[a] : k_even[a], px ? k_odd[b] : k_even[b]};
    return n;
}

// packs one wfrag; `deconv`: w is [cin][cout][3][3], else [cout][cin][3][3]
static int pack_frags(Plan& plan, Op& op, const float* w, bool deconv, int parity, size_t& off_out, std::string& err, const std::string& what) {
    Tap taps[9];
    const int nt = taps_of(deconv ? OP_DECONV : OP_CONV, parity, taps);
    const int NTtot = op.NT * op.groups;
    off_out = grow(plan.blob, (size_t)op.n_chunks * nt * NTtot * 64 * 8 * 2);
    uint16_t* f = reinterpret_cast<uint16_t*>(plan.blob.data() + off_out);
    for (int ch = 0; ch < op.n_chunks; ++ch)
        for (int t = 0; t < nt; ++t)
            for (int ntg = 0; ntg < NTtot; ++ntg)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int c = CK * ch + 8 * (lane >> 4) + j, n = 16 * ntg + (lane & 15);
                        uint16_t v = 0;
                        if (c < op.cin && n < op.cout) {
                            const size_t idx = deconv ? (((size_t)c * op.cout + n) * 3 + taps[t].ky) * 3 + taps[t].kx
                                                      : (((size_t)n * op.cin + c) * 3 + taps[t].ky) * 3 + taps[t].kx;
                            if (!store_weight(w[idx], plan.act_dtype, v)) return bad(err, what + ": a weight overflows the storage type (use bf16, or rescale)");
                        }
                        f[((((size_t)ch * nt + t) * NTtot + ntg) * 64 + lane) * 8 + j] = v;
                    }
    return SD_OK;
}

int build_plan(int in_channels, const int32_t* blocks, const int32_t* block_len, int dec_last, int n_class, const float* W, size_t n_floats,
               int act_dtype, Plan& plan, std::string& err) {
    if (!blocks || !block_len || !W) return bad(err, "fcn: null argument");
    if (act_dtype != SD_F16 && act_dtype != SD_BF16) return bad(err, "fcn: act_dtype must be SD_F16 or SD_BF16");
    if (in_channels < 1 || in_channels > 4) return bad(err, "fcn: in_channels must be 1 to 4");
    if (dec_last < 1 || dec_last > MAX_C) return bad(err, "fcn: dec_last must be 1 to 512");
    if (n_class < 1 || n_class > MAX_CLASS) return bad(err, "fcn: n_class must be 1 to 16");
    int n_convs = 0;
    for (int b = 0; b < N_BLOCKS; ++b) {
        if (block_len[b] < 1 || block_len[b] > MAX_BLOCK_CONVS) return bad(err, "fcn: block " + std::to_string(b) + ": 1 to 3 convolutions");
        n_convs += block_len[b];
    }
    for (int i = 0; i < n_convs; ++i)
        if (blocks[i] < 1 || blocks[i] > MAX_C) return bad(err, "fcn: convolution " + std::to_string(i) + ": channels must be 1 to 512");
    plan = Plan{};
    plan.act_dtype = act_dtype, plan.in_channels = in_channels, plan.n_class = n_class, plan.dec_last = dec_last;

    // the ops and the float count the description implies, before anything is read
    int x_ch[N_BLOCKS], x_buf[N_BLOCKS];
    size_t need = 0;
    {
        int cin = in_channels, i = 0, prev = -1;
        for (int b = 0; b < N_BLOCKS; ++b)
            for (int j = 0; j < block_len[b]; ++j, ++i) {
                Op op;
                op.kind = OP_CONV, op.cin = cin, op.cout = blocks[i];
                op.first = i == 0, op.pool = j == block_len[b] - 1;
                op.in_shift = b, op.out_shift = op.pool ? b + 1 : b;
                op.in_buf = prev, op.out_buf = i;
                need += (size_t)op.cout * cin * 9 + op.cout;
                cin = op.cout, prev = i;
                if (op.pool) x_ch[b] = op.cout, x_buf[b] = i;
                plan.ops.push_back(op);
            }
        for (int d = 0; d < 5; ++d) {
            Op op;
            op.kind = OP_DECONV, op.cin = cin, op.cout = d < 4 ? x_ch[3 - d] : dec_last;
            op.in_shift = 5 - d, op.out_shift = 4 - d;
            op.in_buf = prev, op.out_buf = i, op.skip_buf = d < 4 ? x_buf[3 - d] : -1;
            need += (size_t)op.cout * cin * 9 + 5 * (size_t)op.cout;
            cin = op.cout, prev = i++;
            plan.ops.push_back(op);
        }
        Op op;
        op.kind = OP_CLASSIFY, op.cin = dec_last, op.cout = n_class, op.in_buf = prev, op.out_buf = i;
        need += (size_t)n_class * dec_last + n_class;
        plan.ops.push_back(op);
    }
    if (need != n_floats) return bad(err, "fcn: weights hold " + std::to_string(n_floats) + " floats, the description needs " + std::to_string(need));
    for (size_t e = 0; e < n_floats; ++e)
        if (!std::isfinite(W[e])) return bad(err, "fcn: non-finite weight at float " + std::to_string(e));

    const float* w = W;
    for (size_t i = 0; i < plan.ops.size(); ++i) {
        Op& op = plan.ops[i];
        const std::string what = "fcn: op " + std::to_string(i);
        op.cin_p = op.first ? 4 : rup(op.cin, 8);
        op.cout_p = op.kind == OP_CLASSIFY ? op.cout : rup(op.cout, 8);
        if (op.kind == OP_CLASSIFY) {
            op.macs_per_in_px = (double)op.cin * op.cout;
            op.bias_off = grow(plan.blob, (size_t)op.cin * op.cout * 4);
            std::memcpy(plan.blob.data() + op.bias_off, w, (size_t)op.cin * op.cout * 4);
            w += (size_t)op.cin * op.cout;
            op.scale_off = grow(plan.blob, (size_t)op.cout * 4);
            std::memcpy(plan.blob.data() + op.scale_off, w, (size_t)op.cout * 4);
            w += op.cout;
            continue;
        }
        const int NTall = rup(op.cout, 16) / 16;
        op.groups = (NTall + MAX_NT - 1) / MAX_NT;
        op.NT = (NTall + op.groups - 1) / op.groups;
        op.n_chunks = rup(op.cin, CK) / CK;
        op.macs_per_in_px = 9.0 * op.cin * op.cout;
        const size_t nw = (size_t)op.cout * op.cin * 9;
        const int n_par = op.kind == OP_DECONV ? 4 : 1;
        for (int par = 0; par < n_par; ++par) {
            const int rc = pack_frags(plan, op, w, op.kind == OP_DECONV, par, op.wfrag_off[par], err, what);
            if (rc != SD_OK) return rc;
        }
        w += nw;
        const size_t nb = (size_t)op.NT * op.groups * 16;
        op.bias_off = grow(plan.blob, nb * 4);
        std::memcpy(plan.blob.data() + op.bias_off, w, (size_t)op.cout * 4);
        w += op.cout;
        if (op.kind == OP_DECONV) {
            const float *gamma = w, *beta = w + op.cout, *mean = w + 2 * (size_t)op.cout, *var = w + 3 * (size_t)op.cout;
            op.scale_off = grow(plan.blob, nb * 4);
            op.shift_off = grow(plan.blob, nb * 4);
            float* sc = reinterpret_cast<float*>(plan.blob.data() + op.scale_off);
            float* sh = reinterpret_cast<float*>(plan.blob.data() + op.shift_off);
            for (int n = 0; n < op.cout; ++n) {
                if (!((double)var[n] + BN_EPS > 0)) return bad(err, what + ": BatchNorm running_var + eps is not positive");
                const double s = (double)gamma[n] / std::sqrt((double)var[n] + BN_EPS);
                sc[n] = (float)s, sh[n] = (float)((double)beta[n] - (double)mean[n] * s);
                if (!std::isfinite(sc[n]) || !std::isfinite(sh[n])) return bad(err, what + ": BatchNorm constants overflow float32");
            }
            w += 4 * (size_t)op.cout;
        }
    }
    plan.blob.resize(rup_sz(plan.blob.size(), 256), 0);
    return SD_OK;
}

int infer_shapes(const Plan& p, int H, int W, std::vector<Dims>& dims, std::string& err) {
    if (H < 32 || W < 32 || H > 16384 || W > 16384 || H % 32 || W % 32)
        return bad(err, "fcn: H and W must be multiples of 32 in 32 ... 16384 (the skip additions do not fit otherwise), got " + std::to_string(H) + " x " +
                            std::to_string(W));
    dims.clear();
    for (const Op& op : p.ops) dims.push_back({op.cout, op.cout_p, H >> op.out_shift, W >> op.out_shift});
    return SD_OK;
}

int workspace(const Plan& p, size_t n_planes, int H, int W, Workspace& ws, std::string& err) {
    std::vector<Dims> dims;
    const int rc = infer_shapes(p, H, W, dims, err);
    if (rc != SD_OK) return rc;
    if (n_planes < 1 || n_planes > ((size_t)1 << 24)) return bad(err, "fcn: n_planes out of range");
    ws = Workspace{};
    size_t off = 0;
    for (size_t i = 0; i + 1 < p.ops.size(); ++i) {
        ws.off.push_back(off);
        off += rup_sz(n_planes * dims[i].h * dims[i].w * dims[i].cp * 2, 256);
    }
    ws.total = off;
    return SD_OK;
}

double macs_per_view(const Plan& p, int H, int W) {
    std::vector<Dims> dims;
    std::string err;
    if (infer_shapes(p, H, W, dims, err) != SD_OK) return 0.0;
    double m = 0.0;
    for (const Op& op : p.ops) m += op.macs_per_in_px * (double)(H >> op.in_shift) * (W >> op.in_shift);
    return m;
}

}  // namespace sdfcn
