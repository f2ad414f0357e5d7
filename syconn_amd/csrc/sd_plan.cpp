// The host-only plan builder of the U-Net path (sd_plan.h): validation, BatchNorm folding, the six weight layouts of the blob,
// the fusion decisions, the workspace layout and the region-of-interest analysis.
#include "sd_plan.h"

#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

bool upconv_rows_kernel(int nchunk, int Cd) {
    const bool no_wl = sdplan::process_switches().no_upconv_wl;
    return (nchunk == 4 && Cd == 32) || (nchunk == 3 && Cd == 32) || (nchunk == 2 && Cd == 16) || (nchunk == 8 && Cd == 64 && !no_wl) ||
           (nchunk == 6 && Cd == 48) || (nchunk == 12 && Cd == 96 && !no_wl);
}

namespace sdplan {

PlanSwitches read_plan_switches() {
    auto on = [](const char* name) { return getenv(name) != nullptr; };
    return {on("SD_KEEP_ALL"), on("SD_NO_FUSE"), on("SD_NO_WS_REUSE"), on("SD_NO_FIRST_FUSE"), on("SD_NO_GN_FUSE"), on("SD_NO_GN_DEFER"),
            on("SD_NO_GN_POOL_RAW"), on("SD_SPLIT_NO_FINAL_FUSE"), on("SD_GN_SKIP_NOT_DEFERRED"), on("SD_NO_DEC0")};      // (member order)
}

const ProcessSwitches& process_switches() {
    static const ProcessSwitches s{getenv("SD_NO_NT3") != nullptr, getenv("SD_ROI_NO_DEC0") != nullptr,
                                   getenv("SD_ROI_NO_ENCODER") != nullptr, getenv("SD_NO_UPCONV_WL") != nullptr};
    return s;
}

namespace {

// float -> bf16 (round to nearest even) / fp16 bits
inline uint16_t f2bf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline uint16_t f2f16(float f) {
    _Float16 h = (_Float16)f;
    uint16_t b;
    std::memcpy(&b, &h, 2);
    return b;
}
inline uint16_t cvt(float f, int dtype) { return dtype == SD_BF16 ? f2bf16(f) : f2f16(f); }
inline float back(uint16_t bits, int dtype) {
    if (dtype == SD_BF16) { uint32_t u = (uint32_t)bits << 16; float f; std::memcpy(&f, &u, 4); return f; }
    _Float16 h; std::memcpy(&h, &bits, 2); return (float)h;
}

// f(0) .. f(n - 1) on up to 48 host threads (independent items writing disjoint memory)
template <class F>
void parallel_for(int n, F f) {
    const int nt = std::max(1, std::min({n, 48, (int)std::thread::hardware_concurrency()}));
    if (nt == 1) { for (int i = 0; i < n; ++i) f(i); return; }
    std::atomic<int> next{0};
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&] { for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) f(i); });
    for (auto& x : th) x.join();
}

// split-fp16 plan: power of two 2^k that brings the largest folded weight of the layer into [2^14, 2^15) -- the lo parts
// of all weights that matter are then normal fp16 numbers (hi + lo carries 22+ bits); bias and epilogue follow (exact)
float split_scale(float maxabs) {
    if (!(maxabs > 0.f) || !std::isfinite(maxabs)) return 1.f;
    const int k = std::max(-60, std::min(60, 14 - std::ilogb(maxabs)));
    return std::ldexp(1.f, k);
}
// element of virtual chunk `r` (0 .. 3n-1) of an n-chunk split input: planes [hi | hi | lo] meet weights [lo | hi | hi]
uint16_t split_part(float v, int r, int n) {
    const uint16_t hi = f2f16(v);
    return r >= n ? hi : f2f16(v - back(hi, SD_F16));
}

// The final layer's fp32 weights (times `scale`) as hi + lo parts of `dtype` in MFMA A-fragment order: [k-step][hi, lo][64 lanes]
// [8]; row = class (lane & 31).  Element jj of k-step s is the channel
//   natural order (k_final_mfma):         16 s + 8 (lane >> 5) + jj
//   blocked order (conv epilogue, dec0):  32 (s / 2) + 8 (2 (s & 1) + (jj >> 2)) + 4 (lane >> 5) + (jj & 3)
void pack_hilo_frags(uint16_t* fp, int nsteps, bool blocked, const sd_op_desc& fd, const float* W, int dtype, float scale) {
    for (int s = 0; s < nsteps; ++s)
        for (int l = 0; l < 64; ++l)
            for (int jj = 0; jj < 8; ++jj) {
                const int co = l & 31;
                const int ch = blocked ? (s / 2) * 32 + 8 * (2 * (s & 1) + (jj >> 2)) + 4 * (l >> 5) + (jj & 3)
                                       : s * SD_CHUNK + 8 * (l >> 5) + jj;
                const float wv = (co < fd.cout && ch < fd.cin0) ? W[fd.w_off + (size_t)co * fd.cin0 + ch] * scale : 0.f;
                const uint16_t hi = cvt(wv, dtype);
                fp[((size_t)(s * 2 + 0) * 64 + l) * 8 + jj] = hi;
                fp[((size_t)(s * 2 + 1) * 64 + l) * 8 + jj] = cvt(wv - back(hi, dtype), dtype);
            }
}

// One model under construction: the checked inputs, the plan being filled and the folded BatchNorm of the op at hand.
struct Builder {
    const float* W;
    size_t n_floats;
    Plan& P;
    std::vector<float> sc, sh;      // folded per-output-channel scale / shift of an eval-mode BatchNorm

    bool chk(int64_t off, size_t n) const { return off >= 0 && (size_t)off + n <= n_floats; }
    size_t alloc(size_t bytes) { size_t o = rup_sz(P.blob.size(), 256); P.blob.resize(o + bytes, 0); return o; }
    template <class T> T* at(size_t off) { return reinterpret_cast<T*>(P.blob.data() + off); }
    int pack_dtype() const { return P.split ? SD_F16 : P.act_dtype; }      // element type of the packed MFMA weight fragments
    float folded_bias(const sd_op_desc& d, int c) const { return W[d.b_off + c] * sc[c] + sh[c]; }

    bool fold_bn(const sd_op_desc& d, int cout) {
        sc.assign(cout, 1.f);
        sh.assign(cout, 0.f);
        if (d.norm != 1) return true;
        if (!chk(d.gamma_off, cout) || !chk(d.beta_off, cout) || !chk(d.mean_off, cout) || !chk(d.var_off, cout)) return false;
        for (int c = 0; c < cout; ++c) {
            const float s = W[d.gamma_off + c] / std::sqrt(W[d.var_off + c] + d.eps);
            sc[c] = s;
            sh[c] = W[d.beta_off + c] - W[d.mean_off + c] * s;
        }
        return true;
    }
    // folded weight of a convolution: PyTorch layout [cout][cin][kz][9]
    float wat(const sd_op_desc& d, int cin, int co, int ci, int kz, int t9) const {
        return W[d.w_off + ((size_t)co * cin + ci) * (d.kz * 9) + kz * 9 + t9] * sc[co];
    }

    bool other_reader(int buf, size_t from) const {
        for (size_t k = from; k < P.ops.size(); ++k)
            if (P.ops[k].d.src0 == buf || P.ops[k].d.src1 == buf) return true;
        return false;
    }
    // every add_* returns nullptr, or the reason the plan is invalid
    const char* add_conv(Op& op) {
        const sd_op_desc& d = op.d;
        if (d.ky != 3 || d.kx != 3 || (d.kz != 1 && d.kz != 3)) return "conv: only 3x3x3 and 1x3x3 kernels";
        if (d.src0 < 0 || d.dst <= 0 || d.cout <= 0) return "conv: bad buffer ids";
        const int cin = d.cin0 + (d.src1 >= 0 ? d.cin1 : 0);
        if (!chk(d.w_off, (size_t)d.cout * cin * d.kz * 9) || !chk(d.b_off, d.cout)) return "conv: weight offsets";
        if (!fold_bn(d, d.cout)) return "conv: norm offsets";
        P.bufC[d.dst] = d.cout;
        P.bufCp[d.dst] = rup(d.cout, SD_CHUNK);
        if (d.src0 == 0) {
            if (d.cin0 != 1 || d.src1 >= 0) return "first conv must have exactly one input channel";
            op.first = true;
            pack_first_f32(op);
            if (d.kz == 1 && !P.split) pack_first_u8(op);
            return nullptr;
        }
        if (P.bufC[d.src0] != d.cin0) return "conv: cin0 does not match producer of src0";
        if (d.src1 >= 0 && P.bufC[d.src1] != d.cin1) return "conv: cin1 does not match producer of src1";
        pack_conv(op);
        return nullptr;
    }

    // first convolution, exact-f32 MFMA chain: [ntile][nstep][64 lanes] floats, two taps per k-step
    void pack_first_f32(Op& op) {
        const sd_op_desc& d = op.d;
        const int taps = d.kz * 9;
        const int ntile = (P.bufCp[d.dst] + 31) / 32, nstep = (taps + 1) / 2;
        op.wpack_off = alloc((size_t)ntile * nstep * 64 * 4);
        op.bias_off = alloc((size_t)ntile * 32 * 4 + 16);
        float* wp = at<float>(op.wpack_off);
        float* bp = at<float>(op.bias_off);
        for (int nt = 0; nt < ntile; ++nt)
            for (int s = 0; s < nstep; ++s)
                for (int l = 0; l < 64; ++l) {
                    // (taps is odd: the last k slot of the MFMA chain is free and carries the folded BIAS -- the kernels feed it
                    // a 1.0, which makes the bias the last fma of the chain = the separate add it replaces, bit for bit)
                    const int n = nt * 32 + (l & 31), tap = 2 * s + (l >> 5);
                    wp[(nt * nstep + s) * 64 + l] = (n < d.cout && tap < taps) ? wat(d, 1, n, 0, tap / 9, tap % 9)
                                                    : (n < d.cout && tap == taps) ? folded_bias(d, n) : 0.f;
                }
        for (int n = 0; n < d.cout; ++n) bp[n] = folded_bias(d, n);
    }

    // uint8 input on the bf16 matrix pipe (k_conv_first / k_conv_mfma MODE 5): a uint8 voxel v is EXACT in bf16, so
    // conv(v / 255) = sum_t v_t * W'_t with W' = fp32(w / 255) carried as THREE bf16 parts (hi + mid + lo = all 24
    // mantissa bits; every product v * part is exact in fp32) -- 9 taps x 3 parts + 3 parts of the folded bias
    // (meeting a 1.0) are 30 of the 32 k slots of TWO v_mfma_f32_32x32x16_bf16 instead of five 64-cycle
    // v_mfma_f32_32x32x2_f32.  Slot order (what the kernels' B operand looks like): lanes 0-31 hold taps 0-4,
    // lanes 32-63 taps 5-8 and the constant; B dwords = [(t0,t0) (t1,t1) (t2,t2) (t3,t3)] [(t4,t4) (t0,t1) (t2,t3)
    // (t4,1)] with a dword (a,b) = k slots (2i, 2i+1): a pair (t,t) meets (hi, mid), the mixed pairs meet lo parts.
    void pack_first_u8(Op& op) {
        const sd_op_desc& d = op.d;
        const int ntile = (P.bufCp[d.dst] + 31) / 32;
        op.w3_off = alloc((size_t)ntile * 2 * 64 * 8 * 2);
        uint16_t* w3 = at<uint16_t>(op.w3_off);
        auto part3 = [](float v, uint16_t (&o)[3]) {
            float r = v;
            for (int k = 0; k < 3; ++k) {
                o[k] = f2bf16(r);
                r -= back(o[k], SD_BF16);      // exact
            }
        };
        for (int nt = 0; nt < ntile; ++nt)
            for (int l = 0; l < 64; ++l) {
                const int n = nt * 32 + (l & 31), hf = l >> 5;
                uint16_t tp[5][3] = {}, bpart[3] = {};
                if (n < d.cout) {
                    for (int a = 0; a < 5; ++a) {
                        const int tap = hf * 5 + a;
                        if (tap < 9) part3((float)((double)wat(d, 1, n, 0, 0, tap) / 255.0), tp[a]);
                    }
                    part3(folded_bias(d, n), bpart);
                }
                uint16_t* m0 = w3 + ((size_t)(nt * 2 + 0) * 64 + l) * 8;
                uint16_t* m1 = w3 + ((size_t)(nt * 2 + 1) * 64 + l) * 8;
                for (int a = 0; a < 4; ++a) { m0[2 * a] = tp[a][0]; m0[2 * a + 1] = tp[a][1]; }
                // the fifth read of the upper lanes is the constant (1.0, 1.0), and so is their last dword
                const uint16_t* fifth = hf == 0 ? tp[4] : bpart;
                m1[0] = fifth[0]; m1[1] = fifth[1];
                m1[2] = tp[0][2]; m1[3] = tp[1][2]; m1[4] = tp[2][2]; m1[5] = tp[3][2]; m1[6] = fifth[2]; m1[7] = 0;
            }
    }

    // convolution on the matrix cores: [nb][chunk][kz][9][NT][64 lanes][8] of the storage type
    void pack_conv(Op& op) {
        const sd_op_desc& d = op.d;
        const bool split = P.split;
        const int cin = d.cin0 + (d.src1 >= 0 ? d.cin1 : 0), taps = d.kz * 9;
        const int nch0 = P.bufCp[d.src0] / SD_CHUNK, nch1 = d.src1 >= 0 ? P.bufCp[d.src1] / SD_CHUNK : 0;
        const int ntile = (d.cout + 31) / 32;
        // output channels per workgroup: 64 (NT=2); 96 (NT=3) where that divides the layer without padding tiles
        // (the 48-filter family: 96/192/384/768 channels) -- a 64-wide split would spend 25 % of the MFMAs of a
        // 96-channel layer on zero columns; NT=3 also needs fewer LDS fragment reads per MFMA (5 per 6)
        op.NT = (ntile % 3 == 0 && !process_switches().no_nt3) ? 3 : (ntile >= 2 ? 2 : 1);
        op.NB = (ntile + op.NT - 1) / op.NT;
        const int m0 = split ? 3 : 1;      // (split-fp16 plan: virtual chunks)
        const int nchunks = (nch0 + nch1) * m0;
        float wscale = 1.f;
        if (split) {
            float mx = 0.f;
            for (int co = 0; co < d.cout; ++co)
                for (size_t k = 0; k < (size_t)cin * taps; ++k) mx = std::max(mx, std::fabs(W[d.w_off + (size_t)co * cin * taps + k] * sc[co]));
            wscale = split_scale(mx);
            op.oscale = 1.f / wscale;
        }
        const size_t gbytes = (size_t)9 * op.NT * 1024;
        op.wpack_off = alloc((size_t)op.NB * nchunks * d.kz * gbytes);
        op.bias_off = alloc((size_t)op.NB * op.NT * 32 * 4 + 16);
        uint16_t* wp = at<uint16_t>(op.wpack_off);
        float* bp = at<float>(op.bias_off);
        // (the packing of a 7.8 M-parameter net took 0.15 s on one core -- 15 % of a 1024 x 1024 x 256 file-system-mode job:
        // the (block, chunk) groups are independent)
        parallel_for(op.NB * nchunks, [&](int g0) {
            const int nb = g0 / nchunks, c = g0 % nchunks;
            const bool s0 = c < nch0 * m0;
            const int r = s0 ? c : c - nch0 * m0, nsrc = s0 ? nch0 : nch1;       // chunk within its source
            // weight groups in the order the kernel's stages read them: [kz][9 taps (ky, kx)]; 3x3x3 layers with NT <= 2 (ZROLL in
            // sd_conv_mfma.h): [stage ky][step (kx, kz)] -- those outputs are summed in the order (chunk, ky, kx, kz)
            for (int kz = 0; kz < d.kz; ++kz)
                for (int t9 = 0; t9 < 9; ++t9)
                    for (int j = 0; j < op.NT; ++j)
                        for (int l = 0; l < 64; ++l)
                            for (int e = 0; e < 8; ++e) {
                                const int n = (nb * op.NT + j) * 32 + (l & 31);
                                const int k = (r % nsrc) * SD_CHUNK + (l >> 5) * 8 + e;
                                // index into the concatenated weight input-channel axis
                                const int ci = s0 ? (k < d.cin0 ? k : -1) : (k < d.cin1 ? d.cin0 + k : -1);
                                // (ZROLL layers: group index `kz` and in-group index `t9` name the tap (kz, ky, kx) = (t9 % 3, kz, t9 / 3))
                                const float v = (n < d.cout && ci >= 0) ? (d.kz == 3 && op.NT != 3 ? wat(d, cin, n, ci, t9 % 3, kz * 3 + t9 / 3) : wat(d, cin, n, ci, kz, t9)) * wscale : 0.f;
                                const size_t idx = ((((((size_t)nb * nchunks + c) * d.kz + kz) * 9 + t9) * op.NT + j) * 64 + l) * 8 + e;
                                wp[idx] = split ? split_part(v, r, nsrc) : cvt(v, P.act_dtype);
                            }
        });
        for (int n = 0; n < d.cout; ++n) bp[n] = folded_bias(d, n) * wscale;
    }

    // up-convolution: [nb][chunk][NT=2][64 lanes][8]; column n = tap * Cd + co
    const char* add_upconv(Op& op) {
        const sd_op_desc& d = op.d;
        const bool split = P.split;
        if (d.src0 <= 0 || d.dst <= 0 || (d.kz != 1 && d.kz != 2)) return "upconv: bad arguments";
        if (P.bufC[d.src0] != d.cin0) return "upconv: cin0 does not match producer";
        const int taps = d.kz * 4;
        if (!chk(d.w_off, (size_t)d.cin0 * d.cout * taps) || !chk(d.b_off, d.cout)) return "upconv: weight offsets";
        if (!fold_bn(d, d.cout)) return "upconv: norm offsets";
        const int Cd = rup(d.cout, SD_CHUNK);
        P.bufC[d.dst] = d.cout;
        P.bufCp[d.dst] = Cd;
        const int ntot = taps * Cd;
        op.NT = 2;
        op.NB = (ntot + 63) / 64;
        const int nreal = P.bufCp[d.src0] / SD_CHUNK;
        const int nchunk = nreal * (split ? 3 : 1);      // (split-fp16 plan: virtual chunks)
        const float* w = W + d.w_off;
        float wscale = 1.f;
        if (split) {
            float mx = 0.f;
            for (int ci = 0; ci < d.cin0; ++ci)
                for (int co = 0; co < d.cout; ++co)
                    for (int t = 0; t < taps; ++t) mx = std::max(mx, std::fabs(w[((size_t)ci * d.cout + co) * taps + t] * sc[co]));
            wscale = split_scale(mx);
            op.oscale = 1.f / wscale;
        }
        op.wpack_off = alloc((size_t)op.NB * nchunk * 2 * 64 * 8 * 2);
        op.bias_off = alloc((size_t)op.NB * 64 * 4 + 16);
        uint16_t* wp = at<uint16_t>(op.wpack_off);
        float* bp = at<float>(op.bias_off);
        for (int nb = 0; nb < op.NB; ++nb)
            for (int c = 0; c < nchunk; ++c)
                for (int j = 0; j < 2; ++j)
                    for (int l = 0; l < 64; ++l)
                        for (int e = 0; e < 8; ++e) {
                            const int n = (nb * 2 + j) * 32 + (l & 31);
                            const int tap = n / Cd, co = n % Cd;
                            const int ci = (c % nreal) * SD_CHUNK + (l >> 5) * 8 + e;
                            float v = 0.f;
                            if (tap < taps && co < d.cout && ci < d.cin0) v = w[((size_t)ci * d.cout + co) * taps + tap] * sc[co] * wscale;
                            wp[((((size_t)nb * nchunk + c) * 2 + j) * 64 + l) * 8 + e] = split ? split_part(v, c, nreal) : cvt(v, P.act_dtype);
                        }
        for (int n = 0; n < ntot; ++n) {
            const int co = n % Cd;
            bp[n] = co < d.cout ? folded_bias(d, co) * wscale : 0.f;
        }
        return nullptr;
    }

    // GroupNorm: gamma[Cp] then beta[Cp], floats
    const char* add_groupnorm(Op& op) {
        const sd_op_desc& d = op.d;
        if (d.src0 <= 0 || d.groups <= 0) return "groupnorm: bad arguments";
        const int C = P.bufC[d.src0], Cp = P.bufCp[d.src0];
        if (C % d.groups) return "groupnorm: channels not divisible by groups";
        if ((size_t)Cp * 16 > SD_GN_SCALE_OFF || SD_GN_SCALE_OFF + (size_t)Cp * 8 > WS_SCRATCH) return "groupnorm: too many channels";
        if (!chk(d.gamma_off, C) || !chk(d.beta_off, C)) return "groupnorm: offsets";
        op.aux_off = alloc((size_t)2 * Cp * 4);
        float* gp = at<float>(op.aux_off);
        for (int c = 0; c < C; ++c) { gp[c] = W[d.gamma_off + c]; gp[Cp + c] = W[d.beta_off + c]; }
        return nullptr;
    }

    // final 1x1x1 layer: fp32 weights [8][Cs], bias [8], and the same weights as hi + lo fragments in natural channel order
    const char* add_final(Op& op) {
        const sd_op_desc& d = op.d;
        if (d.src0 <= 0 || d.cout <= 0 || d.cout > 8) return "final conv: 1..8 output classes supported";
        if (P.bufC[d.src0] != d.cin0) return "final: cin0 does not match producer";
        if (!chk(d.w_off, (size_t)d.cout * d.cin0) || !chk(d.b_off, d.cout)) return "final: weight offsets";
        const int Cs = P.bufCp[d.src0];
        op.wpack_off = alloc((size_t)8 * Cs * 4);
        op.bias_off = alloc(8 * 4);
        float* wp = at<float>(op.wpack_off);
        float* bp = at<float>(op.bias_off);
        for (int co = 0; co < d.cout; ++co) {
            for (int ci = 0; ci < d.cin0; ++ci) wp[co * Cs + ci] = W[d.w_off + (size_t)co * d.cin0 + ci];
            bp[co] = W[d.b_off + co];
        }
        const int nch = Cs / SD_CHUNK;
        op.aux_off = alloc((size_t)nch * 2 * 64 * 8 * 2);
        pack_hilo_frags(at<uint16_t>(op.aux_off), nch, false, d, W, pack_dtype(), 1.f);
        P.final_cout = d.cout;
        return nullptr;
    }

    const char* add(Op& op) {
        const sd_op_desc& d = op.d;
        switch (d.kind) {
        case SD_OP_CONV: return add_conv(op);
        case SD_OP_POOL:
            if (d.src0 <= 0 || d.dst <= 0 || (d.kz != 1 && d.kz != 2)) return "pool: bad arguments";
            P.bufC[d.dst] = P.bufC[d.src0];
            P.bufCp[d.dst] = P.bufCp[d.src0];
            return nullptr;
        case SD_OP_UPCONV: return add_upconv(op);
        case SD_OP_GROUPNORM: return add_groupnorm(op);
        case SD_OP_FINAL: return add_final(op);
        default: return "unknown op kind";
        }
    }

    // ---- fusions: one pass for both plan families; where the split-fp16 plan differs, the condition says so ----------------------

    // first conv (1 -> 32 / 48, 1x3x3) -> conv (1x3x3) of one input: the second conv computes its halo of the first conv's output on
    // the fly -- the split plan as hi / lo planes (k_conv_mfma MODE 4).  Decided per launch: only the resident-weight form of the
    // kernel can do it.
    void fuse_first(const PlanSwitches& sw) {
        if (sw.no_first_fuse) return;
        for (size_t i = 0; i + 1 < P.ops.size(); ++i) {
            const Op& f = P.ops[i];
            Op& c = P.ops[i + 1];
            // (17 ... 32 / 33 ... 48 filters: padding channels have zero weights and bias; the split kernel serves 32 only)
            const int Cf = f.first ? P.bufCp[f.d.dst] : 0;
            const bool width_ok = Cf == 32 || (Cf == 48 && !P.split);
            if (f.d.kind == SD_OP_CONV && f.first && f.d.kz == 1 && width_ok && c.d.kind == SD_OP_CONV && !c.first && c.d.kz == 1 &&
                c.d.src0 == f.d.dst && c.d.src1 < 0 && !other_reader(f.d.dst, i + 2))
                c.fuse_first = (int)i;
        }
    }

    // can reader `r` (op k) of buffer b apply the scale / shift table of GroupNorm `g` itself?
    bool reader_applies_gn(const Op& g, const Op& r, size_t k, int b, const PlanSwitches& sw) const {
        if (r.d.kind == SD_OP_FINAL) return true;
        if (P.split) return false;      // split plan: only k_final_split applies a table (in fp32 on the exact values it reads anyway)
        switch (r.d.kind) {
        case SD_OP_CONV: return !r.first && P.bufCp[b] <= 256;      // LDS table: 128 B per 16 channels and tile
        case SD_OP_UPCONV:      // only the row kernel absorbs the apply cheaply; else keep the pass
            return upconv_rows_kernel(P.bufCp[b] / SD_CHUNK, rup(r.d.cout, SD_CHUNK));
        case SD_OP_POOL: return g.gn_pool == (int)k;
        case SD_OP_GROUPNORM:      // src1 of a GroupNorm only lends its extents (crop region); another GroupNorm of the buffer: no
            return r.d.src0 != b && !sw.gn_skip_not_deferred;
        default: return false;
        }
    }

    // Deferred GroupNorm apply: the op only turns the statistics into a scale / shift table; the tensor stays raw and
    // every reader normalises on the fly (convolutions in their LDS halo, up-convolutions and the final layer on their
    // register fragments, a pooling fused into the GroupNorm op writes the normalised pooled tensor only) -- the
    // normalised tensor is never written nor re-read.  Possible when every later reader of the buffer is such an op.
    void defer_groupnorms(const PlanSwitches& sw) {
        // (SD_NO_GN_FUSE: the split plan's deferral does not hang on the statistics fusion)
        if (sw.no_gn_defer || sw.keep_all || (sw.no_gn_fuse && !P.split)) return;
        for (size_t i = 0; i < P.ops.size(); ++i) {
            Op& g = P.ops[i];
            if (g.d.kind != SD_OP_GROUPNORM) continue;
            const int b = g.d.src0;
            bool ok = true, any = false;
            for (size_t k = i + 1; k < P.ops.size() && ok; ++k) {
                const Op& r = P.ops[k];
                if (r.d.src0 != b && r.d.src1 != b) continue;
                any = true;
                ok = reader_applies_gn(g, r, k, b, sw);
            }
            if (ok && any) { g.gn_defer = true; P.buf_gn[b] = (int)i; }
        }
        for (int b = 1; b < P.nbuf; ++b)
            if (P.buf_gn[b] >= 0) {
                P.gn_tab_off[b] = P.ws_base;
                P.ws_base += rup_sz((size_t)2 * P.bufCp[b] * 4, 256);
            }
    }

    // conv i with fused statistics of GroupNorm i + 1, which is deferred and feeds the pooling i + 2: the conv also pools its RAW
    // output (per channel the window's maximum or, for gamma < 0, minimum: relu(a x + b) is monotone in x) and the readers of the
    // pooled tensor apply the scale / shift table like the readers of the full-resolution one: the apply + pool pass disappears.
    // Needs the deferred-input kernel form (MODE 2 carries the epilogue) and deferral-capable readers.
    void fuse_pool_raw(size_t i) {
        Op& c = P.ops[i];
        Op& g = P.ops[i + 1];
        const Op& po = P.ops[i + 2];
        const int pb = po.d.dst;
        bool ok = (c.d.kz == 3) == (po.d.kz == 2) && P.bufCp[pb] <= 256 &&
                  (P.buf_gn[c.d.src0] >= 0 || (c.d.src1 >= 0 && P.buf_gn[c.d.src1] >= 0));
        for (size_t k = i + 3; k < P.ops.size() && ok; ++k) {
            const Op& r = P.ops[k];
            if (r.d.src0 != pb && r.d.src1 != pb) continue;
            if (r.d.kind == SD_OP_CONV) ok = !r.first;
            else if (r.d.kind == SD_OP_UPCONV) ok = upconv_rows_kernel(P.bufCp[pb] / SD_CHUNK, rup(r.d.cout, SD_CHUNK));
            else ok = r.d.kind == SD_OP_FINAL || (r.d.kind == SD_OP_GROUPNORM && r.d.src0 != pb);
        }
        if (!ok) return;
        c.fuse_pool_raw = (int)i + 2;
        g.pool_in_conv = true;
        P.buf_gn[pb] = (int)i + 1;
        P.gn_tab_off[pb] = P.gn_tab_off[g.d.src0];      // one table for the tensor and its pooled version
        const int ntile = c.NT * c.NB;
        c.pooldir_off = alloc((size_t)ntile * 2 * 8 * 4);
        uint32_t* dq = at<uint32_t>(c.pooldir_off);
        // register r = 4 s + t of lane half h holds the channels 32 tile + 16 s + 8 (t >> 1) + 4 h + 2 (t & 1) + {0, 1}
        for (int tile = 0; tile < ntile; ++tile)
            for (int h = 0; h < 2; ++h)
                for (int r = 0; r < 8; ++r) {
                    uint32_t w = 0;
                    for (int e = 0; e < 2; ++e) {
                        const int ch = 32 * tile + 16 * (r >> 2) + 8 * ((r & 3) >> 1) + 4 * h + 2 * (r & 1) + e;
                        if (ch < P.bufC[g.d.src0] && W[g.d.gamma_off + ch] < 0.f) w |= 0xffffu << (16 * e);
                    }
                    dq[(tile * 2 + h) * 8 + r] = w;
                }
    }

    // the final 1x1x1 behind the last convolution, in its epilogue: fp32 weights as hi + lo fragments of the storage type in blocked
    // channel order (pack_hilo_frags); the split plan scales them by a power of two like every layer's weights
    void fuse_final(size_t i) {
        Op& c = P.ops[i];
        Op& fo = P.ops[i + 1];
        c.fuse_final = (int)(i + 1);
        fo.skipped = true;
        float fscale = 1.f;
        if (P.split) {
            float mx = 0.f;
            for (size_t k = 0; k < (size_t)fo.d.cout * fo.d.cin0; ++k) mx = std::max(mx, std::fabs(W[fo.d.w_off + k]));
            fscale = split_scale(mx);
            c.final_oscale = 1.f / fscale;
        }
        c.fwfrag_off = alloc((size_t)c.NT * 2 * 2 * 64 * 8 * 2);
        pack_hilo_frags(at<uint16_t>(c.fwfrag_off), c.NT * 2, true, fo.d, W, pack_dtype(), fscale);
    }

    // Level-0 decoder as one streaming launch: planar up-convolution 64 -> 32, merge conv (32 + 32 -> 32), conv 32 -> 32
    // with the fused final layer, all with folded BatchNorm + ReLU (no GroupNorm between them) and no other reader of
    // the two intermediate tensors.
    void fuse_dec0() {
        const std::vector<int>& Cp = P.bufCp;
        for (size_t i = 0; i + 3 < P.ops.size(); ++i) {
            Op& u = P.ops[i];
            Op& c1 = P.ops[i + 1];
            Op& c2 = P.ops[i + 2];
            if (u.d.kind != SD_OP_UPCONV || u.d.kz != 1 || !u.d.relu || Cp[u.d.src0] != 64 || Cp[u.d.dst] != 32) continue;
            if (c1.d.kind != SD_OP_CONV || c1.first || c1.d.kz != 1 || !c1.d.relu || c1.d.src0 != u.d.dst || c1.d.src1 < 0 ||
                Cp[c1.d.src1] != 32 || Cp[c1.d.dst] != 32 || c1.NT != 1 || c1.NB != 1 || c1.fuse_gn >= 0 ||
                c1.fuse_pool >= 0 || c1.fuse_final >= 0)
                continue;
            if (c2.d.kind != SD_OP_CONV || c2.d.kz != 1 || !c2.d.relu || c2.d.src0 != c1.d.dst || c2.d.src1 >= 0 ||
                Cp[c2.d.dst] != 32 || c2.NT != 1 || c2.NB != 1 || c2.fuse_final != (int)i + 3)
                continue;
            if (P.buf_gn[u.d.src0] >= 0 || P.buf_gn[c1.d.src1] >= 0) continue;
            bool other = false;
            for (size_t k = 0; k < P.ops.size(); ++k) {
                const sd_op_desc& r = P.ops[k].d;
                if (k != i + 1 && (r.src0 == u.d.dst || r.src1 == u.d.dst)) other = true;
                if (k != i + 2 && (r.src0 == c1.d.dst || r.src1 == c1.d.dst)) other = true;
            }
            if (other) continue;
            u.dec0_c1 = (int)i + 1; u.dec0_c2 = (int)i + 2;
            c1.in_dec0 = c2.in_dec0 = true;      // (skipped per launch: dec0_shape_ok)
        }
    }

    // epilogue fusions (SD_NO_FUSE=1 keeps every layer a separate launch, for layer-wise debugging)
    void fuse(const PlanSwitches& sw) {
        const bool split = P.split;
        std::vector<Op>& ops = P.ops;
        fuse_first(sw);
        // GroupNorm (whole buffer) directly followed by the pooling of its output: one pass
        for (size_t i = 0; i + 1 < ops.size() && !sw.no_gn_fuse; ++i) {
            Op& g = ops[i];
            Op& nx = ops[i + 1];
            if (g.d.kind == SD_OP_GROUPNORM && g.d.src1 < 0 && nx.d.kind == SD_OP_POOL && nx.d.src0 == g.d.src0) {
                g.gn_pool = (int)(i + 1);
                nx.skipped = true;
            }
        }
        defer_groupnorms(sw);
        for (size_t i = 0; i + 1 < ops.size(); ++i) {
            Op& c = ops[i];
            Op& nx = ops[i + 1];
            if (c.d.kind != SD_OP_CONV || c.first || nx.d.src0 != c.d.dst) continue;
            // GroupNorm right behind a conv over the conv's whole output: statistics in the conv epilogue (split plan: the kernel
            // forms with two or more column tiles carry that epilogue)
            const bool stats_form = !split || c.NT >= 2;
            if (nx.d.kind == SD_OP_GROUPNORM && nx.d.src1 < 0 && !sw.no_gn_fuse && stats_form) {
                c.fuse_gn = (int)(i + 1);
                nx.stats_done = true;
                // (raw pooling: the deferred-input kernel form, which the split plan does not have)
                if (!split && nx.gn_defer && nx.gn_pool == (int)i + 2 && !sw.no_gn_pool_raw) fuse_pool_raw(i);
                continue;
            }
            // the pooling behind a convolution runs in that convolution's epilogue.  The fused pooling maximum works on the packed,
            // rounded outputs as integers: exact behind a ReLU only; the split plan pools the fp32 values, any sign
            const bool pool_sign_ok = split || c.d.relu;
            // the split plan has the final epilogue in its planar kernel only
            const bool final_form = !split || (c.d.kz == 1 && !sw.split_no_final_fuse);
            if (nx.d.kind == SD_OP_POOL && (c.d.kz == 3) == (nx.d.kz == 2) && pool_sign_ok) {
                c.fuse_pool = (int)(i + 1);
                nx.skipped = true;
            } else if (nx.d.kind == SD_OP_FINAL && c.NB == 1 && i + 2 == ops.size() && final_form) {
                fuse_final(i);
            }
        }
        if (!split && !sw.keep_all && !sw.no_dec0) fuse_dec0();
    }
};

}  // namespace

int build_plan(const sd_op_desc* ops, int n_ops, const float* W, size_t n_floats, int act_dtype, const PlanSwitches& sw, Plan& plan,
               std::string& err) {
    plan = Plan{};
    plan.act_dtype = act_dtype;
    plan.split = act_dtype == SD_F16X2;
    plan.keep_all = sw.keep_all;
    plan.ws_reuse = !sw.keep_all && !sw.no_fuse && !sw.no_ws_reuse;
    int nbuf = 1;
    for (int i = 0; i < n_ops; ++i) nbuf = std::max(nbuf, std::max(ops[i].src0, std::max(ops[i].src1, ops[i].dst)) + 1);
    plan.nbuf = nbuf;
    plan.bufC.assign(nbuf, 0);
    plan.bufCp.assign(nbuf, 0);
    plan.bufC[0] = 1;
    plan.bufCp[0] = 1;
    Builder b{W, n_floats, plan, {}, {}};
    for (int i = 0; i < n_ops; ++i) {
        Op op;
        op.d = ops[i];
        if (const char* why = b.add(op)) { err = why; return SD_ERR_INVALID; }
        plan.ops.push_back(op);
    }
    if (plan.ops.empty() || plan.ops.back().d.kind != SD_OP_FINAL) { err = "the plan must end with SD_OP_FINAL"; return SD_ERR_INVALID; }
    plan.buf_gn.assign(nbuf, -1);
    plan.gn_tab_off.assign(nbuf, 0);
    plan.ws_base = WS_SCRATCH;
    if (!sw.no_fuse) b.fuse(sw);
    return SD_OK;
}

// ---- shapes and workspace of one tile ------------------------------------------------------------------------------------------

// shapes the fused level-0 decoder serves (sd_dec0.hip: cursor arithmetic) and is worth it for: it walks x-strips of 64
// columns at the cost of full strips, so a width that fills its last strip badly is faster layer by layer (measured: 66
// columns = 2 strips at 52 % -> 0.26 vs 0.21 ms; 331 columns = 6 strips at 86 % -> 1.24 vs 1.36 ms).  Others run the layers.
// (ONE predicate for plan_workspace, the forward pass and launch_dec0: the kernel's own limits -- 32-bit stream positions, 24-bit
// row arithmetic, H >= 8 for the cursor wraps -- are part of it, so a shape that passes here never fails in the launcher after
// the intermediate buffers have been dropped from the workspace)
bool dec0_shape_ok(const Dims& o) {
    // (strips of 56 columns where they cover the width with fewer stream positions -- launch_dec0 picks; the fill rule
    // counts positions: strips x (width + 4), 68 per 64-column strip)
    const long cost = std::min<long>((long)((o.w + 63) / 64) * 68, (long)((o.w + 55) / 56) * 60);
    const long hp = 2 * (o.h / 2 + 1);
    return o.h >= 8 && (long)o.d * o.h < (1l << 24) && o.w < (1 << 24) && (long)o.d * hp * 68 <= (1l << 30) &&
           (long)o.d * o.h * o.w < (1l << 31) && (long)o.w * 10 * 68 >= cost * 64 * 7;
}

// the sub-box the fused level-0 decoder computes for the model's output box of interest: two voxel shells wider in y / x (its two
// 3x3 convolutions zero-pad at the box border), starting on even y / x (the level-1 tensor is addressed at half resolution)
Box dec0_view(const Roi& roi, const Dims& o) {
    Box v;
    const int n[3] = {o.d, o.h, o.w};
    v.any = false;
    for (int a = 0; a < 3; ++a) {
        const int r = a == 0 ? 0 : 2;
        v.lo[a] = std::max(0, roi.lo[a] - r);
        if (a > 0) v.lo[a] &= ~1;
        v.hi[a] = std::min(n[a], roi.hi[a] + r);
        v.any |= v.lo[a] > 0 || v.hi[a] < n[a];
    }
    return v;
}

// with an output box of interest the fused level-0 decoder runs on its sub-box if that is a shape it serves; else its layers
// run one by one on theirs
bool use_dec0(const Roi& roi, const Dims& o) {
    if (!dec0_shape_ok(o)) return false;
    if (!roi.set) return true;
    if (process_switches().roi_no_dec0) return false;
    for (int a = 0; a < 3; ++a)
        if (roi.lo[a] < 0 || roi.hi[a] > (a == 0 ? o.d : a == 1 ? o.h : o.w) || roi.lo[a] >= roi.hi[a]) return false;
    const Box v = dec0_view(roi, o);
    return dec0_shape_ok(Dims{v.hi[0] - v.lo[0], v.hi[1] - v.lo[1], v.hi[2] - v.lo[2]});
}

size_t place_buffers(const std::vector<int>& first, const std::vector<int>& last, const std::vector<size_t>& bytes, size_t base,
                     bool reuse, std::vector<size_t>& off) {
    const int nb = (int)bytes.size();
    off.assign(nb, 0);
    if (!reuse) {
        size_t cur = base;
        for (int b = 1; b < nb; ++b) { off[b] = cur; cur += bytes[b]; }
        return cur;
    }
    std::vector<int> order;
    for (int b = 1; b < nb; ++b)
        if (last[b] >= 0 && bytes[b]) order.push_back(b);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return first[a] != first[b] ? first[a] < first[b] : a < b; });
    std::vector<int> placed;
    size_t top = base;
    for (int b : order) {
        // candidate offsets: the base and the end of every placed buffer that is alive at the same time
        std::vector<std::pair<size_t, size_t>> busy;      // [begin, end) ranges this buffer must avoid
        for (int q : placed)
            if (first[q] <= last[b] && first[b] <= last[q]) busy.push_back({off[q], off[q] + bytes[q]});
        std::sort(busy.begin(), busy.end());
        size_t cur = base;
        for (const auto& r : busy) {
            if (cur + bytes[b] <= r.first) break;
            cur = std::max(cur, r.second);
        }
        off[b] = cur;
        top = std::max(top, cur + bytes[b]);
        placed.push_back(b);
    }
    return top;
}

void plan_lifetimes(const Plan& p, bool dec0, std::vector<int>& first, std::vector<int>& last) {
    const int nops = (int)p.ops.size();
    first.assign(p.nbuf, nops);
    last.assign(p.nbuf, -1);
    auto touch_w = [&](int b, int i) { if (b > 0) { first[b] = std::min(first[b], i); last[b] = std::max(last[b], i); } };
    auto touch_r = [&](int b, int i) { if (b > 0) last[b] = std::max(last[b], i); };
    for (int i = 0; i < nops; ++i) {
        const Op& op = p.ops[i];
        const sd_op_desc& d = op.d;
        if (op.in_dec0 && dec0) continue;               // runs inside the up-convolution's launch, writes no buffer
        if (op.dec0_c1 >= 0 && dec0) {                  // reads the level-1 tensor and the skip tensor, writes the network output
            touch_r(d.src0, i);
            touch_r(p.ops[op.dec0_c1].d.src1, i);
            continue;
        }
        touch_r(d.src0, i);
        touch_r(d.src1, i);
        if (d.kind != SD_OP_FINAL) touch_w(d.dst, i);
        // outputs of ops executed inside this op's launch are written NOW, not at their own position in the plan
        if (op.fuse_pool >= 0) touch_w(p.ops[op.fuse_pool].d.dst, i);
        if (op.gn_pool >= 0) touch_w(p.ops[op.gn_pool].d.dst, i);
        if (op.fuse_pool_raw >= 0) touch_w(p.ops[op.fuse_pool_raw].d.dst, i);
        // a first convolution computed inside its consumer may also run as its own launch (decided per launch)
    }
}

// Workspace layout for one tile.  Every activation buffer lives from the op that writes it to the last op that reads
// it; buffers whose lifetimes do not overlap share memory (first-fit over the buffers in order of their first write).
// A U-Net keeps only the encoder skip tensors alive across the bottleneck, so a 178x243x331 reference-geometry tile needs
// about a third of the sum of all activations -- which is what lets several such tiles run in one launch set.
// `ws_reuse == false` (SD_KEEP_ALL / SD_NO_FUSE / SD_NO_WS_REUSE: layer-wise debugging reads buffers back after the
// forward) gives every buffer its own range.
size_t plan_workspace(const Plan& p, const std::vector<Dims>& dims, const Roi& roi, std::vector<size_t>& off) {
    std::vector<size_t> bytes(p.nbuf, 0);
    for (int b = 1; b < p.nbuf; ++b) bytes[b] = rup_sz((size_t)dims[b].d * dims[b].h * dims[b].w * p.bufCp[b] * (p.split ? 4 : 2), 256);
    std::vector<int> first, last;
    plan_lifetimes(p, use_dec0(roi, dims[0]), first, last);
    // (ws_base: behind the statistics scratch + the scale / shift tables of deferred GroupNorm applies)
    return place_buffers(first, last, bytes, p.ws_base, p.ws_reuse, off);
}

// ---- output box of interest: which sub-box every decoder op computes -----------------------------------------------------------
// need[b] = the part of buffer b that must hold CORRECT values; an op that can work on a sub-box computes view = need[dst]
// widened by its kernel radius (clipped to the tensor): the kernel zero-pads at the view's border, so the outermost shell of
// the view is wrong where that border is not the tensor's -- it lies outside need[dst] by construction, and everything it
// reads is real data (need[src] = view), so no uninitialised value is ever touched.  Ops that cannot (first conv, fused
// pooling / statistics, separate pooling / final / GroupNorm launches) compute everything and need everything.
namespace {

struct Needs {
    const std::vector<Dims>& dims;
    std::vector<Box> need;      // any == false: nothing needed yet
    void extents(int b, int* n) const { n[0] = dims[b].d; n[1] = dims[b].h; n[2] = dims[b].w; }
    void add(int b, const Box& x) {
        if (b <= 0) return;
        Box& t = need[b];
        for (int a = 0; a < 3; ++a) {
            t.lo[a] = t.any ? std::min(t.lo[a], x.lo[a]) : x.lo[a];
            t.hi[a] = t.any ? std::max(t.hi[a], x.hi[a]) : x.hi[a];
        }
        t.any = true;
    }
    void add_full(int b) {
        if (b > 0) add(b, Box{{0, 0, 0}, {dims[b].d, dims[b].h, dims[b].w}, true});
    }
};

// the view of convolution `op` (not the first): any == false if it computes its whole output
Box conv_view(const Plan& p, const Op& op, const Roi& roi, const Needs& N) {
    const sd_op_desc& d = op.d;
    Box c{{0, 0, 0}, {0, 0, 0}, false};
    if (op.fuse_final >= 0) { for (int a = 0; a < 3; ++a) { c.lo[a] = roi.lo[a]; c.hi[a] = roi.hi[a]; } c.any = true; }
    else c = N.need[d.dst];
    int n[3];
    N.extents(d.dst, n);
    // fused MaxPool (1,2,2) / (2,2,2) behind a planar / 3x3x3 convolution: what the pooled tensor is needed for, in
    // this convolution's coordinates
    const int kzp = d.kz == 3 ? 2 : 1;
    if (op.fuse_pool >= 0 && N.need[p.ops[op.fuse_pool].d.dst].any) {
        const Box& q = N.need[p.ops[op.fuse_pool].d.dst];
        const int f[3] = {kzp, 2, 2};
        Box up; up.any = true;
        for (int a = 0; a < 3; ++a) { up.lo[a] = q.lo[a] * f[a]; up.hi[a] = std::min(n[a], q.hi[a] * f[a]); }
        if (c.any) for (int a = 0; a < 3; ++a) { c.lo[a] = std::min(c.lo[a], up.lo[a]); c.hi[a] = std::max(c.hi[a], up.hi[a]); }
        else c = up;
    }
    // in y / x only plain convolutions work on a sub-box; along z also those with fused pooling or the first
    // convolution inside (a z-range is a shift of every base pointer: planes are never addressed through the extent)
    const bool yx = op.fuse_pool < 0 && op.fuse_pool_raw < 0 && op.fuse_gn < 0 && op.fuse_first < 0;
    const bool zok = op.fuse_pool_raw < 0 && op.fuse_gn < 0 && (yx || !process_switches().roi_no_encoder);
    Box v{{0, 0, 0}, {0, 0, 0}, false};
    if (!c.any || !zok) return v;
    const int r[3] = {d.kz / 2, 1, 1};
    for (int a = 0; a < 3; ++a) {
        v.lo[a] = (a == 0 || yx) ? std::max(0, c.lo[a] - r[a]) : 0;
        v.hi[a] = (a == 0 || yx) ? std::min(n[a], c.hi[a] + r[a]) : n[a];
    }
    if (op.fuse_pool >= 0 && kzp == 2) {      // whole pooling windows: an even start, an even end (or the tensor's own)
        v.lo[0] &= ~1;
        v.hi[0] = std::min(n[0], (v.hi[0] + 1) & ~1);
    }
    for (int a = 0; a < 3; ++a) v.any |= v.lo[a] > 0 || v.hi[a] < n[a];
    return v;
}

}  // namespace

std::vector<Box> plan_views(const Plan& p, const std::vector<Dims>& dims, const Roi& roi, bool dec0) {
    const size_t nops = p.ops.size();
    std::vector<Box> view(nops, Box{{0, 0, 0}, {0, 0, 0}, false});          // any == false: the whole tensor
    bool has_gn = false;
    for (const Op& op : p.ops) has_gn |= op.d.kind == SD_OP_GROUPNORM;
    if (!roi.set || has_gn || p.keep_all) return view;
    Needs N{dims, std::vector<Box>(p.nbuf, Box{{0, 0, 0}, {0, 0, 0}, false})};
    for (size_t k = nops; k-- > 0;) {
        const Op& op = p.ops[k];
        const sd_op_desc& d = op.d;
        if (op.skipped || (op.in_dec0 && dec0)) continue;
        if (d.kind == SD_OP_UPCONV && op.dec0_c1 >= 0 && dec0) {      // the fused level-0 decoder on its sub-box
            const int skip = p.ops[op.dec0_c1].d.src1;
            const Box v = dec0_view(roi, dims[skip]);
            if (v.any) {
                view[k] = v;
                N.add(skip, v);
                Box l; l.any = true;
                for (int a = 0; a < 3; ++a) { l.lo[a] = a == 0 ? v.lo[a] : v.lo[a] / 2; l.hi[a] = a == 0 ? v.hi[a] : (v.hi[a] + 1) / 2; }
                N.add(d.src0, l);
            } else { N.add_full(d.src0); N.add_full(skip); }
        } else if (d.kind == SD_OP_CONV && !op.first) {
            const Box v = conv_view(p, op, roi, N);
            if (v.any) { view[k] = v; N.add(d.src0, v); N.add(d.src1, v); }
            else { N.add_full(d.src0); N.add_full(d.src1); }
        } else if (d.kind == SD_OP_UPCONV && N.need[d.dst].any) {
            const Box& c = N.need[d.dst];
            int n[3];
            N.extents(d.src0, n);
            const int f[3] = {d.kz, 2, 2};
            Box v; v.any = false;
            for (int a = 0; a < 3; ++a) {
                v.lo[a] = std::max(0, c.lo[a] / f[a]);
                v.hi[a] = std::min(n[a], (c.hi[a] + f[a] - 1) / f[a]);
                v.any |= v.lo[a] > 0 || v.hi[a] < n[a];
            }
            if (v.any) { view[k] = v; N.add(d.src0, v); } else N.add_full(d.src0);
        } else {
            N.add_full(d.src0); N.add_full(d.src1);
        }
    }
    return view;
}

}  // namespace sdplan
