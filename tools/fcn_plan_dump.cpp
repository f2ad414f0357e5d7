// Looks at an FCN plan without a GPU: builds it with sd_fcn_plan.cpp alone and prints every op's fields, the blob digest, and per
// geometry the shapes, the workspace layout and the multiply-adds per view.
//
//   hipcc -O2 -std=c++17 syconn_amd/csrc/sd_fcn_plan.cpp tools/fcn_plan_dump.cpp -o fcn_plan_dump
//   fcn_plan_dump NET.bin [--dtypes f16,bf16] [--geom H,W[:n_planes]] ... [--unpack OUT.bin]
//
// NET.bin: "SDFCN01\0", int32 in_channels, dec_last, n_class, n_convs, block_len[5], int64 n_floats, n_convs x int32 output channels,
// n_floats x float32 (the arguments of sd_fcn_create).
// --unpack (first dtype only): the blob read BACK in the order of the float32 input -- 3 x 3 weights from the MFMA fragments by the
// lane map and the tap tables of sd_fcn.h (a transposed convolution's from its four parity fragments), biases, per decoder step the
// two BatchNorm constants (scale, shift) in place of the four BatchNorm tensors, the classifier as stored -- so that packing can be
// compared with rounding alone; "pad_nonzero" counts fragment / bias elements outside every real (c, n) that are not zero, "dup" the
// weights found in more than one place or in none.
#include "../syconn_amd/csrc/sd_fcn.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace sdfcn;      // (with sdnet: fnv1a64, from_storage)

struct Geom { int h, w; size_t n; };

static int dtype_of(const std::string& s) { return s == "f16" ? SD_F16 : s == "bf16" ? SD_BF16 : s == "f32" ? SD_F32 : -1; }

static void unpack(const Plan& p, std::vector<float>& out) {
    const int dt = p.act_dtype;
    for (size_t oi = 0; oi < p.ops.size(); ++oi) {
        const Op& op = p.ops[oi];
        if (op.kind == OP_CLASSIFY) {
            const float* w = reinterpret_cast<const float*>(p.blob.data() + op.bias_off);
            const float* b = reinterpret_cast<const float*>(p.blob.data() + op.scale_off);
            out.insert(out.end(), w, w + (size_t)op.cin * op.cout);
            out.insert(out.end(), b, b + op.cout);
            continue;
        }
        const bool dec = op.kind == OP_DECONV;
        const int NTtot = op.NT * op.groups, n_par = dec ? 4 : 1;
        std::vector<float> w((size_t)op.cin * op.cout * 9, 0.f);
        std::vector<int> found(w.size(), 0);
        size_t pad_nonzero = 0;
        for (int par = 0; par < n_par; ++par) {
            Tap taps[9];
            const int nt = taps_of(op.kind, par, taps);
            const uint16_t* f = reinterpret_cast<const uint16_t*>(p.blob.data() + op.wfrag_off[par]);
            for (int ch = 0; ch < op.n_chunks; ++ch)
                for (int t = 0; t < nt; ++t)
                    for (int ntg = 0; ntg < NTtot; ++ntg)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int j = 0; j < 8; ++j) {
                                const int c = CK * ch + 8 * (lane >> 4) + j, n = 16 * ntg + (lane & 15);
                                const uint16_t v = f[((((size_t)ch * nt + t) * NTtot + ntg) * 64 + lane) * 8 + j];
                                if (c >= op.cin || n >= op.cout) {
                                    pad_nonzero += v != 0;
                                    continue;
                                }
                                const size_t idx = dec ? (((size_t)c * op.cout + n) * 3 + taps[t].ky) * 3 + taps[t].kx
                                                       : (((size_t)n * op.cin + c) * 3 + taps[t].ky) * 3 + taps[t].kx;
                                w[idx] = from_storage(v, dt);
                                ++found[idx];
                            }
        }
        size_t dup = 0;
        for (int v : found) dup += v != 1;
        out.insert(out.end(), w.begin(), w.end());
        const float* b = reinterpret_cast<const float*>(p.blob.data() + op.bias_off);
        out.insert(out.end(), b, b + op.cout);
        for (int n = op.cout; n < 16 * NTtot; ++n) pad_nonzero += b[n] != 0.f;
        if (dec) {
            const float* sc = reinterpret_cast<const float*>(p.blob.data() + op.scale_off);
            const float* sh = reinterpret_cast<const float*>(p.blob.data() + op.shift_off);
            out.insert(out.end(), sc, sc + op.cout);
            out.insert(out.end(), sh, sh + op.cout);
            for (int n = op.cout; n < 16 * NTtot; ++n) pad_nonzero += (sc[n] != 0.f) + (sh[n] != 0.f);
        }
        printf("unpack op %zu pad_nonzero %zu dup %zu\n", oi, pad_nonzero, dup);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: fcn_plan_dump NET.bin [--dtypes f16,bf16] [--geom H,W[:n]] [--unpack OUT.bin]\n"); return 2; }
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char magic[8];
    int32_t hdr[9];
    int64_t n_floats = 0;
    if (fread(magic, 1, 8, fp) != 8 || memcmp(magic, "SDFCN01\0", 8) != 0 || fread(hdr, 4, 9, fp) != 9 || fread(&n_floats, 8, 1, fp) != 1 || hdr[3] < 0 ||
        hdr[3] > 64 || n_floats < 0 || n_floats > ((int64_t)1 << 28)) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<int32_t> blocks(hdr[3]);
    std::vector<float> W((size_t)n_floats);
    if (fread(blocks.data(), 4, blocks.size(), fp) != blocks.size() || fread(W.data(), 4, W.size(), fp) != W.size()) {
        fprintf(stderr, "short file\n");
        return 2;
    }
    fclose(fp);
    // the builder reads sum(block_len) channel entries: a header whose block lengths (each one clamped to what the builder accepts)
    // name more entries than the file holds is refused here
    int named = 0;
    for (int b = 0; b < N_BLOCKS; ++b) named += hdr[4 + b] >= 1 && hdr[4 + b] <= MAX_BLOCK_CONVS ? hdr[4 + b] : 0;
    if (named > hdr[3]) { fprintf(stderr, "block lengths name more convolutions than the file holds\n"); return 2; }
    std::vector<std::string> dtypes = {"f16", "bf16"};
    std::vector<Geom> geoms;
    const char* unpack_path = nullptr;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--dtypes" && i + 1 < argc) {
            dtypes.clear();
            std::string s = argv[++i];
            size_t pos = 0;
            while (pos <= s.size()) {
                const size_t c = s.find(',', pos);
                dtypes.push_back(s.substr(pos, c == std::string::npos ? std::string::npos : c - pos));
                if (c == std::string::npos) break;
                pos = c + 1;
            }
        } else if (a == "--geom" && i + 1 < argc) {
            Geom g{0, 0, 1};
            unsigned long long n = 1;
            const int got = sscanf(argv[++i], "%d,%d:%llu", &g.h, &g.w, &n);
            if (got < 2) { fprintf(stderr, "bad --geom\n"); return 2; }
            g.n = got == 3 ? (size_t)n : 1;
            geoms.push_back(g);
        } else if (a == "--unpack" && i + 1 < argc) {
            unpack_path = argv[++i];
        } else {
            fprintf(stderr, "unknown argument %s\n", a.c_str());
            return 2;
        }
    }
    bool first = true;
    for (const std::string& dn : dtypes) {
        Plan p;
        std::string err;
        const int rc = build_plan(hdr[0], blocks.data(), hdr + 4, hdr[1], hdr[2], W.data(), W.size(), dtype_of(dn), p, err);
        if (rc != SD_OK) {
            printf("dtype %s rc %d error: %s\n", dn.c_str(), rc, err.c_str());
            continue;
        }
        printf("dtype %s rc 0 blob %zu fnv %016llx in_channels %d dec_last %d n_class %d\n", dn.c_str(), p.blob.size(),
               (unsigned long long)fnv1a64(p.blob.data(), p.blob.size()), p.in_channels, p.dec_last, p.n_class);
        for (size_t i = 0; i < p.ops.size(); ++i) {
            const Op& o = p.ops[i];
            printf("op %zu kind %d cin %d cout %d cin_p %d cout_p %d first %d pool %d in_shift %d out_shift %d in %d out %d skip %d chunks %d NT %d groups %d "
                   "macs_px %.0f\n",
                   i, o.kind, o.cin, o.cout, o.cin_p, o.cout_p, (int)o.first, (int)o.pool, o.in_shift, o.out_shift, o.in_buf, o.out_buf, o.skip_buf, o.n_chunks,
                   o.NT, o.groups, o.macs_per_in_px);
        }
        for (const Geom& g : geoms) {
            Workspace ws;
            std::vector<Dims> dims;
            if (workspace(p, g.n, g.h, g.w, ws, err) != SD_OK || infer_shapes(p, g.h, g.w, dims, err) != SD_OK) {
                printf("geom %d %d n %zu error: %s\n", g.h, g.w, g.n, err.c_str());
                continue;
            }
            printf("geom %d %d n %zu workspace %zu macs %.0f\n", g.h, g.w, g.n, ws.total, macs_per_view(p, g.h, g.w));
            for (size_t i = 0; i < ws.off.size(); ++i) printf("out %zu %d %d %d cp %d off %zu\n", i, dims[i].c, dims[i].h, dims[i].w, dims[i].cp, ws.off[i]);
        }
        if (unpack_path && first) {
            std::vector<float> out;
            unpack(p, out);
            FILE* fo = fopen(unpack_path, "wb");
            if (!fo || fwrite(out.data(), 4, out.size(), fo) != out.size()) { fprintf(stderr, "cannot write %s\n", unpack_path); return 2; }
            fclose(fo);
            printf("unpack floats %zu\n", out.size());
        }
        first = false;
    }
    return 0;
}
