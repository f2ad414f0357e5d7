// Looks at a view-net plan without a GPU: builds it with sd_viewnet_plan.cpp alone and prints every Layer / Fc field, the blob
// digest, and per geometry the shapes, the workspace layout and the multiply-adds per sample.
//
//   hipcc -O2 -std=c++17 syconn_amd/csrc/sd_viewnet_plan.cpp tools/viewnet_plan_dump.cpp -o viewnet_plan_dump
//   viewnet_plan_dump NET.bin [--dtypes f16,bf16] [--geom D,H,W[:n_samples]] ... [--unpack OUT.bin]
//
// NET.bin: "SDVNET1\0", int32 n_layers, n_fc, in_channels, n_scalar, act, int64 n_floats, n_layers x (cout, k, pool) int32,
// (n_fc + 1) x int32 Linear sizes, n_floats x float32 (the arguments of sd_viewnet_create).
// --unpack (first dtype only): the blob read BACK into the order of the float32 input -- convolution weights from the MFMA fragments
// by the lane map of sd_viewnet.h, the first layer's bias with 0.5 sum(stored w) added back, Linear weights as stored -- so that
// packing can be compared with rounding alone; "pad_nonzero" counts fragment elements outside every real (k, n) that are not zero.
#include "../syconn_amd/csrc/sd_viewnet.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace sdvn;      // (with sdnet: fnv1a64, from_storage)

struct Geom { int d, h, w; size_t n; };

static int dtype_of(const std::string& s) { return s == "f16" ? SD_F16 : s == "bf16" ? SD_BF16 : s == "f32" ? SD_F32 : -1; }

static void unpack(const Plan& p, std::vector<float>& out) {
    const int dt = p.act_dtype;
    for (size_t li = 0; li < p.layers.size(); ++li) {
        const Layer& L = p.layers[li];
        const uint16_t* f = reinterpret_cast<const uint16_t*>(p.blob.data() + L.wfrag_off);
        const size_t nel = (size_t)L.nks * L.NT * 64 * 8;
        std::vector<char> seen(nel, 0);
        const int taps = L.k * L.k;
        std::vector<double> wsum(L.cout, 0.0);
        for (int n = 0; n < L.cout; ++n)
            for (int c = 0; c < L.cin; ++c)
                for (int tap = 0; tap < taps; ++tap) {
                    const int kk = tap * L.cin_p + c;      // B[kk][n] sits in k-step kk / 32, lane group (kk % 32) / 8, element kk % 8
                    const size_t e = ((((size_t)(kk / 32) * L.NT + n / 16) * 64) + ((kk % 32) / 8) * 16 + n % 16) * 8 + kk % 8;
                    seen[e] = 1;
                    const float v = from_storage(f[e], dt);
                    wsum[n] += v;
                    out.push_back(v);
                }
        size_t pad_nonzero = 0;
        for (size_t e = 0; e < nel; ++e) pad_nonzero += !seen[e] && f[e] != 0;
        const float* b = reinterpret_cast<const float*>(p.blob.data() + L.bias_off);
        for (int n = 0; n < L.cout; ++n) out.push_back(li == 0 ? (float)((double)b[n] + 0.5 * wsum[n]) : b[n]);
        for (int n = L.cout; n < 16 * L.NT; ++n) pad_nonzero += b[n] != 0.f;
        printf("unpack layer %zu pad_nonzero %zu\n", li, pad_nonzero);
    }
    for (const Fc& F : p.fc) {
        const float* w = reinterpret_cast<const float*>(p.blob.data() + F.w_off);
        const float* b = reinterpret_cast<const float*>(p.blob.data() + F.b_off);
        out.insert(out.end(), w, w + (size_t)F.nin * F.nout);
        out.insert(out.end(), b, b + F.nout);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: viewnet_plan_dump NET.bin [--dtypes f16,bf16] [--geom D,H,W[:n]] [--unpack OUT.bin]\n"); return 2; }
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char magic[8];
    int32_t hdr[5];
    int64_t n_floats = 0;
    if (fread(magic, 1, 8, fp) != 8 || memcmp(magic, "SDVNET1\0", 8) != 0 || fread(hdr, 4, 5, fp) != 5 || fread(&n_floats, 8, 1, fp) != 1 ||
        hdr[0] < 0 || hdr[0] > 64 || hdr[1] < 0 || hdr[1] > 64 || n_floats < 0 || n_floats > ((int64_t)1 << 28)) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<sd_viewnet_layer_desc> layers(hdr[0]);
    std::vector<int32_t> fc(hdr[1] + 1);
    std::vector<float> W((size_t)n_floats);
    if (fread(layers.data(), sizeof(sd_viewnet_layer_desc), layers.size(), fp) != layers.size() || fread(fc.data(), 4, fc.size(), fp) != fc.size() ||
        fread(W.data(), 4, W.size(), fp) != W.size()) {
        fprintf(stderr, "short file\n");
        return 2;
    }
    fclose(fp);
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
            Geom g{0, 0, 0, 1};
            unsigned long long n = 1;
            const int got = sscanf(argv[++i], "%d,%d,%d:%llu", &g.d, &g.h, &g.w, &n);
            if (got < 3) { fprintf(stderr, "bad --geom\n"); return 2; }
            g.n = got == 4 ? (size_t)n : 1;
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
        const int rc = build_plan(layers.data(), (int)layers.size(), fc.data(), hdr[1], hdr[2], hdr[3], hdr[4], W.data(), W.size(), dtype_of(dn), p, err);
        if (rc != SD_OK) {
            printf("dtype %s rc %d error: %s\n", dn.c_str(), rc, err.c_str());
            continue;
        }
        printf("dtype %s rc 0 blob %zu fnv %016llx act %d in_channels %d n_scalar %d\n", dn.c_str(), p.blob.size(),
               (unsigned long long)fnv1a64(p.blob.data(), p.blob.size()), p.act, p.in_channels, p.n_scalar);
        for (size_t i = 0; i < p.layers.size(); ++i) {
            const Layer& L = p.layers[i];
            printf("layer %zu cin %d cout %d k %d pool %d cin_p %d cout_p %d NT %d K %d nks %d wfrag %zu aoff %zu bias %zu lds %zu\n", i, L.cin, L.cout,
                   L.k, L.pool, L.cin_p, L.cout_p, L.NT, L.K, L.nks, L.wfrag_off, L.aoff_off, L.bias_off, L.lds_bytes);
        }
        for (size_t j = 0; j < p.fc.size(); ++j) printf("fc %zu nin %d nout %d w %zu b %zu\n", j, p.fc[j].nin, p.fc[j].nout, p.fc[j].w_off, p.fc[j].b_off);
        for (const Geom& g : geoms) {
            Workspace ws;
            std::vector<Dims> dims;
            if (workspace(p, g.n, g.d, g.h, g.w, ws, err) != SD_OK || infer_shapes(p, g.d, g.h, g.w, dims, err) != SD_OK) {
                printf("geom %d %d %d n %zu error: %s\n", g.d, g.h, g.w, g.n, err.c_str());
                continue;
            }
            printf("geom %d %d %d n %zu workspace %zu macs %.0f\n", g.d, g.h, g.w, g.n, ws.total, macs_per_sample(p, g.d, g.h, g.w));
            for (size_t i = 0; i < dims.size(); ++i) printf("out %zu %d %d off %zu\n", i, dims[i].h, dims[i].w, ws.layer_off[i]);
            for (size_t j = 0; j < ws.hidden_off.size(); ++j) printf("hidden %zu off %zu\n", j, ws.hidden_off[j]);
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
