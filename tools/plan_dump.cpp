// Looks at a U-Net plan without a GPU: builds it with sd_plan.cpp alone and prints the blob digest, every Op field, the
// per-buffer tables and, per tile shape (and output box of interest), the shapes, the workspace layout and the views.
//
//   hipcc -O2 -std=c++17 -pthread syconn_amd/csrc/sd_plan.cpp tools/plan_dump.cpp -o plan_dump
//   plan_dump PLAN.bin [--dtypes bf16,f16,f16x2] [--lifetimes] [--tile D,H,W | --tile D,H,W:z0,y0,x0-z1,y1,x1] ...
//
// PLAN.bin: "SDPLAN1\0", int32 n_ops, int64 n_floats, n_ops x sd_op_desc, n_floats x float32 -- from Python:
//   ops, blob, _ = plan_from_model(model); arr = (OpDesc * len(ops))(*ops)
//   f.write(b'SDPLAN1\0' + struct.pack('<iq', len(ops), blob.size) + bytes(arr) + blob.tobytes())
// The plan switches (SD_NO_FUSE, SD_KEEP_ALL, ...) are read from the environment as the library reads them.
#include "../syconn_amd/csrc/sd_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace sdplan;

static uint64_t fnv1a64(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

static void dump_op(int i, const Op& o) {
    const sd_op_desc& d = o.d;
    printf("op %d kind %d src %d %d dst %d cin %d %d cout %d k %d %d %d relu %d norm %d groups %d eps %a off %lld %lld %lld %lld %lld %lld\n",
           i, d.kind, d.src0, d.src1, d.dst, d.cin0, d.cin1, d.cout, d.kz, d.ky, d.kx, d.relu, d.norm, d.groups, (double)d.eps,
           (long long)d.w_off, (long long)d.b_off, (long long)d.gamma_off, (long long)d.beta_off, (long long)d.mean_off, (long long)d.var_off);
    printf("op %d wpack %zu bias %zu aux %zu w3 %zu NT %d NB %d first %d fuse_pool %d fuse_final %d fuse_first %d fuse_gn %d "
           "fuse_pool_raw %d pooldir %zu stats_done %d gn_pool %d pool_in_conv %d gn_defer %d fwfrag %zu oscale %a final_oscale %a "
           "skipped %d dec0 %d %d in_dec0 %d\n",
           i, o.wpack_off, o.bias_off, o.aux_off, o.w3_off, o.NT, o.NB, (int)o.first, o.fuse_pool, o.fuse_final, o.fuse_first, o.fuse_gn,
           o.fuse_pool_raw, o.pooldir_off, (int)o.stats_done, o.gn_pool, (int)o.pool_in_conv, (int)o.gn_defer, o.fwfrag_off,
           (double)o.oscale, (double)o.final_oscale, (int)o.skipped, o.dec0_c1, o.dec0_c2, (int)o.in_dec0);
}

static void dump_tables(int nbuf, const std::vector<int>& bufC, const std::vector<int>& bufCp, const std::vector<int>& buf_gn,
                        const std::vector<size_t>& gn_tab_off, size_t ws_base, int final_cout, bool keep_all, bool ws_reuse) {
    printf("nbuf %d ws_base %zu final_cout %d keep_all %d ws_reuse %d\n", nbuf, ws_base, final_cout, (int)keep_all, (int)ws_reuse);
    for (int b = 0; b < nbuf; ++b) printf("buf %d C %d Cp %d gn %d tab %zu\n", b, bufC[b], bufCp[b], buf_gn[b], gn_tab_off[b]);
}

struct Tile { int d, h, w; Roi roi; };

static void dump_tile(const Plan& p, const Tile& t, bool lifetimes) {
    printf("tile %d %d %d", t.d, t.h, t.w);
    if (t.roi.set) printf(" roi %d %d %d - %d %d %d", t.roi.lo[0], t.roi.lo[1], t.roi.lo[2], t.roi.hi[0], t.roi.hi[1], t.roi.hi[2]);
    printf("\n");
    std::vector<Dims> dims;
    std::vector<size_t> off;
    std::string err;
    if (infer_shapes(p.ops, p.nbuf, t.d, t.h, t.w, dims, err) != SD_OK) { printf("shapes: %s\n", err.c_str()); return; }
    const bool dec0 = use_dec0(t.roi, dims[0]);
    const size_t top = plan_workspace(p, dims, t.roi, off);
    printf("use_dec0 %d workspace %zu\n", (int)dec0, rup_sz(top, 256));
    // (with reuse off only the total is part of the contract: the order of the ranges is free)
    for (int b = 0; b < p.nbuf; ++b) {
        printf("dims %d %d %d %d", b, dims[b].d, dims[b].h, dims[b].w);
        if (p.ws_reuse) printf(" off %zu", off[b]);
        printf("\n");
    }
    if (lifetimes) {
        std::vector<int> first, last;
        plan_lifetimes(p, dec0, first, last);
        for (int b = 1; b < p.nbuf; ++b)
            printf("life %d first %d last %d off %zu bytes %zu\n", b, first[b], last[b], off[b],
                   rup_sz((size_t)dims[b].d * dims[b].h * dims[b].w * p.bufCp[b] * (p.split ? 4 : 2), 256));
    }
    const std::vector<Box> view = plan_views(p, dims, t.roi, dec0);
    for (size_t k = 0; k < view.size(); ++k)
        if (view[k].any)
            printf("view %zu %d %d %d - %d %d %d\n", k, view[k].lo[0], view[k].lo[1], view[k].lo[2], view[k].hi[0], view[k].hi[1], view[k].hi[2]);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: plan_dump PLAN.bin [--dtypes a,b] [--lifetimes] [--tile D,H,W[:z0,y0,x0-z1,y1,x1]] ...\n"); return 2; }
    std::vector<std::string> dtypes = {"bf16", "f16", "f16x2"};
    std::vector<Tile> tiles;
    bool lifetimes = false;
    for (int a = 2; a < argc; ++a) {
        const std::string s = argv[a];
        if (s == "--lifetimes") lifetimes = true;
        else if (s == "--dtypes" && a + 1 < argc) {
            dtypes.clear();
            std::string v = argv[++a];
            for (size_t pos = 0; pos <= v.size();) {
                const size_t e = std::min(v.find(',', pos), v.size());
                dtypes.push_back(v.substr(pos, e - pos));
                pos = e + 1;
            }
        } else if (s == "--tile" && a + 1 < argc) {
            Tile t{};
            const int n = sscanf(argv[++a], "%d,%d,%d:%d,%d,%d-%d,%d,%d", &t.d, &t.h, &t.w, &t.roi.lo[0], &t.roi.lo[1], &t.roi.lo[2],
                                 &t.roi.hi[0], &t.roi.hi[1], &t.roi.hi[2]);
            if ((n != 3 && n != 9) || t.d <= 0 || t.h <= 0 || t.w <= 0) { fprintf(stderr, "bad --tile %s\n", argv[a]); return 2; }
            t.roi.set = n == 9;
            tiles.push_back(t);
        } else { fprintf(stderr, "unknown argument %s\n", s.c_str()); return 2; }
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    char magic[8];
    int32_t n_ops = 0;
    int64_t n_floats = 0;
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "SDPLAN1", 8) != 0 || fread(&n_ops, 4, 1, f) != 1 || fread(&n_floats, 8, 1, f) != 1 ||
        n_ops <= 0 || n_ops > (1 << 20) || n_floats < 0 || n_floats > ((int64_t)1 << 32)) {
        fprintf(stderr, "%s: not a plan file\n", argv[1]);
        return 2;
    }
    std::vector<sd_op_desc> ops(n_ops);
    std::vector<float> W((size_t)n_floats + 1);      // (+1: never an empty vector's null data())
    if (fread(ops.data(), sizeof(sd_op_desc), n_ops, f) != (size_t)n_ops || fread(W.data(), 4, (size_t)n_floats, f) != (size_t)n_floats) {
        fprintf(stderr, "%s: truncated\n", argv[1]);
        return 2;
    }
    fclose(f);
    for (const std::string& name : dtypes) {
        const int dt = name == "bf16" ? SD_BF16 : name == "f16" ? SD_F16 : name == "f16x2" ? SD_F16X2 : -1;
        if (dt < 0) { fprintf(stderr, "unknown dtype %s\n", name.c_str()); return 2; }
        Plan p;
        std::string err;
        const int rc = build_plan(ops.data(), n_ops, W.data(), (size_t)n_floats, dt, read_plan_switches(), p, err);
        printf("dtype %s rc %d%s%s\n", name.c_str(), rc, rc ? " error: " : "", err.c_str());
        if (rc != SD_OK) continue;
        printf("blob %zu %016llx\n", p.blob.size(), (unsigned long long)fnv1a64(p.blob.data(), p.blob.size()));
        for (size_t i = 0; i < p.ops.size(); ++i) dump_op((int)i, p.ops[i]);
        dump_tables(p.nbuf, p.bufC, p.bufCp, p.buf_gn, p.gn_tab_off, p.ws_base, p.final_cout, p.keep_all, p.ws_reuse);
        for (const Tile& t : tiles) dump_tile(p, t, lifetimes);
    }
    return 0;
}
