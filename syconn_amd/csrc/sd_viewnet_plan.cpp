// The host-only plan builder of the multi-view network (sd_viewnet.h): validation, weight rounding, the MFMA fragment order, the
// channel and K padding, the first layer's normalisation fold, shapes and the workspace layout.
#include "sd_viewnet.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace sdvn {

int build_plan(const sd_viewnet_layer_desc* layers, int n_layers, const int32_t* fc, int n_fc, int in_channels, int n_scalar, int act,
               const float* W, size_t n_floats, int act_dtype, Plan& plan, std::string& err) {
    if (!layers || !fc || !W) return bad(err, "viewnet: null argument");
    if (act_dtype != SD_F16 && act_dtype != SD_BF16) return bad(err, "viewnet: act_dtype must be SD_F16 or SD_BF16");
    if (act != ACT_RELU && act != ACT_LEAKY) return bad(err, "viewnet: act must be 0 (relu) or 1 (leaky_relu)");
    if (n_layers < 1 || n_layers > 16) return bad(err, "viewnet: 1 to 16 layers");
    if (n_fc < 1 || n_fc > MAX_FC) return bad(err, "viewnet: 1 to 4 Linear layers");
    if (in_channels < 1 || in_channels > 4) return bad(err, "viewnet: in_channels must be 1 to 4");
    if (n_scalar < 0 || n_scalar > 64) return bad(err, "viewnet: n_scalar must be 0 to 64");
    plan = Plan{};
    plan.act_dtype = act_dtype;
    plan.act = act;
    plan.in_channels = in_channels;
    plan.n_scalar = n_scalar;
    // the float count the description implies, before anything is read
    size_t need = 0;
    int cin = in_channels;
    for (int i = 0; i < n_layers; ++i) {
        const sd_viewnet_layer_desc& d = layers[i];
        if (d.k != 1 && d.k != 2 && d.k != 4 && d.k != 5) return bad(err, "viewnet: layer " + std::to_string(i) + ": k must be 1, 2, 4 or 5");
        if (d.pool != 1 && d.pool != 2) return bad(err, "viewnet: layer " + std::to_string(i) + ": pool must be 1 or 2");
        if (d.cout < 1 || d.cout > 16 * MAX_NT) return bad(err, "viewnet: layer " + std::to_string(i) + ": cout must be 1 to 80");
        need += (size_t)d.cout * cin * d.k * d.k + d.cout;
        cin = d.cout;
    }
    for (int j = 0; j <= n_fc; ++j)
        if (fc[j] < 1 || fc[j] > (1 << 20)) return bad(err, "viewnet: Linear sizes must be 1 to 2^20");
    if (fc[0] <= n_scalar) return bad(err, "viewnet: the first Linear takes no features");
    if (2 * sizeof(float) * (size_t)*std::max_element(fc, fc + n_fc + 1) > MAX_LDS) return bad(err, "viewnet: a Linear vector exceeds 8192 values");
    for (int j = 0; j < n_fc; ++j) need += (size_t)fc[j] * fc[j + 1] + fc[j + 1];
    if (need != n_floats) return bad(err, "viewnet: weights hold " + std::to_string(n_floats) + " floats, the description needs " + std::to_string(need));

    const float* w = W;
    cin = in_channels;
    for (int i = 0; i < n_layers; ++i) {
        const sd_viewnet_layer_desc& d = layers[i];
        const bool first = i == 0;
        Layer L;
        L.cin = cin, L.cout = d.cout, L.k = d.k, L.pool = d.pool;
        L.cin_p = first ? 4 : rup(cin, 8);
        L.cout_p = rup(d.cout, 8);
        L.NT = rup(d.cout, 16) / 16;
        const int taps = d.k * d.k;
        L.K = first ? rup(taps, 2) * 4 : taps * L.cin_p;
        L.nks = rup(L.K, 32) / 32;
        L.macs_per_out = (double)taps * cin * d.cout;
        const int twin = TILE_W + d.k - 1, thin = TILE_H + d.k - 1;
        L.lds_bytes = (size_t)thin * twin * L.cin_p * 2;
        if (L.lds_bytes > MAX_LDS) return bad(err, "viewnet: layer " + std::to_string(i) + ": halo tile exceeds the LDS budget");
        const float* bias = w + (size_t)d.cout * cin * taps;
        for (size_t e = 0; e < (size_t)d.cout * cin * taps + d.cout; ++e)
            if (!std::isfinite(w[e])) return bad(err, "viewnet: layer " + std::to_string(i) + ": non-finite weight");
        // B fragments
        L.wfrag_off = grow(plan.blob, (size_t)L.nks * L.NT * 64 * 8 * 2);
        std::vector<double> wsum(d.cout, 0.0);
        {
            uint16_t* f = reinterpret_cast<uint16_t*>(plan.blob.data() + L.wfrag_off);
            for (int ks = 0; ks < L.nks; ++ks)
                for (int nt = 0; nt < L.NT; ++nt)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int kk = 32 * ks + 8 * (lane >> 4) + j, n = 16 * nt + (lane & 15);
                            const int tap = kk / L.cin_p, c = kk % L.cin_p;
                            uint16_t v = 0;
                            if (tap < taps && c < cin && n < d.cout) {
                                if (!store_weight(w[((size_t)n * cin + c) * taps + tap], act_dtype, v))
                                    return bad(err, "viewnet: layer " + std::to_string(i) + ": a weight overflows the storage type (use bf16, or rescale)");
                                wsum[n] += (double)from_storage(v, act_dtype);
                            }
                            f[(((size_t)ks * L.NT + nt) * 64 + lane) * 8 + j] = v;
                        }
        }
        // A offsets
        L.aoff_off = grow(plan.blob, (size_t)L.nks * 4 * 2 * 4);
        {
            int32_t* a = reinterpret_cast<int32_t*>(plan.blob.data() + L.aoff_off);
            auto tap_off = [&](int tap) { return tap < taps ? ((tap / d.k) * twin + tap % d.k) * L.cin_p : 0; };
            for (int ks = 0; ks < L.nks; ++ks)
                for (int kg = 0; kg < 4; ++kg) {
                    const int kk = 32 * ks + 8 * kg;
                    int o0, o1;
                    if (first) {
                        o0 = tap_off(kk / 4), o1 = tap_off(kk / 4 + 1);
                    } else {
                        const int tap = kk / L.cin_p;
                        o0 = o1 = tap < taps ? tap_off(tap) + kk % L.cin_p : 0;
                    }
                    a[(ks * 4 + kg) * 2 + 0] = o0, a[(ks * 4 + kg) * 2 + 1] = o1;
                }
        }
        // bias; the first layer's carries the -0.5 of the normalisation over the STORED weights
        L.bias_off = grow(plan.blob, (size_t)L.NT * 16 * 4);
        {
            float* b = reinterpret_cast<float*>(plan.blob.data() + L.bias_off);
            for (int n = 0; n < d.cout; ++n) b[n] = first ? (float)((double)bias[n] - 0.5 * wsum[n]) : bias[n];
        }
        w = bias + d.cout;
        cin = d.cout;
        plan.layers.push_back(L);
    }
    for (int j = 0; j < n_fc; ++j) {
        Fc F;
        F.nin = fc[j], F.nout = fc[j + 1];
        const size_t nw = (size_t)F.nin * F.nout;
        for (size_t e = 0; e < nw + F.nout; ++e)
            if (!std::isfinite(w[e])) return bad(err, "viewnet: Linear " + std::to_string(j) + ": non-finite weight");
        F.w_off = grow(plan.blob, nw * 4);
        std::memcpy(plan.blob.data() + F.w_off, w, nw * 4);
        F.b_off = grow(plan.blob, (size_t)F.nout * 4);
        std::memcpy(plan.blob.data() + F.b_off, w + nw, (size_t)F.nout * 4);
        w += nw + F.nout;
        plan.fc.push_back(F);
    }
    plan.blob.resize(rup_sz(plan.blob.size(), 256), 0);
    return SD_OK;
}

int infer_shapes(const Plan& p, int D, int H, int W, std::vector<Dims>& dims, std::string& err) {
    if (D < 1 || H < 1 || W < 1 || D > 4096 || H > 16384 || W > 16384) return bad(err, "viewnet: D, H, W out of range");
    dims.clear();
    int h = H, w = W;
    for (size_t i = 0; i < p.layers.size(); ++i) {
        const Layer& L = p.layers[i];
        h = (h - L.k + 1) / L.pool, w = (w - L.k + 1) / L.pool;
        if (h < 1 || w < 1)
            return bad(err, "viewnet: layer " + std::to_string(i) + " has an empty output for a " + std::to_string(H) + " x " + std::to_string(W) + " view");
        dims.push_back({h, w});
    }
    const long long flat = (long long)p.layers.back().cout * D * h * w;
    if (flat + p.n_scalar != p.fc[0].nin)
        return bad(err, "viewnet: the layers give " + std::to_string(flat) + " features + " + std::to_string(p.n_scalar) + " scalars, the first Linear takes " +
                            std::to_string(p.fc[0].nin));
    return SD_OK;
}

int workspace(const Plan& p, size_t n_samples, int D, int H, int W, Workspace& ws, std::string& err) {
    std::vector<Dims> dims;
    const int rc = infer_shapes(p, D, H, W, dims, err);
    if (rc != SD_OK) return rc;
    if (n_samples < 1 || n_samples > ((size_t)1 << 24)) return bad(err, "viewnet: n_samples out of range");
    ws = Workspace{};
    size_t off = 0;
    for (size_t i = 0; i < p.layers.size(); ++i) {
        ws.layer_off.push_back(off);
        off += rup_sz(n_samples * D * dims[i].h * dims[i].w * p.layers[i].cout_p * 2, 256);
    }
    for (size_t j = 0; j + 1 < p.fc.size(); ++j) {
        ws.hidden_off.push_back(off);
        off += rup_sz(n_samples * p.fc[j].nout * 4, 256);
    }
    ws.total = off;
    return SD_OK;
}

double macs_per_sample(const Plan& p, int D, int H, int W) {
    std::vector<Dims> dims;
    std::string err;
    if (infer_shapes(p, D, H, W, dims, err) != SD_OK) return 0.0;
    double m = 0.0;
    for (size_t i = 0; i < p.layers.size(); ++i)
        m += p.layers[i].macs_per_out * D * (double)(dims[i].h * p.layers[i].pool) * (dims[i].w * p.layers[i].pool);
    for (const Fc& f : p.fc) m += (double)f.nin * f.nout;
    return m;
}

}  // namespace sdvn
