// The host side that the C entries of the 2D view networks (sd_viewnet.hip, sd_fcn.hip) share: the model handle (a plan and its blob
// on the device), the event-timed forward, and the copies back to the host (flags, stored tensors).
#pragma once
#include <hip/hip_runtime.h>
#include "sd_netplan.h"

int sd_fail_msg(int code, const char* msg);      // sd_api.hip: sets sd_last_error()

namespace sdnet {

inline int fail(const std::string& msg, int code = SD_ERR_INVALID) { return sd_fail_msg(code, msg.c_str()); }

template <typename Plan> struct Net {
    Plan plan;
    char* dev_blob = nullptr;
    ~Net() {
        if (dev_blob) (void)hipFree(dev_blob);
    }
};

// the packed blob to the device; the host copy is freed
inline int upload_blob(std::vector<char>& blob, char** dev, const std::string& who) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(dev), blob.size());
    if (e == hipSuccess) e = hipMemcpy(*dev, blob.data(), blob.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(who + ": " + hipGetErrorString(e), e == hipErrorOutOfMemory ? SD_ERR_NOMEM : SD_ERR_HIP);
    std::vector<char>().swap(blob);
    return SD_OK;
}

// *out = a new handle whose plan `build(plan, err)` made, or null
template <typename H, typename Build> int create_net(H** out, const std::string& who, Build&& build) {
    if (!out) return fail(who + ": null output");
    *out = nullptr;
    H* m = new H;
    std::string err;
    int rc = build(m->plan, err);
    rc = rc != SD_OK ? fail(err, rc) : upload_blob(m->plan.blob, &m->dev_blob, who);
    if (rc != SD_OK) {
        delete m;
        return rc;
    }
    *out = m;
    return SD_OK;
}

// run(ev) records n events on `stream`, in front of the first launch and behind every stage; ms_out: the n - 1 times between them
template <typename Run> int timed(size_t n, void* stream, float* ms_out, const std::string& who, Run&& run) {
    std::vector<hipEvent_t> ev(n, nullptr);
    int rc = SD_OK;
    for (size_t i = 0; i < n && rc == SD_OK; ++i)
        if (hipEventCreate(&ev[i]) != hipSuccess) rc = fail(who + ": event creation failed", SD_ERR_HIP);
    if (rc == SD_OK) rc = run(ev.data());
    if (rc == SD_OK && hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)) != hipSuccess) rc = fail(who + ": synchronise failed", SD_ERR_HIP);
    for (size_t i = 0; i + 1 < n && rc == SD_OK; ++i)
        if (hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]) != hipSuccess) rc = fail(who + ": elapsed time failed", SD_ERR_HIP);
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

inline int copy_out(void* dst_host, const void* src_dev, size_t bytes, void* stream, const std::string& who) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(who + ": copy failed", SD_ERR_HIP);
    return SD_OK;
}

// the n flags of a forward (the *_overflow entries)
inline int read_flags(const void* m, const int32_t* flags_dev, int n, void* stream, int32_t* out, const std::string& who) {
    if (!m || !flags_dev || !out) return fail(who + ": null argument");
    return copy_out(out, flags_dev, n * sizeof(int32_t), stream, who);
}

// a stored tensor T[n_px][cp] as float [n_px][c]
inline int read_stored(const void* src_dev, size_t n_px, int c, int cp, int dtype, float* out_host, void* stream, const std::string& who) {
    std::vector<uint16_t> raw(n_px * cp);
    const int rc = copy_out(raw.data(), src_dev, raw.size() * 2, stream, who);
    if (rc != SD_OK) return rc;
    for (size_t i = 0; i < n_px; ++i)
        for (int k = 0; k < c; ++k) out_host[i * c + k] = from_storage(raw[i * cp + k], dtype);
    return SD_OK;
}

}  // namespace sdnet
