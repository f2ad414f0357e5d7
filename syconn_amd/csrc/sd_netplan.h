// What the host-only plan builders of the 2D view networks (sd_viewnet_plan.cpp, sd_fcn_plan.cpp) and their dump tools share: the
// workgroup tile, rounding up, the blob's aligned ranges, the storage type <-> float conversions with the weight overflow test, and the
// blob digest of the tools.  No HIP include, header-only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/syconn_dense.h"

namespace sdnet {

constexpr int TILE_H = 8, TILE_W = 32;      // positions of one workgroup (4 waves x 4 MFMA row tiles of 16), sd_planar_mma.h

inline int rup(int v, int m) { return (v + m - 1) / m * m; }
inline size_t rup_sz(size_t v, size_t m) { return (v + m - 1) / m * m; }

inline int bad(std::string& err, const std::string& msg) {
    err = msg;
    return SD_ERR_INVALID;
}
inline size_t grow(std::vector<char>& blob, size_t bytes) {      // a zeroed, 256-byte aligned range at the end of the blob
    const size_t off = rup_sz(blob.size(), 256);
    blob.resize(off + bytes, 0);
    return off;
}

// storage type <-> float (the plan's rounding: nearest even)
inline uint16_t to_storage(float f, int dtype) {
    if (dtype == SD_BF16) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);      // NaN
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    }
    const _Float16 h = (_Float16)f;
    uint16_t b;
    std::memcpy(&b, &h, 2);
    return b;
}
inline float from_storage(uint16_t bits, int dtype) {
    if (dtype == SD_BF16) {
        const uint32_t u = (uint32_t)bits << 16;
        float f;
        std::memcpy(&f, &u, 4);
        return f;
    }
    _Float16 h;
    std::memcpy(&h, &bits, 2);
    return (float)h;
}
// one element of a B fragment: the (finite) weight rounded to the storage type; false if it rounds to infinity
inline bool store_weight(float w, int dtype, uint16_t& v) {
    v = to_storage(w, dtype);
    return (v & 0x7fffu) != (dtype == SD_BF16 ? 0x7f80u : 0x7c00u);
}

inline uint64_t fnv1a64(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

}  // namespace sdnet
