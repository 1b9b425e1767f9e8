// What a VP8 frame header's numbers mean, written once for the reader (vp8_host.cpp) and the writer of such numbers
// (vp8_enc_host.cpp): the six dequantisation steps of a quantiser index (RFC 6386 section 14.1, as libwebp clamps them) and
// the loop-filter strength of a macroblock (libwebp's PrecomputeFilterStrengths).  Host only, plain C++.
#pragma once
#include <stdint.h>

#include "vp8_tables.hpp"

namespace vp8_params {

struct Quant {
    int y1[2], y2[2], uv[2];             // [0] DC step, [1] AC step
};

inline int clipi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// q: the quantiser index of the macroblock's segment; dq: the header's deltas y1 dc, y2 dc, y2 ac, uv dc, uv ac
inline void quant_steps(int q, const int dq[5], Quant& m) {
    using namespace vp8_tables;
    m.y1[0] = DC_TABLE[clipi(q + dq[0], 127)];
    m.y1[1] = AC_TABLE[clipi(q, 127)];
    m.y2[0] = DC_TABLE[clipi(q + dq[1], 127)] * 2;
    m.y2[1] = (AC_TABLE[clipi(q + dq[2], 127)] * 101581) >> 16;
    if (m.y2[1] < 8) m.y2[1] = 8;
    m.uv[0] = DC_TABLE[clipi(q + dq[3], 117)];
    m.uv[1] = AC_TABLE[clipi(q + dq[4], 127)];
}

// ceil(2^32 / q): floor(x / q) == (x * r) >> 32 for 0 <= x < 65536 and 2 <= q < 65536 (the error x (r q - 2^32) / (q 2^32)
// stays below 1 / q); q = 1 would need 2^32 itself and is no step: they start at 4
inline uint32_t reciprocal(int q) { return (uint32_t)((((uint64_t)1 << 32) + (uint32_t)q - 1) / (uint32_t)q); }

// level: the macroblock's filter level with segment and deltas applied, not yet clamped
inline void filter_strength(int level, int sharpness, int filter_type, uint8_t& flevel, uint8_t& ilevel, uint8_t& hev) {
    level = clipi(level, 63);
    int il = 0, hv = 0;
    if (level > 0) {
        il = level;
        if (sharpness > 0) {
            il >>= sharpness > 4 ? 2 : 1;
            if (il > 9 - sharpness) il = 9 - sharpness;
        }
        if (il < 1) il = 1;
        hv = level >= 40 ? 2 : level >= 15 ? 1 : 0;
    }
    flevel = (uint8_t)(filter_type ? level : 0);
    ilevel = (uint8_t)il;
    hev = (uint8_t)hv;
}

}  // namespace vp8_params
