// Host half of the lossy WebP re-save: the numbers a quality stands for (quantiser index, steps, loop-filter strength,
// mode bias) and the layout of the batch's records, coefficients and planes.  The steps and the filter strength come from
// the code that reads them out of a frame header (vp8_params.hpp), so that a decoder of the written file and the encoder's
// own reconstruction cannot disagree.  Plain C++, no HIP: tests/fuzz/vp8_enc_check.cpp compiles this file.
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "vipcup_hip.h"
#include "vp8_params.hpp"

void vip_set_error(const char* fmt, ...);

// the per-image pixel cap (vp8_encode.hip asks too)
uint64_t vip_vp8_encode_max_pixels() {
    const char* s = getenv("VIP_MAX_JPEG_PIXELS");      // the per-image cap of the JPEG path covers WebP too
    if (s && *s) {
        const long long v = atoll(s);
        if (v > 0) return (uint64_t)v;
    }
    return (uint64_t)64 << 20;
}

namespace {

// Fitted to libwebp's encoder on the CPU ("Lossy WebP re-save"): the share of macroblocks with sub-block modes,
// and the frame's loop-filter level as a function of the quantiser index.
constexpr int I4_BIAS_K = 61;
constexpr int FILTER_A = 13, FILTER_B = -242;

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }      // the kernel stores 16 bytes at a time

// libwebp's quality curve (QualityToCompression) and its map onto the quantiser index, in float64
int base_q_of(int quality) {
    const double c = quality / 100.0;
    const double l = c < 0.75 ? c * (2.0 / 3.0) : 2.0 * c - 1.0;
    const int q = (int)(127.0 * (1.0 - pow(l, 1.0 / 3.0)));
    return vp8_params::clipi(q, 127);
}

}  // namespace

extern "C" int vip_vp8_encode_params_h(int quality, vip_vp8_enc_params* E) {
    if (!E) {
        vip_set_error("vip_vp8_encode_params_h: null pointer");
        return VIP_ERR_BAD_ARG;
    }
    if (quality < 1 || quality > 100) {
        vip_set_error("vip_vp8_encode_params_h: quality %d: expected 1..100", quality);
        return VIP_ERR_BAD_ARG;
    }
    memset(E, 0, sizeof(*E));
    E->quality = quality;
    E->base_q = base_q_of(quality);
    const int dq[5] = {0, 0, 0, 0, 0};
    vp8_params::Quant Q;
    vp8_params::quant_steps(E->base_q, dq, Q);
    for (int i = 0; i < 2; ++i) {
        E->y1[i] = Q.y1[i];
        E->y2[i] = Q.y2[i];
        E->uv[i] = Q.uv[i];
        E->y1_inv[i] = vp8_params::reciprocal(Q.y1[i]);
        E->y2_inv[i] = vp8_params::reciprocal(Q.y2[i]);
        E->uv_inv[i] = vp8_params::reciprocal(Q.uv[i]);
    }
    E->filter_level = vp8_params::clipi((FILTER_A * E->base_q + FILTER_B) >> 4, 63);
    uint8_t fl, il, hv;
    vp8_params::filter_strength(E->filter_level, 0, E->filter_level ? 2 : 0, fl, il, hv);
    E->flevel = fl;
    E->ilevel = il;
    E->hev = hv;
    E->i4_bias = (I4_BIAS_K * E->y1[1] * E->y1[1]) >> 4;
    return VIP_OK;
}

extern "C" int vip_vp8_encode_layout_h(const int32_t* sizes_hw_h, int n, int quality, vip_vp8_desc* desc_h, size_t* stream_bytes_h,
                                       size_t* scratch_bytes_h) {
    if (!sizes_hw_h || !desc_h || !stream_bytes_h || !scratch_bytes_h || n <= 0) {
        vip_set_error("vip_vp8_encode_layout_h: bad argument (null pointer or n <= 0)");
        return VIP_ERR_BAD_ARG;
    }
    vip_vp8_enc_params E;
    const int st = vip_vp8_encode_params_h(quality, &E);
    if (st != VIP_OK) return st;
    const uint64_t cap = vip_vp8_encode_max_pixels();
    size_t off = 0, plane = 0;
    for (int i = 0; i < n; ++i) {
        const int h = sizes_hw_h[2 * i], w = sizes_hw_h[2 * i + 1];
        if (h <= 0 || w <= 0 || h > 16383 || w > 16383) {
            vip_set_error("vip_vp8_encode_layout_h: image %d: %dx%d pixels: a VP8 frame has 1..16383 per side", i, w, h);
            return VIP_ERR_BAD_ARG;
        }
        if ((uint64_t)w * h > cap) {
            vip_set_error("vip_vp8_encode_layout_h: image %d: %dx%d exceeds VIP_MAX_JPEG_PIXELS=%llu", i, w, h, (unsigned long long)cap);
            return VIP_ERR_BAD_ARG;
        }
        vip_vp8_desc& D = desc_h[i];
        memset(&D, 0, sizeof(D));
        D.width = w;
        D.height = h;
        D.mb_w = (w + 15) >> 4;
        D.mb_h = (h + 15) >> 4;
        D.filter_type = E.filter_level ? 2 : 0;
        const size_t nmb = (size_t)D.mb_w * D.mb_h;
        D.stream_off = (int64_t)off;
        D.mb_off = 0;
        D.coef_off = (int64_t)align16(nmb * sizeof(vip_vp8_mb));
        D.coef_blocks = (int64_t)(nmb * 25);
        D.plane_off = (int64_t)plane;
        off += align16((size_t)D.coef_off + nmb * 25 * 32);
        plane += nmb * 384;
    }
    *stream_bytes_h = off;
    *scratch_bytes_h = plane < 16 ? 16 : plane;
    return VIP_OK;
}
