// Test infrastructure (CPU only): the lossy WebP re-save without a GPU.  The encoder arithmetic (csrc/vp8_enc.hpp), the
// numbers of a quality (csrc/vp8_enc_host.cpp) and the decoder arithmetic (csrc/vp8_recon.hpp) are compiled as plain C++
// and run serially, macroblocks in raster order, sub-blocks in raster order.  tests/test_vp8_encode_cpu.py writes the modes
// and levels out as a key frame and compares Pillow's decode of it with the RGB from here.  Built as
//   g++ -I include -I vip-cup-2022_amd/csrc vp8_enc_check.cpp ../../vip-cup-2022_amd/csrc/vp8_enc_host.cpp
// usage: vp8_enc_check [--k K] (<quality> <width> <height> <file.rgb>)...
//   file.rgb: height x width x 3 bytes.  Writes next to it, with <tag> = q<quality>: <file.rgb>.<tag>.mb (the vip_vp8_mb
//   records), .lv (int16 levels [mb][25][16], raster), .cf (the dequantised coefficient area, 25 blocks per macroblock),
//   .pl (the planes before the loop filter) and .out (the decoded RGB), and prints "width height base_q filter_level i4_macroblocks macroblocks".
//   --k K: another mode-bias factor than the product's (for fitting it).
//   vp8_enc_check --roundtrip N SEED: max |idct(fdct(x)) - x| over N random residual blocks in -255..255 and the same for
//   WHT then inverse WHT over N sets of luma DCs a forward DCT can give, and how often the quantiser's reciprocal
//   multiplication differs from a division over every step 2..1023 and value; prints the three.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "vipcup_hip.h"
#include "vp8_enc.hpp"
#include "vp8_params.hpp"

static char last_error[512];
void vip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
}

static int edge_sum(const uint8_t* plane, int stride, int size, int mx, int my, bool top) {
    int s = 0;
    for (int i = 0; i < size; ++i) {
        if (top) s += my > 0 ? plane[(int64_t)(my * size - 1) * stride + mx * size + i] : 0;
        else s += mx > 0 ? plane[(int64_t)(my * size + i) * stride + mx * size - 1] : 0;
    }
    return s;
}

static void check_i16(const int16_t* cf, const int16_t* lv, const vip_vp8_enc_params& E, int b) {
    for (int i = 0; i < 16; ++i) {
        const int v = lv[i] * vp8e_step(E, b, i);
        if (v < -32768 || v > 32767 || v != cf[i]) {
            fprintf(stderr, "dequantised value %d of block %d does not fit int16\n", v, b);
            exit(6);
        }
    }
}

static void encode_mb(const uint8_t* rgb, int w, int h, const Vp8Planes& P, const vip_vp8_enc_params& E, int mx, int my, vip_vp8_mb* mbs,
                      int16_t* coefs, int16_t* levels) {
    const size_t idx = (size_t)my * P.mb_w + mx;
    uint8_t src[VP8E_SRC_BYTES];
    for (int q = 0; q < 64; ++q) vp8e_convert_quad(rgb, w, w, h, mx, my, q & 7, q >> 3, src);
    const int dc_y = vp8_dc_value(edge_sum(P.y, P.ys, 16, mx, my, true), edge_sum(P.y, P.ys, 16, mx, my, false), 16, mx, my);
    const int dc_u = vp8_dc_value(edge_sum(P.u, P.cs, 8, mx, my, true), edge_sum(P.u, P.cs, 8, mx, my, false), 8, mx, my);
    const int dc_v = vp8_dc_value(edge_sum(P.v, P.cs, 8, mx, my, true), edge_sum(P.v, P.cs, 8, mx, my, false), 8, mx, my);
    // modes: DC, TM, VE, HE are 0..3, so "the first in that order" is the lowest number
    int uvmode = 0, ymode = 0;
    long best_uv = -1, s16 = -1;
    for (int mode = 0; mode < 4; ++mode) {
        long s = 0;
        for (int item = 0; item < 32; ++item) s += vp8e_sse_chroma_item(src, P, mode, mx, my, item, dc_u, dc_v);
        if (best_uv < 0 || s < best_uv) best_uv = s, uvmode = mode;
        s = 0;
        for (int item = 0; item < 64; ++item) s += vp8e_sse_luma16_item(src, P, mode, mx, my, item, dc_y);
        if (s16 < 0 || s < s16) s16 = s, ymode = mode;
    }
    int16_t* lv = levels + idx * 400;
    memset(lv, 0, 400 * sizeof(int16_t));
    uint8_t bmodes[16];
    long s4 = 0;
    for (int b = 0; b < 16; ++b) {
        const int bx = b & 3, by = b >> 2;
        int e[13];
        vp8_edges4(P, mx, my, bx, by, e);
        long best = -1;
        int bm = 0;
        int d[16];
        for (int mode = 0; mode < 10; ++mode) {
            long s = 0;
            vp8_pred4_block(mode, e, d);
            for (int k = 0; k < 4; ++k) s += vp8e_sse_sub_row(src, d, bx, by, k);
            if (best < 0 || s < best) best = s, bm = mode;
        }
        bmodes[b] = (uint8_t)bm;
        s4 += best;
        vp8_pred4_block(bm, e, d);
        vp8e_code_sub_block(src, d, E, bx, by, lv + b * 16);
        int16_t cf[16];
        bool any, only0;
        vp8e_dequant_block(lv + b * 16, E, b, cf, &any, &only0);
        for (int k = 0; k < 4; ++k) vp8e_recon_sub_row(P, mx, my, bx, by, k, d, cf, any, only0);
    }
    const bool i4 = s4 + E.i4_bias < s16;
    if (!i4) {
        int dc[16];
        for (int b = 0; b < 16; ++b) vp8e_code_large_block(src, P, E, mx, my, b, ymode, dc_y, lv + b * 16, &dc[b]);
        vp8e_code_y2(dc, E, lv + 24 * 16);
    }
    for (int b = 16; b < 24; ++b) vp8e_code_large_block(src, P, E, mx, my, b, uvmode, b < 20 ? dc_u : dc_v, lv + b * 16, nullptr);
    // the record and the coded blocks back to back
    uint32_t nz = 0, dconly = 0;
    int16_t cf[25][16];
    for (int b = 0; b < 25; ++b) {
        bool any, only0;
        vp8e_dequant_block(lv + b * 16, E, b, cf[b], &any, &only0);
        check_i16(cf[b], lv + b * 16, E, b);
        nz |= (uint32_t)any << b;
        dconly |= (uint32_t)only0 << b;
    }
    vip_vp8_mb& M = mbs[idx];
    vp8e_record(M, E, i4, ymode, bmodes, uvmode, nz, dconly, cf[24], (uint32_t)(idx * 25));
    int16_t* out = coefs + idx * 400;
    memset(out, 0, 400 * sizeof(int16_t));
    for (int b = 0; b < 25; ++b)
        if ((M.nz >> b) & 1u) {
            memcpy(out, cf[b], 32);
            out += 16;
        }
    // the decoder's reconstruction; sub-block luma stands already
    for (int item = i4 ? 64 : 0; item < 96; ++item) vp8_recon_item(P, M, coefs, mx, my, item, dc_y, dc_u, dc_v);
}

static void dump(const std::string& name, const void* p, size_t n) {
    FILE* fp = fopen(name.c_str(), "wb");
    if (!fp || fwrite(p, 1, n, fp) != n) {
        fprintf(stderr, "cannot write %s\n", name.c_str());
        exit(5);
    }
    fclose(fp);
}

static uint32_t rng_state;
static int rnd(int lo, int hi) {                             // xorshift32
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return lo + (int)(rng_state % (uint32_t)(hi - lo + 1));
}

static int roundtrip(int n, int seed) {
    rng_state = (uint32_t)seed * 2654435761u + 1u;
    int worst_dct = 0, worst_wht = 0;
    for (int t = 0; t < n; ++t) {
        int x[16], c[16];
        const int kind = t % 4, amp = kind == 0 ? 255 : kind == 1 ? 16 : kind == 2 ? 255 : 3;
        const int base = kind == 2 ? rnd(-255, 255) : 0;
        for (int i = 0; i < 16; ++i) {
            x[i] = kind == 2 ? base : rnd(-amp, amp);        // kind 2: a flat block, the extreme of the DC
        }
        vp8e_fdct(x, c);
        int16_t cf[16];
        for (int i = 0; i < 16; ++i) cf[i] = (int16_t)c[i];
        for (int k = 0; k < 4; ++k) {
            int r[4];
            vp8_idct_row(cf, 0, false, k, r);
            for (int i = 0; i < 4; ++i) worst_dct = vp8_abs(r[i] - x[k * 4 + i]) > worst_dct ? vp8_abs(r[i] - x[k * 4 + i]) : worst_dct;
        }
        // DC sets: what a forward DCT gives, -2040..2040
        int dc[16], y2[16];
        for (int i = 0; i < 16; ++i) dc[i] = kind == 2 ? base * 8 : rnd(-amp * 8, amp * 8);
        vp8e_fwht(dc, y2);
        int16_t y2s[16];
        for (int i = 0; i < 16; ++i) y2s[i] = (int16_t)y2[i];
        for (int b = 0; b < 16; ++b) worst_wht = vp8_abs(vp8_wht_dc(y2s, b) - dc[b]) > worst_wht ? vp8_abs(vp8_wht_dc(y2s, b) - dc[b]) : worst_wht;
    }
    // the quantiser divides by multiplying: every step with every value it is specified for
    long bad = 0;
    for (int q = 2; q < 1024; ++q) {
        const uint32_t inv = vp8_params::reciprocal(q);
        for (int c = 0; c < 65536 - ((3 * q) >> 3); ++c) {
            int want = (c + ((3 * q) >> 3)) / q;
            if (want > VP8E_MAX_LEVEL) want = VP8E_MAX_LEVEL;
            bad += vp8e_quant(c, q, inv) != want || vp8e_quant(-c, q, inv) != -want;
        }
    }
    printf("%d %d %ld\n", worst_dct, worst_wht, bad);
    return 0;
}

int main(int argc, char** argv) {
    int a = 1, k_override = -1;
    if (argc >= 4 && !strcmp(argv[1], "--roundtrip")) return roundtrip(atoi(argv[2]), atoi(argv[3]));
    if (argc >= 3 && !strcmp(argv[1], "--k")) {
        k_override = atoi(argv[2]);
        a = 3;
    }
    for (; a + 3 < argc; a += 4) {
        const int quality = atoi(argv[a]), w = atoi(argv[a + 1]), h = atoi(argv[a + 2]);
        const std::string path = argv[a + 3];
        vip_vp8_enc_params E;
        vip_vp8_desc D;
        const int32_t hw[2] = {h, w};
        size_t stream_bytes = 0, scratch_bytes = 0;
        if (vip_vp8_encode_params_h(quality, &E) != VIP_OK || vip_vp8_encode_layout_h(hw, 1, quality, &D, &stream_bytes, &scratch_bytes) != VIP_OK) {
            fprintf(stderr, "%s: %s\n", path.c_str(), last_error);
            return 4;
        }
        if (k_override >= 0) E.i4_bias = (k_override * E.y1[1] * E.y1[1]) >> 4;
        std::vector<uint8_t> rgb((size_t)w * h * 3);
        FILE* fp = fopen(path.c_str(), "rb");
        if (!fp || fread(rgb.data(), 1, rgb.size(), fp) != rgb.size()) return 3;
        fclose(fp);
        const size_t nmb = (size_t)D.mb_w * D.mb_h;
        std::vector<vip_vp8_mb> mbs(nmb);
        std::vector<int16_t> coefs(nmb * 400), levels(nmb * 400);
        std::vector<uint8_t> planes(nmb * 384);
        const Vp8Planes P = vp8_planes(planes.data(), D.mb_w, D.mb_h);
        int n_i4 = 0;
        for (int my = 0; my < D.mb_h; ++my)
            for (int mx = 0; mx < D.mb_w; ++mx) {
                encode_mb(rgb.data(), w, h, P, E, mx, my, mbs.data(), coefs.data(), levels.data());
                n_i4 += mbs[(size_t)my * D.mb_w + mx].ymode == VIP_VP8_B_PRED;
            }
        const std::string tag = path + ".q" + std::to_string(quality);
        dump(tag + ".pl", planes.data(), planes.size());
        if (D.filter_type)
            for (int my = 0; my < D.mb_h; ++my)
                for (int mx = 0; mx < D.mb_w; ++mx) {
                    const vip_vp8_mb& M = mbs[(size_t)my * D.mb_w + mx];
                    for (int item = 0; item < 32; ++item) vp8_filter_item(P, M, D.filter_type, mx, my, item, false);
                    for (int item = 0; item < 32; ++item) vp8_filter_item(P, M, D.filter_type, mx, my, item, true);
                }
        std::vector<uint8_t> out((size_t)w * h * 3);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) vp8_rgb_px(P, w, h, x, y, &out[((size_t)y * w + x) * 3]);
        dump(tag + ".mb", mbs.data(), nmb * sizeof(vip_vp8_mb));
        dump(tag + ".lv", levels.data(), levels.size() * 2);
        dump(tag + ".cf", coefs.data(), coefs.size() * 2);
        dump(tag + ".out", out.data(), out.size());
        printf("%d %d %d %d %d %zu\n", w, h, E.base_q, E.filter_level, n_i4, nmb);
    }
    return 0;
}
