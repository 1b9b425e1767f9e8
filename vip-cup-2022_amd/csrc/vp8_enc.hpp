// The arithmetic of the lossy WebP re-save, written once for the device (vp8_encode.hip) and for a plain C++ build
// (tests/fuzz/vp8_enc_check.cpp runs it serially on the CPU): forward colour conversion, prediction errors, forward DCT /
// WHT, quantisation and the macroblock record.  The rules are the project's own (include/vipcup_hip.h states them); what a
// decoder must agree with - prediction, inverse transforms - is vp8_recon.hpp's, called from here.  Everything is integer,
// and as in vp8_recon.hpp the unit of work is small and free of any order of its own: the callers own the order.
#pragma once
#include "vp8_recon.hpp"

// the source samples of one macroblock: Y [16][16], U [8][8], V [8][8]
constexpr int VP8E_SRC_BYTES = 384;
constexpr int VP8E_SRC_U = 256, VP8E_SRC_V = 320;
constexpr int VP8E_MAX_LEVEL = 2047;

// ---- colour ----------------------------------------------------------------------------------------------------

VP8_HD int vp8e_luma(int r, int g, int b) { return (16839 * r + 33059 * g + 6420 * b + (16 << 16) + 32768) >> 16; }
// r, g, b: sums over a 2 x 2 block
VP8_HD int vp8e_chroma_u(int r, int g, int b) { return vp8_clip8((-9719 * r - 19081 * g + 28800 * b + (128 << 18) + (1 << 17)) >> 18); }
VP8_HD int vp8e_chroma_v(int r, int g, int b) { return vp8_clip8((28800 * r - 24116 * g - 4684 * b + (128 << 18) + (1 << 17)) >> 18); }

// One 2 x 2 quad (qx, qy in 0..7) of macroblock (mx, my): four luma samples and one U, V into src.  rgb: the image's
// pixels [.][row_px][3], w x h of them valid; coordinates past the image take the last column / row.
VP8_HD void vp8e_convert_quad(const uint8_t* rgb, int64_t row_px, int w, int h, int mx, int my, int qx, int qy, uint8_t* src) {
    int sr = 0, sg = 0, sb = 0;
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            int x = mx * 16 + qx * 2 + dx, y = my * 16 + qy * 2 + dy;
            x = x > w - 1 ? w - 1 : x;
            y = y > h - 1 ? h - 1 : y;
            const uint8_t* p = rgb + ((int64_t)y * row_px + x) * 3;
            const int r = p[0], g = p[1], b = p[2];
            src[(qy * 2 + dy) * 16 + qx * 2 + dx] = (uint8_t)vp8e_luma(r, g, b);
            sr += r;
            sg += g;
            sb += b;
        }
    src[VP8E_SRC_U + qy * 8 + qx] = (uint8_t)vp8e_chroma_u(sr, sg, sb);
    src[VP8E_SRC_V + qy * 8 + qx] = (uint8_t)vp8e_chroma_v(sr, sg, sb);
}

// ---- forward transforms ----------------------------------------------------------------------------------------

// 4 x 4 forward DCT of a residual block (raster order), the integer form of VP8 encoders (libvpx's short_fdct4x4)
VP8_HD void vp8e_fdct(const int in[16], int out[16]) {
    int t[16];
    for (int i = 0; i < 4; ++i) {
        const int* ip = in + 4 * i;
        const int a1 = (ip[0] + ip[3]) * 8, b1 = (ip[1] + ip[2]) * 8, c1 = (ip[1] - ip[2]) * 8, d1 = (ip[0] - ip[3]) * 8;
        t[4 * i + 0] = a1 + b1;
        t[4 * i + 2] = a1 - b1;
        t[4 * i + 1] = (c1 * 2217 + d1 * 5352 + 14500) >> 12;
        t[4 * i + 3] = (d1 * 2217 - c1 * 5352 + 7500) >> 12;
    }
    for (int i = 0; i < 4; ++i) {
        const int a1 = t[i] + t[12 + i], b1 = t[4 + i] + t[8 + i], c1 = t[4 + i] - t[8 + i], d1 = t[i] - t[12 + i];
        out[i] = (a1 + b1 + 7) >> 4;
        out[8 + i] = (a1 - b1 + 7) >> 4;
        out[4 + i] = ((c1 * 2217 + d1 * 5352 + 12000) >> 16) + (d1 != 0);
        out[12 + i] = (d1 * 2217 - c1 * 5352 + 51000) >> 16;
    }
}

// forward WHT of the sixteen luma DCs of a macroblock (libvpx's short_walsh4x4)
VP8_HD void vp8e_fwht(const int in[16], int out[16]) {
    int t[16];
    for (int i = 0; i < 4; ++i) {
        const int* ip = in + 4 * i;
        const int a1 = (ip[0] + ip[2]) * 4, d1 = (ip[1] + ip[3]) * 4, c1 = (ip[1] - ip[3]) * 4, b1 = (ip[0] - ip[2]) * 4;
        t[4 * i + 0] = a1 + d1 + (a1 != 0);
        t[4 * i + 1] = b1 + c1;
        t[4 * i + 2] = b1 - c1;
        t[4 * i + 3] = a1 - d1;
    }
    for (int i = 0; i < 4; ++i) {
        const int a1 = t[i] + t[8 + i], d1 = t[4 + i] + t[12 + i], c1 = t[4 + i] - t[12 + i], b1 = t[i] - t[8 + i];
        int a2 = a1 + d1, b2 = b1 + c1, c2 = b1 - c1, d2 = a1 - d1;
        a2 += a2 < 0;
        b2 += b2 < 0;
        c2 += c2 < 0;
        d2 += d2 < 0;
        out[i] = (a2 + 3) >> 3;
        out[4 + i] = (b2 + 3) >> 3;
        out[8 + i] = (c2 + 3) >> 3;
        out[12 + i] = (d2 + 3) >> 3;
    }
}

// level = sign(c) min(2047, (|c| + ((3 q) >> 3)) / q), the division as one multiplication: inv = ceil(2^32 / q)
// (vp8_params.hpp's reciprocal), exact while |c| + ((3 q) >> 3) < 65536 - and no coefficient here reaches 2^15
VP8_HD int vp8e_quant(int c, int q, uint32_t inv) {
    const uint32_t a = (uint32_t)(c < 0 ? -c : c) + (uint32_t)((3 * q) >> 3);
    int l = (int)(((uint64_t)a * inv) >> 32);
    if (l > VP8E_MAX_LEVEL) l = VP8E_MAX_LEVEL;
    return c < 0 ? -l : l;
}

// ---- prediction errors -----------------------------------------------------------------------------------------

VP8_HD int vp8e_sse4(const uint8_t* s, const int pred[4]) {
    int e = 0;
    for (int i = 0; i < 4; ++i) {
        const int d = (int)s[i] - pred[i];
        e += d * d;
    }
    return e;
}

// squared error of four pixels of a 16 x 16 luma prediction: item 0..63 = row (item >> 2), columns 4 (item & 3) ..
VP8_HD int vp8e_sse_luma16_item(const uint8_t* src, const Vp8Planes& P, int mode, int mx, int my, int item, int dc_y) {
    const int x = (item & 3) * 4, y = item >> 2;
    int pred[4];
    vp8_pred_large_row(P.y, P.ys, 16, mode, mx, my, x, y, dc_y, pred);
    return vp8e_sse4(src + y * 16 + x, pred);
}

// the same of a chroma prediction: item 0..15 U, 16..31 V; inside a plane row (item >> 1) & 7, columns 4 (item & 1) ..
VP8_HD int vp8e_sse_chroma_item(const uint8_t* src, const Vp8Planes& P, int mode, int mx, int my, int item, int dc_u, int dc_v) {
    const bool v = item >= 16;
    const int x = (item & 1) * 4, y = (item >> 1) & 7;
    int pred[4];
    vp8_pred_large_row(v ? P.v : P.u, P.cs, 8, mode, mx, my, x, y, v ? dc_v : dc_u, pred);
    return vp8e_sse4(src + (v ? VP8E_SRC_V : VP8E_SRC_U) + y * 8 + x, pred);
}

// row k of a 4x4 prediction d (vp8_pred4_block), by selects: k differs between lanes and d stays in registers
VP8_HD void vp8e_row_of(const int d[16], int k, int out[4]) {
    for (int x = 0; x < 4; ++x) out[x] = k == 0 ? d[x] : k == 1 ? d[4 + x] : k == 2 ? d[8 + x] : d[12 + x];
}

// row k of sub-block (bx, by) under the prediction d
VP8_HD int vp8e_sse_sub_row(const uint8_t* src, const int d[16], int bx, int by, int k) {
    int pred[4];
    vp8e_row_of(d, k, pred);
    return vp8e_sse4(src + (by * 4 + k) * 16 + bx * 4, pred);
}

// ---- blocks ----------------------------------------------------------------------------------------------------

// levels (raster order) of a transformed block: q[0] / inv[0] for [0], q[1] / inv[1] for the rest
VP8_HD void vp8e_quant_block(const int c[16], const int32_t q[2], const uint32_t inv[2], int16_t lv[16]) {
    lv[0] = (int16_t)vp8e_quant(c[0], q[0], inv[0]);
    for (int i = 1; i < 16; ++i) lv[i] = (int16_t)vp8e_quant(c[i], q[1], inv[1]);
}

// Block b of a macroblock with 16 x 16 luma prediction (b 0..15) or of any macroblock's chroma (16..19 U, 20..23 V),
// predicted with `mode`: its levels; a luma block's DC goes to the WHT, so it comes back in *dc and lv[0] is 0.
VP8_HD void vp8e_code_large_block(const uint8_t* src, const Vp8Planes& P, const vip_vp8_enc_params& E, int mx, int my, int b, int mode,
                                  int dcval, int16_t lv[16], int* dc) {
    int res[16], c[16], pred[4];
    if (b < 16) {
        const int x = (b & 3) * 4, y = (b >> 2) * 4;
        for (int k = 0; k < 4; ++k) {
            vp8_pred_large_row(P.y, P.ys, 16, mode, mx, my, x, y + k, dcval, pred);
            for (int i = 0; i < 4; ++i) res[k * 4 + i] = (int)src[(y + k) * 16 + x + i] - pred[i];
        }
        vp8e_fdct(res, c);
        vp8e_quant_block(c, E.y1, E.y1_inv, lv);
        lv[0] = 0;
        *dc = c[0];
    } else {
        const int cb = b & 3, x = (cb & 1) * 4, y = (cb >> 1) * 4;
        const uint8_t* s = src + (b < 20 ? VP8E_SRC_U : VP8E_SRC_V);
        for (int k = 0; k < 4; ++k) {
            vp8_pred_large_row(b < 20 ? P.u : P.v, P.cs, 8, mode, mx, my, x, y + k, dcval, pred);
            for (int i = 0; i < 4; ++i) res[k * 4 + i] = (int)s[(y + k) * 8 + x + i] - pred[i];
        }
        vp8e_fdct(res, c);
        vp8e_quant_block(c, E.uv, E.uv_inv, lv);
    }
}

// Y2 of a macroblock with 16 x 16 luma prediction from the sixteen DCs vp8e_code_large_block returned
VP8_HD void vp8e_code_y2(const int dc[16], const vip_vp8_enc_params& E, int16_t lv[16]) {
    int c[16];
    vp8e_fwht(dc, c);
    vp8e_quant_block(c, E.y2, E.y2_inv, lv);
}

// levels of sub-block (bx, by) under the prediction d
VP8_HD void vp8e_code_sub_block(const uint8_t* src, const int d[16], const vip_vp8_enc_params& E, int bx, int by, int16_t lv[16]) {
    int res[16], c[16];
    for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 4; ++i) res[k * 4 + i] = (int)src[(by * 4 + k) * 16 + bx * 4 + i] - d[k * 4 + i];
    vp8e_fdct(res, c);
    vp8e_quant_block(c, E.y1, E.y1_inv, lv);
}

// the step that dequantises position i of block b (0..15 luma, 16..23 chroma, 24 Y2)
VP8_HD int vp8e_step(const vip_vp8_enc_params& E, int b, int i) {
    if (b < 16) return i > 0 ? E.y1[1] : E.y1[0];
    if (b < 24) return i > 0 ? E.uv[1] : E.uv[0];
    return i > 0 ? E.y2[1] : E.y2[0];
}

// what the decoder will see of a block; *any / *only0: a non-zero level / none but [0]
VP8_HD void vp8e_dequant_block(const int16_t lv[16], const vip_vp8_enc_params& E, int b, int16_t cf[16], bool* any, bool* only0) {
    bool ac = false;
    for (int i = 0; i < 16; ++i) {
        cf[i] = (int16_t)(lv[i] * vp8e_step(E, b, i));
        if (i > 0 && lv[i]) ac = true;
    }
    *any = ac || lv[0] != 0;
    *only0 = !ac && lv[0] != 0;
}

// Row k of sub-block (bx, by) as the decoder reconstructs it - the steps of vp8_recon_sub_item on the prediction d that
// stands already and on the block's own coefficients: not coded -> no residual, only [0] -> the DC-only inverse
VP8_HD void vp8e_recon_sub_row(const Vp8Planes& P, int mx, int my, int bx, int by, int k, const int d[16], const int16_t cf[16], bool any,
                               bool only0) {
    int pred[4], res[4];
    vp8e_row_of(d, k, pred);
    vp8_idct_row(any ? cf : nullptr, 0, only0, k, res);
    vp8_store4(P.y + (int64_t)(my * 16 + by * 4 + k) * P.ys + mx * 16 + bx * 4, pred, res);
}

// The record of a macroblock from its decisions: nz / dc_only over the 25 blocks (bit b: vp8e_dequant_block's any / only0,
// luma blocks of a 16 x 16 macroblock and Y2 never dc_only), y2: the dequantised Y2 block (read when bit 24 of nz is set).
// The filter's inner-edge flag is the decoder's rule: sub-block modes, or anything the inverse transforms would add.
VP8_HD void vp8e_record(vip_vp8_mb& M, const vip_vp8_enc_params& E, bool i4, int ymode, const uint8_t bmodes[16], int uvmode, uint32_t nz,
                        uint32_t dc_only, const int16_t* y2, uint32_t coef_idx) {
    M = vip_vp8_mb{};
    M.ymode = (uint8_t)(i4 ? VIP_VP8_B_PRED : ymode);
    M.uvmode = (uint8_t)uvmode;
    for (int i = 0; i < 16; ++i) M.bmodes[i] = i4 ? bmodes[i] : (uint8_t)0;          // zero as the host decoder leaves them
    nz &= i4 ? 0xffffffu : 0x1ffffffu;
    dc_only &= i4 ? 0xffffffu : 0xff0000u;
    bool any = (nz & 0xffffffu) != 0;
    if ((nz >> 24) & 1u)
        for (int b = 0; b < 16; ++b) any = any || vp8_wht_dc(y2, b) != 0;
    M.nz = nz;
    M.dc_only = dc_only;
    M.coef_idx = coef_idx;
    M.skip = (uint8_t)(nz == 0);
    M.flevel = (uint8_t)E.flevel;
    M.ilevel = (uint8_t)E.ilevel;
    M.hev = (uint8_t)E.hev;
    M.inner = (uint8_t)(i4 || any);
}
