// The pixel arithmetic of the lossy WebP path, written once for the device (vp8_pipeline.hip) and for a plain C++ build
// (tests/fuzz/vp8_recon_check.cpp runs it serially on the CPU): intra prediction, inverse WHT / DCT, the in-loop filter,
// the "fancy" chroma upsampler and the YUV -> RGB conversion, each as libwebp's decoder computes it.  Everything is
// integer; the unit of work is small (four pixels of one block row, one line across one edge, one output pixel) and
// free of any order of its own - the callers own the order: macroblock (x, y) after (x-1, y), (x, y-1), (x-1, y-1) and
// (x+1, y-1), and inside a macroblock with sub-block modes the same rule over its 16 sub-blocks.
#pragma once
#include <stdint.h>

#include "vipcup_hip.h"

#if defined(__HIPCC__)
#define VP8_HD __host__ __device__ __forceinline__
#else
#define VP8_HD inline
#endif

// the planes of one image: Y [16 mb_h][16 mb_w], U and V [8 mb_h][8 mb_w]
struct Vp8Planes {
    uint8_t *y, *u, *v;
    int ys, cs;                          // strides
    int mb_w, mb_h;
};

VP8_HD Vp8Planes vp8_planes(uint8_t* base, int mb_w, int mb_h) {
    Vp8Planes P;
    P.y = base;
    P.u = base + (int64_t)mb_w * mb_h * 256;
    P.v = P.u + (int64_t)mb_w * mb_h * 64;
    P.ys = mb_w * 16;
    P.cs = mb_w * 8;
    P.mb_w = mb_w;
    P.mb_h = mb_h;
    return P;
}

VP8_HD int vp8_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
VP8_HD int vp8_mul1(int a) { return ((a * 20091) >> 16) + a; }
VP8_HD int vp8_mul2(int a) { return (a * 35468) >> 16; }
VP8_HD int vp8_popc(uint32_t v) {
    int n = 0;
    for (; v; v &= v - 1) ++n;
    return n;
}

// ---- inverse transforms --------------------------------------------------------------------------------------

// DC of luma block b (0..15) from the 16 Y2 coefficients: libwebp's TransformWHT, results kept as int16
VP8_HD int vp8_wht_dc(const int16_t* in, int b) {
    int tmp[16];
    for (int i = 0; i < 4; ++i) {
        const int a0 = in[0 + i] + in[12 + i], a1 = in[4 + i] + in[8 + i], a2 = in[4 + i] - in[8 + i], a3 = in[0 + i] - in[12 + i];
        tmp[0 + i] = a0 + a1;
        tmp[8 + i] = a0 - a1;
        tmp[4 + i] = a3 + a2;
        tmp[12 + i] = a3 - a2;
    }
    const int i = b >> 2;
    const int dc = tmp[0 + i * 4] + 3;
    const int a0 = dc + tmp[3 + i * 4], a1 = tmp[1 + i * 4] + tmp[2 + i * 4], a2 = tmp[1 + i * 4] - tmp[2 + i * 4], a3 = dc - tmp[3 + i * 4];
    const int j = b & 3;
    const int v = j == 0 ? a0 + a1 : j == 1 ? a3 + a2 : j == 2 ? a0 - a1 : a3 - a2;
    return (int16_t)(v >> 3);
}

// row k of the 4x4 inverse DCT of `in` (16 coefficients in raster order, or null: none) with dc added to in[0]; the
// values are what libwebp adds to the prediction (already >> 3).  dc_only: every other coefficient is known to be zero.
VP8_HD void vp8_idct_row(const int16_t* in, int dc, bool dc_only, int k, int r[4]) {
    if (!in || dc_only) {
        const int v = ((in ? in[0] + dc : dc) + 4) >> 3;
        r[0] = r[1] = r[2] = r[3] = v;
        return;
    }
    int t[4];
    for (int i = 0; i < 4; ++i) {
        const int c0 = in[i] + (i == 0 ? dc : 0), c1 = in[4 + i], c2 = in[8 + i], c3 = in[12 + i];
        const int a = c0 + c2, b = c0 - c2;
        const int c = vp8_mul2(c1) - vp8_mul1(c3), d = vp8_mul1(c1) + vp8_mul2(c3);
        t[i] = k == 0 ? a + d : k == 1 ? b + c : k == 2 ? b - c : a - d;
    }
    const int e = t[0] + 4;
    const int a = e + t[2], b = e - t[2];
    const int c = vp8_mul2(t[1]) - vp8_mul1(t[3]), d = vp8_mul1(t[1]) + vp8_mul2(t[3]);
    r[0] = (a + d) >> 3;
    r[1] = (b + c) >> 3;
    r[2] = (b - c) >> 3;
    r[3] = (a - d) >> 3;
}

// the coefficients of block b of a macroblock, or null when it is not coded
VP8_HD const int16_t* vp8_block(const vip_vp8_mb& M, const int16_t* coefs, int b) {
    if (!((M.nz >> b) & 1u)) return nullptr;
    return coefs + ((int64_t)M.coef_idx + vp8_popc(M.nz & ((1u << b) - 1u))) * 16;
}

// ---- prediction ----------------------------------------------------------------------------------------------
// Samples outside the image: 127 above it (the corner included), 129 left of it.

// the value of a 16x16 / 8x8 DC prediction from the sums of the `size` samples above and left (libwebp's CheckMode)
VP8_HD int vp8_dc_value(int sum_top, int sum_left, int size, int mx, int my) {
    const int sh = size == 16 ? 4 : 3;
    if (mx > 0 && my > 0) return (sum_top + sum_left + size) >> (sh + 1);
    if (my > 0) return (sum_top + (size >> 1)) >> sh;
    if (mx > 0) return (sum_left + (size >> 1)) >> sh;
    return 128;
}

// four predicted pixels of a 16x16 luma or 8x8 chroma macroblock: row y (inside the macroblock), columns x .. x + 3
VP8_HD void vp8_pred_large_row(const uint8_t* plane, int stride, int size, int mode, int mx, int my, int x, int y, int dcval,
                               int out[4]) {
    const int px0 = mx * size, py0 = my * size;
    if (mode == VIP_VP8_B_DC) {
        out[0] = out[1] = out[2] = out[3] = dcval;
        return;
    }
    if (mode == VIP_VP8_B_HE) {
        out[0] = out[1] = out[2] = out[3] = mx == 0 ? 129 : plane[(int64_t)(py0 + y) * stride + px0 - 1];
        return;
    }
    int top[4];
    for (int i = 0; i < 4; ++i) top[i] = my == 0 ? 127 : plane[(int64_t)(py0 - 1) * stride + px0 + x + i];
    if (mode == VIP_VP8_B_VE) {
        for (int i = 0; i < 4; ++i) out[i] = top[i];
        return;
    }
    const int left = mx == 0 ? 129 : plane[(int64_t)(py0 + y) * stride + px0 - 1];
    const int corner = my == 0 ? 127 : mx == 0 ? 129 : plane[(int64_t)(py0 - 1) * stride + px0 - 1];
    for (int i = 0; i < 4; ++i) out[i] = vp8_clip8(top[i] + left - corner);
}

// the 13 samples around luma sub-block (bx, by) of macroblock (mx, my): e[0] = corner, e[1..8] = the row above (A..H,
// the last four "above right"), e[9..12] = the column to the left (I..L).  The sub-blocks of the right column take their
// above-right samples from the macroblock row above, whatever their own row.
VP8_HD void vp8_edges4(const Vp8Planes& P, int mx, int my, int bx, int by, int e[13]) {
    const int X0 = mx * 16 + bx * 4, Y0 = my * 16 + by * 4;
    const uint8_t* y = P.y;
    const int s = P.ys;
    if (Y0 == 0) {
        for (int i = 0; i < 9; ++i) e[i] = 127;
    } else {
        const uint8_t* row = y + (int64_t)(Y0 - 1) * s;
        e[0] = X0 == 0 ? 129 : row[X0 - 1];
        for (int i = 0; i < 4; ++i) e[1 + i] = row[X0 + i];
        if (bx < 3) {
            for (int i = 4; i < 8; ++i) e[1 + i] = row[X0 + i];
        } else if (my == 0) {
            for (int i = 4; i < 8; ++i) e[1 + i] = 127;
        } else {
            const uint8_t* above = y + (int64_t)(my * 16 - 1) * s;
            for (int i = 4; i < 8; ++i) e[1 + i] = mx == P.mb_w - 1 ? above[mx * 16 + 15] : above[X0 + i];
        }
    }
    for (int j = 0; j < 4; ++j) e[9 + j] = X0 == 0 ? 129 : y[(int64_t)(Y0 + j) * s + X0 - 1];
}

#define VP8_AVG3(a, b, c) (((a) + 2 * (b) + (c) + 2) >> 2)
#define VP8_AVG2(a, b) (((a) + (b) + 1) >> 1)

// the 4x4 prediction of one sub-block, d[x + 4 y]
VP8_HD void vp8_pred4_block(int mode, const int e[13], int d[16]) {
    const int X = e[0], A = e[1], B = e[2], C = e[3], D = e[4], E = e[5], F = e[6], G = e[7], H = e[8];
    const int I = e[9], J = e[10], K = e[11], L = e[12];
#define DST(x, y) d[(x) + (y) * 4]
    switch (mode) {
        case VIP_VP8_B_DC: {
            const int dc = (A + B + C + D + I + J + K + L + 4) >> 3;
            for (int i = 0; i < 16; ++i) d[i] = dc;
            break;
        }
        case VIP_VP8_B_TM:
            for (int y = 0; y < 4; ++y)
                for (int x = 0; x < 4; ++x) DST(x, y) = vp8_clip8(e[1 + x] + e[9 + y] - X);
            break;
        case VIP_VP8_B_VE: {
            const int v0 = VP8_AVG3(X, A, B), v1 = VP8_AVG3(A, B, C), v2 = VP8_AVG3(B, C, D), v3 = VP8_AVG3(C, D, E);
            for (int y = 0; y < 4; ++y) {
                DST(0, y) = v0;
                DST(1, y) = v1;
                DST(2, y) = v2;
                DST(3, y) = v3;
            }
            break;
        }
        case VIP_VP8_B_HE: {
            const int h0 = VP8_AVG3(X, I, J), h1 = VP8_AVG3(I, J, K), h2 = VP8_AVG3(J, K, L), h3 = VP8_AVG3(K, L, L);
            for (int x = 0; x < 4; ++x) {
                DST(x, 0) = h0;
                DST(x, 1) = h1;
                DST(x, 2) = h2;
                DST(x, 3) = h3;
            }
            break;
        }
        case VIP_VP8_B_RD:
            DST(0, 3) = VP8_AVG3(J, K, L);
            DST(1, 3) = DST(0, 2) = VP8_AVG3(I, J, K);
            DST(2, 3) = DST(1, 2) = DST(0, 1) = VP8_AVG3(X, I, J);
            DST(3, 3) = DST(2, 2) = DST(1, 1) = DST(0, 0) = VP8_AVG3(A, X, I);
            DST(3, 2) = DST(2, 1) = DST(1, 0) = VP8_AVG3(B, A, X);
            DST(3, 1) = DST(2, 0) = VP8_AVG3(C, B, A);
            DST(3, 0) = VP8_AVG3(D, C, B);
            break;
        case VIP_VP8_B_VR:
            DST(0, 0) = DST(1, 2) = VP8_AVG2(X, A);
            DST(1, 0) = DST(2, 2) = VP8_AVG2(A, B);
            DST(2, 0) = DST(3, 2) = VP8_AVG2(B, C);
            DST(3, 0) = VP8_AVG2(C, D);
            DST(0, 3) = VP8_AVG3(K, J, I);
            DST(0, 2) = VP8_AVG3(J, I, X);
            DST(0, 1) = DST(1, 3) = VP8_AVG3(I, X, A);
            DST(1, 1) = DST(2, 3) = VP8_AVG3(X, A, B);
            DST(2, 1) = DST(3, 3) = VP8_AVG3(A, B, C);
            DST(3, 1) = VP8_AVG3(B, C, D);
            break;
        case VIP_VP8_B_LD:
            DST(0, 0) = VP8_AVG3(A, B, C);
            DST(1, 0) = DST(0, 1) = VP8_AVG3(B, C, D);
            DST(2, 0) = DST(1, 1) = DST(0, 2) = VP8_AVG3(C, D, E);
            DST(3, 0) = DST(2, 1) = DST(1, 2) = DST(0, 3) = VP8_AVG3(D, E, F);
            DST(3, 1) = DST(2, 2) = DST(1, 3) = VP8_AVG3(E, F, G);
            DST(3, 2) = DST(2, 3) = VP8_AVG3(F, G, H);
            DST(3, 3) = VP8_AVG3(G, H, H);
            break;
        case VIP_VP8_B_VL:
            DST(0, 0) = VP8_AVG2(A, B);
            DST(1, 0) = DST(0, 2) = VP8_AVG2(B, C);
            DST(2, 0) = DST(1, 2) = VP8_AVG2(C, D);
            DST(3, 0) = DST(2, 2) = VP8_AVG2(D, E);
            DST(0, 1) = VP8_AVG3(A, B, C);
            DST(1, 1) = DST(0, 3) = VP8_AVG3(B, C, D);
            DST(2, 1) = DST(1, 3) = VP8_AVG3(C, D, E);
            DST(3, 1) = DST(2, 3) = VP8_AVG3(D, E, F);
            DST(3, 2) = VP8_AVG3(E, F, G);
            DST(3, 3) = VP8_AVG3(F, G, H);
            break;
        case VIP_VP8_B_HD:
            DST(0, 0) = DST(2, 1) = VP8_AVG2(I, X);
            DST(0, 1) = DST(2, 2) = VP8_AVG2(J, I);
            DST(0, 2) = DST(2, 3) = VP8_AVG2(K, J);
            DST(0, 3) = VP8_AVG2(L, K);
            DST(3, 0) = VP8_AVG3(A, B, C);
            DST(2, 0) = VP8_AVG3(X, A, B);
            DST(1, 0) = DST(3, 1) = VP8_AVG3(I, X, A);
            DST(1, 1) = DST(3, 2) = VP8_AVG3(J, I, X);
            DST(1, 2) = DST(3, 3) = VP8_AVG3(K, J, I);
            DST(1, 3) = VP8_AVG3(L, K, J);
            break;
        default:                                             // VIP_VP8_B_HU
            DST(0, 0) = VP8_AVG2(I, J);
            DST(2, 0) = DST(0, 1) = VP8_AVG2(J, K);
            DST(2, 1) = DST(0, 2) = VP8_AVG2(K, L);
            DST(1, 0) = VP8_AVG3(I, J, K);
            DST(3, 0) = DST(1, 1) = VP8_AVG3(J, K, L);
            DST(3, 1) = DST(1, 2) = VP8_AVG3(K, L, L);
            DST(3, 2) = DST(2, 2) = DST(0, 3) = DST(1, 3) = DST(2, 3) = DST(3, 3) = L;
            break;
    }
#undef DST
}

// row k of the 4x4 prediction of one sub-block
VP8_HD void vp8_pred4_row(int mode, const int e[13], int k, int out[4]) {
    int d[16];
    vp8_pred4_block(mode, e, d);
    for (int x = 0; x < 4; ++x) out[x] = d[k * 4 + x];
}

VP8_HD void vp8_store4(uint8_t* p, const int pred[4], const int res[4]) {
    for (int i = 0; i < 4; ++i) p[i] = (uint8_t)vp8_clip8(pred[i] + res[i]);
}

// One item of a macroblock with 16x16 luma prediction, or of any macroblock's chroma: item = block * 4 + row, blocks
// 0..15 luma, 16..19 U, 20..23 V.  Reads only samples outside the macroblock.  dc_y / dc_u / dc_v: vp8_dc_value of the planes.
VP8_HD void vp8_recon_item(const Vp8Planes& P, const vip_vp8_mb& M, const int16_t* coefs, int mx, int my, int item, int dc_y,
                           int dc_u, int dc_v) {
    const int b = item >> 2, k = item & 3;
    int pred[4], res[4];
    if (b < 16) {
        const int x = (b & 3) * 4, y = (b >> 2) * 4 + k;
        vp8_pred_large_row(P.y, P.ys, 16, M.ymode, mx, my, x, y, dc_y, pred);
        const int dc = (M.nz >> 24) & 1u ? vp8_wht_dc(vp8_block(M, coefs, 24), b) : 0;
        vp8_idct_row(vp8_block(M, coefs, b), dc, false, k, res);
        vp8_store4(P.y + (int64_t)(my * 16 + y) * P.ys + mx * 16 + x, pred, res);
    } else {
        uint8_t* plane = b < 20 ? P.u : P.v;
        const int c = b & 3;
        const int x = (c & 1) * 4, y = (c >> 1) * 4 + k;
        vp8_pred_large_row(plane, P.cs, 8, M.uvmode, mx, my, x, y, b < 20 ? dc_u : dc_v, pred);
        vp8_idct_row(vp8_block(M, coefs, b), 0, (M.dc_only >> b) & 1u, k, res);
        vp8_store4(plane + (int64_t)(my * 8 + y) * P.cs + mx * 8 + x, pred, res);
    }
}

// Row k of luma sub-block (bx, by) of a macroblock with sub-block modes; the sub-blocks left, above, above-left and
// above-right of it (inside the macroblock) are done.
VP8_HD void vp8_recon_sub_item(const Vp8Planes& P, const vip_vp8_mb& M, const int16_t* coefs, int mx, int my, int bx, int by, int k) {
    const int b = by * 4 + bx;
    int e[13], pred[4], res[4];
    vp8_edges4(P, mx, my, bx, by, e);
    vp8_pred4_row(M.bmodes[b], e, k, pred);
    vp8_idct_row(vp8_block(M, coefs, b), 0, (M.dc_only >> b) & 1u, k, res);
    vp8_store4(P.y + (int64_t)(my * 16 + by * 4 + k) * P.ys + mx * 16 + bx * 4, pred, res);
}

// ---- in-loop filter ------------------------------------------------------------------------------------------

VP8_HD int vp8_abs(int v) { return v < 0 ? -v : v; }
VP8_HD int vp8_sclip1(int v) { return v < -128 ? -128 : v > 127 ? 127 : v; }
VP8_HD int vp8_sclip2(int v) { return v < -16 ? -16 : v > 15 ? 15 : v; }

VP8_HD void vp8_filter2(uint8_t* p, int64_t step) {
    const int p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step];
    const int a = 3 * (q0 - p0) + vp8_sclip1(p1 - q1);
    const int a1 = vp8_sclip2((a + 4) >> 3), a2 = vp8_sclip2((a + 3) >> 3);
    p[-step] = (uint8_t)vp8_clip8(p0 + a2);
    p[0] = (uint8_t)vp8_clip8(q0 - a1);
}
VP8_HD void vp8_filter4(uint8_t* p, int64_t step) {
    const int p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step];
    const int a = 3 * (q0 - p0);
    const int a1 = vp8_sclip2((a + 4) >> 3), a2 = vp8_sclip2((a + 3) >> 3);
    const int a3 = (a1 + 1) >> 1;
    p[-2 * step] = (uint8_t)vp8_clip8(p1 + a3);
    p[-step] = (uint8_t)vp8_clip8(p0 + a2);
    p[0] = (uint8_t)vp8_clip8(q0 - a1);
    p[step] = (uint8_t)vp8_clip8(q1 - a3);
}
VP8_HD void vp8_filter6(uint8_t* p, int64_t step) {
    const int p2 = p[-3 * step], p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step], q2 = p[2 * step];
    const int a = vp8_sclip1(3 * (q0 - p0) + vp8_sclip1(p1 - q1));
    const int a1 = (27 * a + 63) >> 7, a2 = (18 * a + 63) >> 7, a3 = (9 * a + 63) >> 7;
    p[-3 * step] = (uint8_t)vp8_clip8(p2 + a3);
    p[-2 * step] = (uint8_t)vp8_clip8(p1 + a2);
    p[-step] = (uint8_t)vp8_clip8(p0 + a1);
    p[0] = (uint8_t)vp8_clip8(q0 - a1);
    p[step] = (uint8_t)vp8_clip8(q1 - a2);
    p[2 * step] = (uint8_t)vp8_clip8(q2 - a3);
}

// one line across one edge; step = distance between the samples of the line; thresh2 = 2 * limit + 1
VP8_HD void vp8_simple_edge(uint8_t* p, int64_t step, int thresh2) {
    const int p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step];
    if (4 * vp8_abs(p0 - q0) + vp8_abs(p1 - q1) <= thresh2) vp8_filter2(p, step);
}
VP8_HD void vp8_normal_edge(uint8_t* p, int64_t step, int thresh2, int it, int hev_t, bool mb_edge) {
    const int p3 = p[-4 * step], p2 = p[-3 * step], p1 = p[-2 * step], p0 = p[-step];
    const int q0 = p[0], q1 = p[step], q2 = p[2 * step], q3 = p[3 * step];
    if (4 * vp8_abs(p0 - q0) + vp8_abs(p1 - q1) > thresh2) return;
    if (vp8_abs(p3 - p2) > it || vp8_abs(p2 - p1) > it || vp8_abs(p1 - p0) > it || vp8_abs(q3 - q2) > it || vp8_abs(q2 - q1) > it ||
        vp8_abs(q1 - q0) > it)
        return;
    const bool hev = vp8_abs(p1 - p0) > hev_t || vp8_abs(q1 - q0) > hev_t;
    if (hev) vp8_filter2(p, step);
    else if (mb_edge) vp8_filter6(p, step);
    else vp8_filter4(p, step);
}

// One line of a macroblock's filter: item 0..15 a luma line, 16..23 a U line, 24..31 a V line.  vertical = false: the
// line is a row and crosses the left edge (mx > 0) and then the inner vertical edges; true: a column, crossing the top
// edge (my > 0) and the inner horizontal edges.  libwebp's order per macroblock is all rows, then all columns.
VP8_HD void vp8_filter_item(const Vp8Planes& P, const vip_vp8_mb& M, int filter_type, int mx, int my, int item, bool vertical) {
    if (M.flevel == 0) return;
    const int limit = 2 * M.flevel + M.ilevel;
    const int t_mb = 2 * (limit + 4) + 1, t_in = 2 * limit + 1;
    const bool luma = item < 16;
    if (filter_type == 1 && !luma) return;
    uint8_t* plane = luma ? P.y : item < 24 ? P.u : P.v;
    const int stride = luma ? P.ys : P.cs, size = luma ? 16 : 8, line = luma ? item : (item & 7);
    uint8_t* p = plane + (int64_t)my * size * stride + mx * size;
    int64_t step;
    if (!vertical) {
        p += (int64_t)line * stride;
        step = 1;
    } else {
        p += line;
        step = stride;
    }
    const bool edge = vertical ? my > 0 : mx > 0;
    if (filter_type == 1) {
        if (edge) vp8_simple_edge(p, step, t_mb);
        if (M.inner)
            for (int k = 4; k < 16; k += 4) vp8_simple_edge(p + k * step, step, t_in);
    } else {
        if (edge) vp8_normal_edge(p, step, t_mb, M.ilevel, M.hev, true);
        if (M.inner)
            for (int k = 4; k < size; k += 4) vp8_normal_edge(p + k * step, step, t_in, M.ilevel, M.hev, false);
    }
}

// ---- output --------------------------------------------------------------------------------------------------

VP8_HD int vp8_yuv_clip(int v) { return (v & ~16383) == 0 ? v >> 6 : v < 0 ? 0 : 255; }
VP8_HD int vp8_mult_hi(int v, int c) { return (v * c) >> 8; }

// libwebp's fancy upsampler at one pixel of one chroma plane: n the nearest sample, a1 / a2 the two next to it, o the
// one opposite; on the image's border the missing row or column mirrors the nearest one
VP8_HD int vp8_upsample(const uint8_t* c, int stride, int cw, int ch, int x, int y) {
    const int nr = y >> 1, nc = x >> 1;
    int fr = (y & 1) ? nr + 1 : nr - 1, fc = (x & 1) ? nc + 1 : nc - 1;
    fr = fr < 0 ? 0 : fr > ch - 1 ? ch - 1 : fr;
    const int n = c[(int64_t)nr * stride + nc], a2 = c[(int64_t)fr * stride + nc];
    if (fc < 0 || fc > cw - 1) return (3 * n + a2 + 2) >> 2;
    const int a1 = c[(int64_t)nr * stride + fc], o = c[(int64_t)fr * stride + fc];
    const int diag = (n + a1 + a2 + o + 8 + 2 * (a1 + a2)) >> 3;
    return (diag + n) >> 1;
}

VP8_HD void vp8_rgb_px(const Vp8Planes& P, int w, int h, int x, int y, uint8_t rgb[3]) {
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1;
    const int Y = P.y[(int64_t)y * P.ys + x];
    const int U = vp8_upsample(P.u, P.cs, cw, ch, x, y), V = vp8_upsample(P.v, P.cs, cw, ch, x, y);
    const int yy = vp8_mult_hi(Y, 19077);
    rgb[0] = (uint8_t)vp8_yuv_clip(yy + vp8_mult_hi(V, 26149) - 14234);
    rgb[1] = (uint8_t)vp8_yuv_clip(yy - vp8_mult_hi(U, 6419) - vp8_mult_hi(V, 13320) + 8708);
    rgb[2] = (uint8_t)vp8_yuv_clip(yy + vp8_mult_hi(U, 33050) - 17685);
}
