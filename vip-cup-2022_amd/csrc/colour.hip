// A 3 x 3 colour matrix, a per-image mean term, an offset and a look-up table on decoded u8 RGB pixels, all in integers: the one kernel
// under the colour stress perturbations (pipeline.gray, bgr, hue, saturation, contrast, brightness, gamma; --stress-gray / -bgr / -hue /
// -saturation / -contrast / -brightness / -gamma), the inference-time form of dataset/augment.py's RandomGray (:142-146), RandomBGR
// (:148-151) and RandomJitter (:122-129).  Every image of a mixed-size batch keeps its size.
//
// Arithmetic (part of the interface; include/vipcup_hip.h).  Pixel (R, G, B) of image i, output channel c, coefficients M[3][3], K[3],
// O[3] in Q16, signed 32-bit integers throughout:
//   s_c   = M[c][0] R + M[c][1] G + M[c][2] B + K[c] mean_u8[i][c] + O[c] + 32768
//   v_c   = clamp(s_c >> 16, 0, 255)                                arithmetic shift: floor, also for a negative sum
//   out_c = lut ? lut[v_c] : v_c
// The entry point admits |M[c][k]| <= 2^18, |K[c]| <= 2^18 and |O[c]| <= 2^25 only, so with samples and means of at most 255
//   |s_c| <= 3 * 255 * 2^18 + 255 * 2^18 + 2^25 + 2^15 = (1020 + 128) * 2^18 + 2^15 = 300 974 080 < 2^31:
// no sum leaves 32 bits.
//
// One launch per variant per batch.  The kernel streams 3 bytes in and 3 bytes out per pixel through rgb_tile.hpp's streaming tile (a
// workgroup owns 128 pixels x 8 rows; aligned dwords in, an LDS image per side that keeps the row's byte phase, aligned dwords out;
// nothing outside an image's pixels is read or written); what is here is one pixel's arithmetic.  A look-up table is copied into LDS
// once per workgroup.  The per-image constant K[c] mean + O[c] + 32768 is wave-uniform.  The launch needs nothing from the host but
// the slot shapes and the 15 coefficients, which travel as kernel arguments: no copy, no allocation, no atomics, bit-reproducible.
#include "rgb_tile.hpp"

namespace {

using namespace rgb_tile;

struct ColourCoef {
    int32_t m[9], k[3], o[3];
};

__global__ __launch_bounds__(THREADS) void colour_rgb_u8_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ sizes,
                                                                int maxH, int maxW, uint8_t* __restrict__ dst, int dstMaxH, int dstMaxW,
                                                                ColourCoef cf, const uint8_t* __restrict__ mean,
                                                                const uint8_t* __restrict__ lut, int tiles_x, int tiles_y) {
    __shared__ uint32_t tin[TILE_H * ROW_DW], tout[TILE_H * ROW_DW];
    __shared__ uint8_t lut_s[256];
    Tile t;
    if (!locate((int)blockIdx.x, src, sizes, maxH, maxW, dst, dstMaxH, dstMaxW, tiles_x, tiles_y, t)) return;
    if (lut) lut_s[threadIdx.x] = lut[threadIdx.x];               // 256 threads, 256 entries
    load_rows(t, tin);
    int base[3];                                                   // wave-uniform: K[c] mean + O[c] + the rounding half
#pragma unroll
    for (int c = 0; c < 3; ++c) base[c] = (mean ? cf.k[c] * (int)mean[t.img * 4 + c] : 0) + cf.o[c] + 32768;
    __syncthreads();
    for_each_pixel(t, tin, tout, [&](int, int, const uint8_t* p, uint8_t* o) {
        const int R = p[0], G = p[1], B = p[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int s = cf.m[c * 3] * R + cf.m[c * 3 + 1] * G + cf.m[c * 3 + 2] * B + base[c];
            const int v = min(max(s >> 16, 0), 255);
            o[c] = lut ? lut_s[v] : (uint8_t)v;
        }
    });
    __syncthreads();
    store_rows(t, tout);
}

}  // namespace

extern "C" int vip_colour_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH, int dstMaxW,
                                 const int32_t* coef_h, const uint8_t* mean_u8, const uint8_t* lut_d, int n, void* stream) {
    const char* what = "vip_colour_rgb_u8";
    Grid g;
    if (int st = check_slots(what, src_u8, sizes_hw, maxH, maxW, dst_u8, dstMaxH, dstMaxW, n, COUNT_BOTH, TILE_H, TILE_W * 3, &g)) return st;
    VIP_REQUIRE(coef_h, VIP_ERR_BAD_ARG, "%s: null pointer", what);
    ColourCoef cf;
    bool any_k = false;
    for (int c = 0; c < 15; ++c) {
        const long v = coef_h[c], lim = c < 12 ? (1L << 18) : (1L << 25);
        VIP_REQUIRE(v >= -lim && v <= lim, VIP_ERR_BAD_ARG, "%s: coefficient %d = %ld: |%s| is at most 2^%d", what, c, v,
                    c < 9 ? "M" : c < 12 ? "K" : "O", c < 12 ? 18 : 25);
        (c < 9 ? cf.m[c] : c < 12 ? cf.k[c - 9] : cf.o[c - 12]) = (int32_t)v;
        any_k |= c >= 9 && c < 12 && v != 0;
    }
    VIP_REQUIRE(mean_u8 || !any_k, VIP_ERR_BAD_ARG, "%s: a non-zero K needs mean_u8", what);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(mean_u8) & 3) == 0, VIP_ERR_ALIGNMENT, "%s: mean_u8 must be 4-byte aligned", what);
    hipLaunchKernelGGL(colour_rgb_u8_kernel, dim3((unsigned)g.total), dim3(THREADS), 0, (hipStream_t)stream, src_u8, sizes_hw, maxH, maxW,
                       dst_u8, dstMaxH, dstMaxW, cf, mean_u8, lut_d, g.tiles_x, g.tiles_y);
    return vip_launch_status(what);
}
