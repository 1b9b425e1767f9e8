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
// One launch per variant per batch.  The kernel streams 3 bytes in and 3 bytes out per pixel, so what matters is that both sides move
// whole dwords although a slot row starts at (i maxH + y) maxW 3 - aligned only by accident - and the two slots have different pitches.
// A workgroup (4 waves) owns 128 pixels x 8 rows.  (1) Every tile row is fetched as the ALIGNED dwords of the source that cover it,
// consecutive lanes on consecutive dwords, into an LDS image that keeps the row's phase (its first byte sits at byte `address & 3` of
// its LDS row); a dword that holds bytes of a neighbouring row or slot - the head and the tail of a row - is fetched byte by byte, so
// nothing outside the image's pixels is ever read.  (2) A lane takes one pixel: three byte reads at the source phase, the sums, three
// byte writes into a second LDS image at the DESTINATION row's phase; LDS does the re-alignment.  (3) That image leaves as the aligned
// dwords of the destination, head and tail again byte by byte, so nothing outside the image's pixels is written.  A look-up table is
// copied into LDS once per workgroup.  The per-image constant K[c] mean + O[c] + 32768 is wave-uniform.  The 1-D grid is (tiles of a
// slot) x n and a tile outside its image returns at once (as blur.hip and warp.hip), so the launch needs nothing from the host but the
// slot shapes and the 15 coefficients, which travel as kernel arguments: no copy, no allocation, no atomics, bit-reproducible.
#include "common.hpp"

namespace {

constexpr int TILE_W = 128, TILE_H = 8, WAVES = 4;
constexpr int ROW_DW = TILE_W * 3 / 4 + 1;                        // 96 dwords of interleaved RGB + one for the row's phase (0..3 bytes)

struct ColourCoef {
    int32_t m[9], k[3], o[3];
};

__global__ __launch_bounds__(WAVES * 64) void colour_rgb_u8_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ sizes,
                                                                   int maxH, int maxW, uint8_t* __restrict__ dst, int dstMaxH, int dstMaxW,
                                                                   ColourCoef cf, const uint8_t* __restrict__ mean,
                                                                   const uint8_t* __restrict__ lut, int tiles_x, int tiles_y) {
    __shared__ uint32_t tin[TILE_H * ROW_DW], tout[TILE_H * ROW_DW];
    __shared__ uint8_t lut_s[256];
    const int per_image = tiles_x * tiles_y;
    const int img = (int)blockIdx.x / per_image;
    const int t = (int)blockIdx.x - img * per_image;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int h = sizes[img * 2], w = sizes[img * 2 + 1];
    if (h < 1 || w < 1 || h > maxH || w > maxW || h > dstMaxH || w > dstMaxW) return;   // skipped image
    const int x0 = tx * TILE_W, y0 = ty * TILE_H;
    if (x0 >= w || y0 >= h) return;
    const int rows = min(TILE_H, h - y0), cols = min(TILE_W, w - x0);
    const int row_bytes = cols * 3;
    const uint8_t* stile = src + (((long)img * maxH + y0) * maxW + x0) * 3;
    uint8_t* dtile = dst + (((long)img * dstMaxH + y0) * dstMaxW + x0) * 3;
    const long spitch = (long)maxW * 3, dpitch = (long)dstMaxW * 3;
    uint8_t* tin_u8 = reinterpret_cast<uint8_t*>(tin);
    uint8_t* tout_u8 = reinterpret_cast<uint8_t*>(tout);

    if (lut) lut_s[threadIdx.x] = lut[threadIdx.x];               // 256 threads, 256 entries
    // ---- (1) the source rows as aligned dwords; the LDS row keeps the phase of its global row ----
    for (int k = threadIdx.x; k < rows * ROW_DW; k += WAVES * 64) {
        const int r = k / ROW_DW, j = k - r * ROW_DW;
        const uint8_t* row = stile + r * spitch;
        const int ph = (int)(reinterpret_cast<uintptr_t>(row) & 3);
        const int b = j * 4 - ph;                                  // the row byte at this dword's first byte
        if (b >= row_bytes) continue;
        if (b >= 0 && b + 4 <= row_bytes) {
            tin[k] = *reinterpret_cast<const uint32_t*>(row + b);
        } else {                                                   // the row's head or tail: only its own bytes
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (b + q >= 0 && b + q < row_bytes) tin_u8[k * 4 + q] = row[b + q];
        }
    }
    int base[3];                                                   // wave-uniform: K[c] mean + O[c] + the rounding half
#pragma unroll
    for (int c = 0; c < 3; ++c) base[c] = (mean ? cf.k[c] * (int)mean[img * 4 + c] : 0) + cf.o[c] + 32768;
    __syncthreads();
    // ---- (2) one pixel per lane: from the source phase to the destination phase ----
    const int px = threadIdx.x & (TILE_W - 1);
    if (px < cols) {
        for (int r = threadIdx.x / TILE_W; r < rows; r += WAVES * 64 / TILE_W) {
            const int sph = (int)(reinterpret_cast<uintptr_t>(stile + r * spitch) & 3);
            const int dph = (int)(reinterpret_cast<uintptr_t>(dtile + r * dpitch) & 3);
            const uint8_t* p = tin_u8 + r * (ROW_DW * 4) + sph + px * 3;
            uint8_t* o = tout_u8 + r * (ROW_DW * 4) + dph + px * 3;
            const int R = p[0], G = p[1], B = p[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int s = cf.m[c * 3] * R + cf.m[c * 3 + 1] * G + cf.m[c * 3 + 2] * B + base[c];
                const int v = min(max(s >> 16, 0), 255);
                o[c] = lut ? lut_s[v] : (uint8_t)v;
            }
        }
    }
    __syncthreads();
    // ---- (3) the destination rows as aligned dwords ----
    for (int k = threadIdx.x; k < rows * ROW_DW; k += WAVES * 64) {
        const int r = k / ROW_DW, j = k - r * ROW_DW;
        uint8_t* row = dtile + r * dpitch;
        const int ph = (int)(reinterpret_cast<uintptr_t>(row) & 3);
        const int b = j * 4 - ph;
        if (b >= row_bytes) continue;
        if (b >= 0 && b + 4 <= row_bytes) {
            *reinterpret_cast<uint32_t*>(row + b) = tout[k];
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (b + q >= 0 && b + q < row_bytes) row[b + q] = tout_u8[k * 4 + q];
        }
    }
}

}  // namespace

extern "C" int vip_colour_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH, int dstMaxW,
                                 const int32_t* coef_h, const uint8_t* mean_u8, const uint8_t* lut_d, int n, void* stream) {
    const char* what = "vip_colour_rgb_u8";
    VIP_REQUIRE(src_u8 && sizes_hw && dst_u8 && coef_h, VIP_ERR_BAD_ARG, "%s: null pointer", what);
    VIP_REQUIRE(n > 0 && maxH > 0 && maxW > 0 && dstMaxH > 0 && dstMaxW > 0, VIP_ERR_BAD_ARG, "%s: bad size", what);
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src_u8), s1 = s0 + (size_t)n * maxH * maxW * 3;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst_u8), d1 = d0 + (size_t)n * dstMaxH * dstMaxW * 3;
    VIP_REQUIRE(s1 <= d0 || d1 <= s0, VIP_ERR_BAD_ARG, "%s: source and destination overlap (the kernel cannot run in place)", what);
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
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(sizes_hw) & 3) == 0, VIP_ERR_ALIGNMENT, "%s: sizes must be 4-byte aligned", what);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(mean_u8) & 3) == 0, VIP_ERR_ALIGNMENT, "%s: mean_u8 must be 4-byte aligned", what);
    // an image that is written fits both slots
    const int tiles_x = ((maxW < dstMaxW ? maxW : dstMaxW) + TILE_W - 1) / TILE_W, tiles_y = ((maxH < dstMaxH ? maxH : dstMaxH) + TILE_H - 1) / TILE_H;
    const long total = (long)tiles_x * tiles_y * n;
    VIP_REQUIRE(total <= 0x7FFFFFFFL, VIP_ERR_UNSUPPORTED, "%s: %ld tiles exceed one launch's grid", what, total);
    hipLaunchKernelGGL(colour_rgb_u8_kernel, dim3((unsigned)total), dim3(WAVES * 64), 0, (hipStream_t)stream, src_u8, sizes_hw, maxH, maxW,
                       dst_u8, dstMaxH, dstMaxW, cf, mean_u8, lut_d, tiles_x, tiles_y);
    return vip_launch_status(what);
}
