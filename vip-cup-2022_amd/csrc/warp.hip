// Inverse affine warp of decoded u8 RGB pixels with bilinear taps, all in integers: the one kernel under the geometric stress
// perturbations (pipeline.flip, pipeline.crop, pipeline.rotate, --stress-flip / -crop / -rotate), the inference-time form of
// dataset/augment.py's RandomFlip (:115-120) and ShiftScaleShearRotate (:68-107, tfa.image.rotate / transform).  Each image of a
// mixed-size batch has its own transform and its own output size.
//
// Arithmetic (part of the interface; include/vipcup_hip.h).  Output pixel (x, y) of image i, transform (A, B, TX, C, D, TY) as int64
// - A..D the Q24 coefficients of the inverse map, TX, TY its Q25 offsets, pixel-edge coordinates - with u = 2 x + 1, v = 2 y + 1:
//   SX = A u + B v + TX - 2^24,  SY = C u + D v + TY - 2^24        the source sample-centre coordinate in Q25, int64 throughout
//   ix = SX >> 25 (arithmetic),  wx = (SX >> 15) & 1023             and the same for y
//   top = p[iy][ix] (1024 - wx) + p[iy][ix + 1] wx,  bot likewise on row iy + 1
//   out = (top (1024 - wy) + bot wy + 2^19) >> 20                   <= 255 * 2^20 + 2^19: unsigned 32 bits
// A tap outside the source is 0 (fill 0, black: tfa's `constant`) or the mirrored sample (fill 1: reflect without repeating the edge
// sample - rgb_tile.hpp's `mirror`, as in blur.hip; every tap of a 1-pixel axis is index 0).  With A = D = +-2^24, B = C = 0 and
// whole-pixel offsets both weights are 0 and the warp is an exact copy: flips and crops.
//
// One launch per batch.  The kernel is a gather bound by memory, so a workgroup (4 waves) owns a compact 2-D output tile, 64 pixels x
// 16 rows: under a rotation its source footprint is a tilted rectangle of about the same area, which the CU's L1 holds, and the 64
// lanes of a wave walk one output row, i.e. one straight line through the source.  A lane computes the coordinates of a pixel once,
// gathers its 4 x 3 tap bytes (the interior case without any index arithmetic beyond the two row pointers) and puts the three result
// bytes into an LDS image of the tile; after one barrier the tile's rows (192 bytes each) leave as whole dwords, consecutive lanes on
// consecutive addresses, where the row's end and the destination's alignment allow.  The 1-D grid is (tiles of the destination slot)
// x n and a tile outside its image returns at once (as blur.hip), so the launch needs nothing from the host but the slot shapes.
// No allocation, no atomics: bit-reproducible.
#include "rgb_tile.hpp"

namespace {

constexpr int TILE_W = 64, TILE_H = 16, WAVES = 4;
constexpr int ROW_DW = TILE_W * 3 / 4;                            // 48 dwords of interleaved RGB per tile row

using rgb_tile::mirror;                                           // reflect without repeating the edge sample, here of a 64-bit index

// the two taps i, i + 1 of an axis of n samples: indices that are safe to read, and whether each counts (black fill: outside = 0)
__device__ __forceinline__ void taps_of(long i, int n, int fill, int& i0, int& i1, bool& ok0, bool& ok1) {
    if (i >= 0 && i + 1 < n) {                                    // interior: the common case
        i0 = (int)i;
        i1 = i0 + 1;
        ok0 = ok1 = true;
    } else if (fill == VIP_WARP_FILL_MIRROR) {
        i0 = mirror(i, n);
        i1 = mirror(i + 1, n);
        ok0 = ok1 = true;
    } else {
        ok0 = i >= 0 && i < n;
        ok1 = i + 1 >= 0 && i + 1 < n;
        i0 = ok0 ? (int)i : 0;
        i1 = ok1 ? (int)(i + 1) : 0;
    }
}

__global__ __launch_bounds__(WAVES * 64) void warp_affine_rgb_u8_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ sizes,
                                                                        int maxH, int maxW, uint8_t* __restrict__ dst,
                                                                        const int32_t* __restrict__ dst_sizes, int dstMaxH, int dstMaxW,
                                                                        const int64_t* __restrict__ xform, int fill, int tiles_x, int tiles_y) {
    __shared__ uint32_t tile[TILE_H * ROW_DW];
    const int per_image = tiles_x * tiles_y;
    const int img = (int)blockIdx.x / per_image;
    const int t = (int)blockIdx.x - img * per_image;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int sh = sizes[img * 2], sw = sizes[img * 2 + 1];
    const int oh = dst_sizes[img * 2], ow = dst_sizes[img * 2 + 1];
    if (sh < 1 || sw < 1 || sh > maxH || sw > maxW || oh < 1 || ow < 1 || oh > dstMaxH || ow > dstMaxW) return;   // skipped image
    const int x0 = tx * TILE_W, y0 = ty * TILE_H;
    if (x0 >= ow || y0 >= oh) return;
    const int rows = min(TILE_H, oh - y0);
    const uint8_t* simg = src + (long)img * maxH * maxW * 3;
    uint8_t* dimg = dst + (long)img * dstMaxH * dstMaxW * 3;
    const long A = xform[img * 6], B = xform[img * 6 + 1], TX = xform[img * 6 + 2];
    const long C = xform[img * 6 + 3], D = xform[img * 6 + 4], TY = xform[img * 6 + 5];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t* tile_u8 = reinterpret_cast<uint8_t*>(tile);

    const int x = x0 + lane;
    const long u = 2L * x + 1;
    for (int r = wave; r < rows; r += WAVES) {                     // one wave per output row: a straight line through the source
        if (x >= ow) break;
        const long v = 2L * (y0 + r) + 1;
        const long SX = A * u + B * v + TX - (1L << 24), SY = C * u + D * v + TY - (1L << 24);
        const uint32_t wx = (uint32_t)(SX >> 15) & 1023u, wy = (uint32_t)(SY >> 15) & 1023u;
        int ix0, ix1, iy0, iy1;
        bool okx0, okx1, oky0, oky1;
        taps_of(SX >> 25, sw, fill, ix0, ix1, okx0, okx1);
        taps_of(SY >> 25, sh, fill, iy0, iy1, oky0, oky1);
        const uint8_t* r0 = simg + (long)iy0 * maxW * 3;
        const uint8_t* r1 = simg + (long)iy1 * maxW * 3;
        const uint32_t m00 = (oky0 && okx0) ? 1u : 0u, m01 = (oky0 && okx1) ? 1u : 0u;
        const uint32_t m10 = (oky1 && okx0) ? 1u : 0u, m11 = (oky1 && okx1) ? 1u : 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t top = m00 * r0[ix0 * 3 + c] * (1024u - wx) + m01 * r0[ix1 * 3 + c] * wx;
            const uint32_t bot = m10 * r1[ix0 * 3 + c] * (1024u - wx) + m11 * r1[ix1 * 3 + c] * wx;
            tile_u8[r * (ROW_DW * 4) + lane * 3 + c] = (uint8_t)((top * (1024u - wy) + bot * wy + (1u << 19)) >> 20);
        }
    }
    __syncthreads();
    // ---- the tile's rows as dwords: 48 per row, whole where the row's end and the destination's alignment allow ----
    const int row_bytes = min(TILE_W, ow - x0) * 3;
    for (int k = threadIdx.x; k < rows * ROW_DW; k += WAVES * 64) {
        const int r = k / ROW_DW, b = (k - r * ROW_DW) * 4;
        if (b >= row_bytes) continue;
        rgb_tile::store_pack(dimg + ((long)(y0 + r) * dstMaxW + x0) * 3 + b, b, row_bytes, tile[k]);
    }
}

}  // namespace

extern "C" int vip_warp_affine_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8,
                                      const int32_t* dst_sizes_hw, int dstMaxH, int dstMaxW, const int64_t* xform_d, int fill, int n,
                                      void* stream) {
    const char* what = "vip_warp_affine_rgb_u8";
    rgb_tile::Grid g;                                               // the grid is (tiles of the destination slot) x n
    if (int st = rgb_tile::check_slots(what, src_u8, sizes_hw, maxH, maxW, dst_u8, dstMaxH, dstMaxW, n, rgb_tile::COUNT_DESTINATION, TILE_H,
                                       TILE_W * 3, &g))
        return st;
    VIP_REQUIRE(dst_sizes_hw && xform_d, VIP_ERR_BAD_ARG, "%s: null pointer", what);
    VIP_REQUIRE(fill == VIP_WARP_FILL_BLACK || fill == VIP_WARP_FILL_MIRROR, VIP_ERR_BAD_ARG, "%s: fill %d: expected 0 (black) or 1 (mirror)",
                what, fill);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(dst_sizes_hw) & 3) == 0, VIP_ERR_ALIGNMENT, "%s: sizes must be 4-byte aligned", what);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(xform_d) & 7) == 0, VIP_ERR_ALIGNMENT, "%s: transforms must be 8-byte aligned", what);
    hipLaunchKernelGGL(warp_affine_rgb_u8_kernel, dim3((unsigned)g.total), dim3(WAVES * 64), 0, (hipStream_t)stream, src_u8, sizes_hw, maxH,
                       maxW, dst_u8, dst_sizes_hw, dstMaxH, dstMaxW, xform_d, fill, g.tiles_x, g.tiles_y);
    return vip_launch_status(what);
}
