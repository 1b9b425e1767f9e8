// What the kernels on the decoded u8 RGB batch share (resample, blur, warp, colour, noise, tone): the host's checks of a source slot /
// destination slot pair, the mirrored index, a lane's dword-or-tail store, and the streaming tile of colour.hip, noise.hip and
// tone.hip's apply kernel.  This is the code that keeps every read and write inside an image's own pixels.
//
// The batch is [n, maxH, maxW, 3] u8, image i at the top left of slot i with its (height, width) in sizes[i]; source and destination
// slots may differ in shape.  An image whose size entry is unusable - below 1, or larger than either slot - is SKIPPED: nothing of
// its slot is read or written.
//
// The streaming tile.  These kernels move 3 bytes in and 3 bytes out per pixel, so what matters is that both sides move whole dwords
// although a slot row starts at (i maxH + y) maxW 3 - aligned only by accident - and the two slots have different pitches.  A
// workgroup (4 waves) owns 128 pixels x 8 rows.  (1) load_rows: every tile row is fetched as the ALIGNED dwords of the source that
// cover it, consecutive lanes on consecutive dwords, into an LDS image that keeps the row's phase (its first byte sits at byte
// `address & 3` of its LDS row); a dword that holds bytes of a neighbouring row or slot - the head and the tail of a row - is fetched
// byte by byte, so nothing outside the image's pixels is ever read.  (2) for_each_pixel: a lane takes one pixel: three byte reads at
// the source phase, the kernel's own arithmetic, three byte writes into a second LDS image at the DESTINATION row's phase; LDS does
// the re-alignment.  (3) store_rows: that image leaves as the aligned dwords of the destination, head and tail again byte by byte, so
// nothing outside the image's pixels is written.  The caller puts a barrier between the stages.  The 1-D grid is (tiles of a slot) x n
// and `locate` tells a tile outside its image to leave at once, so a launch needs nothing from the host but the slot shapes: no
// copy, no allocation, no atomics, bit-reproducible.
#pragma once
#include "common.hpp"

namespace rgb_tile {

// ---- host: a source slot / destination slot pair ------------------------------------------------------------------------------
struct Grid {
    int tiles_x, tiles_y;
    long total;                                                   // tiles_x * tiles_y * n, at most 2^31 - 1: one launch's 1-D grid
};

enum Count { COUNT_SOURCE, COUNT_DESTINATION, COUNT_BOTH };       // the slot whose tiles make the grid; BOTH: min(source, destination)

// The checks every entry point with such a pair makes - pointers, sizes, the alignment of `sizes`, no overlap (no kernel runs in
// place) - and the grid of tile_rows x tile_bytes tiles (bytes of the interleaved row) over the counted slot.
inline int check_slots(const char* what, const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, const uint8_t* dst_u8,
                       int dstMaxH, int dstMaxW, int n, Count count, int tile_rows, int tile_bytes, Grid* g) {
    VIP_REQUIRE(src_u8 && sizes_hw && dst_u8, VIP_ERR_BAD_ARG, "%s: null pointer", what);
    VIP_REQUIRE(n > 0 && maxH > 0 && maxW > 0 && dstMaxH > 0 && dstMaxW > 0, VIP_ERR_BAD_ARG, "%s: bad size", what);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(sizes_hw) & 3) == 0, VIP_ERR_ALIGNMENT, "%s: sizes must be 4-byte aligned", what);
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src_u8), s1 = s0 + (size_t)n * maxH * maxW * 3;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst_u8), d1 = d0 + (size_t)n * dstMaxH * dstMaxW * 3;
    VIP_REQUIRE(s1 <= d0 || d1 <= s0, VIP_ERR_BAD_ARG, "%s: source and destination overlap (the kernel cannot run in place)", what);
    // COUNT_BOTH: an image that is written fits both slots
    const int H = count == COUNT_SOURCE ? maxH : count == COUNT_DESTINATION ? dstMaxH : maxH < dstMaxH ? maxH : dstMaxH;
    const int W = count == COUNT_SOURCE ? maxW : count == COUNT_DESTINATION ? dstMaxW : maxW < dstMaxW ? maxW : dstMaxW;
    g->tiles_x = (int)(((long)W * 3 + tile_bytes - 1) / tile_bytes);
    g->tiles_y = (H + tile_rows - 1) / tile_rows;
    g->total = (long)g->tiles_x * g->tiles_y * n;
    VIP_REQUIRE(g->total <= 0x7FFFFFFFL, VIP_ERR_UNSUPPORTED, "%s: %ld tiles exceed one launch's grid", what, g->total);
    return VIP_OK;
}

// ---- device: what any of these kernels may use ---------------------------------------------------------------------------------
// Reflect without repeating the edge sample (tfa's REFLECT, scipy's mode='mirror'): sample i, any int or long, of an axis of n
//   n == 1: 0;   otherwise p = 2 (n - 1), i = i mod p (non-negative), i = p - i if i >= n
// which reflects repeatedly, so a side shorter than the reach is handled by the same formula.
template <typename Index>
__device__ __forceinline__ int mirror(Index i, int n) {
    if (n == 1) return 0;
    const Index p = 2 * (Index)(n - 1);
    i %= p;
    if (i < 0) i += p;
    return (int)(i >= n ? p - i : i);
}

// A lane's four bytes `pack` of a row of row_bytes bytes, from byte b on, to `out` (the address of byte b): one dword where the row's
// end and the destination's alignment allow, otherwise - the row's tail, or a slot row at an odd pitch - byte by byte
__device__ __forceinline__ void store_pack(uint8_t* out, int b, int row_bytes, uint32_t pack) {
    if (b + 4 <= row_bytes && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(out) = pack;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (b + q < row_bytes) out[q] = (uint8_t)(pack >> (8 * q));
    }
}

// ---- device: the streaming tile --------------------------------------------------------------------------------------------------
constexpr int TILE_W = 128, TILE_H = 8, WAVES = 4, THREADS = WAVES * 64;
constexpr int ROW_DW = TILE_W * 3 / 4 + 1;                        // 96 dwords of interleaved RGB + one for the row's phase (0..3 bytes)

struct Tile {
    int img, h, w;                                                // the image and its size
    int x0, y0, rows, cols, row_bytes;                            // the tile's first pixel and its part inside the image
    const uint8_t* stile;                                         // the tile's first byte in the source and in the destination
    uint8_t* dtile;
    long spitch, dpitch;                                          // bytes from a row to the next
};

// tile `tile` of a grid of tiles_x x tiles_y tiles per image; false for a skipped image and for a tile outside its image.  Index: the
// type the caller's tile index has - a 64-bit index makes the division below a 64-bit one, which a 32-bit grid need not pay for.
template <typename Index>
__device__ __forceinline__ bool locate(Index tile, const uint8_t* src, const int32_t* sizes, int maxH, int maxW, uint8_t* dst, int dstMaxH,
                                       int dstMaxW, int tiles_x, int tiles_y, Tile& t) {
    const int per_image = tiles_x * tiles_y;
    t.img = (int)(tile / per_image);
    const int k = (int)(tile - (Index)t.img * per_image);
    const int ty = k / tiles_x, tx = k - ty * tiles_x;
    t.h = sizes[t.img * 2], t.w = sizes[t.img * 2 + 1];
    if (t.h < 1 || t.w < 1 || t.h > maxH || t.w > maxW || t.h > dstMaxH || t.w > dstMaxW) return false;   // skipped image
    t.x0 = tx * TILE_W, t.y0 = ty * TILE_H;
    if (t.x0 >= t.w || t.y0 >= t.h) return false;
    t.rows = min(TILE_H, t.h - t.y0), t.cols = min(TILE_W, t.w - t.x0);
    t.row_bytes = t.cols * 3;
    t.stile = src + (((long)t.img * maxH + t.y0) * maxW + t.x0) * 3;
    t.dtile = dst + (((long)t.img * dstMaxH + t.y0) * dstMaxW + t.x0) * 3;
    t.spitch = (long)maxW * 3, t.dpitch = (long)dstMaxW * 3;
    return true;
}

// (1) the source rows as aligned dwords; the LDS row keeps the phase of its global row
__device__ __forceinline__ void load_rows(const Tile& t, uint32_t* tin) {
    uint8_t* tin_u8 = reinterpret_cast<uint8_t*>(tin);
    for (int k = threadIdx.x; k < t.rows * ROW_DW; k += THREADS) {
        const int r = k / ROW_DW, j = k - r * ROW_DW;
        const uint8_t* row = t.stile + r * t.spitch;
        const int ph = (int)(reinterpret_cast<uintptr_t>(row) & 3);
        const int b = j * 4 - ph;                                  // the row byte at this dword's first byte
        if (b >= t.row_bytes) continue;
        if (b >= 0 && b + 4 <= t.row_bytes) {
            tin[k] = *reinterpret_cast<const uint32_t*>(row + b);
        } else {                                                   // the row's head or tail: only its own bytes
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (b + q >= 0 && b + q < t.row_bytes) tin_u8[k * 4 + q] = row[b + q];
        }
    }
}

// (2) one pixel per lane, from the source phase to the destination phase: f(r, px, p, o) gets row r and pixel px of the tile, its three
// source bytes at p (in tin) and the place of its three destination bytes o (in tout)
template <typename F>
__device__ __forceinline__ void for_each_pixel(const Tile& t, const uint32_t* tin, uint32_t* tout, F&& f) {
    const uint8_t* tin_u8 = reinterpret_cast<const uint8_t*>(tin);
    uint8_t* tout_u8 = reinterpret_cast<uint8_t*>(tout);
    const int px = threadIdx.x & (TILE_W - 1);
    if (px < t.cols) {
        for (int r = threadIdx.x / TILE_W; r < t.rows; r += THREADS / TILE_W) {
            const int sph = (int)(reinterpret_cast<uintptr_t>(t.stile + r * t.spitch) & 3);
            const int dph = (int)(reinterpret_cast<uintptr_t>(t.dtile + r * t.dpitch) & 3);
            f(r, px, tin_u8 + r * (ROW_DW * 4) + sph + px * 3, tout_u8 + r * (ROW_DW * 4) + dph + px * 3);
        }
    }
}

// (3) the destination rows as aligned dwords
__device__ __forceinline__ void store_rows(const Tile& t, const uint32_t* tout) {
    const uint8_t* tout_u8 = reinterpret_cast<const uint8_t*>(tout);
    for (int k = threadIdx.x; k < t.rows * ROW_DW; k += THREADS) {
        const int r = k / ROW_DW, j = k - r * ROW_DW;
        uint8_t* row = t.dtile + r * t.dpitch;
        const int ph = (int)(reinterpret_cast<uintptr_t>(row) & 3);
        const int b = j * 4 - ph;
        if (b >= t.row_bytes) continue;
        if (b >= 0 && b + 4 <= t.row_bytes) {
            *reinterpret_cast<uint32_t*>(row + b) = tout[k];
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (b + q >= 0 && b + q < t.row_bytes) row[b + q] = tout_u8[k * 4 + q];
        }
    }
}

}  // namespace rgb_tile
