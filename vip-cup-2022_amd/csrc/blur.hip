// Smoothing of decoded u8 RGB pixels at their own size: a separable Gaussian blur and a K x K median (K = 3, 5), the two filters of
// dataset/augment.py:131-140 (`Blur`: tfa.image.gaussian_filter2d / median_filter2d) as stress perturbations (pipeline.blur,
// pipeline.median, --stress-blur, --stress-median).  Each image of a mixed-size batch is filtered on its own, each channel separately.
//
// Edges: REFLECT without repeating the edge sample (tfa's default, scipy's mode='mirror'): rgb_tile.hpp's `mirror`, which reflects
// repeatedly, so a side shorter than the radius is handled by the same formula.
//
// Gaussian, all in unsigned 32-bit integers with the 2R + 1 weights of vip_blur_weights_h (non-negative, sum 2^16):
//   horizontal pass   t   = (sum_j w[j] * px[mirror(x + j)] + 128) >> 8           8.8 fixed point, <= 65280: held as u16
//   vertical pass     out = min((sum_j w[j] * t[mirror(y + j)] + 2^23) >> 24, 255)  the sum is <= 65536 * 65280 + 2^23 < 2^32
// Median: the element of rank K * K / 2 of the mirrored K x K window - exact.
//
// One launch per batch.  A workgroup (4 waves) owns an output tile of one image, 16 rows x 256 BYTES of the interleaved RGB row, as the
// resampler does (resample.hip); the 1-D grid is (tiles of the largest image) x n and a tile outside its image returns at once, so the
// launch needs nothing from the host but the slot shape.  The tile plus its halo - R rows above and below, 3 R bytes (rounded up to a
// dword, so that interior dwords stay aligned) left and right - is staged once into LDS as u8, with the mirroring resolved while staging
// on the PIXEL index (a byte keeps its channel).  A tap j of output byte k is then staged byte k + 3 j: a lane's four bytes of a tap are
// an unaligned dword whose byte shift is wave-uniform, two consecutive-address LDS reads and one funnel shift.
//   Gaussian: horizontal pass LDS u8 -> LDS u16 plane (one wave per staged row), vertical pass from there (one wave per output row, the
//             weights wave-uniform through the scalar path), whole dwords stored where the row allows.  16 KiB + 23 KiB of LDS at any
//             radius up to 15; no intermediate in global memory.
//   Median:   the window's K * K dwords are split into even and odd bytes (two u16 lanes per register) and run through a fixed
//             min / max network on packed 16-bit operations: 3 x 3 by sorted columns (max of minima, median of medians, min of maxima),
//             5 x 5 by a 99-exchange selection network.  No data-dependent control flow.
// No allocation, no atomics: bit-reproducible.
//
// Unsharp mask (pipeline.sharpen, --stress-sharpen, the `shp` step of --stress-chain): the sharpening a platform adds after a downscale.
// Integers only, per byte of the interleaved RGB image, each image of a mixed-size batch on its own:
//   B   = the Gaussian above at (sigma, radius): its u8 result, bit for bit (mirrored edges, 8.8 horizontal pass, 2^24 vertical pass)
//   d   = X - B                                            (-255..255)
//   out = X                                                if |d| <= T
//   out = clamp(X + ((a * d + 128) >> 8), 0, 255)          otherwise; >> is an arithmetic shift (floor)
//   a   = round(256 * P / 100)                             P an integer percent in 1..500 (a in 3..1280), T a threshold in 0..255
// Because |a / 256 - P / 100| <= 1 / 512 and |d| <= 255, the result is at most one level from round(X + P / 100 * (X - B)) clamped.
// It is the Gaussian kernel with one more epilogue: the vertical pass's wave takes its lane's four centre bytes from the staged u8 tile
// (row yy + R, byte offset A: already in LDS), forms d, applies the threshold and the gain and stores through store_row.  a and T travel
// as kernel arguments.  One launch, no extra LDS, no intermediate in global memory, bit-reproducible.
#include "rgb_tile.hpp"

namespace {

constexpr int TILE_ROWS = 16, TILE_BYTES = 256, WAVES = 4, MAX_RADIUS = 15;
constexpr int STAGE_DW = 88;                                    // a staged row: 352 bytes >= 256 + 48 + 45, in dwords
constexpr int STAGE_ROWS = TILE_ROWS + 2 * MAX_RADIUS;

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

using rgb_tile::mirror;
using rgb_tile::Grid, rgb_tile::check_slots, rgb_tile::COUNT_SOURCE;

// halo in bytes to the left of the tile: 3 R rounded up to a dword
__device__ __host__ constexpr int halo_bytes(int R) { return (3 * R + 3) & ~3; }

struct TileAt {
    const uint8_t* simg;
    uint8_t* dimg;
    int h, w, b0, y0, y_end;
};

// the image and tile of this workgroup; false when the tile lies outside its image (or the sizes do not fit the slots)
__device__ __forceinline__ bool tile_of_block(const uint8_t* src, const int32_t* sizes, int maxH, int maxW, uint8_t* dst, int dstMaxH,
                                              int dstMaxW, int tiles_x, int tiles_y, TileAt& t) {
    const int per_image = tiles_x * tiles_y;
    const int img = (int)blockIdx.x / per_image;
    const int tile = (int)blockIdx.x - img * per_image;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    t.h = sizes[img * 2];
    t.w = sizes[img * 2 + 1];
    if (t.h < 1 || t.w < 1 || t.h > maxH || t.w > maxW || t.h > dstMaxH || t.w > dstMaxW) return false;
    t.b0 = tx * TILE_BYTES;
    t.y0 = ty * TILE_ROWS;
    if (t.b0 >= t.w * 3 || t.y0 >= t.h) return false;
    t.y_end = min(t.y0 + TILE_ROWS, t.h);
    t.simg = src + (long)img * maxH * maxW * 3;
    t.dimg = dst + (long)img * dstMaxH * dstMaxW * 3;
    return true;
}

// rows y0 - R .. y0 - R + rows - 1 of the image, bytes b0 - A .. b0 - A + 4 STAGE_DW - 1 of each, mirrored, into `stage` (one wave per
// row; a lane's dwords - lane and lane + 64 - and their source offsets are fixed across rows)
__device__ __forceinline__ void stage_tile(uint32_t* stage, const TileAt& t, int maxW, int R, int A, int rows, int lane, int wave) {
    int off[2][4];
    bool straight[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int bb0 = t.b0 - A + (lane + 64 * d) * 4;
        straight[d] = bb0 >= 0 && bb0 + 4 <= t.w * 3;                 // no mirroring: one dword of the row
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int bb = bb0 + q;
            const int px = (bb + 3 * 64) / 3 - 64;                    // floor: bb >= -48
            off[d][q] = mirror(px, t.w) * 3 + (bb - px * 3);
        }
    }
    for (int r = wave; r < rows; r += WAVES) {
        const uint8_t* srow = t.simg + (long)mirror(t.y0 - R + r, t.h) * maxW * 3;
        const bool aligned = (reinterpret_cast<uintptr_t>(srow) & 3) == 0;      // wave-uniform; b0 and A are multiples of 4
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            if (d == 1 && lane + 64 >= STAGE_DW) break;
            uint32_t v;
            if (straight[d] && aligned)
                v = *reinterpret_cast<const uint32_t*>(srow + off[d][0]);
            else
                v = (uint32_t)srow[off[d][0]] | ((uint32_t)srow[off[d][1]] << 8) | ((uint32_t)srow[off[d][2]] << 16) |
                    ((uint32_t)srow[off[d][3]] << 24);
            stage[r * STAGE_DW + lane + 64 * d] = v;
        }
    }
}

// the lane's four bytes at byte offset `o` (wave-uniform) past its own dword of a staged row
__device__ __forceinline__ uint32_t bytes_at(const uint32_t* row_lane, int o) {
    const uint32_t d0 = row_lane[o >> 2], d1 = row_lane[(o >> 2) + 1];
    return (uint32_t)(((static_cast<uint64_t>(d1) << 32) | d0) >> (8 * (o & 3)));
}

// 256 contiguous bytes per wave: whole dwords where the row and the destination's alignment allow
__device__ __forceinline__ void store_row(const TileAt& t, int y, int dstMaxW, int lane, uint32_t pack) {
    const int b = t.b0 + lane * 4;
    rgb_tile::store_pack(t.dimg + (long)y * dstMaxW * 3 + b, b, t.w * 3, pack);
}

// one byte of the unsharp mask: X the source sample, B its blurred value
__device__ __forceinline__ uint32_t sharpen_byte(int X, int B, int amount, int threshold) {
    const int d = X - B;
    return (uint32_t)(abs(d) <= threshold ? X : min(max(X + ((amount * d + 128) >> 8), 0), 255));
}

// SHARPEN: the unsharp mask's epilogue on the blurred value (amount = a, threshold = T); false: the plain Gaussian, which ignores both
template <bool SHARPEN>
__global__ __launch_bounds__(WAVES * 64) void blur_gauss_rgb_u8_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ sizes,
                                                                       int maxH, int maxW, uint8_t* __restrict__ dst, int dstMaxH,
                                                                       int dstMaxW, const int32_t* __restrict__ weights, int R,
                                                                       int tiles_x, int tiles_y, int amount, int threshold) {
    __shared__ uint32_t stage[STAGE_ROWS * STAGE_DW];                 // u8 tile + halo
    __shared__ uint2 mid[STAGE_ROWS * (TILE_BYTES / 4)];              // u16 plane of the horizontal pass: 4 values per lane
    TileAt t;
    if (!tile_of_block(src, sizes, maxH, maxW, dst, dstMaxH, dstMaxW, tiles_x, tiles_y, t)) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int A = halo_bytes(R), taps = 2 * R + 1;
    const int out_rows = t.y_end - t.y0, rows = out_rows + 2 * R;
    stage_tile(stage, t, maxW, R, A, rows, lane, wave);
    __syncthreads();
    // ---- horizontal pass: staged u8 rows -> u16 plane, one wave per row ----
    for (int r = wave; r < rows; r += WAVES) {
        const uint32_t* row = stage + r * STAGE_DW + lane;
        uint32_t a0 = 128, a1 = 128, a2 = 128, a3 = 128;
        for (int j = 0; j < taps; ++j) {
            const uint32_t v = bytes_at(row, A - 3 * R + 3 * j);
            const uint32_t wj = (uint32_t)weights[j];
            a0 += __umul24(v & 255, wj);                                // both factors < 2^24: the full-rate 24-bit multiply-add
            a1 += __umul24((v >> 8) & 255, wj);
            a2 += __umul24((v >> 16) & 255, wj);
            a3 += __umul24(v >> 24, wj);
        }
        mid[r * (TILE_BYTES / 4) + lane] = make_uint2((a0 >> 8) | ((a1 >> 8) << 16), (a2 >> 8) | ((a3 >> 8) << 16));
    }
    __syncthreads();
    // ---- vertical pass from the u16 plane: one wave per output row ----
    for (int yy = wave; yy < out_rows; yy += WAVES) {
        const uint2* col = mid + yy * (TILE_BYTES / 4) + lane;
        uint32_t a0, a1, a2, a3;
        a0 = a1 = a2 = a3 = 1u << 23;
        for (int j = 0; j < taps; ++j) {
            const uint2 v = col[j * (TILE_BYTES / 4)];
            const uint32_t wj = (uint32_t)weights[j];
            a0 += __umul24(v.x & 0xFFFFu, wj);
            a1 += __umul24(v.x >> 16, wj);
            a2 += __umul24(v.y & 0xFFFFu, wj);
            a3 += __umul24(v.y >> 16, wj);
        }
        uint32_t pack = min(a0 >> 24, 255u) | (min(a1 >> 24, 255u) << 8) | (min(a2 >> 24, 255u) << 16) | (min(a3 >> 24, 255u) << 24);
        if constexpr (SHARPEN) {
            const uint32_t x = stage[(yy + R) * STAGE_DW + (A >> 2) + lane];    // the lane's own four source bytes: A is a multiple of 4
            uint32_t sharp = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                sharp |= sharpen_byte((int)((x >> (8 * q)) & 255), (int)((pack >> (8 * q)) & 255), amount, threshold) << (8 * q);
            pack = sharp;
        }
        store_row(t, t.y0 + yy, dstMaxW, lane, pack);
    }
}

// ---- median: min / max networks on two u16 lanes per register ----
__device__ __forceinline__ void cswap(u16x2& a, u16x2& b) {
    const u16x2 lo = __builtin_elementwise_min(a, b), hi = __builtin_elementwise_max(a, b);
    a = lo;
    b = hi;
}
__device__ __forceinline__ u16x2 med3(u16x2 a, u16x2 b, u16x2 c) {
    return __builtin_elementwise_max(__builtin_elementwise_min(a, b), __builtin_elementwise_min(__builtin_elementwise_max(a, b), c));
}

// 3 x 3, p[row * 3 + column]: sort the columns, then the median is med3(largest minimum, median of the medians, smallest maximum)
__device__ __forceinline__ u16x2 median9(u16x2 (&p)[9]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        cswap(p[c], p[3 + c]);
        cswap(p[3 + c], p[6 + c]);
        cswap(p[c], p[3 + c]);
    }
    const u16x2 lo = __builtin_elementwise_max(__builtin_elementwise_max(p[0], p[1]), p[2]);
    const u16x2 hi = __builtin_elementwise_min(__builtin_elementwise_min(p[6], p[7]), p[8]);
    return med3(lo, med3(p[3], p[4], p[5]), hi);
}

// 5 x 5: a selection network of 99 exchanges that leaves the median in p[12] (the published minimal-exchange median-of-25 network;
// tests/test_blur_cpu.py checks this list on every 0 / 1 input, which proves it for all inputs)
__device__ __forceinline__ u16x2 median25(u16x2 (&p)[25]) {
    constexpr unsigned char NET[99][2] = {
        {0, 1},   {3, 4},   {2, 4},   {2, 3},   {6, 7},   {5, 7},   {5, 6},   {9, 10},  {8, 10},  {8, 9},   {12, 13}, {11, 13}, {11, 12},
        {15, 16}, {14, 16}, {14, 15}, {18, 19}, {17, 19}, {17, 18}, {21, 22}, {20, 22}, {20, 21}, {23, 24}, {2, 5},   {3, 6},   {0, 6},
        {0, 3},   {4, 7},   {1, 7},   {1, 4},   {11, 14}, {8, 14},  {8, 11},  {12, 15}, {9, 15},  {9, 12},  {13, 16}, {10, 16}, {10, 13},
        {20, 23}, {17, 23}, {17, 20}, {21, 24}, {18, 24}, {18, 21}, {19, 22}, {8, 17},  {9, 18},  {0, 18},  {0, 9},   {10, 19}, {1, 19},
        {1, 10},  {11, 20}, {2, 20},  {2, 11},  {12, 21}, {3, 21},  {3, 12},  {13, 22}, {4, 22},  {4, 13},  {14, 23}, {5, 23},  {5, 14},
        {15, 24}, {6, 24},  {6, 15},  {7, 16},  {7, 19},  {13, 21}, {15, 23}, {7, 13},  {7, 15},  {1, 9},   {3, 11},  {5, 17},  {11, 17},
        {9, 17},  {4, 10},  {6, 12},  {7, 14},  {4, 6},   {4, 7},   {12, 14}, {10, 14}, {6, 7},   {10, 12}, {6, 10},  {6, 17},  {12, 17},
        {7, 17},  {7, 10},  {12, 18}, {7, 12},  {10, 18}, {12, 20}, {10, 20}, {10, 12}};
#pragma unroll
    for (int e = 0; e < 99; ++e) cswap(p[NET[e][0]], p[NET[e][1]]);
    return p[12];
}

template <int K>
__global__ __launch_bounds__(WAVES * 64) void median_rgb_u8_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ sizes,
                                                                   int maxH, int maxW, uint8_t* __restrict__ dst, int dstMaxH, int dstMaxW,
                                                                   int tiles_x, int tiles_y) {
    constexpr int R = K / 2, A = halo_bytes(R);
    __shared__ uint32_t stage[(TILE_ROWS + 2 * R) * STAGE_DW];
    TileAt t;
    if (!tile_of_block(src, sizes, maxH, maxW, dst, dstMaxH, dstMaxW, tiles_x, tiles_y, t)) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int out_rows = t.y_end - t.y0;
    stage_tile(stage, t, maxW, R, A, out_rows + 2 * R, lane, wave);
    __syncthreads();
    for (int yy = wave; yy < out_rows; yy += WAVES) {
        u16x2 even[K * K], odd[K * K];                                // bytes 0, 2 and bytes 1, 3 of the lane's dword, per window element
#pragma unroll
        for (int dy = 0; dy < K; ++dy)
#pragma unroll
            for (int dx = 0; dx < K; ++dx) {
                const uint32_t v = bytes_at(stage + (yy + dy) * STAGE_DW + lane, A - 3 * R + 3 * dx);
                even[dy * K + dx] = __builtin_bit_cast(u16x2, v & 0x00FF00FFu);
                odd[dy * K + dx] = __builtin_bit_cast(u16x2, (v >> 8) & 0x00FF00FFu);
            }
        uint32_t e, o;
        if constexpr (K == 3) {
            e = __builtin_bit_cast(uint32_t, median9(even));
            o = __builtin_bit_cast(uint32_t, median9(odd));
        } else {
            e = __builtin_bit_cast(uint32_t, median25(even));
            o = __builtin_bit_cast(uint32_t, median25(odd));
        }
        store_row(t, t.y0 + yy, dstMaxW, lane, e | (o << 8));
    }
}

}  // namespace

extern "C" int vip_blur_gauss_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH,
                                     int dstMaxW, const int32_t* weights_d, int radius, int n, void* stream) {
    Grid g;                                                         // (tiles of the source slot) x n
    if (int st = check_slots("vip_blur_gauss_rgb_u8", src_u8, sizes_hw, maxH, maxW, dst_u8, dstMaxH, dstMaxW, n, COUNT_SOURCE, TILE_ROWS, TILE_BYTES, &g))
        return st;
    VIP_REQUIRE(weights_d, VIP_ERR_BAD_ARG, "vip_blur_gauss_rgb_u8: null pointer");
    VIP_REQUIRE(radius >= 1 && radius <= MAX_RADIUS, VIP_ERR_BAD_ARG, "vip_blur_gauss_rgb_u8: radius %d outside 1..%d", radius, MAX_RADIUS);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(weights_d) & 3) == 0, VIP_ERR_ALIGNMENT, "vip_blur_gauss_rgb_u8: weights must be 4-byte aligned");
    hipLaunchKernelGGL(blur_gauss_rgb_u8_kernel<false>, dim3((unsigned)g.total), dim3(WAVES * 64), 0, (hipStream_t)stream, src_u8, sizes_hw,
                       maxH, maxW, dst_u8, dstMaxH, dstMaxW, weights_d, radius, g.tiles_x, g.tiles_y, 0, 0);
    return vip_launch_status("vip_blur_gauss_rgb_u8");
}

extern "C" int vip_sharpen_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH,
                                  int dstMaxW, const int32_t* weights_d, int radius, int amount_q8, int threshold, int n, void* stream) {
    Grid g;                                                         // (tiles of the source slot) x n
    if (int st = check_slots("vip_sharpen_rgb_u8", src_u8, sizes_hw, maxH, maxW, dst_u8, dstMaxH, dstMaxW, n, COUNT_SOURCE, TILE_ROWS, TILE_BYTES, &g))
        return st;
    VIP_REQUIRE(weights_d, VIP_ERR_BAD_ARG, "vip_sharpen_rgb_u8: null pointer");
    VIP_REQUIRE(radius >= 1 && radius <= MAX_RADIUS, VIP_ERR_BAD_ARG, "vip_sharpen_rgb_u8: radius %d outside 1..%d", radius, MAX_RADIUS);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(weights_d) & 3) == 0, VIP_ERR_ALIGNMENT, "vip_sharpen_rgb_u8: weights must be 4-byte aligned");
    VIP_REQUIRE(amount_q8 >= 1 && amount_q8 <= 1280, VIP_ERR_BAD_ARG, "vip_sharpen_rgb_u8: amount_q8 %d outside 1..1280", amount_q8);
    VIP_REQUIRE(threshold >= 0 && threshold <= 255, VIP_ERR_BAD_ARG, "vip_sharpen_rgb_u8: threshold %d outside 0..255", threshold);
    hipLaunchKernelGGL(blur_gauss_rgb_u8_kernel<true>, dim3((unsigned)g.total), dim3(WAVES * 64), 0, (hipStream_t)stream, src_u8, sizes_hw,
                       maxH, maxW, dst_u8, dstMaxH, dstMaxW, weights_d, radius, g.tiles_x, g.tiles_y, amount_q8, threshold);
    return vip_launch_status("vip_sharpen_rgb_u8");
}

extern "C" int vip_median_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH,
                                 int dstMaxW, int k, int n, void* stream) {
    Grid g;                                                         // (tiles of the source slot) x n
    if (int st = check_slots("vip_median_rgb_u8", src_u8, sizes_hw, maxH, maxW, dst_u8, dstMaxH, dstMaxW, n, COUNT_SOURCE, TILE_ROWS, TILE_BYTES, &g))
        return st;
    VIP_REQUIRE(k == 3 || k == 5, VIP_ERR_BAD_ARG, "vip_median_rgb_u8: window %d: expected 3 or 5", k);
    if (k == 3)
        hipLaunchKernelGGL(median_rgb_u8_kernel<3>, dim3((unsigned)g.total), dim3(WAVES * 64), 0, (hipStream_t)stream, src_u8, sizes_hw, maxH,
                           maxW, dst_u8, dstMaxH, dstMaxW, g.tiles_x, g.tiles_y);
    else
        hipLaunchKernelGGL(median_rgb_u8_kernel<5>, dim3((unsigned)g.total), dim3(WAVES * 64), 0, (hipStream_t)stream, src_u8, sizes_hw, maxH,
                           maxW, dst_u8, dstMaxH, dstMaxW, g.tiles_x, g.tiles_y);
    return vip_launch_status("vip_median_rgb_u8");
}
