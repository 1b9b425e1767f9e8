// Additive Gaussian noise (per channel or luminance), multiplicative speckle and salt-and-pepper impulses on decoded u8 RGB pixels, all
// in integers and from a counter-based generator: the one kernel under the noise stress perturbations (pipeline.gaussian_noise,
// mono_noise, speckle, impulse; --stress-noise / -noise-mono / -speckle / -impulse).  The reference's dataset/augment.py has no noise
// augmentation; this goes beyond it, as the resize stress test did.  Every image of a mixed-size batch keeps its size.
//
// Arithmetic (part of the interface; include/vipcup_hip.h).
//   Random words: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85; ten rounds, the key bumped
//   between rounds).  Pixel (x, y) of image i IN THE IMAGE'S OWN COORDINATES has the counter (x, y, 0, 0) and the key (seed, keys[i]); the
//   four output words are w0..w3.  The field depends on seed, key and position only - not on mode, amount, batch index, slot pitch or
//   batch size - so two amounts see the same field at two gains and a file keyed by its name gets the same noise in any batch.
//   Standard normal in Q12: T[i] = round(4096 Phi^-1(i / 4096)) for 0 < i < 4096, T[0] = -16384, T[4096] = 16384 (built by the host in
//   float64, passed as 4097 integers) and
//     z(w) = T[w >> 20] + (((T[(w >> 20) + 1] - T[w >> 20]) * ((w >> 5) & 0x7FFF) + 16384) >> 15)
//   - the inverse CDF, linear inside each of 4096 bins, cut at +-4.  The largest step of T is 2101, so the product stays below
//   2101 * 32767 + 16384 < 2^27.
//   Modes, signed 32-bit integers, arithmetic shifts (floor, also for a negative sum), X the input sample:
//     0 gaussian  out_c = clamp(X_c + ((a z(w_c) + 2^19) >> 20), 0, 255), c = 0, 1, 2     a = round(256 sigma) in 128..12800
//                                                                                           |a z| <= 12800 * 16384 < 2^28
//     1 mono      mode 0 with z(w0) on all three channels (luminance noise)
//     2 speckle   out_c = clamp(X_c + ((X_c a z(w_c) + 2^19) >> 20), 0, 255)                a = round(256 P / 100) in 3..128
//                                                                                           |X a z| <= 255 * 128 * 16384 < 2^29
//     3 impulse   w3 < thr (unsigned): all three channels (w2 & 1) ? 255 : 0; else a copy    thr = round(P / 100 * 2^32) in 4294967..2^31
//   No sum leaves 32 bits.
//
// One launch per variant per batch.  The byte movement is colour.hip's - that file's tile scheme is REPEATED here on purpose (a shared
// header is a refactor of its own, with its own bit-exactness check; colour.hip is untouched): a workgroup (4 waves) owns 128 pixels x 8
// rows; (1) every tile row is fetched as the ALIGNED dwords of the source that cover it into an LDS image that keeps the row's byte phase,
// the head and the tail of a row - dwords that also hold a neighbour's bytes - byte by byte, so nothing outside the image's pixels is
// read; (2) a lane takes one pixel: three byte reads at the source phase, the generator, three byte writes into a second LDS image at the
// DESTINATION row's phase; (3) that image leaves as the aligned dwords of the destination, head and tail byte by byte, so nothing outside
// the image's pixels is written.
// What is new is about 100 integer operations of Philox per pixel and, in modes 0..2, two table reads per normal sample.  The 16 KB table
// has two placements, chosen by a template parameter: gathers from global memory through the vector L1 (one tile per workgroup, as
// colour.hip), or a copy in LDS with the workgroup looping over GROUP consecutive tiles so that the copy - more bytes than a tile - is
// amortised.  The gathers measured faster (256 images of 200 x 200; README.md, profiles/noise_bench.log) and are what vip_noise_rgb_u8
// launches; vip_noise_rgb_u8_placed chooses explicitly, for the benchmark and the tests.  Mode 3 reads no table and copies none.  A tile outside
// its image is skipped, so the launch needs nothing from the host but the slot shapes: no copy, no allocation, no atomics,
// bit-reproducible.
#include "common.hpp"

namespace {

constexpr int TILE_W = 128, TILE_H = 8, WAVES = 4;
constexpr int ROW_DW = TILE_W * 3 / 4 + 1;                        // 96 dwords of interleaved RGB + one for the row's phase (0..3 bytes)
constexpr int TABLE_N = 4097;
constexpr int GROUP = 8;                                          // tiles per workgroup when the table sits in LDS
constexpr int TAB_NONE = -1, TAB_GLOBAL = 0, TAB_LDS = 1;
constexpr int DEFAULT_PLACEMENT = TAB_GLOBAL;                     // the faster one as measured (profiles/noise_bench.log)
constexpr int MODE_GAUSSIAN = 0, MODE_MONO = 1, MODE_SPECKLE = 2, MODE_IMPULSE = 3;

// Philox4x32-10 of the counter (x, y, 0, 0) under the key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t x, uint32_t y, uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
    uint32_t c0 = x, c1 = y, c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// the Q12 standard normal of a word; T has 4097 entries and (w >> 20) + 1 <= 4096
template <typename Table>
__device__ __forceinline__ int normal_q12(uint32_t w, Table T) {
    const int i = (int)(w >> 20);
    const int t0 = T[i], t1 = T[i + 1];
    return t0 + (((t1 - t0) * (int)((w >> 5) & 0x7FFFu) + 16384) >> 15);
}

template <int MODE, int TAB>
__global__ __launch_bounds__(WAVES * 64) void noise_rgb_u8_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ sizes,
                                                                  int maxH, int maxW, uint8_t* __restrict__ dst, int dstMaxH, int dstMaxW,
                                                                  uint32_t amount, uint32_t seed, const uint32_t* __restrict__ keys,
                                                                  const int32_t* __restrict__ table, int tiles_x, int tiles_y, long total) {
    __shared__ uint32_t tin[TILE_H * ROW_DW], tout[TILE_H * ROW_DW];
    __shared__ int32_t tab_s[TAB == TAB_LDS ? TABLE_N : 1];
    constexpr int PER_GROUP = TAB == TAB_LDS ? GROUP : 1;
    uint8_t* tin_u8 = reinterpret_cast<uint8_t*>(tin);
    uint8_t* tout_u8 = reinterpret_cast<uint8_t*>(tout);
    const int per_image = tiles_x * tiles_y;
    const long spitch = (long)maxW * 3, dpitch = (long)dstMaxW * 3;

    if constexpr (TAB == TAB_LDS)                                  // read after the first barrier below
        for (int k = threadIdx.x; k < TABLE_N; k += WAVES * 64) tab_s[k] = table[k];

    for (int g = 0; g < PER_GROUP; ++g) {                          // every condition up to the barriers is uniform over the workgroup
        const long tile = (long)blockIdx.x * PER_GROUP + g;
        if (tile >= total) break;
        const int img = (int)(tile / per_image);
        const int t = (int)(tile - (long)img * per_image);
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int h = sizes[img * 2], w = sizes[img * 2 + 1];
        if (h < 1 || w < 1 || h > maxH || w > maxW || h > dstMaxH || w > dstMaxW) continue;   // skipped image
        const int x0 = tx * TILE_W, y0 = ty * TILE_H;
        if (x0 >= w || y0 >= h) continue;
        const int rows = min(TILE_H, h - y0), cols = min(TILE_W, w - x0);
        const int row_bytes = cols * 3;
        const uint8_t* stile = src + (((long)img * maxH + y0) * maxW + x0) * 3;
        uint8_t* dtile = dst + (((long)img * dstMaxH + y0) * dstMaxW + x0) * 3;

        // ---- (1) the source rows as aligned dwords; the LDS row keeps the phase of its global row ----
        for (int k = threadIdx.x; k < rows * ROW_DW; k += WAVES * 64) {
            const int r = k / ROW_DW, j = k - r * ROW_DW;
            const uint8_t* row = stile + r * spitch;
            const int ph = (int)(reinterpret_cast<uintptr_t>(row) & 3);
            const int b = j * 4 - ph;                              // the row byte at this dword's first byte
            if (b >= row_bytes) continue;
            if (b >= 0 && b + 4 <= row_bytes) {
                tin[k] = *reinterpret_cast<const uint32_t*>(row + b);
            } else {                                               // the row's head or tail: only its own bytes
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (b + q >= 0 && b + q < row_bytes) tin_u8[k * 4 + q] = row[b + q];
            }
        }
        const uint32_t key = keys[img];                            // wave-uniform
        __syncthreads();
        // ---- (2) one pixel per lane: from the source phase to the destination phase ----
        const int px = threadIdx.x & (TILE_W - 1);
        if (px < cols) {
            for (int r = threadIdx.x / TILE_W; r < rows; r += WAVES * 64 / TILE_W) {
                const int sph = (int)(reinterpret_cast<uintptr_t>(stile + r * spitch) & 3);
                const int dph = (int)(reinterpret_cast<uintptr_t>(dtile + r * dpitch) & 3);
                const uint8_t* p = tin_u8 + r * (ROW_DW * 4) + sph + px * 3;
                uint8_t* o = tout_u8 + r * (ROW_DW * 4) + dph + px * 3;
                uint32_t wd[4];
                philox4x32_10((uint32_t)(x0 + px), (uint32_t)(y0 + r), seed, key, wd);
                if constexpr (MODE == MODE_IMPULSE) {
                    const bool hit = wd[3] < amount;
                    const uint8_t v = (wd[2] & 1u) ? 255 : 0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[c] = hit ? v : p[c];
                } else {
                    int z[3];
                    if constexpr (TAB == TAB_LDS) {
                        z[0] = normal_q12(wd[0], tab_s);
                        if constexpr (MODE != MODE_MONO) z[1] = normal_q12(wd[1], tab_s), z[2] = normal_q12(wd[2], tab_s);
                    } else {
                        z[0] = normal_q12(wd[0], table);
                        if constexpr (MODE != MODE_MONO) z[1] = normal_q12(wd[1], table), z[2] = normal_q12(wd[2], table);
                    }
                    if constexpr (MODE == MODE_MONO) z[1] = z[2] = z[0];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int X = p[c];
                        const int az = (int)amount * z[c];
                        const int d = ((MODE == MODE_SPECKLE ? X * az : az) + (1 << 19)) >> 20;
                        o[c] = (uint8_t)min(max(X + d, 0), 255);
                    }
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
        // the next tile's (1) writes tin, which every thread has finished reading at the barrier above; its (2) writes tout after the
        // barrier that follows its (1), which no thread passes before it has left this (3)
    }
}

template <int MODE, int TAB>
void launch(long total, hipStream_t s, const uint8_t* src, const int32_t* sizes, int maxH, int maxW, uint8_t* dst, int dstMaxH, int dstMaxW,
            uint32_t amount, uint32_t seed, const uint32_t* keys, const int32_t* table, int tiles_x, int tiles_y) {
    const long groups = TAB == TAB_LDS ? (total + GROUP - 1) / GROUP : total;
    hipLaunchKernelGGL((noise_rgb_u8_kernel<MODE, TAB>), dim3((unsigned)groups), dim3(WAVES * 64), 0, s, src, sizes, maxH, maxW, dst, dstMaxH,
                       dstMaxW, amount, seed, keys, table, tiles_x, tiles_y, total);
}

}  // namespace

extern "C" int vip_noise_rgb_u8_placed(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH,
                                       int dstMaxW, int mode, int64_t amount, uint32_t seed, const uint32_t* keys_u32, const int32_t* table_i32,
                                       int placement, int n, void* stream) {
    const char* what = "vip_noise_rgb_u8";
    const bool tabled = mode != MODE_IMPULSE;
    VIP_REQUIRE(src_u8 && sizes_hw && dst_u8 && keys_u32 && (table_i32 || !tabled), VIP_ERR_BAD_ARG, "%s: null pointer", what);
    VIP_REQUIRE(n > 0 && maxH > 0 && maxW > 0 && dstMaxH > 0 && dstMaxW > 0, VIP_ERR_BAD_ARG, "%s: bad size", what);
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src_u8), s1 = s0 + (size_t)n * maxH * maxW * 3;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst_u8), d1 = d0 + (size_t)n * dstMaxH * dstMaxW * 3;
    VIP_REQUIRE(s1 <= d0 || d1 <= s0, VIP_ERR_BAD_ARG, "%s: source and destination overlap (the kernel cannot run in place)", what);
    VIP_REQUIRE(mode >= MODE_GAUSSIAN && mode <= MODE_IMPULSE, VIP_ERR_BAD_ARG, "%s: mode %d: no amount is defined for it (modes are 0..3)",
                what, mode);
    const int64_t lo = mode == MODE_IMPULSE ? 4294967 : mode == MODE_SPECKLE ? 3 : 128;
    const int64_t hi = mode == MODE_IMPULSE ? (int64_t)1 << 31 : mode == MODE_SPECKLE ? 128 : 12800;
    VIP_REQUIRE(amount >= lo && amount <= hi, VIP_ERR_BAD_ARG, "%s: amount %lld of mode %d is outside %lld..%lld", what, (long long)amount,
                mode, (long long)lo, (long long)hi);
    VIP_REQUIRE(placement == TAB_GLOBAL || placement == TAB_LDS, VIP_ERR_BAD_ARG, "%s: placement %d: expected 0 (global) or 1 (LDS)", what,
                placement);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(sizes_hw) & 3) == 0, VIP_ERR_ALIGNMENT, "%s: sizes must be 4-byte aligned", what);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(keys_u32) & 3) == 0, VIP_ERR_ALIGNMENT, "%s: keys must be 4-byte aligned", what);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(table_i32) & 3) == 0, VIP_ERR_ALIGNMENT, "%s: table must be 4-byte aligned", what);
    // an image that is written fits both slots
    const int tiles_x = ((maxW < dstMaxW ? maxW : dstMaxW) + TILE_W - 1) / TILE_W, tiles_y = ((maxH < dstMaxH ? maxH : dstMaxH) + TILE_H - 1) / TILE_H;
    const long total = (long)tiles_x * tiles_y * n;
    VIP_REQUIRE(total <= 0x7FFFFFFFL, VIP_ERR_UNSUPPORTED, "%s: %ld tiles exceed one launch's grid", what, total);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t a = (uint32_t)amount;
#define VIP_NOISE_LAUNCH(MODE, TAB) \
    launch<MODE, TAB>(total, s, src_u8, sizes_hw, maxH, maxW, dst_u8, dstMaxH, dstMaxW, a, seed, keys_u32, table_i32, tiles_x, tiles_y)
    if (mode == MODE_IMPULSE) VIP_NOISE_LAUNCH(MODE_IMPULSE, TAB_NONE);
    else if (placement == TAB_LDS) {
        if (mode == MODE_GAUSSIAN) VIP_NOISE_LAUNCH(MODE_GAUSSIAN, TAB_LDS);
        else if (mode == MODE_MONO) VIP_NOISE_LAUNCH(MODE_MONO, TAB_LDS);
        else VIP_NOISE_LAUNCH(MODE_SPECKLE, TAB_LDS);
    } else {
        if (mode == MODE_GAUSSIAN) VIP_NOISE_LAUNCH(MODE_GAUSSIAN, TAB_GLOBAL);
        else if (mode == MODE_MONO) VIP_NOISE_LAUNCH(MODE_MONO, TAB_GLOBAL);
        else VIP_NOISE_LAUNCH(MODE_SPECKLE, TAB_GLOBAL);
    }
#undef VIP_NOISE_LAUNCH
    return vip_launch_status(what);
}

extern "C" int vip_noise_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH, int dstMaxW,
                                int mode, int64_t amount, uint32_t seed, const uint32_t* keys_u32, const int32_t* table_i32, int n,
                                void* stream) {
    return vip_noise_rgb_u8_placed(src_u8, sizes_hw, maxH, maxW, dst_u8, dstMaxH, dstMaxW, mode, amount, seed, keys_u32, table_i32,
                                   DEFAULT_PLACEMENT, n, stream);
}
