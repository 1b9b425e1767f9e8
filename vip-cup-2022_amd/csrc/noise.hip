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
// One launch per variant per batch.  The byte movement is rgb_tile.hpp's streaming tile, shared with colour.hip and tone.hip (a
// workgroup owns 128 pixels x 8 rows; aligned dwords in, an LDS image per side that keeps the row's byte phase, aligned dwords out;
// nothing outside an image's pixels is read or written); what is here is one pixel's generator.
// That is about 100 integer operations of Philox per pixel and, in modes 0..2, two table reads per normal sample.  The 16 KB table
// has two placements, chosen by a template parameter: gathers from global memory through the vector L1 (one tile per workgroup, as
// colour.hip), or a copy in LDS with the workgroup looping over GROUP consecutive tiles so that the copy - more bytes than a tile - is
// amortised.  The gathers measured faster (256 images of 200 x 200; README.md, profiles/noise_bench.log) and are what vip_noise_rgb_u8
// launches; vip_noise_rgb_u8_placed chooses explicitly, for the benchmark and the tests.  Mode 3 reads no table and copies none.  A tile outside
// its image is skipped, so the launch needs nothing from the host but the slot shapes: no copy, no allocation, no atomics,
// bit-reproducible.
#include "rgb_tile.hpp"

namespace {

using namespace rgb_tile;

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
__global__ __launch_bounds__(THREADS) void noise_rgb_u8_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ sizes,
                                                               int maxH, int maxW, uint8_t* __restrict__ dst, int dstMaxH, int dstMaxW,
                                                               uint32_t amount, uint32_t seed, const uint32_t* __restrict__ keys,
                                                               const int32_t* __restrict__ table, int tiles_x, int tiles_y, long total) {
    __shared__ uint32_t tin[TILE_H * ROW_DW], tout[TILE_H * ROW_DW];
    __shared__ int32_t tab_s[TAB == TAB_LDS ? TABLE_N : 1];
    constexpr int PER_GROUP = TAB == TAB_LDS ? GROUP : 1;

    if constexpr (TAB == TAB_LDS)                                  // read after the first barrier below
        for (int k = threadIdx.x; k < TABLE_N; k += THREADS) tab_s[k] = table[k];

    for (int g = 0; g < PER_GROUP; ++g) {                          // every condition up to the barriers is uniform over the workgroup
        const long tile = (long)blockIdx.x * PER_GROUP + g;
        if (tile >= total) break;
        Tile t;
        if (!locate(tile, src, sizes, maxH, maxW, dst, dstMaxH, dstMaxW, tiles_x, tiles_y, t)) continue;
        load_rows(t, tin);
        const uint32_t key = keys[t.img];                          // wave-uniform
        __syncthreads();
        for_each_pixel(t, tin, tout, [&](int r, int px, const uint8_t* p, uint8_t* o) {
            uint32_t wd[4];
            philox4x32_10((uint32_t)(t.x0 + px), (uint32_t)(t.y0 + r), seed, key, wd);
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
        });
        __syncthreads();
        store_rows(t, tout);
        // the next tile's load_rows writes tin, which every thread has finished reading at the barrier above; its pixels are written to tout after the
        // barrier that follows its load_rows, which no thread passes before it has left this store_rows
    }
}

template <int MODE, int TAB>
void launch(long total, hipStream_t s, const uint8_t* src, const int32_t* sizes, int maxH, int maxW, uint8_t* dst, int dstMaxH, int dstMaxW,
            uint32_t amount, uint32_t seed, const uint32_t* keys, const int32_t* table, int tiles_x, int tiles_y) {
    const long groups = TAB == TAB_LDS ? (total + GROUP - 1) / GROUP : total;
    hipLaunchKernelGGL((noise_rgb_u8_kernel<MODE, TAB>), dim3((unsigned)groups), dim3(THREADS), 0, s, src, sizes, maxH, maxW, dst, dstMaxH,
                       dstMaxW, amount, seed, keys, table, tiles_x, tiles_y, total);
}

}  // namespace

extern "C" int vip_noise_rgb_u8_placed(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH,
                                       int dstMaxW, int mode, int64_t amount, uint32_t seed, const uint32_t* keys_u32, const int32_t* table_i32,
                                       int placement, int n, void* stream) {
    const char* what = "vip_noise_rgb_u8";
    const bool tabled = mode != MODE_IMPULSE;
    Grid g;
    if (int st = check_slots(what, src_u8, sizes_hw, maxH, maxW, dst_u8, dstMaxH, dstMaxW, n, COUNT_BOTH, TILE_H, TILE_W * 3, &g)) return st;
    VIP_REQUIRE(keys_u32 && (table_i32 || !tabled), VIP_ERR_BAD_ARG, "%s: null pointer", what);
    VIP_REQUIRE(mode >= MODE_GAUSSIAN && mode <= MODE_IMPULSE, VIP_ERR_BAD_ARG, "%s: mode %d: no amount is defined for it (modes are 0..3)",
                what, mode);
    const int64_t lo = mode == MODE_IMPULSE ? 4294967 : mode == MODE_SPECKLE ? 3 : 128;
    const int64_t hi = mode == MODE_IMPULSE ? (int64_t)1 << 31 : mode == MODE_SPECKLE ? 128 : 12800;
    VIP_REQUIRE(amount >= lo && amount <= hi, VIP_ERR_BAD_ARG, "%s: amount %lld of mode %d is outside %lld..%lld", what, (long long)amount,
                mode, (long long)lo, (long long)hi);
    VIP_REQUIRE(placement == TAB_GLOBAL || placement == TAB_LDS, VIP_ERR_BAD_ARG, "%s: placement %d: expected 0 (global) or 1 (LDS)", what,
                placement);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(keys_u32) & 3) == 0, VIP_ERR_ALIGNMENT, "%s: keys must be 4-byte aligned", what);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(table_i32) & 3) == 0, VIP_ERR_ALIGNMENT, "%s: table must be 4-byte aligned", what);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t a = (uint32_t)amount;
#define VIP_NOISE_LAUNCH(MODE, TAB) \
    launch<MODE, TAB>(g.total, s, src_u8, sizes_hw, maxH, maxW, dst_u8, dstMaxH, dstMaxW, a, seed, keys_u32, table_i32, g.tiles_x, g.tiles_y)
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
