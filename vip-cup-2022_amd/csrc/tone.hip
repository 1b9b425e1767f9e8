// Tone curves that are MEASURED from the picture: auto-contrast (per channel, or one curve from the luma), histogram equalisation and
// contrast-limited adaptive equalisation of the luma (CLAHE), on decoded u8 RGB pixels at each image's own size - the kernels under
// pipeline.autocontrast / equalize / clahe / tone and --stress-autocontrast / -autocontrast-luma / -equalize / -clahe.  The first two
// are Pillow's ImageOps.autocontrast (also preserve_tone=True) and ImageOps.equalize bit for bit; CLAHE is this project's own integer
// definition.  include/vipcup_hip.h has the arithmetic, which is part of the interface.
//
// A variant is three launches with no host round trip; histograms and tables stay on the device.
//   vip_tone_hist_u8       one workgroup per (image, tile slot): the tile's pixels go into an LDS histogram with LDS atomics (integer
//                          counts: the sum does not depend on the order) and the finished histogram leaves with plain stores.  Every
//                          slot of the output is written - an unused slot with zeros - so nothing depends on what the buffer held.
//   vip_tone_lut_u8        one workgroup (256 threads, one per level) per table: the sum over the image's tile slots (global modes), an
//                          inclusive scan (shuffles inside a wave, the waves' totals through LDS), then the mode's rule.  The auto-contrast table is Pillow's float64 expression: 255.0 / d
//                          comes from a table the compiler folds (IEEE round to nearest), the two products and the sum are rounded one
//                          by one (__dmul_rn / __dadd_rn, contraction off).
//   vip_tone_apply_rgb_u8  streams the pixels through rgb_tile.hpp's streaming tile, as colour.hip and noise.hip do, and applies the
//                          image's table(s) from LDS.  CLAHE reads the four neighbouring tile tables at Y and blends them; the tables are either gathered from global
//                          memory through the vector L1 or the at most 3 x 10 tables a workgroup's 128 x 8 pixels can touch are copied
//                          into LDS first (placement 0 / 1; README.md has the measurement).
// No allocation, no global atomics: bit-reproducible.
#include "rgb_tile.hpp"

namespace {

using namespace rgb_tile;                                         // the streaming tile of the apply kernel, and THREADS

constexpr int MAX_SIDE = 1 << 26;                                  // 16 * side stays below 2^31
constexpr int MAX_GRID = 16;
// the tile tables a workgroup's pixels can touch: tiles are at least 16 pixels wide, so their centres lie at least 16 pixels apart; 128
// pixels hold at most 8 centres between their first and last pixel -> k0(first) .. k0(first) + 8, and k1 adds one: 10; 8 rows: 3
constexpr int STAGE_KX = 10, STAGE_KY = 3;

__device__ __forceinline__ int luma_u8(int R, int G, int B) { return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16; }

// grid per axis and tile edges: the rule of pipeline.tone_grid / occlusion_bounds
__device__ __forceinline__ int axis_grid(int side, int G) { return min(G, max(1, side >> 4)); }
__device__ __forceinline__ int axis_edge(int k, int side, int g) { return (int)((unsigned)(k * side) / (unsigned)g); }

// ---------------------------------------------------------------------------------------------------------------------------------
// histograms

template <int C>
__global__ __launch_bounds__(THREADS) void tone_hist_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ sizes, int maxH,
                                                            int maxW, int G, int32_t* __restrict__ hist, int slots) {
    __shared__ int32_t bins[C * 256];
    const int img = (int)blockIdx.x / slots, t = (int)blockIdx.x - img * slots;
    for (int k = threadIdx.x; k < C * 256; k += THREADS) bins[k] = 0;
    const int h = sizes[img * 2], w = sizes[img * 2 + 1];
    int32_t* out = hist + ((long)img * slots + t) * (C * 256);
    bool live = h >= 1 && w >= 1 && h <= maxH && w <= maxW;
    int gy = 1, gx = 1;
    if (live) {
        gy = axis_grid(h, G), gx = axis_grid(w, G);
        live = gy * gx <= slots && t < gy * gx;                    // an image whose grid does not fit the slots counts nothing
    }
    __syncthreads();
    if (live) {
        const int ty = t / gx, tx = t - ty * gx;
        const int y0 = axis_edge(ty, h, gy), y1 = axis_edge(ty + 1, h, gy), x0 = axis_edge(tx, w, gx), x1 = axis_edge(tx + 1, w, gx);
        const int tw = x1 - x0, total = (y1 - y0) * tw;
        const uint8_t* base = src + (((long)img * maxH + y0) * maxW + x0) * 3;
        const long pitch = (long)maxW * 3;
        for (int k = threadIdx.x; k < total; k += THREADS) {
            const int r = (int)((unsigned)k / (unsigned)tw), x = k - r * tw;
            const uint8_t* p = base + r * pitch + x * 3;
            const int R = p[0], Gr = p[1], B = p[2];
            if (C == 3) {
                atomicAdd(&bins[R], 1);
                atomicAdd(&bins[256 + Gr], 1);
                atomicAdd(&bins[512 + B], 1);
            } else {
                atomicAdd(&bins[luma_u8(R, Gr, B)], 1);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < C * 256; k += THREADS) out[k] = bins[k];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// tables

struct ScaleTable {                                                // 255.0 / d, folded by the compiler in IEEE double, round to nearest
    double v[256];
    constexpr ScaleTable() : v() {
        for (int d = 1; d < 256; ++d) v[d] = 255.0 / (double)d;
    }
};
__constant__ const ScaleTable kScale = ScaleTable();

// inclusive scan over the workgroup's 256 values: a shuffle scan inside each wave, the waves' totals through `s`, which is free
// again on return
__device__ __forceinline__ int scan256(int v, int* s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int a = __shfl_up(v, off, 64);
        if (lane >= off) v += a;
    }
    if (lane == 63) s[wave] = v;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int w = 0; w < 3; ++w) before += w < wave ? s[w] : 0;
    __syncthreads();
    return v + before;
}

__device__ __forceinline__ int autocontrast_entry(int i, int lo, int hi) {
    // build.py compiles this file with -ffp-contract=off; the empty asm pins each product in a register besides, so that no
    // multiply-add can be formed from them whatever the flags
    const double scale = kScale.v[hi - lo];
    double offset = __dmul_rn((double)(-lo), scale);
    double prod = __dmul_rn((double)i, scale);
    asm volatile("" : "+v"(offset), "+v"(prod));
    const double x = __dadd_rn(prod, offset);
    return min(max((int)x, 0), 255);                               // (int): towards zero, as Python's int()
}

// one workgroup per table.  Global modes: table (img, c) from the sum of the image's `slots` histograms; CLAHE: table (img, slot).
__global__ __launch_bounds__(256) void tone_lut_kernel(const int32_t* __restrict__ hist, int slots, int C, int mode, int param,
                                                       uint8_t* __restrict__ lut) {
    __shared__ int s[256];
    __shared__ int found[4];
    const int i = threadIdx.x;
    int hv = 0;
    if (mode == VIP_TONE_CLAHE) {
        hv = hist[(long)blockIdx.x * 256 + i];
    } else {
        const int img = (int)blockIdx.x / C, c = (int)blockIdx.x - img * C;
        const int32_t* p = hist + ((long)img * slots * C + c) * 256 + i;
        for (int t = 0; t < slots; ++t) hv += p[(long)t * C * 256];
    }
    if (i < 4) found[i] = i == 2 ? -1 : 0;                          // lo, hi, last non-zero bin, non-zero bins
    const int cum = scan256(hv, s);                                // also orders the write of found[]
    s[i] = cum;
    __syncthreads();
    const int total = s[255];
    const int before = cum - hv;
    int v = i;                                                     // the identity
    if (mode == VIP_TONE_AC || mode == VIP_TONE_ACL) {
        const long cut = ((long)total * param) / 100;
        // lo: the smallest i whose prefix sum exceeds cut; hi: the largest i whose suffix sum (total - before) exceeds cut
        if (cum > cut && before <= cut) found[0] = i;
        const int after = total - cum;                             // the suffix sum of i + 1
        if ((long)(total - before) > cut && (i == 255 || after <= cut)) found[1] = i;
        __syncthreads();
        const int lo = found[0], hi = found[1];
        if (total > 0 && hi > lo) v = autocontrast_entry(i, lo, hi);
    } else if (mode == VIP_TONE_EQ) {
        if (hv != 0) {
            atomicMax(&found[2], i);
            atomicAdd(&found[3], 1);
        }
        __syncthreads();
        if (found[3] >= 2) {
            const int step = (total - (s[found[2]] - (found[2] ? s[found[2] - 1] : 0))) / 255;
            if (step != 0) v = (int)min(((long)(step >> 1) + before) / step, 255L);
        }
    } else {                                                       // CLAHE; an unused slot (no pixels) gets the identity
        const int A = total;
        __syncthreads();                                           // everyone has read s[255]
        if (A > 0) {
            const int clip = (int)max(1L, ((long)param * A) / 2560);
            const int hc = min(hv, clip);
            const int cc = scan256(hc, s);
            s[i] = cc;
            __syncthreads();
            const int E = A - s[255];
            __syncthreads();
            const int q = E >> 8, rem = E & 255;
            const int h2 = hc + q + (((i * rem) >> 8) != (((i + 1) * rem) >> 8) ? 1 : 0);
            const int c2 = scan256(h2, s);
            v = (int)(((long)c2 * 255 + (A >> 1)) / A);
        }
    }
    lut[(long)blockIdx.x * 256 + i] = (uint8_t)v;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// apply

// the two neighbouring tiles of pixel p along an axis of `side` pixels in g tiles, and the weight of the second in 1 / 256:
// k0 | k1 << 8 | wq << 16
__device__ int axis_neighbours(int p, int side, int g) {
    const int X2 = 2 * p + 1;
    int cnt = 0;                                                   // the centres (doubled: b[k] + b[k + 1]) at or below X2
    int prev = 0;
    for (int k = 0; k < g; ++k) {
        const int next = axis_edge(k + 1, side, g);
        cnt += (prev + next <= X2);
        prev = next;
    }
    if (cnt == 0) return 0;
    if (cnt == g) return (g - 1) | ((g - 1) << 8);
    const int k = cnt - 1;
    const int bk = axis_edge(k, side, g), bk1 = axis_edge(k + 1, side, g), bk2 = axis_edge(k + 2, side, g);
    const unsigned num = (unsigned)(X2 - bk - bk1), den = (unsigned)(bk2 - bk);
    const unsigned wq = num < (1u << 23) ? (num << 8) / den : (unsigned)(((unsigned long)num << 8) / den);
    return k | ((k + 1) << 8) | ((int)wq << 16);
}

// KIND 0: one table per channel; 1: one table on all three channels; 2: CLAHE, tables gathered from global memory; 3: CLAHE, tables in LDS
template <int KIND>
__global__ __launch_bounds__(THREADS) void tone_apply_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ sizes, int maxH,
                                                             int maxW, uint8_t* __restrict__ dst, int dstMaxH, int dstMaxW,
                                                             const uint8_t* __restrict__ lut, int G, int slots, int tiles_x, int tiles_y) {
    constexpr bool CLAHE = KIND >= 2;
    constexpr int LUT_DW = KIND == 0 ? 192 : KIND == 1 ? 64 : KIND == 3 ? STAGE_KX * STAGE_KY * 64 : 1;
    __shared__ uint32_t tin[TILE_H * ROW_DW], tout[TILE_H * ROW_DW];
    __shared__ uint32_t lut_s[LUT_DW];
    __shared__ int nx_s[CLAHE ? TILE_W : 1], ny_s[CLAHE ? TILE_H : 1];
    Tile t;
    if (!locate((int)blockIdx.x, src, sizes, maxH, maxW, dst, dstMaxH, dstMaxW, tiles_x, tiles_y, t)) return;
    const int img = t.img, h = t.h, w = t.w, x0 = t.x0, y0 = t.y0, rows = t.rows, cols = t.cols;
    const int gy = CLAHE ? axis_grid(h, G) : 1, gx = CLAHE ? axis_grid(w, G) : 1;
    if (CLAHE && gy * gx > slots) return;                          // its tables do not exist: skipped like an image that does not fit
    const uint8_t* lut_u8 = reinterpret_cast<const uint8_t*>(lut_s);
    const uint8_t* tables = lut + (long)img * slots * 256;         // CLAHE: the image's tile tables

    if (KIND == 0) {
        if (threadIdx.x < 192) lut_s[threadIdx.x] = reinterpret_cast<const uint32_t*>(lut + (long)img * 768)[threadIdx.x];
    } else if (KIND == 1) {
        if (threadIdx.x < 64) lut_s[threadIdx.x] = reinterpret_cast<const uint32_t*>(lut + (long)img * 256)[threadIdx.x];
    } else {
        if (threadIdx.x < cols) nx_s[threadIdx.x] = axis_neighbours(x0 + (int)threadIdx.x, w, gx);
        else if (threadIdx.x >= TILE_W && (int)threadIdx.x - TILE_W < rows) ny_s[threadIdx.x - TILE_W] = axis_neighbours(y0 + (int)threadIdx.x - TILE_W, h, gy);
    }
    load_rows(t, tin);
    int kx_lo = 0, ky_lo = 0, nkx = 1;
    bool staged = false;
    if (KIND == 3) {
        __syncthreads();                                           // the neighbours are known
        kx_lo = nx_s[0] & 255, ky_lo = ny_s[0] & 255;
        nkx = ((nx_s[cols - 1] >> 8) & 255) - kx_lo + 1;
        const int nky = ((ny_s[rows - 1] >> 8) & 255) - ky_lo + 1;
        staged = nkx <= STAGE_KX && nky <= STAGE_KY;               // always (see STAGE_KX); otherwise the gathers below
        if (staged) {
            for (int k = threadIdx.x; k < nky * nkx * 64; k += THREADS) {
                const int tab = k >> 6, j = k & 63;
                const int ky = tab / nkx, kx = tab - ky * nkx;
                lut_s[k] = reinterpret_cast<const uint32_t*>(tables + (long)((ky_lo + ky) * gx + kx_lo + kx) * 256)[j];
            }
        }
    }
    __syncthreads();
    for_each_pixel(t, tin, tout, [&](int r, int px, const uint8_t* p, uint8_t* o) {
        const int R = p[0], Gr = p[1], B = p[2];
        if (KIND == 0) {
            o[0] = lut_u8[R], o[1] = lut_u8[256 + Gr], o[2] = lut_u8[512 + B];
        } else if (KIND == 1) {
            o[0] = lut_u8[R], o[1] = lut_u8[Gr], o[2] = lut_u8[B];
        } else {
            const int Y = luma_u8(R, Gr, B);
            const int ax = nx_s[px], ay = ny_s[r];
            const int kx0 = ax & 255, kx1 = (ax >> 8) & 255, wx = ax >> 16;
            const int ky0 = ay & 255, ky1 = (ay >> 8) & 255, wy = ay >> 16;
            int t00, t01, t10, t11;
            if (KIND == 3 && staged) {
                const uint8_t* r0 = lut_u8 + (ky0 - ky_lo) * nkx * 256 + Y, *r1 = lut_u8 + (ky1 - ky_lo) * nkx * 256 + Y;
                t00 = r0[(kx0 - kx_lo) * 256], t01 = r0[(kx1 - kx_lo) * 256];
                t10 = r1[(kx0 - kx_lo) * 256], t11 = r1[(kx1 - kx_lo) * 256];
            } else {
                const uint8_t* r0 = tables + (long)ky0 * gx * 256 + Y, *r1 = tables + (long)ky1 * gx * 256 + Y;
                t00 = r0[kx0 * 256], t01 = r0[kx1 * 256];
                t10 = r1[kx0 * 256], t11 = r1[kx1 * 256];
            }
            const int V = ((256 - wy) * ((256 - wx) * t00 + wx * t01) + wy * ((256 - wx) * t10 + wx * t11) + 32768) >> 16;
            const int d = V - Y;
            o[0] = (uint8_t)min(max(R + d, 0), 255);
            o[1] = (uint8_t)min(max(Gr + d, 0), 255);
            o[2] = (uint8_t)min(max(B + d, 0), 255);
        }
    });
    __syncthreads();
    store_rows(t, tout);
}

int check_mode(const char* what, int mode, int param) {
    VIP_REQUIRE(mode >= VIP_TONE_AC && mode <= VIP_TONE_CLAHE, VIP_ERR_BAD_ARG, "%s: mode %d: expected 0 (ac), 1 (acl), 2 (eq) or 3 (clahe)", what,
                mode);
    if (mode == VIP_TONE_AC || mode == VIP_TONE_ACL)
        VIP_REQUIRE(param >= 0 && param <= 49, VIP_ERR_BAD_ARG, "%s: cutoff %d: expected a percent in 0..49", what, param);
    else if (mode == VIP_TONE_EQ)
        VIP_REQUIRE(param == 0, VIP_ERR_BAD_ARG, "%s: parameter %d: mode 2 (eq) takes 0", what, param);
    else
        VIP_REQUIRE(param >= 10 && param <= 99, VIP_ERR_BAD_ARG, "%s: clip limit %d tenths: expected 10..99", what, param);
    return VIP_OK;
}

}  // namespace

extern "C" int vip_tone_hist_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int n, int maxH, int maxW, int grid, int channels,
                                int32_t* hist_i32, int slots, void* stream) {
    const char* what = "vip_tone_hist_u8";
    VIP_REQUIRE(src_u8 && sizes_hw && hist_i32, VIP_ERR_BAD_ARG, "%s: null pointer", what);
    VIP_REQUIRE(n > 0 && maxH > 0 && maxW > 0 && maxH <= MAX_SIDE && maxW <= MAX_SIDE, VIP_ERR_BAD_ARG, "%s: bad size", what);
    VIP_REQUIRE(grid >= 1 && grid <= MAX_GRID, VIP_ERR_BAD_ARG, "%s: grid %d: expected 1..%d", what, grid, MAX_GRID);
    VIP_REQUIRE(channels == 1 || channels == 3, VIP_ERR_BAD_ARG, "%s: channels %d: expected 3 (R, G, B) or 1 (luma)", what, channels);
    VIP_REQUIRE(slots >= 1 && slots <= MAX_GRID * MAX_GRID, VIP_ERR_BAD_ARG, "%s: slots %d: expected 1..%d", what, slots, MAX_GRID * MAX_GRID);
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(sizes_hw) & 3) == 0 && (reinterpret_cast<uintptr_t>(hist_i32) & 3) == 0, VIP_ERR_ALIGNMENT,
                "%s: sizes and histograms must be 4-byte aligned", what);
    const long total = (long)n * slots;
    VIP_REQUIRE(total <= 0x7FFFFFFFL, VIP_ERR_UNSUPPORTED, "%s: %ld histograms exceed one launch's grid", what, total);
    if (channels == 3)
        hipLaunchKernelGGL(tone_hist_kernel<3>, dim3((unsigned)total), dim3(THREADS), 0, (hipStream_t)stream, src_u8, sizes_hw, maxH, maxW, grid,
                           hist_i32, slots);
    else
        hipLaunchKernelGGL(tone_hist_kernel<1>, dim3((unsigned)total), dim3(THREADS), 0, (hipStream_t)stream, src_u8, sizes_hw, maxH, maxW, grid,
                           hist_i32, slots);
    return vip_launch_status(what);
}

extern "C" int vip_tone_lut_u8(const int32_t* hist_i32, int n, int slots, int mode, int param, uint8_t* lut_u8, void* stream) {
    const char* what = "vip_tone_lut_u8";
    VIP_REQUIRE(hist_i32 && lut_u8, VIP_ERR_BAD_ARG, "%s: null pointer", what);
    VIP_REQUIRE(n > 0 && slots >= 1 && slots <= MAX_GRID * MAX_GRID, VIP_ERR_BAD_ARG, "%s: bad size", what);
    if (int st = check_mode(what, mode, param)) return st;
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(hist_i32) & 3) == 0 && (reinterpret_cast<uintptr_t>(lut_u8) & 3) == 0, VIP_ERR_ALIGNMENT,
                "%s: histograms and tables must be 4-byte aligned", what);
    const int C = (mode == VIP_TONE_AC || mode == VIP_TONE_EQ) ? 3 : 1;
    const long total = (long)n * (mode == VIP_TONE_CLAHE ? slots : C);
    VIP_REQUIRE(total <= 0x7FFFFFFFL, VIP_ERR_UNSUPPORTED, "%s: %ld tables exceed one launch's grid", what, total);
    hipLaunchKernelGGL(tone_lut_kernel, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, hist_i32, slots, C, mode, param, lut_u8);
    return vip_launch_status(what);
}

extern "C" int vip_tone_apply_rgb_u8_placed(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH,
                                            int dstMaxW, const uint8_t* lut_u8, int mode, int grid, int slots, int placement, int n,
                                            void* stream) {
    const char* what = "vip_tone_apply_rgb_u8";
    VIP_REQUIRE(maxH <= MAX_SIDE && maxW <= MAX_SIDE, VIP_ERR_BAD_ARG, "%s: bad size", what);
    Grid g;
    if (int st = check_slots(what, src_u8, sizes_hw, maxH, maxW, dst_u8, dstMaxH, dstMaxW, n, COUNT_BOTH, TILE_H, TILE_W * 3, &g)) return st;
    VIP_REQUIRE(lut_u8, VIP_ERR_BAD_ARG, "%s: null pointer", what);
    VIP_REQUIRE(mode >= VIP_TONE_AC && mode <= VIP_TONE_CLAHE, VIP_ERR_BAD_ARG, "%s: mode %d: expected 0 (ac), 1 (acl), 2 (eq) or 3 (clahe)", what,
                mode);
    VIP_REQUIRE(placement == 0 || placement == 1, VIP_ERR_BAD_ARG, "%s: placement %d: expected 0 (global gathers) or 1 (LDS copy)", what, placement);
    if (mode == VIP_TONE_CLAHE) {
        VIP_REQUIRE(grid >= 1 && grid <= MAX_GRID, VIP_ERR_BAD_ARG, "%s: grid %d: expected 1..%d", what, grid, MAX_GRID);
        VIP_REQUIRE(slots >= 1 && slots <= MAX_GRID * MAX_GRID, VIP_ERR_BAD_ARG, "%s: slots %d: expected 1..%d", what, slots, MAX_GRID * MAX_GRID);
    }
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(lut_u8) & 3) == 0, VIP_ERR_ALIGNMENT, "%s: tables must be 4-byte aligned", what);
    const dim3 grid_dim((unsigned)g.total), block_dim(THREADS);
    hipStream_t s = (hipStream_t)stream;
#define VIP_TONE_APPLY(KIND) \
    hipLaunchKernelGGL(tone_apply_kernel<KIND>, grid_dim, block_dim, 0, s, src_u8, sizes_hw, maxH, maxW, dst_u8, dstMaxH, dstMaxW, lut_u8, grid, slots, \
                       g.tiles_x, g.tiles_y)
    if (mode == VIP_TONE_AC || mode == VIP_TONE_EQ) VIP_TONE_APPLY(0);
    else if (mode == VIP_TONE_ACL) VIP_TONE_APPLY(1);
    else if (placement == 0) VIP_TONE_APPLY(2);
    else VIP_TONE_APPLY(3);
#undef VIP_TONE_APPLY
    return vip_launch_status(what);
}

// the CLAHE tables' placement that measured faster (README.md)
extern "C" int vip_tone_apply_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH,
                                     int dstMaxW, const uint8_t* lut_u8, int mode, int grid, int slots, int n, void* stream) {
    return vip_tone_apply_rgb_u8_placed(src_u8, sizes_hw, maxH, maxW, dst_u8, dstMaxH, dstMaxW, lut_u8, mode, grid, slots, 0, n, stream);
}
