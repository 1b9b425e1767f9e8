// GPU half of the lossless WebP path: the still-transformed 32-bit ARGB words and the transforms' data (webp_host.cpp)
//   -> undo the transforms in the reverse of the order read -> 8-bit RGB, alpha dropped  [== libwebp's VP8L decoder].
//
// One wave per image.  Every transform works in place in the device copy of the words, at the width recorded when it was
// read; the one that comes last writes the RGB output instead (colour indexing reads packed pixels and writes RGB, so
// it never widens in place when it is last).  Subtract-green, cross-colour and colour indexing are point-wise: the 64
// lanes stride over the pixels, or - cross-colour and subtract-green next to a predictor - they are applied where the
// predictor stages its residuals or stores its results, and take no pass of their own.
//
// The spatial predictor of pixel (y, x) depends on L (y, x-1), T (y-1, x), TL (y-1, x-1) and TR (y-1, x+1).  Mapping: the
// rows go in bands of 64, lane l owns row l of the band and handles column t - 2 l at step t - the PNG kernel's skewed
// wavefront with a skew of two columns.  At that step lane l - 1 finished column x + 1 one step earlier: TR is this step's
// one-lane shuffle of the neighbour's last pixel, T and TL are the two values received before it, L stays in the lane's
// registers.  A band costs xsize + 2 (rows - 1) steps whatever the modes.  Residuals and results are staged through LDS
// in chunks of CW steps: row i of a chunk holds columns t0 - 2 i .. t0 - 2 i + CW - 1 (a parallelogram, so the wavefront
// runs on across chunks), loaded and stored as coalesced words.  The first row of a band takes T, TL and TR from the
// previous band's last row, which is back in the word stream by then.
#include "common.hpp"

namespace {

constexpr int BAND = 64;             // rows per band = lanes of the wave
constexpr int CW = 128;              // steps (= columns per row) per chunk
constexpr int TS = CW + 1;           // tile row stride in words: odd, so the lanes of a step hit distinct LDS banks
constexpr int MB = CW / 4 + 4;       // mode bytes per tile row: the blocks (>= 4 pixels wide) a row's chunk can touch
constexpr uint32_t BLACK = 0xff000000u;

__device__ __forceinline__ uint32_t add_px(uint32_t a, uint32_t b) {       // per channel, mod 256
    return (((a & 0xff00ff00u) + (b & 0xff00ff00u)) & 0xff00ff00u) | (((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu);
}
__device__ __forceinline__ uint32_t avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }
__device__ __forceinline__ int ch(uint32_t v, int s) { return (int)((v >> s) & 255u); }
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

__device__ __forceinline__ uint32_t select_px(uint32_t T, uint32_t L, uint32_t TL) {
    int d = 0;                                           // sum over A, R, G, B of |L - TL| - |T - TL|
#pragma unroll
    for (int s = 0; s < 32; s += 8) d += abs(ch(L, s) - ch(TL, s)) - abs(ch(T, s) - ch(TL, s));
    return d <= 0 ? T : L;
}
__device__ __forceinline__ uint32_t clamp_add_sub(uint32_t L, uint32_t T, uint32_t TL) {
    uint32_t r = 0;
#pragma unroll
    for (int s = 0; s < 32; s += 8) r |= (uint32_t)clamp255(ch(L, s) + ch(T, s) - ch(TL, s)) << s;
    return r;
}
__device__ __forceinline__ uint32_t clamp_add_sub_half(uint32_t a, uint32_t TL) {
    uint32_t r = 0;
#pragma unroll
    for (int s = 0; s < 32; s += 8) {
        const int c = ch(a, s);
        r |= (uint32_t)clamp255(c + (c - ch(TL, s)) / 2) << s;      // C division: towards zero
    }
    return r;
}

__device__ __forceinline__ uint32_t predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
    switch (mode) {
        case 1: return L;
        case 2: return T;
        case 3: return TR;
        case 4: return TL;
        case 5: return avg2(avg2(L, TR), T);
        case 6: return avg2(L, TL);
        case 7: return avg2(L, T);
        case 8: return avg2(TL, T);
        case 9: return avg2(T, TR);
        case 10: return avg2(avg2(L, TL), avg2(T, TR));
        case 11: return select_px(T, L, TL);
        case 12: return clamp_add_sub(L, T, TL);
        case 13: return clamp_add_sub_half(avg2(L, T), TL);
        default: return BLACK;                           // 0, and 14 / 15 (which libwebp maps to 0)
    }
}

__device__ __forceinline__ void store_rgb(uint8_t* rgb, int maxH, int maxW, int y, int x, uint32_t px) {
    if (y >= maxH || x >= maxW) return;
    uint8_t* p = rgb + ((int64_t)y * maxW + x) * 3;
    p[0] = (uint8_t)(px >> 16);
    p[1] = (uint8_t)(px >> 8);
    p[2] = (uint8_t)px;
}

__device__ __forceinline__ uint32_t cross_colour_px(uint32_t px, uint32_t m) {
    const int g2r = (int8_t)(m & 255u), g2b = (int8_t)((m >> 8) & 255u), r2b = (int8_t)((m >> 16) & 255u);
    const int g = (int8_t)((px >> 8) & 255u);
    int r = (int)((px >> 16) & 255u), b = (int)(px & 255u);
    r = (r + ((g2r * g) >> 5)) & 255;
    b = (b + ((g2b * g) >> 5)) & 255;
    b = (b + ((r2b * (int)(int8_t)r) >> 5)) & 255;
    return (px & 0xff00ff00u) | ((uint32_t)r << 16) | (uint32_t)b;
}

__device__ __forceinline__ uint32_t add_green_px(uint32_t px) {
    const uint32_t g = (px >> 8) & 255u;
    return (px & 0xff00ff00u) | (((px & 0x00ff00ffu) + ((g << 16) | g)) & 0x00ff00ffu);
}

// transforms hi, hi - 1, .. lo of the image (all cross-colour or subtract-green, all at the same width) on one pixel
__device__ __forceinline__ uint32_t apply_pointwise(uint32_t px, int y, int x, const vip_webp_desc& D, const uint8_t* base,
                                                    int hi, int lo) {
    for (int k = hi; k >= lo; --k) {
        if (D.type[k] == VIP_WEBP_SUBTRACT_GREEN) {
            px = add_green_px(px);
        } else {
            const int bits = D.bits[k], sw = (D.xsize[k] + (1 << bits) - 1) >> bits;
            px = cross_colour_px(px, ((const uint32_t*)(base + D.data_off[k]))[(int64_t)(y >> bits) * sw + (x >> bits)]);
        }
    }
    return px;
}

// Undo the predictor transform in place on argb[h][xs]; sub = its sub-image (mode in bits 8..11).  The point-wise
// transforms pre_hi .. pre_lo (those undone before the predictor) are applied while the residuals are staged, and with
// rgb != null the transforms post_hi .. post_lo (those undone after it) on the way to the RGB output: the common orders
// take no pass of their own.  An empty range has hi < lo.
__device__ void inverse_predictor(uint32_t* argb, int xs, int h, const uint32_t* sub, int bits, uint8_t* rgb, int maxH,
                                  int maxW, uint32_t* tile, uint32_t* up, uint8_t* modes, const vip_webp_desc& D,
                                  const uint8_t* base, int pre_hi, int pre_lo, int post_hi, int post_lo) {
    const int lane = threadIdx.x;
    const int sw = (xs + (1 << bits) - 1) >> bits;
    for (int r0 = 0; r0 < h; r0 += BAND) {
        const int nr = min(BAND, h - r0);
        const int steps = xs + 2 * (nr - 1);
        uint32_t cur = 0, r1 = 0, r2 = 0, first = 0;     // last result (= L); the values received one and two steps ago
        for (int t0 = 0; t0 < steps; t0 += CW) {
            // stage the chunk: row i holds columns t0 - 2 i + k, k = 0 .. CW-1
#pragma unroll 4
            for (int idx = lane; idx < nr * CW; idx += 64) {
                const int i = idx / CW, k = idx - i * CW;
                const int x = t0 - 2 * i + k;
                if (x >= 0 && x < xs) tile[i * TS + k] = apply_pointwise(argb[(int64_t)(r0 + i) * xs + x], r0 + i, x, D, base, pre_hi, pre_lo);
            }
            for (int idx = lane; idx < nr * MB; idx += 64) {
                const int i = idx / MB, k = idx - i * MB;
                const int bx = (max(t0 - 2 * i, 0) >> bits) + k;
                modes[idx] = bx < sw ? (uint8_t)((sub[(int64_t)((r0 + i) >> bits) * sw + bx] >> 8) & 15u) : 0;
            }
            if (r0 > 0) {                                // columns t0 - 1 .. t0 + CW of the previous band's last row
                for (int k = lane; k < CW + 2; k += 64) {
                    const int x = t0 - 1 + k;
                    up[k] = (x >= 0 && x < xs) ? argb[(int64_t)(r0 - 1) * xs + x] : 0;
                }
            }
            __syncthreads();
            const int bx0 = max(t0 - 2 * lane, 0) >> bits;
            const int tend = min(CW, steps - t0);
            for (int k = 0; k < tend; ++k) {
                const uint32_t recv = __shfl_up(cur, 1, 64);       // lane - 1 finished column x + 1 at the previous step
                const int x = t0 + k - 2 * lane;
                if (lane < nr && x >= 0 && x < xs) {
                    uint32_t T = r1, TL = r2, TR = recv;
                    if (lane == 0 && r0 > 0) {
                        TL = up[k];
                        T = up[k + 1];
                        TR = up[k + 2];
                    }
                    if (x == xs - 1) TR = first;         // libwebp reads top[x + 1]: the first pixel of the current row
                    uint32_t pred;
                    if (r0 + lane == 0) {
                        pred = x == 0 ? BLACK : cur;
                    } else if (x == 0) {
                        pred = T;
                    } else {
                        pred = predict(modes[lane * MB + (x >> bits) - bx0], cur, T, TL, TR);
                    }
                    cur = add_px(tile[lane * TS + k], pred);
                    tile[lane * TS + k] = cur;
                    if (x == 0) first = cur;
                }
                r2 = r1;
                r1 = recv;
            }
            __syncthreads();
            for (int idx = lane; idx < nr * CW; idx += 64) {
                const int i = idx / CW, k = idx - i * CW;
                const int x = t0 - 2 * i + k;
                if (x >= 0 && x < xs) {
                    const uint32_t px = tile[i * TS + k];
                    if (!rgb || i == nr - 1) argb[(int64_t)(r0 + i) * xs + x] = px;      // the next band's T row, or the next pass
                    if (rgb) store_rgb(rgb, maxH, maxW, r0 + i, x, apply_pointwise(px, r0 + i, x, D, base, post_hi, post_lo));
                }
            }
            __syncthreads();
        }
    }
}

// the point-wise transforms that keep the width: in place, or to RGB when last
__device__ void inverse_pointwise(int type, uint32_t* argb, int xs, int h, const uint32_t* data, int bits, uint8_t* rgb,
                                  int maxH, int maxW) {
    constexpr int U = 4;
    const int sw = (xs + (1 << bits) - 1) >> bits;
    const int64_t total = (int64_t)xs * h;
    for (int64_t i0 = threadIdx.x; i0 < total; i0 += 64 * U) {
        uint32_t px[U];                                   // U loads in flight: the stores below may alias, the compiler cannot
#pragma unroll
        for (int u = 0; u < U; ++u) px[u] = i0 + 64 * u < total ? argb[i0 + 64 * u] : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t idx = i0 + 64 * u;
            if (idx >= total) break;
            const int y = (int)(idx / xs), x = (int)(idx - (int64_t)y * xs);
            uint32_t v = px[u];
            if (type == VIP_WEBP_SUBTRACT_GREEN) v = add_green_px(v);
            else if (type == VIP_WEBP_CROSS_COLOR) v = cross_colour_px(v, data[(int64_t)(y >> bits) * sw + (x >> bits)]);
            else if (type == VIP_WEBP_COLOR_INDEXING) v = data[(v >> 8) & 255u];     // bits == 0 here: one index per coded pixel
            if (rgb) store_rgb(rgb, maxH, maxW, y, x, v);
            else argb[idx] = v;
        }
    }
}

// colour indexing with 2, 4 or 8 pixels per coded pixel: argb[h][cw] -> w pixels per row.  To RGB when last; otherwise
// widened in place, rows from the bottom and 64 pixels at a time from the right, so that nothing is overwritten before
// it is read (row y's pixels x >= x0 start at word y w + x0 >= y cw + (x0 >> bits), past every packed word still unread).
__device__ void inverse_indexing_packed(uint32_t* argb, int cw, int w, int h, const uint32_t* pal, int bits, uint8_t* rgb,
                                        int maxH, int maxW) {
    const int per = 1 << bits, width_bits = 8 >> bits;
    const uint32_t mask = (1u << width_bits) - 1u;
    if (rgb) {
        constexpr int U = 4;
        const int64_t total = (int64_t)w * h;
        for (int64_t i0 = threadIdx.x; i0 < total; i0 += 64 * U) {
            uint32_t g[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t idx = i0 + 64 * u < total ? i0 + 64 * u : total - 1;
                const int y = (int)(idx / w), x = (int)(idx - (int64_t)y * w);
                g[u] = pal[(((argb[(int64_t)y * cw + (x >> bits)] >> 8) & 255u) >> ((x & (per - 1)) * width_bits)) & mask];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t idx = i0 + 64 * u;
                if (idx >= total) break;
                const int y = (int)(idx / w);
                store_rgb(rgb, maxH, maxW, y, (int)(idx - (int64_t)y * w), g[u]);
            }
        }
        return;
    }
    for (int y = h - 1; y >= 0; --y) {
        for (int x0 = ((w - 1) / 64) * 64; x0 >= 0; x0 -= 64) {
            const int x = x0 + (int)threadIdx.x;
            uint32_t px = 0;
            if (x < w) {
                const uint32_t g = (argb[(int64_t)y * cw + (x >> bits)] >> 8) & 255u;
                px = pal[(g >> ((x & (per - 1)) * width_bits)) & mask];
            }
            __syncthreads();
            if (x < w) argb[(int64_t)y * w + x] = px;
            __syncthreads();
        }
    }
}

// grid (n): one wave per image
__global__ __launch_bounds__(64) void webp_inverse_kernel(uint8_t* stream, const vip_webp_desc* __restrict__ desc, uint8_t* rgb,
                                                           int maxH, int maxW) {
    __shared__ uint32_t tile[BAND * TS];
    __shared__ uint32_t up[CW + 2];
    __shared__ uint8_t modes[BAND * MB];
    const vip_webp_desc& D = desc[blockIdx.x];
    const int w = D.width, h = D.height;
    if (w <= 0 || h <= 0) return;
    uint8_t* base = stream + D.stream_off;
    uint32_t* argb = (uint32_t*)(base + D.argb_off);
    uint8_t* img = rgb + (int64_t)blockIdx.x * maxH * maxW * 3;
    const int nt = D.n_transforms;
    if (nt == 0) {
        const int64_t total = (int64_t)w * h;
#pragma unroll 4
        for (int64_t idx = threadIdx.x; idx < total; idx += 64) {
            const int y = (int)(idx / w);
            store_rgb(img, maxH, maxW, y, (int)(idx - (int64_t)y * w), argb[idx]);
        }
        return;
    }
    // cross-colour and subtract-green next to the predictor ride along with it (all of one side, or that side runs as passes)
    int kp = -1;
    for (int k = 0; k < nt; ++k)
        if (D.type[k] == VIP_WEBP_PREDICTOR) kp = k;
    bool fuse_pre = kp >= 0, fuse_post = kp >= 0;
    for (int k = 0; k < nt; ++k) {
        const bool rides = D.type[k] == VIP_WEBP_CROSS_COLOR || D.type[k] == VIP_WEBP_SUBTRACT_GREEN;
        if (k > kp && !rides) fuse_pre = false;
        if (k < kp && !rides) fuse_post = false;
    }
    for (int k = nt - 1; k >= 0; --k) {
        if ((fuse_pre && k > kp) || (fuse_post && k < kp)) continue;
        const int type = D.type[k], bits = D.bits[k], xs = D.xsize[k];
        const uint32_t* data = (const uint32_t*)(base + D.data_off[k]);
        uint8_t* out = (k == 0 || (k == kp && fuse_post)) ? img : nullptr;
        if (type == VIP_WEBP_PREDICTOR) {
            inverse_predictor(argb, xs, h, data, bits, out, maxH, maxW, tile, up, modes, D, base, fuse_pre ? nt - 1 : -1,
                              fuse_pre ? kp + 1 : 0, fuse_post ? kp - 1 : -1, 0);
        } else if (type == VIP_WEBP_COLOR_INDEXING && bits > 0) {
            inverse_indexing_packed(argb, (xs + (1 << bits) - 1) >> bits, xs, h, data, bits, out, maxH, maxW);
        } else {
            inverse_pointwise(type, argb, xs, h, data, bits, out, maxH, maxW);
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int vip_webp_inverse_rgb_u8(uint8_t* words, const vip_webp_desc* desc, int n, uint8_t* rgb_u8, int maxH, int maxW,
                                       void* stream) {
    VIP_REQUIRE(words && desc && rgb_u8, VIP_ERR_BAD_ARG, "vip_webp_inverse_rgb_u8: null pointer");
    VIP_REQUIRE(n > 0 && maxH > 0 && maxW > 0, VIP_ERR_BAD_ARG, "vip_webp_inverse_rgb_u8: bad size");
    VIP_REQUIRE(((uintptr_t)words & 3) == 0, VIP_ERR_ALIGNMENT, "vip_webp_inverse_rgb_u8: words not 4-byte aligned");
    hipLaunchKernelGGL(webp_inverse_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, words, desc, rgb_u8, maxH, maxW);
    return vip_launch_status("vip_webp_inverse_rgb_u8");
}
