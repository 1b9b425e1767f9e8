// GPU half of the PNG path (dataset/dataset.py:22-30, tf.image.decode_png(channels=3)):
//   still-filtered scanlines (png_host.cpp) -> undo the None / Sub / Up / Average / Paeth filters -> 8-bit RGB
//   [== libpng with gray 1/2/4 -> 8 expansion, palette -> RGB, alpha stripped, 16 -> 8 by png_set_scale_16, gray -> RGB].
//
// Byte x of row r depends on byte x - bpp of row r and on bytes x and x - bpp of row r - 1, so neither a row per lane
// nor a byte per lane runs in parallel.  Mapping: one wave per (image, Adam7 pass); the rows go in bands of 64, lane l
// owns row l of the band and handles filter unit j (bpp bytes) at step j + l - a skewed wavefront.  At that step lane
// l - 1 finished unit j one step earlier: `up` comes from it by a one-lane shuffle, `upper-left` is the `up` this lane
// received one step earlier, `left` stays in the lane's registers.  A band costs (units + 63) steps whatever the filter
// types.  The band's filtered bytes are staged in LDS in column chunks of TILE_BYTES per row (coalesced loads), the
// unfiltered bytes go back to the tile, and the chunk is expanded to RGB from there.  The first row of a band takes its
// `up` row from the previous band's last row, which is written back in place to the (device) scanline stream.
#include "common.hpp"

namespace {

constexpr int BAND = 64;             // rows per band = lanes of the wave
constexpr int TILE_BYTES = 960;      // filtered bytes per row and chunk: a whole number of units for bpp 1, 2, 3, 4, 6, 8

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// one 8-bit RGB pixel from the unfiltered bytes of its row (row = the tile row, x = pixel index inside the chunk)
__device__ __forceinline__ void expand_pixel(const uint8_t* row, int x, int depth, int color_type, int channels,
                                             const vip_png_desc& D, int palette_size, uint8_t out[3]) {
    if (depth < 8) {                                     // gray or palette, 8 / depth pixels per byte, first pixel in the MSBs
        const int ppb = 8 / depth;
        const int v = (row[x / ppb] >> (8 - depth * (x % ppb + 1))) & ((1 << depth) - 1);
        if (color_type == 3) {
            const bool in = v < palette_size;           // an index past PLTE is black (never read past the table)
            out[0] = in ? D.palette[v][0] : 0;
            out[1] = in ? D.palette[v][1] : 0;
            out[2] = in ? D.palette[v][2] : 0;
        } else {
            const int g = v * (depth == 1 ? 255 : depth == 2 ? 85 : 17);   // bit replication
            out[0] = out[1] = out[2] = (uint8_t)g;
        }
        return;
    }
    const int bps = depth / 8;                           // bytes per sample
    const uint8_t* px = row + x * channels * bps;
    int s[3];
    const int nc = channels >= 3 ? 3 : 1;               // gray / gray+alpha: one colour sample; RGB / RGBA: three
    for (int c = 0; c < nc; ++c) {
        if (bps == 2) {
            const int v = (px[2 * c] << 8) | px[2 * c + 1];
            s[c] = (2 * v + 257) / 514;                  // round(v / 257): png_set_scale_16 (no ties: 257 is odd)
        } else {
            s[c] = px[c];
        }
    }
    if (color_type == 3) {
        const int v = s[0];
        const bool in = v < palette_size;
        out[0] = in ? D.palette[v][0] : 0;
        out[1] = in ? D.palette[v][1] : 0;
        out[2] = in ? D.palette[v][2] : 0;
    } else if (nc == 1) {
        out[0] = out[1] = out[2] = (uint8_t)s[0];
    } else {
        out[0] = (uint8_t)s[0];
        out[1] = (uint8_t)s[1];
        out[2] = (uint8_t)s[2];
    }
}

template <int BPP>
__device__ void unfilter_pass(uint8_t* s, int64_t stride, int pw, int ph, int units, const vip_png_desc& D, int pass,
                              uint8_t* rgb, int maxH, int maxW, uint8_t* tile, uint8_t* uprow) {
    constexpr int W = (BPP + 3) / 4;                     // 32-bit words per unit
    constexpr int CU = TILE_BYTES / BPP;                 // units per chunk
    const int lane = threadIdx.x;
    const int depth = D.bit_depth, color_type = D.color_type, channels = D.channels, palette_size = D.palette_size;
    const int H = D.height, Wd = D.width;
    // Adam7 first column / row and step of pass p, one hex digit per pass (pass 0 in the lowest): 0 4 0 2 0 1 0 etc.
    const int sh = 4 * pass;
    const int x0 = D.interlace ? (0x0102040 >> sh) & 15 : 0, y0 = D.interlace ? (0x1020400 >> sh) & 15 : 0;
    const int dx = D.interlace ? (0x1224488 >> sh) & 15 : 1, dy = D.interlace ? (0x2244888 >> sh) & 15 : 1;
    const int ppu = depth < 8 ? 8 / depth : 1;           // pixels per unit
    for (int r0 = 0; r0 < ph; r0 += BAND) {
        const int nr = min(BAND, ph - r0);
        const int ft = lane < nr ? s[(int64_t)(r0 + lane) * stride] : 0;
        uint32_t cur[W];                                 // the lane's last unfiltered unit (= `left` of the next one)
        uint32_t up_prev[W];                             // the `up` received one step earlier (= `upper-left`)
#pragma unroll
        for (int w = 0; w < W; ++w) cur[w] = up_prev[w] = 0;
        for (int c0 = 0; c0 < units; c0 += CU) {
            const int cu = min(CU, units - c0);
            const int cb = cu * BPP;
            // stage the chunk: rows r0 .. r0+nr-1, bytes [1 + c0*BPP, + cb) of each, in aligned 4-byte words
            {
                const int64_t seg = 1 + (int64_t)c0 * BPP;
                const int nd = cb / 4 + 2;               // words that can hold a segment of cb bytes at any alignment
                for (int idx = lane; idx < nr * nd; idx += 64) {
                    const int i = idx / nd, k = idx - i * nd;
                    const uint8_t* a = s + (int64_t)(r0 + i) * stride + seg;
                    const uintptr_t a0 = (uintptr_t)a & ~(uintptr_t)3;
                    const int b0 = (int)((intptr_t)(a0 + 4 * k) - (intptr_t)a);   // tile column of the word's first byte
                    if (b0 >= cb) continue;
                    const uint32_t v = *(const uint32_t*)(a0 + 4 * k);
                    uint8_t* t = tile + i * TILE_BYTES;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (b0 + q >= 0 && b0 + q < cb) t[b0 + q] = (uint8_t)(v >> (8 * q));
                }
                // `up` row for the band's first row: unit c0-1 .. c0+cu-1 of row r0-1 (already unfiltered), zeros at the edges
                for (int b = lane; b < cb + BPP; b += 64) {
                    const int col = c0 * BPP - BPP + b;   // byte of the row (without its filter byte)
                    uprow[b] = (r0 > 0 && col >= 0) ? s[(int64_t)(r0 - 1) * stride + 1 + col] : 0;
                }
            }
            __syncthreads();
            uint8_t* my = tile + lane * TILE_BYTES;
            const int steps = cu + nr - 1;
            for (int t = 0; t < steps; ++t) {
                uint32_t up[W], ul[W];
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    up[w] = __shfl_up(cur[w], 1, 64);   // lane-1 finished this unit at the previous step
                    ul[w] = up_prev[w];
                    up_prev[w] = up[w];
                }
                const int j = t - lane;
                if (lane < nr && j >= 0 && j < cu) {
                    if (lane == 0) {                     // first row of the band: the previous band's last row
#pragma unroll
                        for (int w = 0; w < W; ++w) up[w] = ul[w] = 0;
#pragma unroll
                        for (int k = 0; k < BPP; ++k) {
                            up[k / 4] |= (uint32_t)uprow[(j + 1) * BPP + k] << (8 * (k % 4));
                            ul[k / 4] |= (uint32_t)uprow[j * BPP + k] << (8 * (k % 4));
                        }
                    }
                    uint32_t nw[W];
#pragma unroll
                    for (int w = 0; w < W; ++w) nw[w] = 0;
#pragma unroll
                    for (int k = 0; k < BPP; ++k) {
                        const int bs = 8 * (k % 4);
                        const int a = (cur[k / 4] >> bs) & 255, b = (up[k / 4] >> bs) & 255, c = (ul[k / 4] >> bs) & 255;
                        const int raw = my[j * BPP + k];
                        const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth(a, b, c) : 0;
                        const uint32_t x = (uint32_t)((raw + pred) & 255);
                        my[j * BPP + k] = (uint8_t)x;
                        nw[k / 4] |= x << bs;
                    }
#pragma unroll
                    for (int w = 0; w < W; ++w) cur[w] = nw[w];
                }
            }
            __syncthreads();
            // the band's last row goes back to the stream: the `up` row of the next band
            if (r0 + nr < ph) {
                uint8_t* dst = s + (int64_t)(r0 + nr - 1) * stride + 1 + (int64_t)c0 * BPP;
                for (int b = lane; b < cb; b += 64) dst[b] = tile[(nr - 1) * TILE_BYTES + b];
            }
            // expand the chunk's pixels and scatter them to their image positions
            const int px0 = c0 * ppu;
            const int npx = min(cu * ppu, pw - px0);
            for (int idx = lane; idx < nr * npx; idx += 64) {
                const int i = idx / npx, x = idx - i * npx;
                const int oy = y0 + (r0 + i) * dy, ox = x0 + (px0 + x) * dx;
                if (oy >= H || ox >= Wd || oy >= maxH || ox >= maxW) continue;
                uint8_t o[3];
                expand_pixel(tile + i * TILE_BYTES, x, depth, color_type, channels, D, palette_size, o);
                uint8_t* p = rgb + ((int64_t)oy * maxW + ox) * 3;
                p[0] = o[0];
                p[1] = o[1];
                p[2] = o[2];
            }
            __syncthreads();
        }
    }
}

// grid (n, 7): x = image, y = Adam7 pass (pass 0 only for a non-interlaced image); one wave per workgroup
__global__ __launch_bounds__(64) void png_unfilter_kernel(uint8_t* stream, const vip_png_desc* __restrict__ desc,
                                                           uint8_t* rgb, int maxH, int maxW) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[BAND * TILE_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t uprow[TILE_BYTES + 8];
    const vip_png_desc& D = desc[blockIdx.x];
    const int pass = blockIdx.y;
    const int pw = D.pass_w[pass], ph = D.pass_h[pass];
    if (pw <= 0 || ph <= 0) return;
    const int64_t rowbytes = ((int64_t)pw * D.channels * D.bit_depth + 7) / 8;
    const int units = (int)(rowbytes / D.bpp);
    uint8_t* s = stream + D.stream_off + D.pass_off[pass];
    uint8_t* img = rgb + (int64_t)blockIdx.x * maxH * maxW * 3;
    switch (D.bpp) {
        case 1: unfilter_pass<1>(s, rowbytes + 1, pw, ph, units, D, pass, img, maxH, maxW, tile, uprow); break;
        case 2: unfilter_pass<2>(s, rowbytes + 1, pw, ph, units, D, pass, img, maxH, maxW, tile, uprow); break;
        case 3: unfilter_pass<3>(s, rowbytes + 1, pw, ph, units, D, pass, img, maxH, maxW, tile, uprow); break;
        case 4: unfilter_pass<4>(s, rowbytes + 1, pw, ph, units, D, pass, img, maxH, maxW, tile, uprow); break;
        case 6: unfilter_pass<6>(s, rowbytes + 1, pw, ph, units, D, pass, img, maxH, maxW, tile, uprow); break;
        case 8: unfilter_pass<8>(s, rowbytes + 1, pw, ph, units, D, pass, img, maxH, maxW, tile, uprow); break;
        default: break;                                  // not a legal PNG: png_host.cpp refuses it
    }
}

}  // namespace

extern "C" int vip_png_unfilter_rgb_u8(uint8_t* filtered, const vip_png_desc* desc, int n, uint8_t* rgb_u8, int maxH, int maxW,
                                       void* stream) {
    VIP_REQUIRE(filtered && desc && rgb_u8, VIP_ERR_BAD_ARG, "vip_png_unfilter_rgb_u8: null pointer");
    VIP_REQUIRE(n > 0 && maxH > 0 && maxW > 0, VIP_ERR_BAD_ARG, "vip_png_unfilter_rgb_u8: bad size");
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(n, 7), dim3(64), 0, (hipStream_t)stream, filtered, desc, rgb_u8, maxH, maxW);
    return vip_launch_status("vip_png_unfilter_rgb_u8");
}
