// Antialiased resampling of decoded u8 RGB pixels to a new size, the operation an image editor or an upload performs before it re-saves
// (the first half of the challenge's "resized and then JPEG-compressed"; pipeline.rescale, --stress-resize).  Not the network-input
// resize: vip_resize_bicubic_norm_* stays TensorFlow's non-antialiased bicubic with /255 folded in.
//
// Arithmetic, per image and channel, all in 32-bit integers with the tables of vip_resample_coeffs_h (22 fractional bits):
//   horizontal pass   u8 = clamp((2^21 + sum_j px[xmin + j] * k[x][j]) >> 22, 0, 255)       (arithmetic shift)
//   vertical pass     the same formula over the ROUNDED u8 rows of the horizontal pass
// a pass whose input and output sizes are equal is skipped.  This is Pillow's 8-bit Image.resize, bit for bit.
//
// One launch per batch.  A workgroup (4 waves) owns an output tile of one image, 16 rows x 256 BYTES of the interleaved RGB row (the
// vertical pass does not care where a pixel starts, so the tile is cut in bytes: one dword per lane, 64 lanes = 256 contiguous bytes).
// It resamples the input rows the tile's vertical window needs horizontally into LDS as u8 (one wave per row; a lane's four bytes and
// their bounds are fixed across rows), then runs the vertical pass from LDS (one wave per output row: bounds and coefficients are
// wave-uniform and come through the scalar path; the LDS reads are one dword per lane at consecutive addresses, conflict-free) and
// stores 256 contiguous bytes per wave.  Images of different sizes share the 1-D grid through a per-image tile prefix.
//
// LDS holds WINDOW_ROWS input rows of the tile.  A tile whose vertical window is taller (a strong shrink) is processed in groups of
// output rows whose window fits - the same kernel, the same arithmetic, no second launch and no intermediate in global memory.  Only a
// single output row whose own window exceeds WINDOW_ROWS cannot be held: the entry point refuses such a batch (VIP_ERR_UNSUPPORTED)
// instead of falling back; at 10 % Lanczos, the strongest shrink pipeline.rescale accepts, a row's window is at most 85 rows.
#include "rgb_tile.hpp"

namespace {

constexpr int TILE_ROWS = 16, TILE_BYTES = 256, WAVES = 4, WINDOW_ROWS = 160;      // LDS: 160 x 256 B = 40 KiB
constexpr int PRECISION_BITS = 22;

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// per-image record, 8 int32: first tile (prefix over the batch), tiles per tile row, then per axis the offsets of the bounds
// ([out][2]: first tap, tap count) and of the coefficients ([out][ksize]) in `tables`, and ksize; horizontal first
struct ImageTab {
    int tile0, tiles_x, hb, hk, hks, vb, vk, vks;
};

__global__ __launch_bounds__(WAVES * 64) void resample_rgb_u8_kernel(const uint8_t* __restrict__ src,
                                                                     const int32_t* __restrict__ src_sizes, int maxH, int maxW,
                                                                     uint8_t* __restrict__ dst,
                                                                     const int32_t* __restrict__ dst_sizes, int maxHo, int maxWo,
                                                                     const ImageTab* __restrict__ tab,
                                                                     const int32_t* __restrict__ tables, int n) {
    __shared__ uint32_t win[WINDOW_ROWS * (TILE_BYTES / 4)];
    // image of this tile: the last one whose first tile is <= blockIdx.x
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].tile0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const int img = lo;
    const ImageTab t = tab[img];
    const int h = src_sizes[img * 2], w = src_sizes[img * 2 + 1];
    const int ho = dst_sizes[img * 2], wo = dst_sizes[img * 2 + 1];
    if (h < 1 || w < 1 || ho < 1 || wo < 1 || h > maxH || w > maxW || ho > maxHo || wo > maxWo || t.tiles_x < 1) return;
    const int tile = (int)blockIdx.x - t.tile0;
    const int ty = tile / t.tiles_x, tx = tile - ty * t.tiles_x;
    const int row_bytes = wo * 3;
    const int b0 = tx * TILE_BYTES;
    const int y_begin = ty * TILE_ROWS, y_end = min(y_begin + TILE_ROWS, ho);
    if (b0 >= row_bytes || y_begin >= ho) return;
    const bool hpass = w != wo, vpass = h != ho;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int32_t* hbounds = tables + t.hb;
    const int32_t* hcoef = tables + t.hk;
    const int32_t* vbounds = tables + t.vb;
    const int32_t* vcoef = tables + t.vk;
    const uint8_t* simg = src + (long)img * maxH * maxW * 3;
    uint8_t* dimg = dst + (long)img * maxHo * maxWo * 3;

    // the lane's four bytes of the row: channel, first tap, tap count, coefficient row - the same for every input row
    int xoff[4], cnt[4], koff[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int b = b0 + lane * 4 + q;
        xoff[q] = cnt[q] = koff[q] = 0;
        if (b < row_bytes) {
            if (hpass) {
                const int x = b / 3, c = b - x * 3;
                int xmin = hbounds[x * 2], m = hbounds[x * 2 + 1];
                xmin = max(xmin, 0);                                   // a table never asks for more, the clamps keep every read inside the image
                m = max(min(min(m, t.hks), w - xmin), 0);
                xoff[q] = xmin * 3 + c;
                cnt[q] = m;
                koff[q] = x * t.hks;
            } else {
                xoff[q] = b;
                cnt[q] = -1;                                           // copy
            }
        }
    }

    for (int ya = y_begin; ya < y_end;) {
        // the group of output rows ya .. yb-1 whose input window win0 .. win0+rows-1 fits in LDS
        int win0, rows, yb;
        if (vpass) {
            win0 = min(max(vbounds[ya * 2], 0), h);
            rows = 0;
            for (yb = ya; yb < y_end; ++yb) {
                const int last = min(max(vbounds[yb * 2], 0) + min(vbounds[yb * 2 + 1], t.vks), h);
                if (last - win0 > WINDOW_ROWS) break;
                rows = max(rows, last - win0);
            }
            if (yb == ya) {                                            // a single row's window does not fit: refused by the entry point
                ya += 1;
                continue;
            }
        } else {
            win0 = ya;
            yb = y_end;
            rows = yb - ya;
        }
        // ---- horizontal pass: input rows win0 .. win0+rows-1 -> LDS, one wave per row ----
        for (int r = wave; r < rows; r += WAVES) {
            const uint8_t* srow = simg + (long)(win0 + r) * maxW * 3;
            uint32_t pack = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int v = 0;
                if (cnt[q] < 0) {
                    v = srow[xoff[q]];
                } else if (cnt[q] > 0) {
                    int acc = 1 << (PRECISION_BITS - 1);
                    const uint8_t* p = srow + xoff[q];
                    const int32_t* k = hcoef + koff[q];
                    for (int j = 0; j < cnt[q]; ++j) acc += (int)p[j * 3] * k[j];
                    v = clip8(acc);
                }
                pack |= (uint32_t)v << (8 * q);
            }
            win[r * (TILE_BYTES / 4) + lane] = pack;
        }
        __syncthreads();
        // ---- vertical pass from LDS: one wave per output row ----
        for (int y = ya + wave; y < yb; y += WAVES) {
            uint32_t pack;
            if (vpass) {
                const int ymin = min(max(vbounds[y * 2], 0), h);
                const int m = min(min(vbounds[y * 2 + 1], t.vks), h - ymin);
                const int32_t* k = vcoef + (long)y * t.vks;
                int a0, a1, a2, a3;
                a0 = a1 = a2 = a3 = 1 << (PRECISION_BITS - 1);
                const uint32_t* col = win + (ymin - win0) * (TILE_BYTES / 4) + lane;
                for (int j = 0; j < m; ++j) {
                    const uint32_t v = col[j * (TILE_BYTES / 4)];
                    const int kj = k[j];
                    a0 += (int)(v & 255) * kj;
                    a1 += (int)((v >> 8) & 255) * kj;
                    a2 += (int)((v >> 16) & 255) * kj;
                    a3 += (int)(v >> 24) * kj;
                }
                pack = (uint32_t)clip8(a0) | ((uint32_t)clip8(a1) << 8) | ((uint32_t)clip8(a2) << 16) | ((uint32_t)clip8(a3) << 24);
            } else {
                pack = win[(y - win0) * (TILE_BYTES / 4) + lane];
            }
            const int b = b0 + lane * 4;
            rgb_tile::store_pack(dimg + (long)y * maxWo * 3 + b, b, row_bytes, pack);
        }
        __syncthreads();
        ya = yb;
    }
}

}  // namespace

extern "C" int vip_resample_rgb_u8(const uint8_t* src_u8, const int32_t* src_sizes_hw, int maxH, int maxW, uint8_t* dst_u8,
                                   const int32_t* dst_sizes_hw, int maxHo, int maxWo, const int32_t* image_tab,
                                   const int32_t* tables, int n, int total_tiles, int max_window, void* stream) {
    VIP_REQUIRE(src_u8 && src_sizes_hw && dst_u8 && dst_sizes_hw && image_tab && tables, VIP_ERR_BAD_ARG,
                "vip_resample_rgb_u8: null pointer");
    VIP_REQUIRE(n > 0 && maxH > 0 && maxW > 0 && maxHo > 0 && maxWo > 0 && total_tiles > 0 && max_window > 0, VIP_ERR_BAD_ARG,
                "vip_resample_rgb_u8: bad size");
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(image_tab) & 3) == 0 && (reinterpret_cast<uintptr_t>(tables) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(src_sizes_hw) & 3) == 0 && (reinterpret_cast<uintptr_t>(dst_sizes_hw) & 3) == 0,
                VIP_ERR_ALIGNMENT, "vip_resample_rgb_u8: sizes, image_tab and tables must be 4-byte aligned");
    VIP_REQUIRE(max_window <= WINDOW_ROWS, VIP_ERR_UNSUPPORTED,
                "vip_resample_rgb_u8: a vertical window of %d input rows per output row exceeds the %d rows held on chip", max_window,
                WINDOW_ROWS);
    hipLaunchKernelGGL(resample_rgb_u8_kernel, dim3(total_tiles), dim3(WAVES * 64), 0, (hipStream_t)stream, src_u8, src_sizes_hw, maxH,
                       maxW, dst_u8, dst_sizes_hw, maxHo, maxWo, reinterpret_cast<const ImageTab*>(image_tab), tables, n);
    return vip_launch_status("vip_resample_rgb_u8");
}

extern "C" int vip_resample_tile_shape(int* rows_h, int* bytes_h, int* window_rows_h) {
    VIP_REQUIRE(rows_h && bytes_h && window_rows_h, VIP_ERR_BAD_ARG, "vip_resample_tile_shape: null pointer");
    *rows_h = TILE_ROWS;
    *bytes_h = TILE_BYTES;
    *window_rows_h = WINDOW_ROWS;
    return VIP_OK;
}
