// Occlusion sensitivity (main.py --occlusion): from the scores of the occluded variants to maps.  The variants themselves come from
// occlude_resize_norm_kernel (jpeg_pipeline.hip) and the ordinary member passes; what is left is a few KB of fp32 per batch
// (latency-bound) and one full-size map per image (store-bound).
//   variant (wy, wx) of an image hides the K x K cells at cell offset (wy, wx) of its G x G grid, W = G - K + 1 offsets per axis,
//   delta = p_plain - p_variant; a cell's value = the mean of delta over the windows that cover it.
#include "common.hpp"

namespace {

// One workgroup per (image i, row r).  Every cell is owned by one thread, which walks the windows covering it in variant order
// (row-major (wy, wx)) with a sequential fp32 sum and one correctly rounded division - vip_tile_aggregate_f32's rule: the result
// is a function of the values alone, whatever the launch shape.  Thread 0 also walks all variants once for the four statistics.
__global__ __launch_bounds__(256) void occlusion_cells_kernel(const float* __restrict__ scores, const float* __restrict__ plain,
                                                              const int* __restrict__ seg, float* __restrict__ cells,
                                                              float* __restrict__ stats, int n, int V, int G, int K, float thr) {
    const int i = blockIdx.x, r = blockIdx.y;
    const int W = G - K + 1;
    const int lo = seg[i], hi = seg[i + 1];
    float* cell = cells + ((long)r * n + i) * G * G;
    float* st = stats + ((long)r * n + i) * 4;
    if (lo < 0 || hi > V || hi - lo != W * W) {
        // no variants (an image smaller than the grid) - or a segment that is not a whole set of windows: nothing is read
        const float nan = __builtin_nanf("");
        for (int c = threadIdx.x; c < G * G; c += 256) cell[c] = nan;
        if (threadIdx.x < 4) st[threadIdx.x] = nan;
        return;
    }
    const float p = plain[(long)r * n + i];
    const float* s = scores + (long)r * V + lo;
    for (int c = threadIdx.x; c < G * G; c += 256) {
        const int gy = c / G, gx = c - gy * G;
        const int wy0 = gy - K + 1 < 0 ? 0 : gy - K + 1, wy1 = gy < W - 1 ? gy : W - 1;
        const int wx0 = gx - K + 1 < 0 ? 0 : gx - K + 1, wx1 = gx < W - 1 ? gx : W - 1;
        float acc = 0.f;
        for (int wy = wy0; wy <= wy1; ++wy)
            for (int wx = wx0; wx <= wx1; ++wx) acc = __fadd_rn(acc, __fsub_rn(p, s[wy * W + wx]));
        cell[c] = __fdiv_rn(acc, (float)((wy1 - wy0 + 1) * (wx1 - wx0 + 1)));
    }
    if (threadIdx.x == 0) {
        float mx = __fsub_rn(p, s[0]), mn = mx;
        int at = 0, flips = 0;
        const bool above = p > thr;
        for (int v = 0; v < W * W; ++v) {
            const float d = __fsub_rn(p, s[v]);
            if (d > mx) {
                mx = d;
                at = v;
            }
            mn = d < mn ? d : mn;
            flips += ((s[v] > thr) != above) ? 1 : 0;
        }
        st[0] = mx;
        st[1] = mn;
        st[2] = (float)at;
        st[3] = (float)flips;
    }
}

// the cell of pixel coordinate p along an axis of length L: the g with (g L) / G <= p < ((g + 1) L) / G
__device__ __forceinline__ int cell_of(int p, int L, int G) {
    int g = (int)(((long)p * G) / L);                  // (g L) / G <= p holds for this g; the next edge may too
    while (g + 1 < G && ((long)(g + 1) * L) / G <= p) ++g;
    return g;
}

// one thread = one pixel of the slot, grid.z = image.  Every pixel of the image takes its cell's value (cell edges = the occluder's
// edges); pixels of the slot outside the image are 0.  U8: round(255 (0.5 + 0.5 v / peak)), peak = max |cell| of the image, found by
// every workgroup from the image's G x G cells (at most 4 KB, cached); 128 everywhere when peak is 0 or a cell is NaN.
template <bool U8>
__global__ __launch_bounds__(256) void occlusion_map_kernel(const float* __restrict__ cells, const int* __restrict__ sizes,
                                                            void* __restrict__ out, int maxH, int maxW, int G) {
    __shared__ float red[256];
    __shared__ int bad[256];
    const int n = blockIdx.z;
    const float* cell = cells + (long)n * G * G;
    float peak = 0.f;
    if (U8) {
        float m = 0.f;
        int nan = 0;
        for (int c = threadIdx.x; c < G * G; c += 256) {
            const float v = cell[c];
            nan |= (v != v) ? 1 : 0;
            m = fmaxf(m, fabsf(v));
        }
        red[threadIdx.x] = m;
        bad[threadIdx.x] = nan;
        __syncthreads();
        for (int step = 128; step > 0; step >>= 1) {
            if ((int)threadIdx.x < step) {
                red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + step]);
                bad[threadIdx.x] |= bad[threadIdx.x + step];
            }
            __syncthreads();
        }
        peak = bad[0] ? 0.f : red[0];
    }
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= maxW || y >= maxH) return;
    const int h = sizes[2 * n], w = sizes[2 * n + 1];
    const long at = ((long)n * maxH + y) * maxW + x;
    const bool inside = y < h && x < w;
    float v = 0.f;
    if (inside && (!U8 || peak > 0.f)) v = cell[cell_of(y, h, G) * G + cell_of(x, w, G)];
    if (U8) {
        uint8_t q = 0;
        if (inside) q = peak > 0.f ? (uint8_t)rintf(255.f * (0.5f + 0.5f * (v / peak))) : (uint8_t)128;
        reinterpret_cast<uint8_t*>(out)[at] = q;
    } else {
        reinterpret_cast<float*>(out)[at] = v;
    }
}

}  // namespace

extern "C" int vip_occlusion_cells_f32(const float* scores, const float* plain, const int32_t* seg, int n, int rows, int V, int G, int K,
                                       float thr, float* cells, float* stats, void* stream) {
    VIP_REQUIRE(scores && plain && seg && cells && stats, VIP_ERR_BAD_ARG, "vip_occlusion_cells_f32: null pointer");
    VIP_REQUIRE(n > 0 && rows > 0 && rows <= 65535 && V > 0, VIP_ERR_BAD_ARG, "vip_occlusion_cells_f32: bad dimension");
    VIP_REQUIRE(G >= 2 && G <= 32 && K >= 1 && K <= G, VIP_ERR_BAD_ARG,
                "vip_occlusion_cells_f32: grid %d / window %d: expected 2 <= grid <= 32 and 1 <= window <= grid", G, K);
    hipLaunchKernelGGL(occlusion_cells_kernel, dim3(n, rows), dim3(256), 0, (hipStream_t)stream, scores, plain, seg, cells, stats, n, V,
                       G, K, thr);
    return vip_launch_status("vip_occlusion_cells_f32");
}

extern "C" int vip_occlusion_map(const float* cells_row, const int32_t* sizes_hw, int n, int maxH, int maxW, int G, void* out, int out_u8,
                                 void* stream) {
    VIP_REQUIRE(cells_row && sizes_hw && out, VIP_ERR_BAD_ARG, "vip_occlusion_map: null pointer");
    VIP_REQUIRE(n > 0 && n <= 65535 && maxH > 0 && maxW > 0, VIP_ERR_BAD_ARG, "vip_occlusion_map: bad size");
    VIP_REQUIRE(G >= 2 && G <= 32, VIP_ERR_BAD_ARG, "vip_occlusion_map: grid %d: expected 2..32", G);
    const dim3 grid((maxW + 63) / 64, (maxH + 3) / 4, n);
    if (out_u8)
        hipLaunchKernelGGL(occlusion_map_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, cells_row, sizes_hw, out, maxH, maxW, G);
    else
        hipLaunchKernelGGL(occlusion_map_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, cells_row, sizes_hw, out, maxH, maxW, G);
    return vip_launch_status("vip_occlusion_map");
}
