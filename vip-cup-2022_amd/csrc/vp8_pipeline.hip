// GPU half of the lossy WebP path: macroblock records + dequantised coefficients (vp8_host.cpp)
//   -> intra prediction + inverse WHT / DCT -> in-loop filter -> fancy chroma upsampling -> 8-bit RGB  [== libwebp's VP8 decoder].
// The arithmetic is in vp8_recon.hpp; this file owns the order.
//
// Reconstruction and filter, vp8_recon_filter_kernel: one workgroup of four waves per image, the image's Y / U / V planes
// in the scratch buffer (they stay in L2; a workgroup is alone on its planes, so a workgroup barrier orders its accesses).
// Macroblock (x, y) predicts from (x-1, y), (x, y-1), (x-1, y-1) and (x+1, y-1): all macroblocks with the same x + 2 y
// are independent, so the image is walked in steps t = x + 2 y, the VP8L predictor's skew of two, and the macroblocks of
// a step go to the four waves, one each, in rounds.  A wave spreads a macroblock as 96 items of four pixels (24 blocks
// x 4 rows): prediction and the block row's inverse DCT in one lane, no exchange between lanes.  A macroblock with
// sub-block modes walks its 16 sub-blocks in the same way one level down, ten sub-steps bx + 2 by of at most two
// sub-blocks, a barrier after each; the round's waves take those barriers together (and skip all ten when no macroblock
// of the round has sub-block modes).  Prediction reads unfiltered pixels, so the filter is a second walk in the same
// order once the whole image stands: per macroblock 32 lanes each filter one row (left edge, then the inner vertical
// edges - the rows are independent), barrier, 32 lanes one column each (top edge, inner horizontal edges), barrier.
//
// Output, vp8_rgb_kernel: point-wise, one thread per pixel over the whole batch.
#include "common.hpp"
#include "vp8_recon.hpp"
#include "vp8_walk.hpp"

namespace {

// grid (n), block (64 NW)
__global__ __launch_bounds__(64 * NW) void vp8_recon_filter_kernel(const uint8_t* stream, size_t stream_bytes, const vip_vp8_desc* desc,
                                                                   uint8_t* scratch, size_t scratch_bytes, int stages) {
    const vip_vp8_desc D = desc[blockIdx.x];
    const int mb_w = D.mb_w, mb_h = D.mb_h;
    if (D.width <= 0 || D.height <= 0 || mb_w != (D.width + 15) >> 4 || mb_h != (D.height + 15) >> 4) return;
    const size_t nmb = (size_t)mb_w * mb_h;
    // what the host wrote is trusted, but not beyond the buffers (uniform over the workgroup)
    if (D.stream_off < 0 || D.mb_off < 0 || D.coef_off < 0 || D.coef_blocks < 0 || D.plane_off < 0) return;
    if ((size_t)D.stream_off > stream_bytes || (size_t)D.mb_off > stream_bytes || (size_t)D.coef_off > stream_bytes) return;
    if ((size_t)D.stream_off + (size_t)D.mb_off + nmb * sizeof(vip_vp8_mb) > stream_bytes) return;
    if ((size_t)D.coef_blocks > stream_bytes / 32 || (size_t)D.stream_off + (size_t)D.coef_off + (size_t)D.coef_blocks * 32 > stream_bytes) return;
    if ((size_t)D.plane_off > scratch_bytes || (size_t)D.plane_off + nmb * 384 > scratch_bytes) return;
    const vip_vp8_mb* mbs = (const vip_vp8_mb*)(stream + D.stream_off + D.mb_off);
    const int16_t* coefs = (const int16_t*)(stream + D.stream_off + D.coef_off);
    // VIP_VP8_STAGE_LDS_PLANES: an image of up to LDS_MBS macroblocks keeps its planes in LDS through both walks and copies
    // them out once at the end; the accesses are then flat ones (one body for both homes of the planes)
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_planes[];
    const bool in_lds = (stages & VIP_VP8_STAGE_LDS_PLANES) && (stages & VIP_VP8_STAGE_RECON) && nmb <= (size_t)LDS_MBS;
    uint8_t* const home = scratch + D.plane_off;
    const Vp8Planes P = vp8_planes(in_lds ? lds_planes : home, mb_w, mb_h);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int steps = mb_w + 2 * (mb_h - 1);

    for (int t = 0; (stages & VIP_VP8_STAGE_RECON) && t < steps; ++t) {
        int ylo, count;
        step_rows(t, mb_w, mb_h, ylo, count);
        for (int base = 0; base < count; base += NW) {
            const bool valid = base + wave < count;          // uniform over the wave
            const int my = ylo + base + wave, mx = t - 2 * my;
            vip_vp8_mb M;
            bool subs = false;
            if (valid) {
                M = mbs[(size_t)my * mb_w + mx];
                if ((uint64_t)M.coef_idx + (uint64_t)vp8_popc(M.nz & 0x1ffffffu) > (uint64_t)D.coef_blocks) M.nz = 0;
                M.nz &= 0x1ffffffu;
                subs = M.ymode == VIP_VP8_B_PRED;
                int dc_y, dc_u, dc_v;
                dc_values(P, mx, my, lane, dc_y, dc_u, dc_v);
                for (int item = subs ? 64 + lane : lane; item < 96; item += 64) vp8_recon_item(P, M, coefs, mx, my, item, dc_y, dc_u, dc_v);
            }
            if (__syncthreads_or(subs)) {
                for (int s = 0; s < 10; ++s) {
                    if (subs && lane < 8) {
                        const int bylo = s > 3 ? (s - 2) >> 1 : 0, byhi = min(3, s >> 1);
                        const int by = bylo + (lane >> 2), bx = s - 2 * by;
                        if (by <= byhi) vp8_recon_sub_item(P, M, coefs, mx, my, bx, by, lane & 3);
                    }
                    __syncthreads();
                }
            }
        }
    }
    const bool filter = (stages & VIP_VP8_STAGE_FILTER) && (D.filter_type == 1 || D.filter_type == 2);
    for (int t = 0; filter && t < steps; ++t) {
        int ylo, count;
        step_rows(t, mb_w, mb_h, ylo, count);
        for (int base = 0; base < count; base += NW) {
            const bool valid = base + wave < count;
            const int my = ylo + base + wave, mx = t - 2 * my;
            vip_vp8_mb M;
            if (valid) M = mbs[(size_t)my * mb_w + mx];
            if (valid && lane < 32) vp8_filter_item(P, M, D.filter_type, mx, my, lane, false);
            __syncthreads();
            if (valid && lane < 32) vp8_filter_item(P, M, D.filter_type, mx, my, lane, true);
            __syncthreads();
        }
    }
    if (in_lds) {                                            // every walk ended on a barrier; nmb * 384 is a multiple of 16
        const uint4* src = (const uint4*)lds_planes;
        uint4* dst = (uint4*)home;
        for (int i = threadIdx.x; i < (int)(nmb * 24); i += 64 * NW) dst[i] = src[i];
    }
}

// grid (ceil(maxW / 64), ceil(maxH / 4), n), block (64, 4): one thread per pixel
__global__ __launch_bounds__(256) void vp8_rgb_kernel(const vip_vp8_desc* __restrict__ desc, const uint8_t* __restrict__ scratch,
                                                      size_t scratch_bytes, uint8_t* __restrict__ rgb, int maxH, int maxW) {
    const vip_vp8_desc& D = desc[blockIdx.z];
    const int w = D.width, h = D.height;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (w <= 0 || h <= 0 || x >= w || y >= h || x >= maxW || y >= maxH) return;
    const int mb_w = D.mb_w, mb_h = D.mb_h;
    if (mb_w != (w + 15) >> 4 || mb_h != (h + 15) >> 4 || D.plane_off < 0 || (size_t)D.plane_off > scratch_bytes ||
        (size_t)D.plane_off + (size_t)mb_w * mb_h * 384 > scratch_bytes)
        return;
    const Vp8Planes P = vp8_planes(const_cast<uint8_t*>(scratch) + D.plane_off, mb_w, mb_h);
    uint8_t px[3];
    vp8_rgb_px(P, w, h, x, y, px);
    uint8_t* o = rgb + (((int64_t)blockIdx.z * maxH + y) * maxW + x) * 3;
    o[0] = px[0];
    o[1] = px[1];
    o[2] = px[2];
}

}  // namespace

// what vip_vp8_reconstruct_rgb_u8 runs: all three stages, the planes where they measured faster
constexpr int DEFAULT_STAGES = VIP_VP8_STAGE_RECON | VIP_VP8_STAGE_FILTER | VIP_VP8_STAGE_OUTPUT;

extern "C" int vip_vp8_default_stages(void) { return DEFAULT_STAGES; }

extern "C" int vip_vp8_reconstruct_rgb_u8(const uint8_t* stream_d, size_t stream_bytes, const vip_vp8_desc* desc, int n, uint8_t* scratch,
                                          size_t scratch_bytes, uint8_t* rgb_u8, int maxH, int maxW, void* stream) {
    return vip_vp8_reconstruct_stages_rgb_u8(stream_d, stream_bytes, desc, n, scratch, scratch_bytes, rgb_u8, maxH, maxW, DEFAULT_STAGES, stream);
}

extern "C" int vip_vp8_reconstruct_stages_rgb_u8(const uint8_t* stream_d, size_t stream_bytes, const vip_vp8_desc* desc, int n,
                                                 uint8_t* scratch, size_t scratch_bytes, uint8_t* rgb_u8, int maxH, int maxW, int stages,
                                                 void* stream) {
    VIP_REQUIRE(stream_d && desc && scratch && rgb_u8, VIP_ERR_BAD_ARG, "vip_vp8_reconstruct_rgb_u8: null pointer");
    VIP_REQUIRE(n > 0 && n <= 65535 && maxH > 0 && maxW > 0, VIP_ERR_BAD_ARG, "vip_vp8_reconstruct_rgb_u8: bad size (n in 1..65535)");
    VIP_REQUIRE(stream_bytes > 0 && scratch_bytes > 0, VIP_ERR_BAD_ARG, "vip_vp8_reconstruct_rgb_u8: empty buffer");
    VIP_REQUIRE(((uintptr_t)stream_d & 7) == 0 && ((uintptr_t)desc & 7) == 0 && ((uintptr_t)scratch & 15) == 0, VIP_ERR_ALIGNMENT,
                "vip_vp8_reconstruct_rgb_u8: stream / desc not 8-byte or scratch not 16-byte aligned");
    VIP_REQUIRE(stages > 0 && stages < 16 && (stages & 7), VIP_ERR_BAD_ARG, "vip_vp8_reconstruct_rgb_u8: stages is a mask of VIP_VP8_STAGE_*");
    if (stages & (VIP_VP8_STAGE_RECON | VIP_VP8_STAGE_FILTER)) {
        hipLaunchKernelGGL(vp8_recon_filter_kernel, dim3(n), dim3(64 * NW), (stages & VIP_VP8_STAGE_LDS_PLANES) ? LDS_BYTES : 0,
                           (hipStream_t)stream, stream_d, stream_bytes, desc, scratch, scratch_bytes, stages);
        const int st = vip_launch_status("vip_vp8_reconstruct_rgb_u8");
        if (st != VIP_OK) return st;
    }
    if (!(stages & VIP_VP8_STAGE_OUTPUT)) return VIP_OK;
    const dim3 grid((maxW + 63) / 64, (maxH + 3) / 4, n);
    VIP_REQUIRE(grid.y <= 65535, VIP_ERR_BAD_ARG, "vip_vp8_reconstruct_rgb_u8: maxH too large");
    hipLaunchKernelGGL(vp8_rgb_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, desc, scratch, scratch_bytes, rgb_u8, maxH, maxW);
    return vip_launch_status("vip_vp8_reconstruct_rgb_u8");
}
