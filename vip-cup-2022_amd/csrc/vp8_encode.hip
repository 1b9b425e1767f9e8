// GPU half of the lossy WebP re-save: 8-bit RGB -> YUV 4:2:0 -> per macroblock the prediction modes, forward DCT / WHT,
// quantisation and the decoder's reconstruction  [the project's own VP8 key-frame encoder, up to the entropy coder].
// The arithmetic is in vp8_enc.hpp (and vp8_recon.hpp for everything a decoder repeats); this file owns the order.
//
// vp8_encode_kernel: one workgroup of four waves per image and the decoder's walk (vp8_walk.hpp): a macroblock predicts
// from reconstructed neighbours, so the image is walked in steps t = x + 2 y, the macroblocks of a step one per wave, a
// workgroup barrier after each round.  Inside a round a wave is alone with its macroblock and orders its own phases with
// wave-level fences only - no workgroup barrier sits in code that only some waves run.  The planes of an image of up to
// 169 macroblocks stay in LDS and are copied out once; a larger image works in the scratch buffer (L2).
//
// One macroblock, one wave:
//   1. each lane converts one 2 x 2 quad of RGB: 4 luma samples, one U, one V into the wave's 384 source bytes (LDS);
//   2. chroma: two modes at a time, 32 lanes x 4 pixels each; luma 16 x 16: a mode at a time, 64 lanes x 4 pixels; sums
//      of squared errors by cross-lane adds, the minimum with the mode number in the low bits (ties to the lowest);
//   3. the sub-block trial, 16 sub-blocks in raster order: lane = mode x row (10 x 4 of 64), SSE by two cross-lane adds,
//      minimum as above; every lane then holds the block's levels (the forward DCT of 16 values is not worth splitting),
//      lanes 0..3 reconstruct one row each in place, a fence, and the next sub-block predicts from it;
//   4. S4 + bias < S16 decides; otherwise lanes 0..15 code the luma blocks against the 16 x 16 prediction and lane 24
//      sends their DCs through the WHT; lanes 16..23 code the chroma blocks either way;
//   5. lane b < 25 dequantises block b; two ballots give the record's nz / dc_only, the coded blocks go back to back;
//   6. the decoder's vp8_recon_item over 96 items (32: chroma only, when the sub-block luma stands already).
// No atomics, no dependence on anything outside the image: the output is bit-reproducible.
#include "common.hpp"
#include "vp8_enc.hpp"
#include "vp8_walk.hpp"

uint64_t vip_vp8_encode_max_pixels();                        // vp8_enc_host.cpp

namespace {

constexpr int ENC_LDS_BYTES = NW * VP8E_SRC_BYTES + LDS_BYTES;      // the waves' source samples, then the planes

// what one wave wrote is read by its other lanes: order it (the wave runs in lockstep, the memory need not)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ int wave_sum(int v, int lanes) {
    for (int o = 1; o < lanes; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min(int v, int from, int lanes) {
    for (int o = from; o < lanes; o <<= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ void store16(int16_t* dst, const int16_t v[16]) {      // dst 32-byte aligned
    uint4 a, b;
    a.x = (uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16);
    a.y = (uint16_t)v[2] | ((uint32_t)(uint16_t)v[3] << 16);
    a.z = (uint16_t)v[4] | ((uint32_t)(uint16_t)v[5] << 16);
    a.w = (uint16_t)v[6] | ((uint32_t)(uint16_t)v[7] << 16);
    b.x = (uint16_t)v[8] | ((uint32_t)(uint16_t)v[9] << 16);
    b.y = (uint16_t)v[10] | ((uint32_t)(uint16_t)v[11] << 16);
    b.z = (uint16_t)v[12] | ((uint32_t)(uint16_t)v[13] << 16);
    b.w = (uint16_t)v[14] | ((uint32_t)(uint16_t)v[15] << 16);
    ((uint4*)dst)[0] = a;
    ((uint4*)dst)[1] = b;
}
__device__ __forceinline__ void load16(const int16_t* src, int16_t v[16]) {
    const uint4 a = ((const uint4*)src)[0], b = ((const uint4*)src)[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    for (int i = 0; i < 8; ++i) {
        v[2 * i] = (int16_t)(w[i] & 0xffffu);
        v[2 * i + 1] = (int16_t)(w[i] >> 16);
    }
}

// one macroblock by one wave; mb: its record, coefs: the image's coefficient area, lv: its 25 x 16 levels
__device__ void encode_mb(const uint8_t* rgb, int64_t row_px, int w, int h, const Vp8Planes& P, const vip_vp8_enc_params& E, int mx, int my,
                          uint8_t* src, vip_vp8_mb* mb, int16_t* coefs, uint32_t coef_idx, int16_t* lv, int lane) {
    // 1
    vp8e_convert_quad(rgb, row_px, w, h, mx, my, lane & 7, lane >> 3, src);
    wave_sync();
    int dc_y, dc_u, dc_v;
    dc_values(P, mx, my, lane, dc_y, dc_u, dc_v);
    // 2: DC, TM, VE, HE are 0..3, so the smallest (sse, mode) pair is the first of the best in that order
    int uv_key = 0x7fffffff, y_key = 0x7fffffff;
    for (int pass = 0; pass < 2; ++pass) {
        const int mode = pass * 2 + (lane >> 5);
        const int s = wave_sum(vp8e_sse_chroma_item(src, P, mode, mx, my, lane & 31, dc_u, dc_v), 32);
        const int key = s * 4 + mode;
        uv_key = min(uv_key, min(__shfl(key, 0, 64), __shfl(key, 32, 64)));
    }
    for (int mode = 0; mode < 4; ++mode) {
        const int s = wave_sum(vp8e_sse_luma16_item(src, P, mode, mx, my, lane, dc_y), 64);
        y_key = min(y_key, s * 4 + mode);
    }
    const int uvmode = uv_key & 3, ymode = y_key & 3, s16 = y_key >> 2;
    // 3
    int my_bmode = 0, s4 = 0;
    for (int b = 0; b < 16; ++b) {
        const int bx = b & 3, by = b >> 2;
        int e[13];
        vp8_edges4(P, mx, my, bx, by, e);
        const int mode = lane >> 2;
        int d[16], s = 0;
        if (mode < 10) {
            vp8_pred4_block(mode, e, d);
            s = vp8e_sse_sub_row(src, d, bx, by, lane & 3);
        }
        s = wave_sum(s, 4);
        const int key = wave_min(mode < 10 ? s * 16 + mode : 0x7fffffff, 4, 64);
        const int bm = key & 15;
        s4 += key >> 4;
        if (lane == b) my_bmode = bm;
        int16_t l16[16], cf[16];
        bool any, only0;
        vp8_pred4_block(bm, e, d);                           // uniform: the chosen mode, for the residual and the reconstruction
        vp8e_code_sub_block(src, d, E, bx, by, l16);
        vp8e_dequant_block(l16, E, b, cf, &any, &only0);
        if (lane == 0) store16(lv + b * 16, l16);
        if (lane < 4) vp8e_recon_sub_row(P, mx, my, bx, by, lane, d, cf, any, only0);
        wave_sync();
    }
    // 4
    const bool i4 = s4 + E.i4_bias < s16;
    {
        int16_t l16[16];
        int dc = 0;
        const bool codes = lane < 24 && (lane >= 16 || !i4);
        if (codes) vp8e_code_large_block(src, P, E, mx, my, lane, lane < 16 ? ymode : uvmode, lane < 16 ? dc_y : lane < 20 ? dc_u : dc_v, l16, &dc);
        int dcs[16];
        for (int i = 0; i < 16; ++i) dcs[i] = __shfl(dc, i, 64);
        if (lane == 24) {
            if (i4) for (int i = 0; i < 16; ++i) l16[i] = 0;
            else vp8e_code_y2(dcs, E, l16);
        }
        if (codes || lane == 24) store16(lv + lane * 16, l16);
    }
    wave_sync();
    // 5
    int16_t l16[16], cf[16], y2[16];
    bool any = false, only0 = false, any24, only24;
    load16(lv + 24 * 16, l16);
    vp8e_dequant_block(l16, E, 24, y2, &any24, &only24);
    if (lane < 25) {
        load16(lv + lane * 16, l16);
        vp8e_dequant_block(l16, E, lane, cf, &any, &only0);
    }
    const uint32_t nz = (uint32_t)__ballot(any), dconly = (uint32_t)__ballot(only0);
    uint8_t bmodes[16];
    for (int i = 0; i < 16; ++i) bmodes[i] = (uint8_t)__shfl(my_bmode, i, 64);
    vip_vp8_mb M;
    vp8e_record(M, E, i4, ymode, bmodes, uvmode, nz, dconly, y2, coef_idx);
    if (lane == 0) *mb = M;
    if (lane < 25) {
        int16_t* out = coefs + (int64_t)coef_idx * 16;
        if ((M.nz >> lane) & 1u) store16(out + vp8_popc(M.nz & ((1u << lane) - 1u)) * 16, cf);
        if (lane >= vp8_popc(M.nz)) {                        // the slots no coded block takes
            for (int i = 0; i < 16; ++i) cf[i] = 0;
            store16(out + lane * 16, cf);
        }
    }
    wave_sync();
    // 6
    for (int item = i4 ? 64 + lane : lane; item < 96; item += 64) vp8_recon_item(P, M, coefs, mx, my, item, dc_y, dc_u, dc_v);
}

// grid (n), block (64 NW), ENC_LDS_BYTES of dynamic LDS
__global__ __launch_bounds__(64 * NW) void vp8_encode_kernel(const uint8_t* __restrict__ rgb, const vip_vp8_desc* desc, int maxH, int maxW,
                                                             vip_vp8_enc_params E, uint8_t* stream, size_t stream_bytes, int16_t* levels,
                                                             size_t levels_elems, uint8_t* scratch, size_t scratch_bytes) {
    const vip_vp8_desc D = desc[blockIdx.x];
    const int mb_w = D.mb_w, mb_h = D.mb_h;
    if (D.width <= 0 || D.height <= 0 || D.width > maxW || D.height > maxH || mb_w != (D.width + 15) >> 4 || mb_h != (D.height + 15) >> 4) return;
    const size_t nmb = (size_t)mb_w * mb_h;
    // what the host wrote is trusted, but not beyond the buffers (uniform over the workgroup)
    if (D.stream_off < 0 || D.mb_off < 0 || D.coef_off < 0 || D.coef_blocks < 0 || D.plane_off < 0) return;
    if (((D.stream_off | D.coef_off) & 15) != 0 || (D.mb_off & 7) != 0 || D.plane_off % 384 != 0) return;
    if ((size_t)D.stream_off > stream_bytes || (size_t)D.mb_off > stream_bytes || (size_t)D.coef_off > stream_bytes) return;
    if ((size_t)D.stream_off + (size_t)D.mb_off + nmb * sizeof(vip_vp8_mb) > stream_bytes) return;
    if ((size_t)D.coef_blocks < nmb * 25 || (size_t)D.stream_off + (size_t)D.coef_off + nmb * 25 * 32 > stream_bytes) return;
    if ((size_t)D.plane_off > scratch_bytes || (size_t)D.plane_off + nmb * 384 > scratch_bytes) return;
    const size_t first_mb = (size_t)D.plane_off / 384;       // the planes lie back to back, so this counts the macroblocks before
    if ((first_mb + nmb) * 400 > levels_elems) return;
    vip_vp8_mb* mbs = (vip_vp8_mb*)(stream + D.stream_off + D.mb_off);
    int16_t* coefs = (int16_t*)(stream + D.stream_off + D.coef_off);
    int16_t* lv = levels + first_mb * 400;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const bool in_lds = nmb <= (size_t)LDS_MBS;
    uint8_t* const home = scratch + D.plane_off;
    const Vp8Planes P = vp8_planes(in_lds ? lds + NW * VP8E_SRC_BYTES : home, mb_w, mb_h);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint8_t* img = rgb + (int64_t)blockIdx.x * maxH * maxW * 3;
    const int steps = mb_w + 2 * (mb_h - 1);
    for (int t = 0; t < steps; ++t) {
        int ylo, count;
        step_rows(t, mb_w, mb_h, ylo, count);
        for (int base = 0; base < count; base += NW) {
            if (base + wave < count) {                       // uniform over the wave
                const int my = ylo + base + wave, mx = t - 2 * my;
                const size_t idx = (size_t)my * mb_w + mx;
                encode_mb(img, maxW, D.width, D.height, P, E, mx, my, lds + wave * VP8E_SRC_BYTES, mbs + idx, coefs, (uint32_t)(idx * 25), lv + idx * 400, lane);
            }
            __syncthreads();
        }
    }
    if (in_lds) {                                            // the walk ended on a barrier; nmb * 384 is a multiple of 16
        const uint4* s = (const uint4*)(lds + NW * VP8E_SRC_BYTES);
        uint4* d = (uint4*)home;
        for (int i = threadIdx.x; i < (int)(nmb * 24); i += 64 * NW) d[i] = s[i];
    }
}

}  // namespace

extern "C" int vip_vp8_encode_rgb_u8(const uint8_t* rgb_u8, const vip_vp8_desc* desc, int n, int maxH, int maxW, int quality, uint8_t* stream_d,
                                     size_t stream_bytes, int16_t* levels_d, size_t levels_elems, uint8_t* scratch, size_t scratch_bytes,
                                     void* stream) {
    VIP_REQUIRE(rgb_u8 && desc && stream_d && levels_d && scratch, VIP_ERR_BAD_ARG, "vip_vp8_encode_rgb_u8: null pointer");
    VIP_REQUIRE(quality >= 1 && quality <= 100, VIP_ERR_BAD_ARG, "vip_vp8_encode_rgb_u8: quality %d: expected 1..100", quality);
    VIP_REQUIRE(n > 0 && n <= 65535 && maxH > 0 && maxW > 0, VIP_ERR_BAD_ARG, "vip_vp8_encode_rgb_u8: bad size (n in 1..65535)");
    VIP_REQUIRE((uint64_t)maxH * (uint64_t)maxW <= vip_vp8_encode_max_pixels(), VIP_ERR_BAD_ARG,
                "vip_vp8_encode_rgb_u8: %dx%d exceeds VIP_MAX_JPEG_PIXELS=%llu", maxW, maxH, (unsigned long long)vip_vp8_encode_max_pixels());
    VIP_REQUIRE(stream_bytes > 0 && levels_elems > 0 && scratch_bytes > 0, VIP_ERR_BAD_ARG, "vip_vp8_encode_rgb_u8: empty buffer");
    VIP_REQUIRE(((uintptr_t)stream_d & 15) == 0 && ((uintptr_t)desc & 7) == 0 && ((uintptr_t)scratch & 15) == 0 && ((uintptr_t)levels_d & 15) == 0,
                VIP_ERR_ALIGNMENT, "vip_vp8_encode_rgb_u8: desc not 8-byte or stream / levels / scratch not 16-byte aligned");
    vip_vp8_enc_params E;
    const int st = vip_vp8_encode_params_h(quality, &E);
    if (st != VIP_OK) return st;
    static const hipError_t lds_ok =
        hipFuncSetAttribute((const void*)vp8_encode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ENC_LDS_BYTES);      // above 64 KB
    VIP_REQUIRE(lds_ok == hipSuccess, VIP_ERR_LAUNCH, "vip_vp8_encode_rgb_u8: %d bytes of LDS refused: %s", ENC_LDS_BYTES, hipGetErrorString(lds_ok));
    hipLaunchKernelGGL(vp8_encode_kernel, dim3(n), dim3(64 * NW), ENC_LDS_BYTES, (hipStream_t)stream, rgb_u8, desc, maxH, maxW, E, stream_d,
                       stream_bytes, levels_d, levels_elems, scratch, scratch_bytes);
    return vip_launch_status("vip_vp8_encode_rgb_u8");
}
