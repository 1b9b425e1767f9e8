// The macroblock walk of the lossy WebP kernels, shared by the decoder (vp8_pipeline.hip) and the encoder (vp8_encode.hip):
// one workgroup of NW waves per image, steps t = x + 2 y, a macroblock per wave.  Device only.
#pragma once
#include "common.hpp"
#include "vp8_recon.hpp"

namespace {

constexpr int NW = 4;                // waves per workgroup = macroblocks in flight per image
constexpr int LDS_MBS = 169;         // planes of up to 13 x 13 macroblocks (200 x 200 pixels) fit 64 KB of LDS
constexpr int LDS_BYTES = LDS_MBS * 384;

// sums of the samples above / left of a macroblock for the DC predictions, by the whole wave: lanes 0..15 and 16..31
// fetch luma, 32..39 / 40..47 U, 48..55 / 56..63 V
__device__ __forceinline__ void dc_values(const Vp8Planes& P, int mx, int my, int lane, int& dc_y, int& dc_u, int& dc_v) {
    int s = 0;
    if (lane < 32) {
        const int i = lane & 15;
        if (lane < 16) s = my > 0 ? P.y[(int64_t)(my * 16 - 1) * P.ys + mx * 16 + i] : 0;
        else s = mx > 0 ? P.y[(int64_t)(my * 16 + i) * P.ys + mx * 16 - 1] : 0;
    } else {
        const uint8_t* c = lane < 48 ? P.u : P.v;
        const int i = lane & 7;
        if (!(lane & 8)) s = my > 0 ? c[(int64_t)(my * 8 - 1) * P.cs + mx * 8 + i] : 0;
        else s = mx > 0 ? c[(int64_t)(my * 8 + i) * P.cs + mx * 8 - 1] : 0;
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);                               // groups of 8
    const int s16 = s + __shfl_xor(s, 8, 64);                // groups of 16
    dc_y = vp8_dc_value(__shfl(s16, 0, 64), __shfl(s16, 16, 64), 16, mx, my);
    dc_u = vp8_dc_value(__shfl(s, 32, 64), __shfl(s, 40, 64), 8, mx, my);
    dc_v = vp8_dc_value(__shfl(s, 48, 64), __shfl(s, 56, 64), 8, mx, my);
}

// the macroblocks of step t: rows ylo .. ylo + count - 1, macroblock (t - 2 y, y)
__device__ __forceinline__ void step_rows(int t, int mb_w, int mb_h, int& ylo, int& count) {
    ylo = t - (mb_w - 1) > 0 ? (t - (mb_w - 1) + 1) >> 1 : 0;
    const int yhi = min(mb_h - 1, t >> 1);
    count = yhi - ylo + 1;
}

}  // namespace
