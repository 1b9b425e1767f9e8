// Fragment-order helpers shared by the kernels that chain MFMAs through registers (mlp_fused.hip, gcvit_block.hip, gcvit_block14.hip):
// weight rows interleaved so that a lane's packed results are 8 consecutive channels, and LayerNorm on activation fragments.
#pragma once
#include "common.hpp"

// LDS row j of a 32-row group holds channel (j>>4)*4 + ((j&15)>>2)*8 + (j&3): MFMA tiles 2h, 2h+1 then give a lane
// the channels 8*lq .. 8*lq+7 of the group
__device__ __forceinline__ int frag_channel32(int j) {      // j < 32: within one group
    const int t = (j >> 4) & 1, r = j & 15;
    return (r >> 2) * 8 + t * 4 + (r & 3);
}
__device__ __forceinline__ int frag_channel(int j) {        // consecutive groups of 32
    const int t = (j >> 4) & 1, r = j & 15;
    return (j & ~31) + (r >> 2) * 8 + t * 4 + (r & 3);
}

// Optional LayerNorm prologue on the activation fragments of one 16-token tile: lane (l15 = token, lq) holds channels
// 32 ks + 8 lq + 0..7 for ks < CK, so a token's C channels sit in 4 lanes (lq = 0..3): in-lane sums + two cross-row
// exchanges.  Two-pass mean / variance in fp32 and the same expression as layernorm_kernel (pointwise.hip); the
// normalised row is rounded to fp16 exactly where the separate LayerNorm launch rounded it.
// gamma / beta: channels 8 i .. 8 i + 7 at g + i * step bytes (step = 32: a plain vector in global memory; the resident
// kernel keeps them in the pads of its LDS weight image, one group per row)
template <int CK>
__device__ __forceinline__ void ln_fragments(U4H8 (&xf)[CK], const char* g, const char* b, int step, float eps, int lq) {
    constexpr int C = 32 * CK;
    float v[CK][8];
    float sum = 0.f;
#pragma unroll
    for (int ks = 0; ks < CK; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[ks][j] = (float)xf[ks].e[j];
            sum += v[ks][j];
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int ks = 0; ks < CK; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = v[ks][j] - mean;
            sq += d * d;
        }
    sq += __shfl_xor(sq, 16, 64);
    sq += __shfl_xor(sq, 32, 64);
    const float rstd = rsqrtf(sq / (float)C + eps);
#pragma unroll
    for (int ks = 0; ks < CK; ++ks) {
        const char *gp = g + (ks * 4 + lq) * step, *bp = b + (ks * 4 + lq) * step;
        const float4 g0 = *reinterpret_cast<const float4*>(gp), g1 = *reinterpret_cast<const float4*>(gp + 16);
        const float4 b0 = *reinterpret_cast<const float4*>(bp), b1 = *reinterpret_cast<const float4*>(bp + 16);
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) xf[ks].e[j] = (f16)((v[ks][j] - mean) * rstd * gg[j] + bb[j]);
    }
}

// The same on a plain gamma / beta vector in global memory (lane group g: channels 32 ks + 8 g .. + 7): mirrors ln_fragments above with
// step = 32 and stays, because called through the strided form (byte pointers, run-time step) the block kernels' code changes.
template <int CK>
__device__ __forceinline__ void ln_fragments(U4H8 (&xf)[CK], const float* __restrict__ gam, const float* __restrict__ bet, float eps,
                                             int g) {
    constexpr int C = 32 * CK;
    float v[CK][8];
    float sum = 0.f;
#pragma unroll
    for (int ks = 0; ks < CK; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[ks][j] = (float)xf[ks].e[j];
            sum += v[ks][j];
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int ks = 0; ks < CK; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = v[ks][j] - mean;
            sq += d * d;
        }
    sq += __shfl_xor(sq, 16, 64);
    sq += __shfl_xor(sq, 32, 64);
    const float rstd = rsqrtf(sq / (float)C + eps);
#pragma unroll
    for (int ks = 0; ks < CK; ++ks) {
        const float4 g0 = *reinterpret_cast<const float4*>(gam + ks * 32 + g * 8), g1 = *reinterpret_cast<const float4*>(gam + ks * 32 + g * 8 + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(bet + ks * 32 + g * 8), b1 = *reinterpret_cast<const float4*>(bet + ks * 32 + g * 8 + 4);
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) xf[ks].e[j] = (f16)((v[ks][j] - mean) * rstd * gg[j] + bb[j]);
    }
}
