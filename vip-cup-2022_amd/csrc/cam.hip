// Grad-CAM evidence maps for heads of the form  GAP -> [LayerNorm] -> Dense -> activation  (include/vipcup_hip.h "Evidence maps").
// Because the head is that short, the gradient Grad-CAM pools has a closed form and no backward pass through the body is needed:
//   v = mean_hw F,  u = LN(v) | v,  z = W u + b,  p = act(z),  s = target(p)
//   dz = ds/dz,  a = W^T dz,  [LN: a <- gamma a;  a <- (a - mean a - uh mean(a uh)) / sd,  uh = (v - mean v) / sd]
//   g = a / HW  ( = mean_hw ds/dF ),  cam[h,w] = max(0, sum_c F[h,w,c] g[c]),  peak = max_hw cam
// vip_cam_*:          one workgroup per image.  F is read twice (a 7 x 7 x 2048 fp16 map is 200 KB, more than the LDS); only v, a / g
//                     and the logits live in LDS.  Pass 1 pools with the loop structure of the head kernels (pointwise.hip
//                     gap_ln_dense_kernel, strict_ops.hip sgap_ln_dense_kernel), so z agrees with the head launch; pass 2 is one wave
//                     per position for the C-long dot product, then the maximum.  fp32 accumulation throughout, a fixed summation
//                     order (bit-repeatable).
// vip_cam_compose_f32: up to 16 members' low-resolution maps -> one full-size map per image (normalise by peak, bilinear resample with
//                     half-pixel centres and edge clamp, weighted mean), written once.
// vip_cam_overlay_u8:  colour table applied to the uint8 map, blended over the resident RGB pixels.
#include "common.hpp"
#include <math.h>

namespace {

constexpr int CAM_MAX_C = 4096;
constexpr int CAM_MAX_N = 64;
constexpr int CAM_MAX_MEMBERS = 16;

// storage policies: 4 consecutive logical elements i .. i+3 (i % 4 == 0) of a tensor whose element 0 is at `b`; FAST = the arithmetic
// of the fp16 head kernels (multiply by 1 / HW, rsqrtf), otherwise that of the strict ones (true division, 1 / sqrtf)
struct CF16 {
    static constexpr bool FAST = true;
    static constexpr int G = 8;                        // channels one thread pools (the grouping of the matching head kernel)
    static __device__ __forceinline__ f32x4 ld(const void* b, long i) {
        const f16x4 h = *reinterpret_cast<const f16x4*>(static_cast<const f16*>(b) + i);
        return (f32x4){(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    }
};
struct CF32 {
    static constexpr bool FAST = false;
    static constexpr int G = 4;
    static __device__ __forceinline__ f32x4 ld(const void* b, long i) { return *reinterpret_cast<const f32x4*>(static_cast<const float*>(b) + i); }
};
struct CH2 {
    static constexpr bool FAST = false;
    static constexpr int G = 4;
    static __device__ __forceinline__ f32x4 ld(const void* b, long i) { return h2_ld4(b, i); }
};

// sum over the 256 threads of the workgroup, the four wave partials added in wave order; `slot` = 4 floats of LDS
__device__ __forceinline__ float block_sum(float s, float* slot) {
    s = wave_reduce_sum(s);
    __syncthreads();                                   // the slot may still be read from its previous use
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = s;
    __syncthreads();
    return slot[0] + slot[1] + slot[2] + slot[3];
}

template <typename S>
__global__ __launch_bounds__(256) void cam_kernel(const void* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  float eps, const float* __restrict__ Wt, const float* __restrict__ bias,
                                                  float* __restrict__ cam, float* __restrict__ peak, float* __restrict__ zout, int HW, int C,
                                                  int ldx, long img_stride, int N, int act, int target) {
    __shared__ __attribute__((aligned(16))) float vh[CAM_MAX_C];                    // v, then (LayerNorm head) uh = (v - mean) / sd
    __shared__ __attribute__((aligned(16))) float ag[CAM_MAX_C];                    // u while the logits are formed, then a, then g
    __shared__ float zs[CAM_MAX_N], dzs[CAM_MAX_N];
    __shared__ float red[4];
    __shared__ float wmax[4];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const long xb = (long)b * img_stride;
    const float inv_hw = 1.f / (float)HW;

    // ---- pass 1: pool --------------------------------------------------------------------------------------------------------
    float s1 = 0.f;
    for (int cg = tid; cg < C / S::G; cg += 256) {
        f32x4 acc[S::G / 4];
#pragma unroll
        for (int q = 0; q < S::G / 4; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int p = 0; p < HW; ++p)
#pragma unroll
            for (int q = 0; q < S::G / 4; ++q) acc[q] += S::ld(x, xb + (long)p * ldx + cg * S::G + q * 4);
#pragma unroll
        for (int j = 0; j < S::G; ++j) {
            const float m = S::FAST ? acc[j >> 2][j & 3] * inv_hw : acc[j >> 2][j & 3] / (float)HW;
            vh[cg * S::G + j] = m;
            s1 += m;
        }
    }
    float rstd = 1.f;
    if (gamma) {                                       // uniform branch: LayerNorm statistics of the pooled vector
        const float mean = block_sum(s1, red) / (float)C;
        float s2 = 0.f;
        for (int c = tid; c < C; c += 256) {
            const float d = vh[c] - mean;
            s2 += d * d;
        }
        const float var = block_sum(s2, red) / (float)C + eps;
        rstd = S::FAST ? rsqrtf(var) : 1.0f / sqrtf(var);
        for (int c = tid; c < C; c += 256) {
            const float uh = (vh[c] - mean) * rstd;
            vh[c] = uh;
            ag[c] = uh * gamma[c] + beta[c];
        }
    } else {
        __syncthreads();
        for (int c = tid; c < C; c += 256) ag[c] = vh[c];
    }
    __syncthreads();

    // ---- logits, dz = d target / d z ---------------------------------------------------------------------------------------------
    for (int n = 0; n < N; ++n) {
        float s = 0.f;
        for (int c = tid; c < C; c += 256) s += ag[c] * Wt[(long)n * C + c];
        s = block_sum(s, red) + (bias ? bias[n] : 0.f);
        if (tid == 0) {
            zs[n] = s;
            zout[(long)b * N + n] = s;
        }
    }
    __syncthreads();
    if (tid < N) {
        // p_k and d p_k / d z_j of the head activation, for k = the class whose probability is the target
        const int k = target < 0 ? 0 : target;
        float d;
        if (act == 1) {                                                    // element-wise sigmoid: p (1 - p) without the cancellation
            d = tid == k ? (1.f / (1.f + expf(-zs[k]))) * (1.f / (1.f + expf(zs[k]))) : 0.f;
        } else if (act == 2) {                                             // softmax: p_k (delta_kj - p_j), 1 - p_k as the sum of the others
            float mx = zs[0];
            for (int j = 1; j < N; ++j) mx = fmaxf(mx, zs[j]);
            float den = 0.f, others = 0.f;
            for (int j = 0; j < N; ++j) {
                const float e = expf(zs[j] - mx);
                den += e;
                if (j != k) others += e;
            }
            const float pk = expf(zs[k] - mx) / den;
            d = tid == k ? pk * (others / den) : -pk * (expf(zs[tid] - mx) / den);
        } else {                                                           // linear
            d = tid == k ? 1.f : 0.f;
        }
        // "score" (target < 0): p0 for one class, 1 - p0 otherwise (vip_prob_to_score_f32)
        dzs[tid] = (target < 0 && N > 1) ? -d : d;
    }
    __syncthreads();

    // ---- a = W^T dz, back through the LayerNorm, g = a / HW ------------------------------------------------------------------------
    float sa = 0.f, sau = 0.f;
    for (int c = tid; c < C; c += 256) {
        float a = 0.f;
        for (int n = 0; n < N; ++n) a += Wt[(long)n * C + c] * dzs[n];
        if (gamma) {
            a *= gamma[c];
            sa += a;
            sau += a * vh[c];
        }
        ag[c] = a;
    }
    if (gamma) {
        const float ma = block_sum(sa, red) / (float)C;
        const float mau = block_sum(sau, red) / (float)C;
        for (int c = tid; c < C; c += 256) ag[c] = (ag[c] - ma - vh[c] * mau) * rstd;
    }
    for (int c = tid; c < C; c += 256) ag[c] = ag[c] / (float)HW;        // each thread rescales what it wrote itself
    __syncthreads();

    // ---- pass 2: one wave per position ---------------------------------------------------------------------------------------------
    const int wave = tid >> 6, lane = tid & 63;
    float mx = 0.f;
    bool bad = false;
    for (int p = wave; p < HW; p += 4) {
        float s = 0.f;
        for (int c4 = lane; c4 < (C >> 2); c4 += 64) {
            const f32x4 f = S::ld(x, xb + (long)p * ldx + c4 * 4);
            const f32x4 g = *reinterpret_cast<const f32x4*>(&ag[c4 * 4]);
            s += f[0] * g[0];
            s += f[1] * g[1];
            s += f[2] * g[2];
            s += f[3] * g[3];
        }
        s = wave_reduce_sum(s);
        const bool finite = fabsf(s) <= 3.4028234e38f;                     // false for NaN and Inf
        bad |= !finite;
        const float v = finite ? fmaxf(s, 0.f) : s;
        mx = fmaxf(mx, v);
        if (lane == 0) cam[(long)b * HW + p] = v;
    }
    if (lane == 0) wmax[wave] = bad ? __builtin_nanf("") : mx;
    __syncthreads();
    if (tid == 0) {
        float m = 0.f;
        bool nan = false;
        for (int w = 0; w < 4; ++w) {
            nan |= wmax[w] != wmax[w];
            m = fmaxf(m, wmax[w]);
        }
        peak[b] = nan ? __builtin_nanf("") : m;                            // a non-finite peak is the caller's error signal
    }
}

template <typename S, int A>
int cam_impl(const char* who, const void* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias,
             float* cam, float* peak, float* z, int B, int HW, int C, int ldx, long img_stride, int N, int act, int target, void* stream) {
    VIP_REQUIRE(x && W && cam && peak && z && (!gamma == !beta), VIP_ERR_BAD_ARG, "%s: null pointer", who);
    VIP_REQUIRE(B > 0 && HW > 0 && C > 0 && N > 0 && eps >= 0.f && ldx >= C && img_stride >= 0, VIP_ERR_BAD_ARG,
                "%s: bad dimension or eps", who);
    VIP_REQUIRE((unsigned)act <= 2u, VIP_ERR_BAD_ARG, "%s: head activation %d (0 linear, 1 sigmoid, 2 softmax)", who, act);
    VIP_REQUIRE(target >= -1 && target < N, VIP_ERR_BAD_ARG, "%s: target %d outside -1 (score) .. %d", who, target, N - 1);
    VIP_REQUIRE(C <= CAM_MAX_C && N <= CAM_MAX_N, VIP_ERR_UNSUPPORTED, "%s: C=%d > %d or N=%d > %d", who, C, CAM_MAX_C, N, CAM_MAX_N);
    VIP_REQUIRE(C % A == 0 && ldx % A == 0 && img_stride % A == 0, VIP_ERR_ALIGNMENT,
                "%s: C, ldx and the image stride must be multiples of %d elements", who, A);
    hipLaunchKernelGGL(cam_kernel<S>, dim3(B), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, eps, W, bias, cam, peak, z, HW, C, ldx,
                       img_stride, N, act, target);
    return vip_launch_status(who);
}

// ---- compose ---------------------------------------------------------------------------------------------------------------------
struct ComposeArgs {
    const float* map[CAM_MAX_MEMBERS];
    const float* peak[CAM_MAX_MEMBERS];
    int gh[CAM_MAX_MEMBERS], gw[CAM_MAX_MEMBERS];
    float weight[CAM_MAX_MEMBERS];
    int M;
};

// source position of output index `dst` (half-pixel centres, edge clamp): src = (dst + 0.5) in / out - 0.5 as the exact rational
// ((2 dst + 1) in - out) / (2 out); i0 = floor, i1 = min(i0 + 1, in - 1), t = src - i0 (0 where src < 0)
__device__ __forceinline__ void lin_coord(int dst, int in, int out, int& i0, int& i1, float& t) {
    const long num = (long)(2 * dst + 1) * in - out;
    const long den = 2L * out;
    if (num <= 0) {
        i0 = 0;
        t = 0.f;
    } else {
        i0 = (int)(num / den);
        t = (float)(num - (long)i0 * den) / (float)den;
    }
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + 1 < in ? i0 + 1 : in - 1;
}

template <bool U8>
__global__ __launch_bounds__(256) void cam_compose_kernel(ComposeArgs a, const int32_t* __restrict__ sizes_hw, int n, int maxH, int maxW,
                                                          void* __restrict__ out) {
    const long total = (long)n * maxH * maxW;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int xo = (int)(idx % maxW);
        const long r = idx / maxW;
        const int yo = (int)(r % maxH);
        const int i = (int)(r / maxH);
        const int h = sizes_hw[2 * i], w = sizes_hw[2 * i + 1];
        float v = 0.f;
        if (yo < h && xo < w) {
            for (int m = 0; m < a.M; ++m) {
                const float pk = a.peak[m][i];
                if (!(pk > 0.f)) continue;                                 // peak == 0: an all-zero map
                const int gh = a.gh[m], gw = a.gw[m];
                int y0, y1, x0, x1;
                float ty, tx;
                lin_coord(yo, gh, h, y0, y1, ty);
                lin_coord(xo, gw, w, x0, x1, tx);
                const float* mp = a.map[m] + (long)i * gh * gw;
                const float top = mp[y0 * gw + x0] + tx * (mp[y0 * gw + x1] - mp[y0 * gw + x0]);
                const float bot = mp[y1 * gw + x0] + tx * (mp[y1 * gw + x1] - mp[y1 * gw + x0]);
                v += a.weight[m] * ((top + ty * (bot - top)) / pk);
            }
        }
        if (U8) {
            const float q = rintf(255.f * v);
            static_cast<uint8_t*>(out)[idx] = (uint8_t)fminf(fmaxf(q, 0.f), 255.f);
        } else {
            static_cast<float*>(out)[idx] = v;
        }
    }
}

// ---- overlay ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cam_overlay_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ map,
                                                          const uint8_t* __restrict__ table, float alpha, long pixels,
                                                          uint8_t* __restrict__ out) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < pixels; idx += (long)gridDim.x * 256) {
        const int level = map[idx];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = rintf((float)rgb[idx * 3 + c] + alpha * (float)table[level * 3 + c]);
            out[idx * 3 + c] = (uint8_t)fminf(fmaxf(v, 0.f), 255.f);
        }
    }
}

inline unsigned cam_grid(long total) {
    long g = (total + 255) / 256;
    if (g > 256L * 32) g = 256L * 32;
    if (g < 1) g = 1;
    return (unsigned)g;
}

}  // namespace

extern "C" int vip_cam_f32(const void* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias, float* cam,
                           float* peak, float* z, int B, int HW, int C, int ldx, long img_stride, int N, int act, int target,
                           void* stream) {
    return cam_impl<CF16, 8>("vip_cam_f32", x, gamma, beta, eps, W, bias, cam, peak, z, B, HW, C, ldx, img_stride, N, act, target, stream);
}

extern "C" int vip_cam_s32(const float* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias, float* cam,
                           float* peak, float* z, int B, int HW, int C, int ldx, long img_stride, int N, int act, int target,
                           void* stream) {
    return cam_impl<CF32, 4>("vip_cam_s32", x, gamma, beta, eps, W, bias, cam, peak, z, B, HW, C, ldx, img_stride, N, act, target, stream);
}

extern "C" int vip_cam_h2(const void* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias, float* cam,
                          float* peak, float* z, int B, int HW, int C, int ldx, long img_stride, int N, int act, int target,
                          void* stream) {
    return cam_impl<CH2, 8>("vip_cam_h2", x, gamma, beta, eps, W, bias, cam, peak, z, B, HW, C, ldx, img_stride, N, act, target, stream);
}

extern "C" int vip_cam_compose_f32(const float* const* maps_h, const int* grid_h_h, const int* grid_w_h, const float* const* peaks_h,
                                   const float* weights_h, int members, const int32_t* sizes_hw, int n, int maxH, int maxW, void* out,
                                   int out_u8, void* stream) {
    VIP_REQUIRE(maps_h && grid_h_h && grid_w_h && peaks_h && weights_h && sizes_hw && out, VIP_ERR_BAD_ARG,
                "vip_cam_compose_f32: null pointer");
    VIP_REQUIRE(members > 0 && members <= CAM_MAX_MEMBERS, VIP_ERR_BAD_ARG, "vip_cam_compose_f32: %d members (1 .. %d)", members,
                CAM_MAX_MEMBERS);
    VIP_REQUIRE(n > 0 && maxH > 0 && maxW > 0 && (out_u8 == 0 || out_u8 == 1), VIP_ERR_BAD_ARG, "vip_cam_compose_f32: bad dimension");
    ComposeArgs a;
    a.M = members;
    for (int m = 0; m < CAM_MAX_MEMBERS; ++m) {
        const bool on = m < members;
        VIP_REQUIRE(!on || (maps_h[m] && peaks_h[m] && grid_h_h[m] > 0 && grid_w_h[m] > 0 && grid_h_h[m] <= 4096 && grid_w_h[m] <= 4096),
                    VIP_ERR_BAD_ARG, "vip_cam_compose_f32: member %d: null map / peak or a grid outside 1 .. 4096", m);
        a.map[m] = on ? maps_h[m] : nullptr;
        a.peak[m] = on ? peaks_h[m] : nullptr;
        a.gh[m] = on ? grid_h_h[m] : 0;
        a.gw[m] = on ? grid_w_h[m] : 0;
        a.weight[m] = on ? weights_h[m] : 0.f;
    }
    const long total = (long)n * maxH * maxW;
    if (out_u8)
        hipLaunchKernelGGL(cam_compose_kernel<true>, dim3(cam_grid(total)), dim3(256), 0, (hipStream_t)stream, a, sizes_hw, n, maxH, maxW, out);
    else
        hipLaunchKernelGGL(cam_compose_kernel<false>, dim3(cam_grid(total)), dim3(256), 0, (hipStream_t)stream, a, sizes_hw, n, maxH, maxW, out);
    return vip_launch_status("vip_cam_compose_f32");
}

extern "C" int vip_cam_overlay_u8(const uint8_t* rgb_u8, const uint8_t* map_u8, const uint8_t* table_u8, float alpha, int n, int maxH,
                                  int maxW, uint8_t* out_u8, void* stream) {
    VIP_REQUIRE(rgb_u8 && map_u8 && table_u8 && out_u8, VIP_ERR_BAD_ARG, "vip_cam_overlay_u8: null pointer");
    VIP_REQUIRE(n > 0 && maxH > 0 && maxW > 0 && alpha >= 0.f && alpha <= 16.f, VIP_ERR_BAD_ARG, "vip_cam_overlay_u8: bad dimension or alpha");
    const long pixels = (long)n * maxH * maxW;
    hipLaunchKernelGGL(cam_overlay_kernel, dim3(cam_grid(pixels)), dim3(256), 0, (hipStream_t)stream, rgb_u8, map_u8, table_u8, alpha, pixels,
                       out_u8);
    return vip_launch_status("vip_cam_overlay_u8");
}
