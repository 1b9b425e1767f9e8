// HorNet global-local filter (kecam hornet/hornet.py:53-81, the body between its two LayerNorms) as ONE launch on every storage:
//   y[b,h,w,2i]   = sum_{dy,dx in -1..1} w3[dy+1][dx+1][i] * x[b,h+dy,w+dx,i]                    (3x3 depthwise, zero padded, no bias)
//   y[b,h,w,2i+1] = sum_{a<H, c<W} g[a][c][i] * x[b,(h-a) mod H,(w-c) mod W, S/2 + i]             (circular depthwise, whole map)
// The second line IS irfft2(rfft2(x) * Wc, s=(H,W)): the map is real-linear and commutes with circular shifts, so it is a circular
// convolution with the real kernel g = irfft2(Wc, s=(H,W)), which the host builds once in float64 (ops.make_global_filter_weight).
// No twiddles, no complex arithmetic: every output is one fp32 sum of at most 256 products, rounded once on the store.
//
// One workgroup (one wave) = one image x QB = 64 / H quads of four channel pairs.  It stages the two channel slices of the map and the
// slice of g in LDS as fp32 (maps are at most 16 x 16), then lane (h, quad) owns output row h of its quad:
//   * W x 4 accumulators in registers; per tap row a it reads the W source pixels of row (h - a) mod H once and the W taps once -
//     2 W 16-byte LDS reads for 4 W^2 FMAs - and the circular column (w - c) mod W is a compile-time register index (W is a template
//     argument: 14, 7, 12, 6 are what the registered members produce);
//   * every other width (2 ... 16) takes the generic form, one LDS read pair per product: slower, same sums in the same order.
// Rows of the staged maps are padded so that the lanes of consecutive h fall into different LDS banks.  No atomics, no inline
// assembly; the order of every sum is fixed by (H, W) alone, so results do not depend on the batch or on the grid.
#include "common.hpp"

namespace {

// storage policies: ld = 4 consecutive logical channels i .. i+3 (i % 4 == 0), st8 = 8 consecutive channels i .. i+7 (i % 8 == 0)
struct GF16 {
    static __device__ __forceinline__ f32x4 ld(const void* b, long i) {
        const f16x4 v = *reinterpret_cast<const f16x4*>(static_cast<const f16*>(b) + i);
        return (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    }
    static __device__ __forceinline__ void st8(void* b, long i, const float (&v)[8], int*) {
        U4H8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.e[j] = (f16)v[j];
        *reinterpret_cast<uint4*>(static_cast<f16*>(b) + i) = o.u;
    }
};
struct GF32 {
    static __device__ __forceinline__ f32x4 ld(const void* b, long i) { return *reinterpret_cast<const f32x4*>(static_cast<const float*>(b) + i); }
    static __device__ __forceinline__ void st8(void* b, long i, const float (&v)[8], int*) {
        f32x4* o = reinterpret_cast<f32x4*>(static_cast<float*>(b) + i);
        o[0] = (f32x4){v[0], v[1], v[2], v[3]};
        o[1] = (f32x4){v[4], v[5], v[6], v[7]};
    }
};
struct GH2 {
    static __device__ __forceinline__ f32x4 ld(const void* b, long i) { return h2_ld4(b, i); }
    static __device__ __forceinline__ void st8(void* b, long i, const float (&v)[8], int* status) {
        U4H8 hi, lo;
        h2_split8(v, hi, lo);
        uint4* o = reinterpret_cast<uint4*>(static_cast<char*>(b) + (i >> 3) * 32);
        o[0] = hi.u;
        o[1] = lo.u;
        if (status && h2_overflows8(v)) *status = VIP_H2_OVERFLOW;
    }
};

constexpr int GF_LANES = 64;       // one wave per workgroup
constexpr int GF_MAX_HW = 16;
constexpr int GF_RING_MAX = 7;
constexpr int gf_ring(int W) { return W % 7 == 0 ? 7 : 6; }        // taps in flight of the register-blocked widths (14, 7 | 12, 6)

struct GfPlan {
    int qb;        // quads (four channel pairs = 8 channels of S) per workgroup
    int rs;        // float4 per staged map row (W * qb + padding)
    int blocks;    // workgroups per image
    size_t lds;    // bytes
};

// Lanes (h, q) and (h + 1, q) read addresses rs float4 apart: rs = +-qb (mod 16 float4 = 64 banks) keeps 16 consecutive lanes on 64
// different banks when qb divides 16, and spreads them otherwise.
inline GfPlan gf_plan(int H, int W, int S) {
    GfPlan p;
    p.qb = GF_LANES / H;
    const int base = W * p.qb;
    int pad = 16;
    for (int want : {p.qb % 16, (16 - p.qb % 16) % 16}) {
        const int d = ((want - base) % 16 + 16) % 16;
        if (d < pad) pad = d;
    }
    p.rs = base + pad;
    const int quads = S / 8;
    p.blocks = (quads + p.qb - 1) / p.qb;
    p.lds = (size_t)(2 * H * p.rs + (H * W + GF_RING_MAX) * p.qb) * sizeof(f32x4);     // + what the tap ring reads ahead of the last tap
    return p;
}

// W > 0: the register-blocked form for that width; W == 0: any width (Wrt) through LDS
template <typename S, int W>
__global__ __launch_bounds__(GF_LANES) void global_local_filter_kernel(const void* __restrict__ x, const float* __restrict__ w3,
                                                                       const float* __restrict__ g, void* __restrict__ y, int H, int Wrt,
                                                                       int Sc, int QB, int rs, int* status) {
    extern __shared__ f32x4 gf_lds[];
    const int Wd = W > 0 ? W : Wrt;
    const int half = Sc >> 1;
    f32x4* xl = gf_lds;                      // [H][rs]: local half, pixel (h, w) quad q at h * rs + w * QB + q
    f32x4* xg = xl + H * rs;                 // [H][rs]: global half
    f32x4* gs = xg + H * rs;                 // [H * Wd][QB]: taps
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * QB;
    const int nq = min(QB, (half >> 2) - q0);
    const int tid = threadIdx.x;
    const long img = (long)b * H * Wd;

    for (int idx = tid; idx < H * Wd * QB; idx += GF_LANES) {
        const int q = idx % QB, p = idx / QB;
        const int h = p / Wd, w = p - h * Wd;
        f32x4 vl = {0.f, 0.f, 0.f, 0.f}, vg = vl, vt = vl;
        if (q < nq) {
            const long e = (img + p) * Sc + (q0 + q) * 4;
            vl = S::ld(x, e);
            vg = S::ld(x, e + half);
            vt = *reinterpret_cast<const f32x4*>(g + (long)p * half + (q0 + q) * 4);
        }
        xl[h * rs + w * QB + q] = vl;
        xg[h * rs + w * QB + q] = vg;
        gs[idx] = vt;
    }
    __syncthreads();
    const int q = tid % QB, h = tid / QB;
    if (h >= H || q >= nq) return;

    f32x4 t3[9];                             // the quad's 3x3 taps (fp32 parameters, [3][3][half])
#pragma unroll
    for (int j = 0; j < 9; ++j) t3[j] = *reinterpret_cast<const f32x4*>(w3 + (long)j * half + (q0 + q) * 4);

    // local half of pixel (h, w), interleaved with the global value, one 8-channel store
    auto finish = [&](int w, f32x4 glob) {
        f32x4 loc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int hh = h + dy - 1;
            if ((unsigned)hh >= (unsigned)H) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int ww = w + dx - 1;
                if ((unsigned)ww < (unsigned)Wd) loc += t3[dy * 3 + dx] * xl[hh * rs + ww * QB + q];
            }
        }
        const float v[8] = {loc[0], glob[0], loc[1], glob[1], loc[2], glob[2], loc[3], glob[3]};
        S::st8(y, (img + h * Wd + w) * Sc + (long)(q0 + q) * 8, v, status);
    };

    if constexpr (W > 0) {
        f32x4 acc[W];
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // The wave is alone on its SIMD (LDS holds four workgroups per CU), so only its own reads in flight hide an LDS round trip: the
        // taps - one linear stream gs[a * W + c] - go through a ring of D registers, D taps ahead of their use (D divides W, so the
        // ring slot of tap c is a compile-time index; the last D reads fall into the D * QB entries the launcher leaves behind the
        // taps).  The source row is read at the top of its tap row: one exposed round trip per 4 W^2 FMAs.
        constexpr int D = gf_ring(W);
        f32x4 ring[D];
        const f32x4* tap = gs + q;
#pragma unroll
        for (int d = 0; d < D; ++d) ring[d] = tap[d * QB];
        int hs = h;                          // (h - a) mod H
#pragma unroll 1
        for (int a = 0; a < H; ++a) {
            f32x4 xr[W];
            const f32x4* src = xg + hs * rs + q;
#pragma unroll
            for (int w = 0; w < W; ++w) xr[w] = src[w * QB];
#pragma unroll
            for (int c = 0; c < W; ++c) {
                const f32x4 t = ring[c % D];
                ring[c % D] = tap[(c + D) * QB];
#pragma unroll
                for (int w = 0; w < W; ++w) acc[w] += t * xr[(w - c + W) % W];
            }
            tap += W * QB;
            hs = hs == 0 ? H - 1 : hs - 1;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) finish(w, acc[w]);
    } else {
        for (int w = 0; w < Wd; ++w) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            int hs = h;
            for (int a = 0; a < H; ++a) {
                const f32x4* src = xg + hs * rs + q;
                const f32x4* tap = gs + a * Wd * QB + q;
                int ws = w;                  // (w - c) mod W
                for (int c = 0; c < Wd; ++c) {
                    acc += tap[c * QB] * src[ws * QB];
                    ws = ws == 0 ? Wd - 1 : ws - 1;
                }
                hs = hs == 0 ? H - 1 : hs - 1;
            }
            finish(w, acc);
        }
    }
}

template <typename S>
int gf_impl(const char* who, const void* x, const float* w3, const float* g, void* y, int B, int H, int W, int Sc, int* status, void* stream) {
    VIP_REQUIRE(x && w3 && g && y, VIP_ERR_BAD_ARG, "%s: null pointer", who);
    VIP_REQUIRE(B > 0 && H > 0 && W > 0 && Sc > 0, VIP_ERR_BAD_ARG, "%s: non-positive dimension", who);
    VIP_REQUIRE(vip_global_local_filter_supported(H, W, Sc) == 1, VIP_ERR_UNSUPPORTED,
                "%s: unsupported map %d x %d with %d channels: needs 2 <= H, W <= %d (the map is held in LDS) and S %% 16 == 0", who, H, W,
                Sc, GF_MAX_HW);
    VIP_REQUIRE(B <= 65535, VIP_ERR_UNSUPPORTED, "%s: B=%d images (max 65535 per launch)", who, B);
    const GfPlan p = gf_plan(H, W, Sc);
    const dim3 grid(p.blocks, B), block(GF_LANES);
    hipStream_t s = (hipStream_t)stream;
#define GF_LAUNCH(WT) \
    hipLaunchKernelGGL((global_local_filter_kernel<S, WT>), grid, block, p.lds, s, x, w3, g, y, H, W, Sc, p.qb, p.rs, status)
    switch (W) {
        case 14: GF_LAUNCH(14); break;
        case 12: GF_LAUNCH(12); break;
        case 7: GF_LAUNCH(7); break;
        case 6: GF_LAUNCH(6); break;
        default: GF_LAUNCH(0); break;
    }
#undef GF_LAUNCH
    return vip_launch_status(who);
}

}  // namespace

extern "C" int vip_global_local_filter_supported(int H, int W, int S) {
    return (H >= 2 && H <= GF_MAX_HW && W >= 2 && W <= GF_MAX_HW && S > 0 && S % 16 == 0) ? 1 : 0;
}

extern "C" int vip_global_local_filter_plan(int H, int W, int S, int* block_channels, int* lds_bytes) {
    if (!vip_global_local_filter_supported(H, W, S)) return 0;
    const GfPlan p = gf_plan(H, W, S);
    if (block_channels) *block_channels = p.qb * 8;
    if (lds_bytes) *lds_bytes = (int)p.lds;
    return p.blocks;
}

extern "C" int vip_global_local_filter_nhwc_f16(const void* x, const float* w3, const float* g, void* y, int B, int H, int W, int S,
                                                void* stream) {
    return gf_impl<GF16>("vip_global_local_filter_nhwc_f16", x, w3, g, y, B, H, W, S, nullptr, stream);
}
extern "C" int vip_global_local_filter_nhwc_s32(const float* x, const float* w3, const float* g, float* y, int B, int H, int W, int S,
                                                void* stream) {
    return gf_impl<GF32>("vip_global_local_filter_nhwc_s32", x, w3, g, y, B, H, W, S, nullptr, stream);
}
extern "C" int vip_global_local_filter_nhwc_h2(const void* x, const float* w3, const float* g, void* y, int B, int H, int W, int S,
                                               int* status, void* stream) {
    return gf_impl<GH2>("vip_global_local_filter_nhwc_h2", x, w3, g, y, B, H, W, S, status, stream);
}
