// Fused two-layer MLP   y = W2 . act(W1 . x + b1) + b2 (+ residual)   for narrow token widths (C = 64 / 96 / 128 / 192).
//
// Replaces the Dense -> GELU -> Dense (+Add) tail of tfimm's ConvNeXtBlock (convnext.py:200-229, layer-scale gamma
// folded into W2/b2 by the host) and of the GCViT / ViT MLP (gcvit/layers/feature.py:20-22,
// tfimm/layers/transformers.py:192-205) where the hidden tensor [M, 4C] would otherwise be written to HBM by one GEMM
// and read back by the next: at ConvNeXt stage 0 (M = 2.5 M tokens, C = 96) that round trip is 3.9 GB per block
// against 1.4 GB for x + residual + y.
//
// Structure (same operand routing as pw_gemm_kernel in conv_igemm.hip):
//   * BOTH weight matrices live in LDS for the whole kernel (fragment-ordered rows, row stride 32 mod 64 bytes:
//     conflict-free ds_read_b128); 159 KB for C = 96 / hidden 384, so one workgroup per CU
//     (16 waves);
//   * a wave owns 32 tokens: their activation fragments (the MFMA B operand: lane = token, 8 consecutive channels =
//     one 16-byte run of the row) are loaded global -> VGPR once per tile;
//   * the hidden layer is produced 32 channels at a time: H^T = W1 X^T (bias as the MFMA C operand), activation in
//     packed fp32, and - because the weight rows are interleaved so that a lane ends up holding 8 CONSECUTIVE hidden
//     channels of its token - the fp16-packed result already IS the B operand of the second GEMM's k-step; it never
//     leaves the register file;
//   * y accumulates in registers over the 12 hidden slices and goes out with the residual in 16-byte stores.
#include "common.hpp"
#include "frag.hpp"

namespace {

struct MlpArgs {
    const f16* x;
    const f16* w1;
    const float* b1;
    const f16* w2;
    const float* b2;
    const f16* res;
    f16* y;
    const float* ln_g;   // optional LayerNorm over C applied to x first (NULL: none)
    const float* ln_b;
    float ln_eps;
    int M, Hd;
    int ldx, ldy, ldr, ldw1, ldw2;
    long x_bytes, y_bytes, res_bytes;
    int s1, s2;      // LDS row strides (bytes) of W1 [Hd rows] and W2 [C rows]
    int n_tiles;     // tiles of 512 tokens
};

// LDS row stride for `chunks` 16-byte chunks: == 32 (mod 64) bytes, conflict-free for the fragment read pattern under
// the ds_read_b128 lane grouping (see plan_pw in conv_igemm.hip).  The kernels take the strides that depend on C alone
// from here at compile time (row offsets become instruction immediates), the launchers take all of them from here.
__host__ __device__ constexpr int mlp_stride(int chunks) {
    while ((chunks & 3) != 2) ++chunks;
    return chunks * 16;
}

template <int CK, int ACT, int PT>
__global__ __launch_bounds__(2048 / PT, 1) void mlp_fused_kernel(MlpArgs a) {
    constexpr int C = 32 * CK, NCT = C / 16, NTHR = 2048 / PT;   // 512 tokens per workgroup: 8 waves x 64 or 16 x 32
    constexpr int S1 = mlp_stride(C / 8);                        // == a.s1
    // read each weight fragment one ahead of its MFMAs (8 more registers).  C = 64: 134 against 139 us at GCViT level 0,
    // every round ahead.  C = 96 (126 registers, still four waves per SIMD): 656 against 666 us in the median at ConvNeXt-T
    // stage 0, but one round of twelve tied, so by the keep rule of DESIGN.md section 3 it stays as it was
    constexpr bool AHEAD = CK != 3;
    constexpr unsigned OOB = 0xFFFFFFF0u;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* w1s = smem;
    char* w2s = smem + a.Hd * S1;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;

    // Every row of the two images ends in a 32-byte pad (mlp_stride: the conflict-free stride), eight floats.  The small
    // vectors live there, so that a tile needs no vector-memory instruction between its x loads and its residual loads:
    //   W1 row 32 q + i (i < 4): b1[32 q + 8 i ..+7]   - the two C-operand reads of slice q for the lanes with lq = i
    //   W2 row i: b2[8 i ..+7];  row C/8 + i: gamma[8 i ..+7];  row C/4 + i: beta[8 i ..+7]      (i < C/8)
    // (a NULL bias is staged as zeros)
    char* b1p = w1s + 2 * C;
    char* b2p = w2s + 2 * a.Hd;
    char* lgp = b2p + (C / 8) * a.s2;
    char* lbp = lgp + (C / 8) * a.s2;
    {   // stage both weight matrices and the small vectors (once per workgroup)
        const __amdgpu_buffer_rsrc_t rb1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.b1, 0, a.b1 ? (unsigned)(a.Hd * 4) : 0u, 0x00020000);
        const __amdgpu_buffer_rsrc_t rb2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.b2, 0, a.b2 ? (unsigned)(C * 4) : 0u, 0x00020000);
        for (int i = tid; i < a.Hd; i += NTHR)
            *reinterpret_cast<float*>(b1p + ((i & ~31) + ((i >> 3) & 3)) * S1 + (i & 7) * 4) =
                __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb1, (unsigned)(i * 4), 0, 0));
        for (int i = tid; i < C; i += NTHR) {
            *reinterpret_cast<float*>(b2p + (i >> 3) * a.s2 + (i & 7) * 4) =
                __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb2, (unsigned)(i * 4), 0, 0));
            if (a.ln_g) {
                *reinterpret_cast<float*>(lgp + (i >> 3) * a.s2 + (i & 7) * 4) = a.ln_g[i];
                *reinterpret_cast<float*>(lbp + (i >> 3) * a.s2 + (i & 7) * 4) = a.ln_b[i];
            }
        }
        const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w1, 0, (unsigned)(2L * a.Hd * a.ldw1), 0x00020000);
        const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w2, 0, (unsigned)(2L * C * a.ldw2), 0x00020000);
        constexpr int cpr1 = CK * 4;
        for (int i = tid; i < a.Hd * cpr1; i += NTHR) {
            const int j = i / cpr1, c = i - j * cpr1;
            const uint4 v = __builtin_bit_cast(
                uint4, __builtin_amdgcn_raw_buffer_load_b128(r1, (unsigned)((frag_channel(j) * a.ldw1 + c * 8) * 2), 0, 0));
            *reinterpret_cast<uint4*>(w1s + j * S1 + c * 16) = v;
        }
        const int cpr2 = a.Hd >> 3;
        for (int i = tid; i < C * cpr2; i += NTHR) {
            const int j = i / cpr2, c = i - j * cpr2;
            const uint4 v = __builtin_bit_cast(
                uint4, __builtin_amdgcn_raw_buffer_load_b128(r2, (unsigned)((frag_channel(j) * a.ldw2 + c * 8) * 2), 0, 0));
            *reinterpret_cast<uint4*>(w2s + j * a.s2 + c * 16) = v;
        }
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (unsigned)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)a.res, 0, a.res ? (unsigned)a.res_bytes : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, (unsigned)a.y_bytes, 0x00020000);
    const char* w1l = w1s + l15 * S1 + lq * 16;
    const char* w2l = w2s + l15 * a.s2 + lq * 16;
    const char* b1l = b1p + lq * S1;
    const int nq = a.Hd >> 5;

    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int m0 = tile * 512 + wave * (16 * PT);
        U4H8 xf[CK][PT];
#pragma unroll
        for (int ks = 0; ks < CK; ++ks)
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                const int m = m0 + p * 16 + l15;
                xf[ks][p].u = __builtin_bit_cast(
                    uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, m < a.M ? (unsigned)((m * a.ldx + ks * 32 + lq * 8) * 2) : OOB, 0, 0));
            }
        // the tile head's LDS addresses are made from an opaque copy of lq: hipcc otherwise keeps every one of them in a
        // register of its own across the slice loop, and C = 96 (128 registers, four waves per SIMD) spills
        int lqh = lq;
        asm volatile("" : "+v"(lqh));
        if (a.ln_g) {   // workgroup-uniform
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                U4H8 col[CK];
#pragma unroll
                for (int ks = 0; ks < CK; ++ks) col[ks] = xf[ks][p];
                ln_fragments<CK>(col, lgp, lbp, a.s2, a.ln_eps, lqh);
#pragma unroll
                for (int ks = 0; ks < CK; ++ks) xf[ks][p] = col[ks];
            }
        }
        // y accumulators start at b2 (lane: channels 32*hh + 8*lq + 4*t + 0..3 for tile 2*hh + t)
        f32x4 acc2[NCT][PT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(b2p + ((ct >> 1) * 4 + lqh) * a.s2 + (ct & 1) * 16);
#pragma unroll
            for (int p = 0; p < PT; ++p) acc2[ct][p] = bv;
        }

        // hidden slice q: H^T[32 x 64 tokens] = W1[32q.., :] . X^T + b1
        U4H8 wf[2];
        auto gemm1 = [&](int q, f32x4 (&acc1)[2][PT]) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                // b1 from the pad of W1 row 32 q + lq (4 distinct addresses per wave, rows apart: no bank conflict)
                const f32x4 bv = *reinterpret_cast<const f32x4*>(b1l + q * 32 * S1 + t * 16);
#pragma unroll
                for (int p = 0; p < PT; ++p) acc1[t][p] = bv;
            }
            // AHEAD: weight fragments are read one ahead of their MFMAs (two register sets): fragment f = 2 ks + t of W1,
            // then W2's first fragment in front of the activation
            auto rd1 = [&](int f) { return *reinterpret_cast<const uint4*>(w1l + (q * 32 + (f & 1) * 16) * S1 + (f >> 1) * 64); };
            if constexpr (AHEAD) wf[0].u = rd1(0);
#pragma unroll
            for (int f = 0; f < 2 * CK; ++f) {
                const int ks = f >> 1, t = f & 1, g = f + 1;
                if constexpr (AHEAD) wf[g & 1].u = g < 2 * CK ? rd1(g) : *reinterpret_cast<const uint4*>(w2l + q * 64);
                else wf[f & 1].u = rd1(f);
#pragma unroll
                for (int p = 0; p < PT; ++p)
                    acc1[t][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[f & 1].h, xf[ks][p].h, acc1[t][p], 0, 0, 0);
            }
        };
        // activation; the packed result is the B operand (k = 8*lq + j <-> hidden channel 32q + 8*lq + j)
        auto act_pack = [&](const f32x4 (&acc1)[2][PT], U4H8 (&hf)[PT]) {
#pragma unroll
            for (int p = 0; p < PT; ++p)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int j = 0; j < 4; j += 2) {
                        const f32x2 v = vip_act2<ACT>((f32x2){acc1[t][p][j], acc1[t][p][j + 1]});
                        hf[p].e[t * 4 + j] = (f16)v.x;
                        hf[p].e[t * 4 + j + 1] = (f16)v.y;
                    }
        };
        // y^T += W2[:, 32q..32q+31] . H
        auto gemm2 = [&](int q, const U4H8 (&hf)[PT]) {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                if constexpr (!AHEAD) wf[ct & 1].u = *reinterpret_cast<const uint4*>(w2l + ct * 16 * a.s2 + q * 64);
                else if (ct + 1 < NCT) wf[(ct + 1) & 1].u = *reinterpret_cast<const uint4*>(w2l + (ct + 1) * 16 * a.s2 + q * 64);
#pragma unroll
                for (int p = 0; p < PT; ++p)
                    acc2[ct][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ct & 1].h, hf[p].h, acc2[ct][p], 0, 0, 0);
            }
        };
        // (Issuing slice q+1's first-layer MFMAs before slice q's activation - a two-slice software pipeline - was
        // measured 6 % SLOWER: +42 VGPRs and no overlap gained; the second resident wave already fills the gaps.)
        U4H8 hf[PT];
#pragma unroll 1
        for (int q = 0; q < nq; ++q) {
            f32x4 h0[2][PT];
            gemm1(q, h0);
            act_pack(h0, hf);
            gemm2(q, hf);
        }

        // epilogue: + residual, fp16, 16-byte stores (lane: token m, channels 32*hh + 8*lq .. +7)
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            const int m = m0 + p * 16 + l15;
            const bool ok = m < a.M;
#pragma unroll
            for (int hh = 0; hh < CK; ++hh) {
                const int n = hh * 32 + lq * 8;
                U4H8 r;
                r.u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                                    rr, ok ? (unsigned)((m * a.ldr + n) * 2) : OOB, 0, 0));
                U4H8 o;
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    const f32x4 av = acc2[2 * hh + (j >> 2)][p];
                    const f32x2 v = (f32x2){av[j & 3], av[(j & 3) + 1]} + (f32x2){(float)r.e[j], (float)r.e[j + 1]};
                    o.e[j] = (f16)v.x;
                    o.e[j + 1] = (f16)v.y;
                }
                __builtin_amdgcn_raw_buffer_store_b128(
                    __builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, o.u), ry,
                    ok ? (unsigned)((m * a.ldy + n) * 2) : OOB, 0, 0);
            }
        }
    }
}

// compute units of the current device (256 when it cannot be asked)
static int mlp_cu_count() {
    static int n_cu = 0;
    if (!n_cu) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
        if (n_cu <= 0) n_cu = 256;
    }
    return n_cu;
}

// Launch geometry of both kernels, the one place it is computed: the launchers below and the dry run vip_mlp_fused_plan() read it.
struct MlpPlan {
    int s1, s2;      // LDS row strides (bytes)
    size_t smem;     // dynamic LDS bytes
    int tile;        // tokens per tile
    int n_tiles;     // work units
    int grid;        // workgroups that walk them (tile += gridDim.x)
};

// LDS-resident weights (C = 64 / 96): 512-token tiles, one workgroup per CU; false when the two matrices do not fit
static bool mlp_plan_resident(int C, int M, int Hd, MlpPlan& p) {
    p.s1 = mlp_stride(C / 8);
    p.s2 = mlp_stride(Hd >> 3);
    p.smem = (size_t)Hd * p.s1 + (size_t)C * p.s2;
    if (p.smem > 160 * 1024 || p.s1 - 2 * C < 32 || p.s2 - 2 * Hd < 32) return false;   // the row pads hold b1, b2, gamma and beta
    p.tile = 512;
    p.n_tiles = (M + 511) / 512;
    const int n_cu = mlp_cu_count();
    p.grid = p.n_tiles < n_cu ? p.n_tiles : n_cu;
    return true;
}

// streamed weights (C = 128 / 192 / 256): 256-token tiles, one workgroup per CU.  LDS: the two weight stages, behind them b1 [Hd]
// and b2 [C] in fp32; false when that does not fit (a hidden width past 24 000 at C = 192)
static size_t mlp_stream_lds(int C, int Hd) {
    return 2 * ((size_t)32 * mlp_stride(C / 8) + (size_t)C * mlp_stride(4)) + 4 * ((size_t)Hd + (size_t)C);
}

static bool mlp_plan_stream(int C, int M, int Hd, MlpPlan& p) {
    p.s1 = mlp_stride(C / 8);
    p.s2 = mlp_stride(4);
    p.smem = mlp_stream_lds(C, Hd);
    if (p.smem > 160 * 1024) return false;
    p.tile = 256;
    p.n_tiles = (M + 255) / 256;
    const int n_cu = mlp_cu_count();
    p.grid = p.n_tiles < n_cu ? p.n_tiles : n_cu;
    return true;
}

template <int CK>
int launch_mlp(MlpArgs a, hipStream_t s) {
    MlpPlan p;
    if (!mlp_plan_resident(32 * CK, a.M, a.Hd, p)) return 1;
    a.s1 = p.s1;
    a.s2 = p.s2;
    a.n_tiles = p.n_tiles;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_fused_kernel<CK, VIP_ACT_GELU, 2>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    // 16 waves x 32 tokens (<= 128 VGPRs, four waves per SIMD) measured 2-8 % ahead of 8 waves x 64 tokens
    hipLaunchKernelGGL((mlp_fused_kernel<CK, VIP_ACT_GELU, 2>), dim3(p.grid), dim3(1024), p.smem, s, a);
    return vip_launch_status("vip_mlp_fused_f16");
}


// ---- C = 128 / 192: the two weight matrices (4C x C and C x 4C) no longer fit in LDS together, so they are STREAMED:
// per 32-channel hidden slice the workgroup stages W1[32q.., :] and W2[:, 32q..] (24 KB at C = 192) into a
// double-buffered LDS image, one barrier per slice, while x (32 tokens per wave, 8 waves) and the y accumulators stay in
// registers for all 4C/32 slices.  The weights come from L2 (2.3 KB per token at C = 192 against 1.15 KB of HBM traffic);
// the hidden tensor never exists in memory.
// The slice loop's only vector-memory instructions are the loads of the NEXT slice's weights, issued at the head of the
// slice into named registers and first waited for after the slice's last MFMA, directly in front of the ds_write into the
// other stage: both biases are staged once per workgroup into LDS (fp32, behind the two stages) and read from there, so
// that no later load stands in the in-order vmcnt queue between the prefetch and its use.
// The staging values are named scalars, not an array: hipcc leaves `uint4 wst[W_IT]` on the stack (48 / 64 bytes of
// scratch per lane at C = 128 / 192, a second memory round trip per slice).  W_IT = 4 (C = 256, built but not offered by
// vip_mlp_fused_supported) runs out of registers and may keep scratch.
template <int CK, int ACT>
__global__ __launch_bounds__(512, 1) void mlp_stream_kernel(MlpArgs a) {
    constexpr int C = 32 * CK, PT = 2, NCT = C / 16, NTHR = 512;
    constexpr int W_IT = C / 64;                    // 16-byte weight chunks staged per thread per slice (8C / 512)
    static_assert(W_IT >= 1 && W_IT <= 4, "staging registers are named for up to four chunks");
    constexpr unsigned OOB = 0xFFFFFFF0u;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int S1 = mlp_stride(C / 8), S2 = mlp_stride(4);   // == a.s1, a.s2
    constexpr int stage_bytes = 32 * S1 + C * S2;   // W1 slice [32][S1] then W2 slice [C][S2]
    float* b1s = reinterpret_cast<float*>(smem + 2 * stage_bytes);   // b1 [Hd] then b2 [C] (zeros for a NULL bias)
    float* b2s = b1s + a.Hd;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (unsigned)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)a.res, 0, a.res ? (unsigned)a.res_bytes : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, (unsigned)a.y_bytes, 0x00020000);
    {
        const __amdgpu_buffer_rsrc_t rb1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.b1, 0, a.b1 ? (unsigned)(a.Hd * 4) : 0u, 0x00020000);
        const __amdgpu_buffer_rsrc_t rb2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.b2, 0, a.b2 ? (unsigned)(C * 4) : 0u, 0x00020000);
        for (int i = tid; i < a.Hd; i += NTHR)
            b1s[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb1, (unsigned)(i * 4), 0, 0));
        for (int i = tid; i < C; i += NTHR)
            b2s[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb2, (unsigned)(i * 4), 0, 0));
    }

    // staging plan of this thread: chunk idx = tid + 512 i; the first 4C chunks are the W1 slice, the rest the W2 slice.
    // Plain pointers (one load instruction per chunk whichever matrix it comes from: a `is_w1 ? load(w1) : load(w2)`
    // would be two predicated loads with a wait each); they RUN: each stands on the slice to be loaded next and is
    // advanced by its step, or taken back to slice 0 after the last slice
    const char *wp0 = nullptr, *wp1 = nullptr, *wp2 = nullptr, *wp3 = nullptr;   // source of the next slice
    unsigned ws0 = 0, ws1 = 0, ws2 = 0, ws3 = 0;                                 // bytes between consecutive slices
    int wd0 = 0, wd1 = 0, wd2 = 0, wd3 = 0;                                      // byte offset inside a stage
    auto plan_w = [&](int i, const char*& wp, unsigned& ws, int& wd) {
        const int idx = tid + NTHR * i;
        if (idx < 4 * C) {
            const int row = idx / (C / 8), c = idx - row * (C / 8);
            wp = reinterpret_cast<const char*>(a.w1) + ((long)frag_channel(row) * a.ldw1 + c * 8) * 2;
            ws = (unsigned)(32 * a.ldw1 * 2);
            wd = row * S1 + c * 16;
        } else {
            const int j = idx - 4 * C, row = j >> 2, c = j & 3;
            wp = reinterpret_cast<const char*>(a.w2) + ((long)frag_channel(row) * a.ldw2 + c * 8) * 2;
            ws = 64u;
            wd = 32 * S1 + row * S2 + c * 16;
        }
    };
    plan_w(0, wp0, ws0, wd0);
    if constexpr (W_IT > 1) plan_w(1, wp1, ws1, wd1);
    if constexpr (W_IT > 2) plan_w(2, wp2, ws2, wd2);
    if constexpr (W_IT > 3) plan_w(3, wp3, ws3, wd3);
    const int nq = a.Hd >> 5;
    uint4 wn0, wn1, wn2, wn3;   // the next slice's chunks, in flight from the head of a slice to its tail
    int nxt = 0;                // the slice the pointers stand on
    // issue the loads of slice `nxt`, then move the pointers on
    auto load_w = [&]() {
        wn0 = *reinterpret_cast<const uint4*>(wp0);
        if constexpr (W_IT > 1) wn1 = *reinterpret_cast<const uint4*>(wp1);
        if constexpr (W_IT > 2) wn2 = *reinterpret_cast<const uint4*>(wp2);
        if constexpr (W_IT > 3) wn3 = *reinterpret_cast<const uint4*>(wp3);
        const bool wrap = nxt + 1 >= nq;    // workgroup-uniform
        auto adv = [&](const char*& wp, unsigned ws) { wp += wrap ? -(long)(ws * (unsigned)nxt) : (long)ws; };
        adv(wp0, ws0);
        if constexpr (W_IT > 1) adv(wp1, ws1);
        if constexpr (W_IT > 2) adv(wp2, ws2);
        if constexpr (W_IT > 3) adv(wp3, ws3);
        nxt = wrap ? 0 : nxt + 1;
    };
    auto store_w = [&](int buf) {
        char* st = smem + buf * stage_bytes;
        *reinterpret_cast<uint4*>(st + wd0) = wn0;
        if constexpr (W_IT > 1) *reinterpret_cast<uint4*>(st + wd1) = wn1;
        if constexpr (W_IT > 2) *reinterpret_cast<uint4*>(st + wd2) = wn2;
        if constexpr (W_IT > 3) *reinterpret_cast<uint4*>(st + wd3) = wn3;
    };

    load_w();
    store_w(0);
    __syncthreads();
    int buf = 0;
    const float* b1l = b1s + lq * 8;
    const float* b2l = b2s + lq * 8;

    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int m0 = tile * (NTHR / 64 * 16 * PT) + wave * (16 * PT);
        U4H8 xf[CK][PT];
#pragma unroll
        for (int ks = 0; ks < CK; ++ks)
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                const int m = m0 + p * 16 + l15;
                xf[ks][p].u = __builtin_bit_cast(
                    uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, m < a.M ? (unsigned)((m * a.ldx + ks * 32 + lq * 8) * 2) : OOB, 0, 0));
            }
        if (a.ln_g) {   // workgroup-uniform
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                U4H8 col[CK];
#pragma unroll
                for (int ks = 0; ks < CK; ++ks) col[ks] = xf[ks][p];
                ln_fragments<CK>(col, reinterpret_cast<const char*>(a.ln_g), reinterpret_cast<const char*>(a.ln_b), 32, a.ln_eps, lq);
#pragma unroll
                for (int ks = 0; ks < CK; ++ks) xf[ks][p] = col[ks];
            }
        }
        // y accumulators start at b2 (lane: channels 32*hh + 8*lq + 4*t + 0..3 for tile 2*hh + t)
        f32x4 acc2[NCT][PT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(b2l + (ct >> 1) * 32 + (ct & 1) * 4);
#pragma unroll
            for (int p = 0; p < PT; ++p) acc2[ct][p] = bv;
        }

#pragma unroll 1
        for (int q = 0; q < nq; ++q) {
            load_w();                                // next slice (slice 0 of the next tile after the last one)
            __builtin_amdgcn_sched_barrier(0);
            const char* w1l = smem + buf * stage_bytes + l15 * S1 + lq * 16;
            const char* w2l = w1l + 32 * S1 + l15 * (S2 - S1);
            f32x4 acc1[2][PT];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const f32x4 bv = *reinterpret_cast<const f32x4*>(b1l + q * 32 + t * 4);
#pragma unroll
                for (int p = 0; p < PT; ++p) acc1[t][p] = bv;
            }
            // weight fragments are read one ahead of their MFMAs (two registers sets): fragment f = 2 ks + t of W1, then
            // W2's first fragment in front of the activation
            U4H8 wf[2];
            wf[0].u = *reinterpret_cast<const uint4*>(w1l);
#pragma unroll
            for (int f = 0; f < 2 * CK; ++f) {
                const int ks = f >> 1, t = f & 1, g = f + 1;
                wf[g & 1].u = g < 2 * CK ? *reinterpret_cast<const uint4*>(w1l + (g & 1) * 16 * S1 + (g >> 1) * 64)
                                         : *reinterpret_cast<const uint4*>(w2l);
#pragma unroll
                for (int p = 0; p < PT; ++p)
                    acc1[t][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[f & 1].h, xf[ks][p].h, acc1[t][p], 0, 0, 0);
            }
            U4H8 hf[PT];
#pragma unroll
            for (int p = 0; p < PT; ++p)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int j = 0; j < 4; j += 2) {
                        const f32x2 v = vip_act2<ACT>((f32x2){acc1[t][p][j], acc1[t][p][j + 1]});
                        hf[p].e[t * 4 + j] = (f16)v.x;
                        hf[p].e[t * 4 + j + 1] = (f16)v.y;
                    }
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                if (ct + 1 < NCT) wf[(ct + 1) & 1].u = *reinterpret_cast<const uint4*>(w2l + (ct + 1) * 16 * S2);
#pragma unroll
                for (int p = 0; p < PT; ++p)
                    acc2[ct][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ct & 1].h, hf[p].h, acc2[ct][p], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            store_w(buf ^ 1);                        // the first wait for the prefetch: after the slice's last MFMA
            __syncthreads();
            buf ^= 1;
        }

#pragma unroll
        for (int p = 0; p < PT; ++p) {
            const int m = m0 + p * 16 + l15;
            const bool ok = m < a.M;
#pragma unroll
            for (int hh = 0; hh < CK; ++hh) {
                const int n = hh * 32 + lq * 8;
                U4H8 r;
                r.u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                                    rr, ok ? (unsigned)((m * a.ldr + n) * 2) : OOB, 0, 0));
                U4H8 o;
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    const f32x4 av = acc2[2 * hh + (j >> 2)][p];
                    const f32x2 v = (f32x2){av[j & 3], av[(j & 3) + 1]} + (f32x2){(float)r.e[j], (float)r.e[j + 1]};
                    o.e[j] = (f16)v.x;
                    o.e[j + 1] = (f16)v.y;
                }
                __builtin_amdgcn_raw_buffer_store_b128(
                    __builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, o.u), ry,
                    ok ? (unsigned)((m * a.ldy + n) * 2) : OOB, 0, 0);
            }
        }
    }
}

template <int CK>
int launch_mlp_stream(MlpArgs a, hipStream_t s) {
    MlpPlan p;
    if (!mlp_plan_stream(32 * CK, a.M, a.Hd, p)) return 1;
    a.s1 = p.s1;
    a.s2 = p.s2;
    a.n_tiles = p.n_tiles;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_stream_kernel<CK, VIP_ACT_GELU>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    hipLaunchKernelGGL((mlp_stream_kernel<CK, VIP_ACT_GELU>), dim3(p.grid), dim3(512), p.smem, s, a);
    return vip_launch_status("vip_mlp_fused_f16(stream)");
}

}  // namespace

extern "C" int vip_mlp_fused_supported(int M, int C, int hidden, int act) {
    if (act != VIP_ACT_GELU || hidden % 32 != 0 || hidden <= 0 || M < 8192) return 0;
    if (C == 192)             // streamed weights (C = 128 and 256 are wired up too but measured slower than two GEMMs)
        return mlp_stream_lds(C, hidden) <= 160 * 1024;
    if (C != 64 && C != 96) return 0;
    const long s1 = mlp_stride(C / 8), s2 = mlp_stride(hidden >> 3);      // LDS-resident weights
    return (long)hidden * s1 + (long)C * s2 <= 160 * 1024;
}

extern "C" int vip_mlp_fused_plan(int M, int C, int hidden, int act, int* workgroups, int* tile_rows) {
    if (!vip_mlp_fused_supported(M, C, hidden, act)) return 0;
    MlpPlan p;
    if (C == 192) {
        if (!mlp_plan_stream(C, M, hidden, p)) return 0;
    } else if (!mlp_plan_resident(C, M, hidden, p)) return 0;
    if (workgroups) *workgroups = p.grid;
    if (tile_rows) *tile_rows = p.tile;
    return p.n_tiles;
}

extern "C" int vip_mlp_fused_f16(const void* x, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* w1,
                                 const float* b1, const void* w2, const float* b2, const void* residual, void* y, int M,
                                 int C, int hidden, int ldx, int ldw1, int ldw2, int ldy, int ldr, int act, void* stream) {
    VIP_REQUIRE(x && w1 && w2 && y, VIP_ERR_BAD_ARG, "vip_mlp_fused_f16: null pointer");
    VIP_REQUIRE((ln_gamma == nullptr) == (ln_beta == nullptr), VIP_ERR_BAD_ARG,
                "vip_mlp_fused_f16: ln_gamma and ln_beta must both be given or both be NULL");
    VIP_REQUIRE(M > 0 && C > 0 && hidden > 0, VIP_ERR_BAD_ARG, "vip_mlp_fused_f16: non-positive dimension");
    VIP_REQUIRE(vip_mlp_fused_supported(M, C, hidden, act), VIP_ERR_UNSUPPORTED,
                "vip_mlp_fused_f16: unsupported shape/activation (C=%d hidden=%d act=%d M=%d); use two vip_gemm_bias_act_f16 calls",
                C, hidden, act, M);
    VIP_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0 && ldw1 % 8 == 0 && ldw2 % 8 == 0 && (!residual || ldr % 8 == 0),
                VIP_ERR_ALIGNMENT, "vip_mlp_fused_f16: leading dimensions must be multiples of 8 halfs");
    VIP_REQUIRE(ldx >= C && ldy >= C && ldw1 >= C && ldw2 >= hidden && (!residual || ldr >= C), VIP_ERR_BAD_ARG,
                "vip_mlp_fused_f16: leading dimension smaller than the row extent");
    MlpArgs a;
    a.x = (const f16*)x; a.w1 = (const f16*)w1; a.b1 = b1; a.w2 = (const f16*)w2; a.b2 = b2;
    a.res = (const f16*)residual; a.y = (f16*)y;
    a.ln_g = ln_gamma; a.ln_b = ln_beta; a.ln_eps = ln_eps;
    a.M = M; a.Hd = hidden; a.ldx = ldx; a.ldy = ldy; a.ldr = ldr; a.ldw1 = ldw1; a.ldw2 = ldw2;
    a.x_bytes = 2L * M * ldx; a.y_bytes = 2L * M * ldy; a.res_bytes = 2L * M * ldr;
    VIP_REQUIRE(a.x_bytes < 0xFFFFFFF0L && a.y_bytes < 0xFFFFFFF0L && a.res_bytes < 0xFFFFFFF0L, VIP_ERR_UNSUPPORTED,
                "vip_mlp_fused_f16: tensor exceeds the 4 GiB buffer-addressing range");
    a.s1 = a.s2 = a.n_tiles = 0;
    int st = 1;
    if (C == 64) st = launch_mlp<2>(a, (hipStream_t)stream);
    else if (C == 96) st = launch_mlp<3>(a, (hipStream_t)stream);
    else if (C == 128) st = launch_mlp_stream<4>(a, (hipStream_t)stream);
    else if (C == 192) st = launch_mlp_stream<6>(a, (hipStream_t)stream);
    else if (C == 256) st = launch_mlp_stream<8>(a, (hipStream_t)stream);
    VIP_REQUIRE(st != 1, VIP_ERR_UNSUPPORTED, "vip_mlp_fused_f16: weights do not fit in LDS");
    return st;
}
