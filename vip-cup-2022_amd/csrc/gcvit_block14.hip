// The GCViT attention half of a block in one launch for the 14 x 14-window level (C = 256, 8 heads of 32; level 2 of GCViT-Tiny:
// 19 of its 31 blocks):
//
//     y = x + proj( window_attention( qkv( LayerNorm(x) ) ) )            (gcvit/layers/block.py:58-79, attention.py:52-83)
//
// Same plan as gcvit_block.hip (weights through LDS, window state in registers, weight rows / columns interleaved so that one MFMA's
// packed result is the next one's operand), re-cut for a window of 196 tokens = 13 MFMA tiles:
//   * ONE workgroup of 8 waves per window; wave w owns token tiles w and w + 8 (five waves own two tiles, three own one): their x^
//     fragments stay in registers (64 VGPRs) for all heads;
//   * per head (loop NOT unrolled): the head's q | k | v weight rows (96 x 256, 51 KB) and its relative-position table are staged in
//     LDS; every wave computes q, k, v for its own tokens - q stays in registers, k and v go to the workgroup's K / V image in the
//     padded order row' = 16 ty + tx of window_core.hpp - then runs win_attn_tile of window_core.hpp on its own query tiles;
//   * the normalised head output O_h (8 halfs per lane and tile) is parked in the rows of y this lane will write anyway (the same 16
//     bytes it later overwrites with the result: a private scratch that costs no memory) - 8 heads of accumulators or outputs do not
//     fit next to the core in 256 registers;
//   * after the last head: proj weight columns of two heads at a time through the same LDS buffer, y^T += Wp O^T for both tiles from
//     the parked fragments, + bias + x, 16-byte stores.
// A block with a global query takes q from q_global [B, 196, C] and computes k, v only.
#include "window_core.hpp"
#include "frag.hpp"

namespace {

struct Gb14Args {
    const f16* x;
    const f16* qg;          // [B][196][C] or NULL
    const float* ln_g;
    const float* ln_b;
    float ln_eps;
    const f16* wqkv;        // [nq * C][ldwq], rows: q (if nq == 3), k, v; each [head][32]
    const float* bqkv;      // [nq * C] or NULL
    const f16* wproj;       // [C][ldwp]
    const float* bproj;     // [C] or NULL
    const float* table;     // [27 * 27][heads]
    f16* y;
    int B, Hp, Wp, nWy, nWx, ldwq, ldwp;
    long n_windows, x_bytes;
    float scale_log2e, inv_scale;
};

constexpr int G14_WS = 14, G14_C = 256, G14_HEADS = 8, G14_CK = 8, G14_N = G14_WS * G14_WS;
constexpr int G14_NT = 13;                                      // 16-token tiles of the dense order
using G14Win = WinCfg<14, 16, 4, 4>;                            // the padded order row' = 16 ty + tx
constexpr int G14_RP = G14Win::RP, G14_TBF = G14Win::TB_FLOATS, G14_KVB = G14Win::ROWB;
static_assert(G14_RP == 224 && G14Win::NKT == 14 && G14_TBF == 2644, "14 key tiles of the padded order; 2644 table floats");
constexpr int G14_WROWB = 2 * G14_C + 32;                       // qkv weight row in LDS (stride = 32 mod 64)
constexpr int G14_PROWB = 2 * 64 + 32;                          // proj weight row of a head PAIR (64 columns)
constexpr int G14_W_OFF = 0;
constexpr int G14_W_BYTES = 96 * G14_WROWB;                     // >= 256 * G14_PROWB
constexpr int G14_KV_OFF = G14_W_OFF + G14_W_BYTES;
constexpr int G14_TB_OFF = G14_KV_OFF + 2 * G14_RP * G14_KVB;
constexpr int G14_SMEM = G14_TB_OFF + (G14_TBF * 4 + 15) / 16 * 16;
static_assert(256 * G14_PROWB <= G14_W_BYTES, "proj pair image fits the weight buffer");
static_assert(G14_KV_OFF == 52224 && G14_TB_OFF == 80896 && G14_SMEM == 91472, "LDS plan");

template <bool GLOBALQ>
__global__ __launch_bounds__(512, 2) void gcvit_attn_block14_kernel(Gb14Args a) {
    constexpr int C = G14_C, CK = G14_CK, NTHR = 512, NCT = C / 16;
    constexpr int NQ = GLOBALQ ? 2 : 3;
    constexpr unsigned OOB = 0xFFFFFFF0u;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* wbuf = smem + G14_W_OFF;
    char* k_lds = smem + G14_KV_OFF;
    char* v_lds = k_lds + G14_RP * G14_KVB;
    float* tb = reinterpret_cast<float*>(smem + G14_TB_OFF);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;

    // the padding slots of the K / V image are never written by a token: finite once and for all
    for (int i = tid; i < 2 * G14_RP * G14_KVB / 16; i += NTHR) *reinterpret_cast<uint4*>(k_lds + i * 16) = make_uint4(0, 0, 0, 0);

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (unsigned)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, (unsigned)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rbq =
        __builtin_amdgcn_make_buffer_rsrc((void*)a.bqkv, 0, a.bqkv ? (unsigned)(NQ * C * 4) : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rbp = __builtin_amdgcn_make_buffer_rsrc((void*)a.bproj, 0, a.bproj ? (unsigned)(C * 4) : 0u, 0x00020000);
    const char* wql = wbuf + l15 * G14_WROWB + g * 16;
    const char* wpl = wbuf + l15 * G14_PROWB + g * 16;
    const float sc = a.scale_log2e;
    const int wpi = a.nWy * a.nWx;

    // this lane's tokens: slot s -> tile wave + 8 s, dense index n = 16 tile + l15 = 14 ty + tx
    bool tile_ok[2];
    int qyv[2], qxv[2], krow[2];
    bool tok_ok[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int tile = wave + 8 * s;
        tile_ok[s] = tile < G14_NT;                          // wave-uniform
        const int n = tile * 16 + l15;
        tok_ok[s] = tile_ok[s] && n < G14_N;
        const int nc = n < G14_N ? n : G14_N - 1;
        qyv[s] = nc / G14_WS;
        qxv[s] = nc - qyv[s] * G14_WS;
        krow[s] = qyv[s] * 16 + qxv[s];
    }

    for (long w = blockIdx.x; w < a.n_windows; w += gridDim.x) {          // workgroup-uniform
        const int b = (int)(w / wpi);
        const int wrem = (int)(w - (long)b * wpi);
        const int wy = wrem / a.nWx, wx = wrem - wy * a.nWx;
        unsigned xoff[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const long pix = ((long)b * a.Hp + wy * G14_WS + qyv[s]) * a.Wp + wx * G14_WS + qxv[s];
            xoff[s] = tok_ok[s] ? (unsigned)(pix * C * 2) : OOB;
        }
        U4H8 xf[CK][2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int ks = 0; ks < CK; ++ks)
                xf[ks][s].u = __builtin_bit_cast(
                    uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, xoff[s] == OOB ? OOB : xoff[s] + (ks * 32 + g * 8) * 2, 0, 0));
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            U4H8 col[CK];
#pragma unroll
            for (int ks = 0; ks < CK; ++ks) col[ks] = xf[ks][s];
            ln_fragments<CK>(col, a.ln_g, a.ln_b, a.ln_eps, g);
#pragma unroll
            for (int ks = 0; ks < CK; ++ks) xf[ks][s] = col[ks];
        }

#pragma unroll 1
        for (int head = 0; head < G14_HEADS; ++head) {
            // ---- stage this head's q | k | v weight rows (fragment order) and its bias table; the previous head's readers are past
            // the barrier that closed its attention pass ----
            for (int i = tid; i < NQ * 32 * (C / 8); i += NTHR) {
                const int j = i >> 5, c = i & 31;                                 // LDS row (part * 32 + jj), 16-byte chunk
                const int row = (j >> 5) * C + head * 32 + frag_channel32(j & 31);
                *reinterpret_cast<uint4*>(wbuf + j * G14_WROWB + c * 16) = *reinterpret_cast<const uint4*>(a.wqkv + (long)row * a.ldwq + c * 8);
            }
            win_table_fill_loop<G14Win>(tb, a.table, G14_HEADS, head, a.inv_scale, tid, NTHR);
            __syncthreads();

            // ---- [q | k | v]^T = W x^T + b for this wave's tokens ----
            U4H8 qf[2];
#pragma unroll
            for (int part = 0; part < NQ; ++part) {
                U4H8 wf[2][CK];
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int ks = 0; ks < CK; ++ks)
                        wf[t][ks].u = *reinterpret_cast<const uint4*>(wql + (part * 32 + t * 16) * G14_WROWB + ks * 64);
                f32x4 bv[2];
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    bv[t] = __builtin_bit_cast(
                        f32x4, __builtin_amdgcn_raw_buffer_load_b128(rbq, (unsigned)((part * C + head * 32 + g * 8 + t * 4) * 4), 0, 0));
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (!tile_ok[s]) continue;                                    // wave-uniform
                    f32x4 acc[2] = {bv[0], bv[1]};
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int ks = 0; ks < CK; ++ks)
                            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[t][ks].h, xf[ks][s].h, acc[t], 0, 0, 0);
                    U4H8 pk;                                                      // head channels 8 g .. 8 g + 7 of the lane's token
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        pk.e[i] = (f16)acc[0][i];
                        pk.e[4 + i] = (f16)acc[1][i];
                    }
                    const int row = krow[s];
                    if (!GLOBALQ && part == 0) qf[s] = pk;
                    else if (part == NQ - 2) {
                        if (tok_ok[s]) *reinterpret_cast<uint4*>(k_lds + row * G14_KVB + win_k_slot(row, g) * 16) = pk.u;
                    } else {
                        if (tok_ok[s]) *reinterpret_cast<uint4*>(v_lds + row * G14_KVB + win_v_chunk(row, g) * 16) = pk.u;
                    }
                }
            }
            if constexpr (GLOBALQ) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int n = qyv[s] * G14_WS + qxv[s];
                    const uint4 v = *reinterpret_cast<const uint4*>(a.qg + ((long)b * G14_N + n) * C + head * 32 + g * 8);
                    qf[s].u = tok_ok[s] ? v : make_uint4(0, 0, 0, 0);
                }
            }
            __syncthreads();

            // ---- attention on this wave's query tiles; the head's output goes to the lane's own 16 bytes of y (scratch) ----
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (!tile_ok[s]) continue;
                const U4H8 of = win_attn_tile<G14Win, false, false>(qf[s], k_lds, v_lds, tb, qyv[s], qxv[s], l15, g, sc);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, of.u),
                                                       ry, xoff[s] == OOB ? OOB : xoff[s] + (head * 32 + g * 8) * 2, 0, 0);
            }
            __syncthreads();
        }

        // ---- proj: y^T = Wp O^T + b over head pairs (64 weight columns at a time through the weight buffer) ----
        f32x4 yacc[NCT][2];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const f32x4 bv = __builtin_bit_cast(
                f32x4, __builtin_amdgcn_raw_buffer_load_b128(rbp, (unsigned)(((ct >> 1) * 32 + g * 8 + (ct & 1) * 4) * 4), 0, 0));
            yacc[ct][0] = yacc[ct][1] = bv;
        }
#pragma unroll 1
        for (int hp = 0; hp < G14_HEADS / 2; ++hp) {
            for (int i = tid; i < C * 8; i += NTHR) {
                const int j = i >> 3, c = i & 7;                                  // LDS row, chunk = head-in-pair * 4 + lane group
                const int ch = frag_channel(j);
                const f16* src = a.wproj + (long)ch * a.ldwp + (2 * hp + (c >> 2)) * 32 + 4 * (c & 3);
                const uint2 lo = *reinterpret_cast<const uint2*>(src), hi = *reinterpret_cast<const uint2*>(src + 16);
                *reinterpret_cast<uint4*>(wbuf + j * G14_PROWB + c * 16) = make_uint4(lo.x, lo.y, hi.x, hi.y);
            }
            // the parked head outputs of this lane (its own stores, completed before the barriers in between; sc0 sc1: past the L1)
            U4H8 of[2][2];
#pragma unroll
            for (int hl = 0; hl < 2; ++hl)
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    of[hl][s].u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                                                ry, xoff[s] == OOB ? OOB : xoff[s] + ((2 * hp + hl) * 32 + g * 8) * 2, 0, 17));
            __syncthreads();
#pragma unroll
            for (int hl = 0; hl < 2; ++hl)
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    U4H8 pw;
                    pw.u = *reinterpret_cast<const uint4*>(wpl + ct * 16 * G14_PROWB + hl * 64);
#pragma unroll
                    for (int s = 0; s < 2; ++s)
                        if (tile_ok[s]) yacc[ct][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pw.h, of[hl][s].h, yacc[ct][s], 0, 0, 0);
                }
            __syncthreads();
        }

        // ---- epilogue: + x, fp16, 16-byte stores (lane: token, channels 32 hh + 8 g .. + 7) ----
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int hh = 0; hh < CK; ++hh) {
                const unsigned off = xoff[s] == OOB ? OOB : xoff[s] + (hh * 32 + g * 8) * 2;
                U4H8 r;
                r.u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
                U4H8 o;
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    const f32x4 av = yacc[2 * hh + (j >> 2)][s];
                    const f32x2 v = (f32x2){av[j & 3], av[(j & 3) + 1]} + (f32x2){(float)r.e[j], (float)r.e[j + 1]};
                    o.e[j] = (f16)v.x;
                    o.e[j + 1] = (f16)v.y;
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, o.u),
                                                       ry, off, 0, 0);
            }
    }
}

}  // namespace

// the 14 x 14-window configuration of vip_gcvit_attn_block_f16 (gcvit_block.hip): C = 256, 8 heads
int vip_gcvit_attn_block14(const void* x, const void* q_global, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* wqkv,
                           int ldwq, const float* bqkv, const void* wproj, int ldwp, const float* bproj, const float* table, void* y,
                           int B, int Hp, int Wp, float scale, hipStream_t s) {
    Gb14Args a;
    a.x = (const f16*)x; a.qg = (const f16*)q_global; a.ln_g = ln_gamma; a.ln_b = ln_beta; a.ln_eps = ln_eps;
    a.wqkv = (const f16*)wqkv; a.bqkv = bqkv; a.wproj = (const f16*)wproj; a.bproj = bproj; a.table = table; a.y = (f16*)y;
    a.B = B; a.Hp = Hp; a.Wp = Wp; a.nWy = Hp / G14_WS; a.nWx = Wp / G14_WS; a.ldwq = ldwq; a.ldwp = ldwp;
    a.n_windows = (long)B * a.nWy * a.nWx;
    a.x_bytes = 2L * B * Hp * Wp * G14_C;
    a.scale_log2e = scale * 1.44269504088896f;
    a.inv_scale = 1.f / scale;
    long wgs = a.n_windows < 256 ? a.n_windows : 256;            // one 89 KB, 8-wave workgroup per CU
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gcvit_attn_block14_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, G14_SMEM);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gcvit_attn_block14_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, G14_SMEM);
        attr_set = true;
    }
    if (q_global) hipLaunchKernelGGL(gcvit_attn_block14_kernel<true>, dim3((unsigned)wgs), dim3(512), G14_SMEM, s, a);
    else hipLaunchKernelGGL(gcvit_attn_block14_kernel<false>, dim3((unsigned)wgs), dim3(512), G14_SMEM, s, a);
    return vip_launch_status("vip_gcvit_attn_block_f16(ws 14)");
}
