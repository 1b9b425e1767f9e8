// The fp16 window-attention core on the matrix cores, head_dim 32: the geometry, the LDS images and the per-tile arithmetic that
// window_attn.hip, gcvit_block.hip, gcvit_block14.hip and swin_attn.hip share (attn_h2.hip takes the swizzles for its head_dim 32
// images).
//
// LAYOUT CONTRACT.  Tokens of a window are re-indexed as row' = ty * P + tx (P = 8 for windows up to 8, 16 for 14), padded to whole
// 32-key steps.  K and V images in LDS have 64-byte rows (32 halfs) and no padding:
//   * K: 16-byte chunk c of row r sits at slot win_k_slot(r, c) = c ^ pi[(r >> 2) & 3], pi = {0, 2, 3, 1}: the fragment read (lane & 15
//     = row, lane >> 4 = chunk) is a conflict-free ds_read_b128;
//   * V: the two 32-byte halves (one 16-channel output tile each) are swapped on rows with bit 2 set (win_v_half; as 16-byte chunks
//     win_v_chunk): conflict-free ds_read_b64_tr_b16.
// S^T = K Q^T has keys on the accumulator rows (register (t, r) of lane group g: key row' 16 t + 4 g + r) and the lane's query on the
// column, so the softmax over keys is register-local plus two lane exchanges and the probabilities are the B operand of O^T = V^T P^T as
// they stand: MFMA k-slot (g, j) carries key 32 s + 4 g + j (j < 4) / 32 s + 16 + 4 g + (j - 4).  A lane ends with head channels
// 4 g .. 4 g + 3 and 16 + 4 g .. of its query.
// GCViT's relative-position table is a per-head LDS image (WinCfg, win_table_value): a block of -1e30, then [2 ws - 1] rows of TW floats
// holding table / scale, so that the bias of score register (t, r) is base(query, lane group) + a compile-time immediate and padded key
// slots are redirected to the -1e30 block by swapping the base register.
//
// CONCURRENCY RULE (window_attn.hip CONCURRENCY NOTE).  The bias values are read into the accumulators BEFORE the
// first MFMA and go in as its C operand.  The sequence "MFMA with C = 0, LDS read, packed add on the MFMA result" returned wrong values
// next to MFMA-heavy co-runners and must not come back, here or in the two tiles that mirror win_attn_tile.
//
// A helper stays out of a kernel where calling it changes that kernel's machine code (tools/asm_compare.py against the parent): hipcc's
// output depends on where a function boundary stood even when everything is inlined.  Such places carry a comment naming the helper.
#pragma once
#include "common.hpp"

typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));

constexpr int WIN_ROWB = 64;                            // bytes per K / V row

template <int WS, int P, int LOG2P, int WPI>
struct WinCfg {
    static constexpr int WIN = WS, PITCH = P, LOG2_PITCH = LOG2P;
    static constexpr int RP = (WS * P + 31) / 32 * 32;  // key rows (64 / 224)
    static constexpr int NKT = RP / 16;                 // 16-key tiles
    static constexpr int NQT = (WS * WS + 15) / 16;     // 16-query tiles over the DENSE token order (4 / 13)
    static constexpr int IPW = 4 / WPI;
    static constexpr int ROWB = WIN_ROWB;
    // bias-table row stride (floats).  ws 14: 48, not 32 - with a 32-float stride the two token rows a query tile
    // spans land on the same LDS banks (2-way conflicts on 28 % of the table reads); 48 shifts them by 16 banks.
    static constexpr int TW = (P == 16) ? 48 : 2 * P;
    static constexpr int KSTEP = TW * 16 / P;           // table-offset step of one 16-key tile
    static constexpr int KCMAX = KSTEP * NKT;
    static constexpr int NEGSZ = KCMAX + 4;
    static constexpr int TOFF = NEGSZ + KCMAX;
    static constexpr int TROWS = 2 * WS - 1;
    static constexpr int TB_FLOATS = TOFF + TROWS * TW;
    static constexpr int K_OFF = 0;
    static constexpr int V_OFF = RP * ROWB;
    static constexpr int T_OFF = 2 * RP * ROWB;
    static constexpr int ITEM_BYTES = (T_OFF + TB_FLOATS * 4 + 15) / 16 * 16;
    static constexpr int SMEM = ITEM_BYTES * IPW;
    static constexpr int QPW = (NQT + WPI - 1) / WPI;   // query tiles per wave
};

// ---- swizzles (both are involutions) ----
__device__ __forceinline__ int win_k_slot(int row, int ch) {
    const int q = (row >> 2) & 3;
    return ch ^ ((0x78 >> (q * 2)) & 3);  // pi = {0,2,3,1}
}
__device__ __forceinline__ int win_v_chunk(int row, int ch) { return ch ^ (((row >> 2) & 1) << 1); }
__device__ __forceinline__ int win_v_half(int row, int dt) { return dt ^ ((row >> 2) & 1); }

// ---- bias-table image of one head ----
// element i of the image: the -1e30 block, table / scale at the TW stride, zero pad.  PAST_END: i may lie past the image (no load there).
template <class Cfg, bool PAST_END>
__device__ __forceinline__ float win_table_value(const float* table, int heads, int head, int i, float inv_scale) {
    const int e = i - Cfg::TOFF;
    const int ry = e / Cfg::TW, rx = e - ry * Cfg::TW;
    const bool in_tab = PAST_END ? (i >= Cfg::TOFF) & (i < Cfg::TB_FLOATS) & (rx < Cfg::TROWS) : (i >= Cfg::TOFF) & (rx < Cfg::TROWS);
    const int gi = in_tab ? (ry * Cfg::TROWS + rx) * heads + head : 0;
    const float t = table[gi];
    return in_tab ? t * inv_scale : (i < Cfg::TOFF ? -1.0e30f : 0.f);
}
// the whole image by nthr threads, thread tid.  window_attn.hip keeps loops of its own around win_table_value (all loads, then all
// stores: its fill sits on the kernel's load chain); gcvit_block.hip one loop over all its heads' images.
template <class Cfg>
__device__ __forceinline__ void win_table_fill_loop(float* tb, const float* table, int heads, int head, float inv_scale, int tid, int nthr) {
    for (int i = tid; i < Cfg::TB_FLOATS; i += nthr) tb[i] = win_table_value<Cfg, false>(table, heads, head, i, inv_scale);
}

// ---- one 16-query tile ----
// maximum over the keys of the lane's query
template <int NKT>
__device__ __forceinline__ float win_score_max(const f32x4 (&acc)[NKT]) {
    float m = -1.0e30f;
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
        m = fmaxf(fmaxf(m, acc[t][0]), acc[t][1]);   // v_max3_f32
        m = fmaxf(fmaxf(m, acc[t][2]), acc[t][3]);
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    return fmaxf(m, __shfl_xor(m, 32, 64));
}

// acc <- p = exp2(sc * s' - sc * max s'), s' = q.k + bias / scale, sc = scale * log2 e: one packed FMA + one exp2 per score.  Returns
// the sum over the keys.
template <int NKT>
__device__ __forceinline__ float win_softmax_exp2(f32x4 (&acc)[NKT], float m, float sc) {
    const f32x2 nm = {-m * sc, -m * sc};
    f32x2 ls2 = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
            const f32x2 e = (f32x2){acc[t][r], acc[t][r + 1]} * sc + nm;      // v_pk_fma_f32
            const f32x2 p = {__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};
            acc[t][r] = p.x;
            acc[t][r + 1] = p.y;
            ls2 += p;                                                         // v_pk_add_f32
        }
    }
    float lsum = ls2.x + ls2.y;
    lsum += __shfl_xor(lsum, 16, 64);
    return lsum + __shfl_xor(lsum, 32, 64);
}

// One 16-query tile against a K / V image, as the block kernels run it: S^T = K Q^T + bias, softmax over the keys, O^T = V^T P^T,
// normalised and packed as the proj MFMA's B operand (k-slot (g, j) = head channel 4g + j (j < 4) / 16 + 4g + (j - 4)).  (qy, qx): the
// lane's query in the window, clamped into it for padding lanes; sc = scale * log2 e.
//   READ_FIRST: all K fragments are read before the first score MFMA, or fragment by fragment.
//   OPERANDS_FIRST: the P.V MFMAs take all their operands (P^T fragments, V^T fragments) from registers that are complete before the
//   first of them issues, or they are converted / read step by step between the MFMAs (14 key tiles of operands do not fit next to the
//   14 x 14 block kernel's other state).
// window_attn.hip's win_query_tile and swin_attn.hip's tile loop mirror this function and end in a store; as calls into pieces of it
// their kernels' code changes (profiles/attn_core_refactor_asm.log), so they keep their own text.
template <class Cfg, bool READ_FIRST, bool OPERANDS_FIRST>
__device__ __forceinline__ U4H8 win_attn_tile(const U4H8& qfrag, const char* k_lds, const char* v_lds, const float* tb, int qy, int qx,
                                              int l15, int g, float sc) {
    constexpr int NKT = Cfg::NKT, WS = Cfg::WIN, P = Cfg::PITCH;
    // lane-dependent part of the key term 2k' - kx  (k' = 16t + 4g + r)
    const int lane_term = (P == 16) ? 4 * g : (g >> 1) * Cfg::TW + 4 * (g & 1);
    const int tr_q = l15 >> 2, tr_p = l15 & 3;
    const float* tbase = tb + (Cfg::TOFF + qy * Cfg::TW + qx + (WS - 1) * (Cfg::TW + 1) - lane_term - Cfg::KCMAX);
    // The accumulators START as the relative-position bias (padded key slots: -1e30): one LDS read with an immediate offset per score,
    // issued and returned before the first MFMA, then C operand of S^T = K Q^T + bias.
    f32x4 acc[NKT];
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int mask = 0;                       // lane groups whose key slot (t, r) is padding (compile-time)
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const int kp = 16 * t + 4 * gg + r;
                if (((kp & (P - 1)) >= WS) || ((kp >> Cfg::LOG2_PITCH) >= WS)) mask |= 1 << gg;
            }
            if (mask == 15) {
                acc[t][r] = -1.0e30f;
            } else {
                const int imm = Cfg::KCMAX - (Cfg::KSTEP * t + r);
                const float* bp = (mask == 0) ? tbase : (((mask >> g) & 1) ? tb : tbase);
                acc[t][r] = bp[imm];
            }
        }
    if constexpr (READ_FIRST) {
        U4H8 kf[NKT];
#pragma unroll
        for (int t = 0; t < NKT; ++t) {
            const int row = t * 16 + l15;
            kf[t].u = *reinterpret_cast<const uint4*>(k_lds + row * WIN_ROWB + win_k_slot(row, g) * 16);
        }
#pragma unroll
        for (int t = 0; t < NKT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[t].h, qfrag.h, acc[t], 0, 0, 0);
    } else {
#pragma unroll
        for (int t = 0; t < NKT; ++t) {
            const int row = t * 16 + l15;
            U4H8 kf;
            kf.u = *reinterpret_cast<const uint4*>(k_lds + row * WIN_ROWB + win_k_slot(row, g) * 16);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf.h, qfrag.h, acc[t], 0, 0, 0);
        }
    }
    const float m = win_score_max<NKT>(acc);
    const float lsum = win_softmax_exp2<NKT>(acc, m, sc);

    // O^T = V^T P^T : A = V^T (two 16-wide head-dim tiles) via transposed LDS reads, B = P^T from the accumulators: MFMA k-slot (g, j)
    // carries key 32s + 4g + j (j < 4) / 32s + 16 + 4g + (j-4).
    union VF {
        fp16x4_t t[2];
        f16x8 v;
    };
    f32x4 o[2];
    o[0] = o[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (OPERANDS_FIRST) {
        U4H8 pfa[NKT / 2];
        VF vfa[NKT / 2][2];
#pragma unroll
        for (int s = 0; s < NKT / 2; ++s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pfa[s].e[j] = (f16)acc[2 * s][j];
                pfa[s].e[4 + j] = (f16)acc[2 * s + 1][j];
            }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const int row = 32 * s + 16 * hh + 4 * g + tr_q;
                    const int half = dt ^ ((row >> 2) & 1);  // win_v_half, = dt ^ (g & 1)
                    vfa[s][dt].t[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4f16(
                        (__attribute__((address_space(3))) fp16x4_t*)(v_lds + row * WIN_ROWB + half * 32 + tr_p * 8));
                }
        }
#pragma unroll
        for (int s = 0; s < NKT / 2; ++s)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vfa[s][dt].v, pfa[s].h, o[dt], 0, 0, 0);
    } else {
#pragma unroll
        for (int s = 0; s < NKT / 2; ++s) {
            U4H8 pf;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pf.e[j] = (f16)acc[2 * s][j];
                pf.e[4 + j] = (f16)acc[2 * s + 1][j];
            }
            VF vf[2];
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const int row = 32 * s + 16 * hh + 4 * g + tr_q;
                    const int half = dt ^ ((row >> 2) & 1);
                    vf[dt].t[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4f16(
                        (__attribute__((address_space(3))) fp16x4_t*)(v_lds + row * WIN_ROWB + half * 32 + tr_p * 8));
                }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[dt].v, pf.h, o[dt], 0, 0, 0);
        }
    }
    const float inv = 1.f / lsum;
    U4H8 of;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        of.e[r] = (f16)(o[0][r] * inv);
        of.e[4 + r] = (f16)(o[1][r] * inv);
    }
    return of;
}
