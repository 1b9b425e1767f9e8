// Swin Transformer V2 shifted cosine window attention (kecam swin_transformer_v2.py:164-262 without its two Dense layers) as ONE
// launch on the UNPADDED feature map:
//   out[b, y, x, head*32 + :] = softmax_k( tau[head] * qn . kn + table[idx(q, k)][head] + (region(q) != region(k) ? -100 : 0) ) v
// Pad, roll, window partition, window reverse, un-roll and crop of the layer are folded into the addressing.  With
// Hp = ceil(H / ws) ws, Wp = ceil(W / ws) ws the token at ROLLED position (Y, X) of window (Y / ws, X / ws) is the map's token at
// y = (Y + shift) mod Hp, x = (X + shift) mod Wp.  If y >= H or x >= W the token is PADDED: its key is the zero vector (kn = 0, the
// qkv Dense has no key bias), its value is v_bias (or 0), its query is never evaluated and nothing is stored for it.  Padded keys are
// NOT masked - they sit in every softmax of their window with the logit 0 + table (the reference pads before it partitions).
//   qn = q * rsqrt(max(sum q^2, 1e-6)) (tf.nn.l2_normalize: a maximum under the root), kn likewise, both in fp32;
//   idx = (qr - kr + ws - 1)(2 ws - 1) + (qc - kc + ws - 1) on window coordinates;
//   region(Y, X) = 3 r(Y, Hp) + r(X, Wp), r(t, L) = [t >= L - ws] + [t >= L - shift] on rolled, padded coordinates (shift > 0 only).
//
// fp16 storage (swin_attn_kernel): work item = (image, window, head), one wave per item, four items per workgroup; head_dim 32.
// Tokens are re-indexed as row' = 8 ty + tx (the P = 8 re-indexing of window_core.hpp), so ws <= 8 gives four 16-key tiles; ws 8 is
// the dense case, ws < 8 leaves DEAD slots (ty >= ws or tx >= ws: no token at all, unlike a padded token), killed by value: their
// accumulators start at -1e30.  K is normalised in fp32 while it is staged into LDS, Q (times tau) as its fragments are loaded.
// S^T = Kn Qn^T with v_mfma_f32_16x16x32_f16 and the table entry plus the mask term as the MFMA's C OPERAND (the concurrency rule at
// the top of window_core.hpp: no "MFMA with C = 0, LDS read, packed add" sequence), softmax over keys register-local plus two
// cross-lane exchanges, O^T = V^T P^T with V^T fragments from transposed LDS reads - the LDS images and fragment reads of
// window_core.hpp.  Wrapped gathers, v_bias rows and skipped stores are plain C++ addressing.  No atomics: every output is a function
// of its own window alone, in a fixed order - bit-reproducible and independent of the batch.
//
// packed and fp32 storages (swin_attn_strict_kernel): one fp32 VALU template, the conventions of sattn_kernel (strict_ops.hip) - one
// thread per query token, Kn / V of the item in LDS as fp32, online softmax with libm expf, true divisions.
#include "window_core.hpp"
#include <math.h>

namespace {

constexpr int SW_MAX_WS = 8;
constexpr int SW_HD = 32;
constexpr int SW_ROWS = 64;                        // key slots: 8 x 8
constexpr int SW_ROWB = WIN_ROWB;                  // bytes per fp16 row
constexpr int SW_TB = 232;                         // (2 * 8 - 1)^2 = 225 table floats per head, rounded up
constexpr int SW_ITEM_BYTES = 2 * SW_ROWS * SW_ROWB + SW_TB * 4;
constexpr float SW_EPS = 1e-6f;
constexpr float SW_MASK = -100.f;
constexpr float SW_DEAD = -1.0e30f;
constexpr float SW_LOG2E = 1.44269504088896f;

struct SwinArgs {
    const void* qkv;
    const float* vbias;
    const float* tau;
    const float* table;
    void* out;
    int B, H, W, C, heads, ws, shift, Hp, Wp, nWy, nWx, items;
    int* status;
};

__device__ __forceinline__ int sw_r(int t, int L, int ws, int shift) { return (t >= L - ws) + (t >= L - shift); }

// pixel y * W + x of the map behind window slot (ty, tx); -1: a padded token
__device__ __forceinline__ int sw_pix(const SwinArgs& a, int wy, int wx, int ty, int tx) {
    int y = wy * a.ws + ty + a.shift, x = wx * a.ws + tx + a.shift;
    if (y >= a.Hp) y -= a.Hp;
    if (x >= a.Wp) x -= a.Wp;
    return (y < a.H && x < a.W) ? y * a.W + x : -1;
}

__global__ __launch_bounds__(256) void swin_attn_kernel(SwinArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[4 * SW_ITEM_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int item = blockIdx.x * 4 + wave;
    const bool item_ok = item < a.items;
    if (!item_ok) item = a.items - 1;
    const int head = item % a.heads;
    int wq = item / a.heads;
    const int wx = wq % a.nWx;
    wq /= a.nWx;
    const int wy = wq % a.nWy;
    const int b = wq / a.nWy;

    char* k_lds = smem + wave * SW_ITEM_BYTES;
    char* v_lds = k_lds + SW_ROWS * SW_ROWB;
    float* tb = reinterpret_cast<float*>(v_lds + SW_ROWS * SW_ROWB);
    const int ws = a.ws, shift = a.shift, tw = 2 * ws - 1;
    const int ld = 3 * a.C;
    const f16* qkv = static_cast<const f16*>(a.qkv);
    const long img = (long)b * a.H * a.W;
    const int l15 = lane & 15, g = lane >> 4;
    const float tau = a.tau[head];
    const int nqt = (ws * 8 + 15) >> 4;               // 16-query tiles that hold a live slot (wave-uniform)

    // ---- Q fragments (slot order, like the keys), normalised and scaled by tau in fp32; dead and padded queries are zero ----
    U4H8 qf[4];
    int qpix[4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        const int qn = qt * 16 + l15;
        const int ty = qn >> 3, tx = qn & 7;
        const int pix = (ty < ws && tx < ws) ? sw_pix(a, wy, wx, ty, tx) : -1;
        qpix[qt] = pix;
        const f16* src = pix >= 0 ? qkv + (img + pix) * ld + head * SW_HD + g * 8 : qkv;
        U4H8 raw;
        raw.u = *reinterpret_cast<const uint4*>(src);
        float f[8], s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            f[j] = (float)raw.e[j];
            s = fmaf(f[j], f[j], s);
        }
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        const float sc = tau / sqrtf(fmaxf(s, SW_EPS));
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[qt].e[j] = pix >= 0 ? (f16)(f[j] * sc) : (f16)0.f;
    }

    // ---- stage Kn / V: lane = (row, 16-byte chunk), four passes of 16 rows.  Loads are unconditional (a token that is not on the
    // map reads a safe address and is replaced afterwards) ----
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = it * 16 + (lane >> 2), ch = lane & 3;
        const int ty = row >> 3, tx = row & 7;
        const bool live = ty < ws && tx < ws;
        const int pix = live ? sw_pix(a, wy, wx, ty, tx) : -1;
        const f16* src = pix >= 0 ? qkv + (img + pix) * ld + a.C + head * SW_HD + ch * 8 : qkv;
        U4H8 kr, vr, kn;
        kr.u = *reinterpret_cast<const uint4*>(src);
        vr.u = *reinterpret_cast<const uint4*>(pix >= 0 ? src + a.C : qkv);
        float f[8], s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            f[j] = (float)kr.e[j];
            s = fmaf(f[j], f[j], s);
        }
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        const float rinv = 1.f / sqrtf(fmaxf(s, SW_EPS));
#pragma unroll
        for (int j = 0; j < 8; ++j) kn.e[j] = pix >= 0 ? (f16)(f[j] * rinv) : (f16)0.f;
        if (pix < 0) {
            vr.u = make_uint4(0, 0, 0, 0);
            if (live && a.vbias) {                    // a padded token: value_bias
#pragma unroll
                for (int j = 0; j < 8; ++j) vr.e[j] = (f16)a.vbias[head * SW_HD + ch * 8 + j];
            }
        }
        *reinterpret_cast<uint4*>(k_lds + row * SW_ROWB + win_k_slot(row, ch) * 16) = kn.u;
        // chunk win_v_chunk(row, ch), written out: as a call here the kernel's code changes
        *reinterpret_cast<uint4*>(v_lds + row * SW_ROWB + (ch ^ (((row >> 2) & 1) << 1)) * 16) = vr.u;
    }
    for (int i = lane; i < tw * tw; i += 64) tb[i] = a.table[(long)i * a.heads + head];
    __syncthreads();

    // keys of this lane's accumulator registers: row' = 16 t + 4 g + r  ->  ky = 2 t + (g >> 1), kx = 4 (g & 1) + r
    int kyo[4], kxo[4], kry[4], krx[4];
    bool kyd[4], kxd[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ky = 2 * i + (g >> 1), kx = 4 * (g & 1) + i;
        kyd[i] = ky >= ws;
        kxd[i] = kx >= ws;
        kyo[i] = ky * tw;
        kxo[i] = kx;
        kry[i] = shift ? 3 * sw_r(wy * ws + ky, a.Hp, ws, shift) : 0;
        krx[i] = shift ? sw_r(wx * ws + kx, a.Wp, ws, shift) : 0;
    }
    const int tr_q = l15 >> 2, tr_p = l15 & 3;

#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        if (qt >= nqt) break;  // wave-uniform
        const int qn = qt * 16 + l15;
        const int qy = min(qn >> 3, ws - 1), qx = min(qn & 7, ws - 1);
        const int rq = shift ? 3 * sw_r(wy * ws + qy, a.Hp, ws, shift) + sw_r(wx * ws + qx, a.Wp, ws, shift) : 0;
        const int tbase = (qy + ws - 1) * tw + (qx + ws - 1);
        // S^T tiles: rows = keys 16 t + 4 g + r, column = this lane's query.  The accumulators START as table + mask (dead slots:
        // -1e30) and go in as the C operand of S^T = Kn Qn^T + C.  From the K fragment reads to the store this mirrors win_attn_tile
        // <.., true, true> of window_core.hpp with its own start, softmax expression and store; as calls into pieces of that function
        // the kernel's code changes, so the text stays here.
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool dead = kyd[t] || kxd[r];
                const float bias = tb[dead ? 0 : tbase - kyo[t] - kxo[r]];
                acc[t][r] = dead ? SW_DEAD : bias + ((kry[t] + krx[r]) != rq ? SW_MASK : 0.f);
            }
        U4H8 kf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int row = t * 16 + l15;
            kf[t].u = *reinterpret_cast<const uint4*>(k_lds + row * SW_ROWB + win_k_slot(row, g) * 16);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[t].h, qf[qt].h, acc[t], 0, 0, 0);
        const float m = win_score_max<4>(acc);
        float lsum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f((acc[t][r] - m) * SW_LOG2E);
                acc[t][r] = p;
                lsum += p;
            }
        lsum += __shfl_xor(lsum, 16, 64);
        lsum += __shfl_xor(lsum, 32, 64);

        // O^T = V^T P^T : A = V^T (two 16-wide head-dim tiles) via transposed LDS reads, B = P^T from the accumulators: MFMA k-slot
        // (g, j) carries key 32 s + 4 g + j (j < 4) / 32 s + 16 + 4 g + (j - 4).  All operands are complete before the first MFMA.
        f32x4 o[2];
        o[0] = o[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        U4H8 pfa[2];
        union VF {
            fp16x4_t t[2];
            f16x8 v;
        } vfa[2][2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
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
                    const int half = dt ^ ((row >> 2) & 1);  // 32-byte halves swapped on odd row quads
                    vfa[s][dt].t[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4f16(
                        (__attribute__((address_space(3))) fp16x4_t*)(v_lds + row * SW_ROWB + half * 32 + tr_p * 8));
                }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vfa[s][dt].v, pfa[s].h, o[dt], 0, 0, 0);

        // store: lane owns its query, head-dim d = 16 dt + 4 g + (0..3).  Lane pairs (g, g ^ 1) swap one 8-byte half so that every
        // lane holds 8 consecutive channels: one 16-byte store per lane, at the query's UNROLLED map position, real queries only.
        {
            const float inv = 1.f / lsum;
            union { f16x4 h; unsigned u[2]; } o0, o1, snd, rcv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o0.h[r] = (f16)(o[0][r] * inv);
                o1.h[r] = (f16)(o[1][r] * inv);
            }
            const bool odd = g & 1;
            snd.u[0] = odd ? o0.u[0] : o1.u[0];
            snd.u[1] = odd ? o0.u[1] : o1.u[1];
            rcv.u[0] = __shfl_xor(snd.u[0], 16, 64);
            rcv.u[1] = __shfl_xor(snd.u[1], 16, 64);
            if (item_ok && qpix[qt] >= 0) {
                f16* dst = static_cast<f16*>(a.out) + (img + qpix[qt]) * a.C + head * SW_HD + (odd ? 16 + 4 * (g - 1) : 4 * g);
                uint4 v;
                v.x = odd ? rcv.u[0] : o0.u[0];
                v.y = odd ? rcv.u[1] : o0.u[1];
                v.z = odd ? o1.u[0] : rcv.u[0];
                v.w = odd ? o1.u[1] : rcv.u[1];
                *reinterpret_cast<uint4*>(dst) = v;
            }
        }
    }
}

// ---- packed / fp32 storages -------------------------------------------------------------------------------------------------------
struct SW32 {
    static __device__ __forceinline__ f32x4 ld(const void* b, long i) { return *reinterpret_cast<const f32x4*>(static_cast<const float*>(b) + i); }
    static __device__ __forceinline__ void st(void* b, long i, f32x4 v, int*) { *reinterpret_cast<f32x4*>(static_cast<float*>(b) + i) = v; }
};
struct SWH2 {
    static __device__ __forceinline__ f32x4 ld(const void* b, long i) { return h2_ld4(b, i); }
    static __device__ __forceinline__ void st(void* b, long i, f32x4 v, int* status) { h2_st4(b, i, v, status); }
};

template <typename S>
__global__ __launch_bounds__(64) void swin_attn_strict_kernel(SwinArgs a) {
    __shared__ __attribute__((aligned(16))) float kl[SW_ROWS * SW_HD];
    __shared__ __attribute__((aligned(16))) float vl[SW_ROWS * SW_HD];
    __shared__ float tl[SW_TB];
    __shared__ int kreg[SW_ROWS];
    int item = blockIdx.x;
    const int head = item % a.heads;
    item /= a.heads;
    const int wx = item % a.nWx;
    item /= a.nWx;
    const int wy = item % a.nWy;
    const int b = item / a.nWy;
    const int ws = a.ws, shift = a.shift, tw = 2 * ws - 1, N = ws * ws;
    const int t = threadIdx.x;
    const int ty = t / ws, tx = t - ty * ws;
    const long ld = 3L * a.C;
    const long img = (long)b * a.H * a.W;
    const int pix = t < N ? sw_pix(a, wy, wx, ty, tx) : -1;
    const long tok = (img + (pix >= 0 ? pix : 0)) * ld + head * SW_HD;
    const int reg = (shift && t < N) ? 3 * sw_r(wy * ws + ty, a.Hp, ws, shift) + sw_r(wx * ws + tx, a.Wp, ws, shift) : 0;

    if (t < N) {
        f32x4 kv[SW_HD / 4], vv[SW_HD / 4];
        float s = 0.f;
#pragma unroll
        for (int d4 = 0; d4 < SW_HD / 4; ++d4) {
            kv[d4] = vv[d4] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (pix >= 0) {
                kv[d4] = S::ld(a.qkv, tok + a.C + d4 * 4);
                vv[d4] = S::ld(a.qkv, tok + 2 * a.C + d4 * 4);
            } else if (a.vbias) {
                vv[d4] = *reinterpret_cast<const f32x4*>(a.vbias + head * SW_HD + d4 * 4);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) s = fmaf(kv[d4][e], kv[d4][e], s);
        }
        const float rinv = 1.f / sqrtf(fmaxf(s, SW_EPS));
#pragma unroll
        for (int d4 = 0; d4 < SW_HD / 4; ++d4) {
            *reinterpret_cast<f32x4*>(kl + t * SW_HD + d4 * 4) = kv[d4] * rinv;
            *reinterpret_cast<f32x4*>(vl + t * SW_HD + d4 * 4) = vv[d4];
        }
        kreg[t] = reg;
    }
    for (int i = t; i < tw * tw; i += 64) tl[i] = a.table[(long)i * a.heads + head];
    __syncthreads();
    if (t >= N || pix < 0) return;

    float q[SW_HD], o[SW_HD];
    {
        float s = 0.f;
#pragma unroll
        for (int d4 = 0; d4 < SW_HD / 4; ++d4) {
            const f32x4 v = S::ld(a.qkv, tok + d4 * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                q[d4 * 4 + e] = v[e];
                s = fmaf(v[e], v[e], s);
            }
        }
        const float sc = a.tau[head] / sqrtf(fmaxf(s, SW_EPS));
#pragma unroll
        for (int d = 0; d < SW_HD; ++d) q[d] *= sc;
    }
#pragma unroll
    for (int d = 0; d < SW_HD; ++d) o[d] = 0.f;
    float m = -3.0e38f, l = 0.f;
    int ky = 0, kx = 0;
    for (int j = 0; j < N; ++j) {
        const float* kr = kl + j * SW_HD;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
        for (int d4 = 0; d4 < SW_HD / 4; ++d4) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + d4 * 4);
            s0 = fmaf(q[d4 * 4], kv[0], s0);
            s1 = fmaf(q[d4 * 4 + 1], kv[1], s1);
            s2 = fmaf(q[d4 * 4 + 2], kv[2], s2);
            s3 = fmaf(q[d4 * 4 + 3], kv[3], s3);
        }
        float s = (s0 + s1) + (s2 + s3);
        s += tl[(ty - ky + ws - 1) * tw + (tx - kx + ws - 1)];
        if (kreg[j] != reg) s += SW_MASK;
        if (++kx == ws) { kx = 0; ++ky; }
        if (s > m) {                                      // new running maximum: rescale what has been accumulated
            const float al = expf(m - s);
            l *= al;
#pragma unroll
            for (int d = 0; d < SW_HD; ++d) o[d] *= al;
            m = s;
        }
        const float p = expf(s - m);
        l += p;
        const float* vr = vl + j * SW_HD;
#pragma unroll
        for (int d4 = 0; d4 < SW_HD / 4; ++d4) {
            const f32x4 vv = *reinterpret_cast<const f32x4*>(vr + d4 * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[d4 * 4 + e] = fmaf(p, vv[e], o[d4 * 4 + e]);
        }
    }
    const long dst = (img + pix) * a.C + head * SW_HD;
#pragma unroll
    for (int d4 = 0; d4 < SW_HD / 4; ++d4)
        S::st(a.out, dst + d4 * 4, (f32x4){o[d4 * 4] / l, o[d4 * 4 + 1] / l, o[d4 * 4 + 2] / l, o[d4 * 4 + 3] / l}, a.status);
}

// argument checks and geometry shared by the three entry points; no launch
int sw_prepare(const char* who, SwinArgs& a, const void* qkv, const float* v_bias, const float* tau, const float* table, void* out, int B,
               int H, int W, int C, int heads, int ws, int shift, int* status) {
    VIP_REQUIRE(qkv && tau && table && out, VIP_ERR_BAD_ARG, "%s: null pointer (only v_bias may be null)", who);
    VIP_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && heads > 0, VIP_ERR_BAD_ARG, "%s: non-positive dimension", who);
    VIP_REQUIRE(vip_swin_attn_supported(C, heads, ws, shift) == 1, VIP_ERR_UNSUPPORTED,
                "%s: unsupported configuration C=%d heads=%d ws=%d shift=%d: needs head_dim = C / heads = 32, 2 <= ws <= %d and shift 0 or "
                "ws / 2 (rounded down)", who, C, heads, ws, shift, SW_MAX_WS);
    int Hp = 0, Wp = 0, items = 0;
    VIP_REQUIRE(vip_swin_attn_plan(B, H, W, heads, ws, shift, &Hp, &Wp, &items) == 1, VIP_ERR_UNSUPPORTED,
                "%s: too many windows (B=%d map %dx%d ws=%d heads=%d)", who, B, H, W, ws, heads);
    a.qkv = qkv; a.vbias = v_bias; a.tau = tau; a.table = table; a.out = out;
    a.B = B; a.H = H; a.W = W; a.C = C; a.heads = heads; a.ws = ws; a.shift = shift;
    a.Hp = Hp; a.Wp = Wp; a.nWy = Hp / ws; a.nWx = Wp / ws; a.items = items;
    a.status = status;
    return VIP_OK;
}

}  // namespace

extern "C" int vip_swin_attn_supported(int C, int heads, int ws, int shift) {
    return (heads > 0 && C == heads * SW_HD && ws >= 2 && ws <= SW_MAX_WS && (shift == 0 || shift == ws / 2)) ? 1 : 0;
}

extern "C" int vip_swin_attn_plan(int B, int H, int W, int heads, int ws, int shift, int* Hp, int* Wp, int* items) {
    if (B <= 0 || H <= 0 || W <= 0 || heads <= 0 || ws < 2 || ws > SW_MAX_WS || !(shift == 0 || shift == ws / 2)) return 0;
    const int hp = (H + ws - 1) / ws * ws, wp = (W + ws - 1) / ws * ws;
    const long n = (long)B * (hp / ws) * (wp / ws) * heads;
    if (n >= (1L << 30) || (long)B * H * W * 3 * heads * SW_HD >= (1L << 40)) return 0;
    if (Hp) *Hp = hp;
    if (Wp) *Wp = wp;
    if (items) *items = (int)n;
    return 1;
}

extern "C" int vip_swin_attn_fwd_f16(const void* qkv, const float* v_bias, const float* tau, const float* bias_table, void* out, int B,
                                     int H, int W, int C, int heads, int ws, int shift, void* stream) {
    SwinArgs a;
    const int st = sw_prepare("vip_swin_attn_fwd_f16", a, qkv, v_bias, tau, bias_table, out, B, H, W, C, heads, ws, shift, nullptr);
    if (st != VIP_OK) return st;
    hipLaunchKernelGGL(swin_attn_kernel, dim3((a.items + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
    return vip_launch_status("vip_swin_attn_fwd_f16");
}

extern "C" int vip_swin_attn_fwd_s32(const float* qkv, const float* v_bias, const float* tau, const float* bias_table, float* out, int B,
                                     int H, int W, int C, int heads, int ws, int shift, void* stream) {
    SwinArgs a;
    const int st = sw_prepare("vip_swin_attn_fwd_s32", a, qkv, v_bias, tau, bias_table, out, B, H, W, C, heads, ws, shift, nullptr);
    if (st != VIP_OK) return st;
    hipLaunchKernelGGL(swin_attn_strict_kernel<SW32>, dim3(a.items), dim3(64), 0, (hipStream_t)stream, a);
    return vip_launch_status("vip_swin_attn_fwd_s32");
}

extern "C" int vip_swin_attn_fwd_h2(const void* qkv, const float* v_bias, const float* tau, const float* bias_table, void* out, int B, int H,
                                    int W, int C, int heads, int ws, int shift, int* status, void* stream) {
    SwinArgs a;
    const int st = sw_prepare("vip_swin_attn_fwd_h2", a, qkv, v_bias, tau, bias_table, out, B, H, W, C, heads, ws, shift, status);
    if (st != VIP_OK) return st;
    hipLaunchKernelGGL(swin_attn_strict_kernel<SWH2>, dim3(a.items), dim3(64), 0, (hipStream_t)stream, a);
    return vip_launch_status("vip_swin_attn_fwd_h2");
}
