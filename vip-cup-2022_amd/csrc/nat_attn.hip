// Neighbourhood attention (kecam nat/nat.py:65-116 without its two Dense layers) as ONE launch on the UNPADDED feature map.  With
// K = kernel_size, r = K / 2, Hp = max(H, K), Wp = max(W, K) the query at (y, x) attends to the K x K block of tokens whose origin is
//   sy = clamp(y - r, 0, Hp - K), sx = clamp(x - r, 0, Wp - K):
//   out[b, y, x, head*32 + :] = softmax over (ky, kx) in [sy, sy + K) x [sx, sx + K) of
//       ( 2^-2.5 q . k[ky, kx] + table[head][(ky - y + K - 1)(2K - 1) + (kx - x + K - 1)] ) applied to v[ky, kx]
// The table index is the ABSOLUTE key-minus-query offset, not the key's position inside the clamped block: the two agree in the
// interior and differ along every edge.  The reference's extract_patches -> replicate-pad -> gather (49 copies of K and V) is index
// arithmetic here.  On a map below the kernel (H < K or W < K) the tokens with y in [H, Hp) or x in [W, Wp) are PADDED: real keys
// whose k | v is kv_pad (the qkv Dense's bias, or 0), never queries, nothing is stored for them.
//
// fp16 storage (nat_attn_kernel): work item = (image, 8 x 8 query tile, head), one workgroup of four waves; wave w owns query rows 2w and
// 2w + 1 of the tile (one 16-query MFMA tile).  The union of the tile's blocks lies inside the 14 x 14 HALO whose origin is the block
// origin of the tile's first query; halo slot (hy, hx) is key row' = 16 hy + hx - the P = 16 geometry, swizzled K / V images and
// transposed V fragment reads of window_core.hpp.  A 16-key tile is one halo row, and the two query rows of a wave touch at most K + 1
// of them, so a wave runs 8 key tiles, not 14 (wave-uniform; fewer where the clamp or the map's edge leaves fewer).  S^T = K Q^T on the
// matrix cores with the bias as the MFMA's C OPERAND (the concurrency rule at the top of window_core.hpp): table / scale for a slot
// inside the lane's query's block, -1e30 for every other slot (outside the block, outside the map, a dead slot); softmax over keys
// register-local plus two cross-lane exchanges, p = exp2((s - max) scale log2 e) so that a winner is exactly 1; O^T = V^T P^T,
// normalised after the product.  Loads of slots that are not on the map are redirected to a valid address and replaced.  No atomics:
// every output is a function of its own neighbourhood in a fixed order - bit-reproducible and independent of the batch.
//
// packed and fp32 storages (nat_attn_strict_kernel): one fp32 VALU template in the conventions of swin_attn_strict_kernel - the same
// work item, one thread per query, the halo's K / V in LDS as fp32 (rows padded to 36 floats: threads read DIFFERENT slots), online
// softmax with libm expf, true divisions.
#include "window_core.hpp"
#include <math.h>

namespace {

constexpr int NA_HD = 32;
constexpr int NA_TILE = 8;                          // queries per tile edge
constexpr int NA_HALO = 14;                         // NA_TILE + 7 - 1 halo slots per edge
constexpr int NA_ROWS = NA_HALO * 16;               // key rows of the P = 16 image
constexpr int NA_ROWB = WIN_ROWB;
constexpr int NA_NT = 8;                            // 16-key tiles (halo rows) per wave: 7 + 1
constexpr int NA_TB = 176;                          // (2 * 7 - 1)^2 = 169 table floats, rounded up
constexpr int NA_SROW = 36;                         // floats per K / V row of the fp32 template
constexpr float NA_SCALE = 0.17677669529663687f;    // 2^-2.5 = 32^-0.5
constexpr float NA_INV_SCALE = 5.656854249492381f;
constexpr float NA_DEAD = -1.0e30f;
constexpr float NA_LOG2E = 1.44269504088896f;

struct NatArgs {
    const void* qkv;
    const float* kvpad;
    const float* table;
    void* out;
    int B, H, W, C, heads, K, Hp, Wp, nTy, nTx, items;
    int* status;
};

__device__ __forceinline__ int na_clamp(int v, int hi) { return min(max(v, 0), hi); }

// geometry of one work item: tile origin, halo origin and live extent
struct NatItem {
    int b, head, Y0, X0, oy, ox, ey, ex;
};
__device__ __forceinline__ NatItem na_item(const NatArgs& a, int item) {
    NatItem it;
    it.head = item % a.heads;
    item /= a.heads;
    const int tx = item % a.nTx;
    item /= a.nTx;
    const int ty = item % a.nTy;
    it.b = item / a.nTy;
    const int r = a.K >> 1;
    it.Y0 = ty * NA_TILE;
    it.X0 = tx * NA_TILE;
    it.oy = na_clamp(it.Y0 - r, a.Hp - a.K);
    it.ox = na_clamp(it.X0 - r, a.Wp - a.K);
    it.ey = na_clamp(min(it.Y0 + NA_TILE - 1, a.H - 1) - r, a.Hp - a.K) + a.K - it.oy;   // <= 14: the clamp is monotone, 1-Lipschitz
    it.ex = na_clamp(min(it.X0 + NA_TILE - 1, a.W - 1) - r, a.Wp - a.K) + a.K - it.ox;
    return it;
}

__global__ __launch_bounds__(256) void nat_attn_kernel(NatArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * NA_ROWS * NA_ROWB + NA_TB * 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const NatItem it = na_item(a, blockIdx.x);
    const int head = it.head, K = a.K, r = K >> 1, tw = 2 * K - 1;
    char* k_lds = smem;
    char* v_lds = smem + NA_ROWS * NA_ROWB;
    float* tb = reinterpret_cast<float*>(smem + 2 * NA_ROWS * NA_ROWB);
    const int ld = 3 * a.C;
    const f16* qkv = static_cast<const f16*>(a.qkv);
    const long img = (long)it.b * a.H * a.W;
    const int l15 = lane & 15, g = lane >> 4;

    // ---- stage K / V of the halo: thread = (row, 16-byte chunk), passes of 64 rows; a pass is one halo row per wave, so the test
    // against the live extent is wave-uniform.  Loads are unconditional: a slot that is not on the map reads a safe address and is
    // replaced afterwards (padded token: kv_pad; dead slot hx >= ex: zeros, its score is -1e30) ----
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
        const int row = ps * 64 + (tid >> 2), ch = tid & 3;
        const int hy = row >> 4, hx = row & 15;
        if (hy >= it.ey) break;
        const int y = it.oy + hy, x = it.ox + hx;
        const bool live = hx < it.ex;
        const bool real = live && y < a.H && x < a.W;
        const f16* src = real ? qkv + (img + (long)y * a.W + x) * ld + a.C + head * NA_HD + ch * 8 : qkv;
        U4H8 kr, vr;
        kr.u = *reinterpret_cast<const uint4*>(src);
        vr.u = *reinterpret_cast<const uint4*>(real ? src + a.C : qkv);
        if (!real) {
            kr.u = vr.u = make_uint4(0, 0, 0, 0);
            if (live && a.kvpad) {                    // a padded token: the qkv Dense's bias
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    kr.e[j] = (f16)a.kvpad[head * NA_HD + ch * 8 + j];
                    vr.e[j] = (f16)a.kvpad[a.C + head * NA_HD + ch * 8 + j];
                }
            }
        }
        *reinterpret_cast<uint4*>(k_lds + row * NA_ROWB + win_k_slot(row, ch) * 16) = kr.u;
        *reinterpret_cast<uint4*>(v_lds + row * NA_ROWB + win_v_chunk(row, ch) * 16) = vr.u;
    }
    for (int i = tid; i < tw * tw; i += 256) tb[i] = a.table[(long)head * tw * tw + i] * NA_INV_SCALE;
    __syncthreads();

    const int qrow0 = it.Y0 + 2 * wave;
    if (qrow0 >= a.H) return;                         // wave-uniform; no barrier follows
    // the lane's query, clamped onto the map for lanes past its edge (nothing is stored for them)
    const int qyr = qrow0 + (l15 >> 3), qxr = it.X0 + (l15 & 7);
    const bool q_ok = qyr < a.H && qxr < a.W;
    const int qy = min(qyr, a.H - 1), qx = min(qxr, a.W - 1);
    const int sy = na_clamp(qy - r, a.Hp - K), sx = na_clamp(qx - r, a.Wp - K);
    U4H8 qf;
    qf.u = *reinterpret_cast<const uint4*>(qkv + (img + (long)qy * a.W + qx) * ld + head * NA_HD + g * 8);
    // halo rows of this wave's two query rows: [t0, t0 + nt), nt <= K + 1 (wave-uniform)
    const int t0 = na_clamp(qrow0 - r, a.Hp - K) - it.oy;
    const int nt = na_clamp(min(qrow0 + 1, a.H - 1) - r, a.Hp - K) + K - it.oy - t0;

    // S^T tiles: rows = keys (halo row t0 + i, hx = 4 g + r), column = this lane's query.  The accumulators START as table / scale for a
    // slot inside the query's block and -1e30 elsewhere and go in as the C operand of S^T = K Q^T + C.
    f32x4 acc[NA_NT];
    {
        int col[4];
        bool okx[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int kx = it.ox + 4 * g + rr;
            okx[rr] = kx >= sx && kx < sx + K;
            col[rr] = kx - qx + K - 1;
        }
#pragma unroll
        for (int i = 0; i < NA_NT; ++i) {
            const int ky = it.oy + t0 + i;
            const bool oky = ky >= sy && ky < sy + K;
            const int rowi = (ky - qy + K - 1) * tw;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const bool ok = oky && okx[rr];
                const float bias = tb[ok ? rowi + col[rr] : 0];
                acc[i][rr] = ok ? bias : NA_DEAD;
            }
        }
    }
    U4H8 kf[NA_NT];
#pragma unroll
    for (int i = 0; i < NA_NT; ++i) {
        const int row = min(t0 + i, it.ey - 1) * 16 + l15;        // a tile past the live rows re-reads the last one; its scores are dead
        kf[i].u = *reinterpret_cast<const uint4*>(k_lds + row * NA_ROWB + win_k_slot(row, g) * 16);
    }
#pragma unroll
    for (int i = 0; i < NA_NT; ++i)
        if (i < nt) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[i].h, qf.h, acc[i], 0, 0, 0);
    const float m = win_score_max<NA_NT>(acc);
    float lsum = 0.f;
#pragma unroll
    for (int i = 0; i < NA_NT; ++i)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const float p = __builtin_amdgcn_exp2f((acc[i][rr] - m) * (NA_SCALE * NA_LOG2E));
            acc[i][rr] = p;
            lsum += p;
        }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);

    // O^T = V^T P^T : A = V^T (two 16-wide head-dim tiles) via transposed LDS reads, B = P^T from the accumulators: MFMA k-slot (g, j)
    // carries key 4 g + j of halo row t0 + 2 s (j < 4) / of halo row t0 + 2 s + 1 (j >= 4).  All operands are complete before the
    // first MFMA.
    const int tr_q = l15 >> 2, tr_p = l15 & 3;
    f32x4 o[2];
    o[0] = o[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    U4H8 pfa[NA_NT / 2];
    union VF {
        fp16x4_t t[2];
        f16x8 v;
    } vfa[NA_NT / 2][2];
#pragma unroll
    for (int s = 0; s < NA_NT / 2; ++s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pfa[s].e[j] = (f16)acc[2 * s][j];
            pfa[s].e[4 + j] = (f16)acc[2 * s + 1][j];
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int row = min(t0 + 2 * s + hh, it.ey - 1) * 16 + 4 * g + tr_q;
                vfa[s][dt].t[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4f16(
                    (__attribute__((address_space(3))) fp16x4_t*)(v_lds + row * NA_ROWB + win_v_half(row, dt) * 32 + tr_p * 8));
            }
    }
#pragma unroll
    for (int s = 0; s < NA_NT / 2; ++s)
        if (2 * s < nt) {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vfa[s][dt].v, pfa[s].h, o[dt], 0, 0, 0);
        }

    // store: lane owns its query, head-dim d = 16 dt + 4 g + (0..3).  Lane pairs (g, g ^ 1) swap one 8-byte half so that every lane
    // holds 8 consecutive channels: one 16-byte store per lane, queries on the map only.
    const float inv = 1.f / lsum;
    union { f16x4 h; unsigned u[2]; } o0, o1, snd, rcv;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        o0.h[rr] = (f16)(o[0][rr] * inv);
        o1.h[rr] = (f16)(o[1][rr] * inv);
    }
    const bool odd = g & 1;
    snd.u[0] = odd ? o0.u[0] : o1.u[0];
    snd.u[1] = odd ? o0.u[1] : o1.u[1];
    rcv.u[0] = __shfl_xor(snd.u[0], 16, 64);
    rcv.u[1] = __shfl_xor(snd.u[1], 16, 64);
    if (q_ok) {
        f16* dst = static_cast<f16*>(a.out) + (img + (long)qy * a.W + qx) * a.C + head * NA_HD + (odd ? 16 + 4 * (g - 1) : 4 * g);
        uint4 v;
        v.x = odd ? rcv.u[0] : o0.u[0];
        v.y = odd ? rcv.u[1] : o0.u[1];
        v.z = odd ? o1.u[0] : rcv.u[0];
        v.w = odd ? o1.u[1] : rcv.u[1];
        *reinterpret_cast<uint4*>(dst) = v;
    }
}

// ---- packed / fp32 storages -------------------------------------------------------------------------------------------------------
struct NA32 {
    static __device__ __forceinline__ f32x4 ld(const void* b, long i) { return *reinterpret_cast<const f32x4*>(static_cast<const float*>(b) + i); }
    static __device__ __forceinline__ void st(void* b, long i, f32x4 v, int*) { *reinterpret_cast<f32x4*>(static_cast<float*>(b) + i) = v; }
};
struct NAH2 {
    static __device__ __forceinline__ f32x4 ld(const void* b, long i) { return h2_ld4(b, i); }
    static __device__ __forceinline__ void st(void* b, long i, f32x4 v, int* status) { h2_st4(b, i, v, status); }
};

template <typename S>
__global__ __launch_bounds__(64) void nat_attn_strict_kernel(NatArgs a) {
    __shared__ __attribute__((aligned(16))) float kl[NA_HALO * NA_HALO * NA_SROW];
    __shared__ __attribute__((aligned(16))) float vl[NA_HALO * NA_HALO * NA_SROW];
    __shared__ float tl[NA_TB];
    const NatItem it = na_item(a, blockIdx.x);
    const int head = it.head, K = a.K, r = K >> 1, tw = 2 * K - 1;
    const int t = threadIdx.x;
    const long ld = 3L * a.C;
    const long img = (long)it.b * a.H * a.W;

    for (int s = t; s < NA_HALO * NA_HALO; s += 64) {
        const int hy = s / NA_HALO, hx = s - hy * NA_HALO;
        if (hy >= it.ey || hx >= it.ex) continue;     // never read: every block lies inside the live extent
        const int y = it.oy + hy, x = it.ox + hx;
        const bool real = y < a.H && x < a.W;
        const long tok = (img + (real ? (long)y * a.W + x : 0)) * ld + head * NA_HD;
#pragma unroll
        for (int d4 = 0; d4 < NA_HD / 4; ++d4) {
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (real) {
                kv = S::ld(a.qkv, tok + a.C + d4 * 4);
                vv = S::ld(a.qkv, tok + 2 * a.C + d4 * 4);
            } else if (a.kvpad) {                     // a padded token: the qkv Dense's bias
                kv = *reinterpret_cast<const f32x4*>(a.kvpad + head * NA_HD + d4 * 4);
                vv = *reinterpret_cast<const f32x4*>(a.kvpad + a.C + head * NA_HD + d4 * 4);
            }
            *reinterpret_cast<f32x4*>(kl + s * NA_SROW + d4 * 4) = kv;
            *reinterpret_cast<f32x4*>(vl + s * NA_SROW + d4 * 4) = vv;
        }
    }
    for (int i = t; i < tw * tw; i += 64) tl[i] = a.table[(long)head * tw * tw + i];
    __syncthreads();
    const int qy = it.Y0 + (t >> 3), qx = it.X0 + (t & 7);
    if (qy >= a.H || qx >= a.W) return;
    const int sy = na_clamp(qy - r, a.Hp - K), sx = na_clamp(qx - r, a.Wp - K);

    float q[NA_HD], o[NA_HD];
    const long qtok = (img + (long)qy * a.W + qx) * ld + head * NA_HD;
#pragma unroll
    for (int d4 = 0; d4 < NA_HD / 4; ++d4) {
        const f32x4 v = S::ld(a.qkv, qtok + d4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) q[d4 * 4 + e] = v[e];
    }
#pragma unroll
    for (int d = 0; d < NA_HD; ++d) o[d] = 0.f;
    float m = -3.0e38f, l = 0.f;
    for (int jy = 0; jy < K; ++jy) {
        const int ky = sy + jy;
        for (int jx = 0; jx < K; ++jx) {
            const int kx = sx + jx;
            const int slot = (ky - it.oy) * NA_HALO + (kx - it.ox);
            const float* kr = kl + slot * NA_SROW;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
            for (int d4 = 0; d4 < NA_HD / 4; ++d4) {
                const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + d4 * 4);
                s0 = fmaf(q[d4 * 4], kv[0], s0);
                s1 = fmaf(q[d4 * 4 + 1], kv[1], s1);
                s2 = fmaf(q[d4 * 4 + 2], kv[2], s2);
                s3 = fmaf(q[d4 * 4 + 3], kv[3], s3);
            }
            const float s = ((s0 + s1) + (s2 + s3)) * NA_SCALE + tl[(ky - qy + K - 1) * tw + (kx - qx + K - 1)];
            if (s > m) {                              // new running maximum: rescale what has been accumulated
                const float al = expf(m - s);
                l *= al;
#pragma unroll
                for (int d = 0; d < NA_HD; ++d) o[d] *= al;
                m = s;
            }
            const float p = expf(s - m);
            l += p;
            const float* vr = vl + slot * NA_SROW;
#pragma unroll
            for (int d4 = 0; d4 < NA_HD / 4; ++d4) {
                const f32x4 vv = *reinterpret_cast<const f32x4*>(vr + d4 * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[d4 * 4 + e] = fmaf(p, vv[e], o[d4 * 4 + e]);
            }
        }
    }
    const long dst = (img + (long)qy * a.W + qx) * a.C + head * NA_HD;
#pragma unroll
    for (int d4 = 0; d4 < NA_HD / 4; ++d4)
        S::st(a.out, dst + d4 * 4, (f32x4){o[d4 * 4] / l, o[d4 * 4 + 1] / l, o[d4 * 4 + 2] / l, o[d4 * 4 + 3] / l}, a.status);
}

// argument checks and geometry shared by the three entry points; no launch
int na_prepare(const char* who, NatArgs& a, const void* qkv, const float* kv_pad, const float* table, void* out, int B, int H, int W, int C,
               int heads, int K, int* status) {
    VIP_REQUIRE(qkv && table && out, VIP_ERR_BAD_ARG, "%s: null pointer (only kv_pad may be null)", who);
    VIP_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && heads > 0, VIP_ERR_BAD_ARG, "%s: non-positive dimension", who);
    VIP_REQUIRE(K == 3 || K == 5 || K == 7, VIP_ERR_UNSUPPORTED, "%s: unsupported kernel_size %d: the kernel serves kernel_size 3, 5 or 7", who, K);
    VIP_REQUIRE(C == heads * NA_HD, VIP_ERR_UNSUPPORTED, "%s: unsupported configuration C=%d heads=%d: needs head_dim = C / heads = 32", who, C,
                heads);
    int Hp = 0, Wp = 0, items = 0;
    VIP_REQUIRE(vip_nat_attn_plan(B, H, W, heads, K, &Hp, &Wp, &items) == 1, VIP_ERR_UNSUPPORTED,
                "%s: too many query tiles (B=%d map %dx%d heads=%d): needs B * tiles * heads < 2^30 and fewer than 2^40 qkv elements", who, B,
                H, W, heads);
    a.qkv = qkv; a.kvpad = kv_pad; a.table = table; a.out = out;
    a.B = B; a.H = H; a.W = W; a.C = C; a.heads = heads; a.K = K;
    a.Hp = Hp; a.Wp = Wp; a.nTy = (H + NA_TILE - 1) / NA_TILE; a.nTx = (W + NA_TILE - 1) / NA_TILE; a.items = items;
    a.status = status;
    return VIP_OK;
}

}  // namespace

extern "C" int vip_nat_attn_plan(int B, int H, int W, int heads, int K, int* Hp, int* Wp, int* items) {
    if (B <= 0 || H <= 0 || W <= 0 || heads <= 0 || !(K == 3 || K == 5 || K == 7)) return 0;
    const long n = (long)B * ((H + NA_TILE - 1) / NA_TILE) * ((W + NA_TILE - 1) / NA_TILE) * heads;
    if (n >= (1L << 30) || (long)B * H * W * 3 * heads * NA_HD >= (1L << 40)) return 0;
    if (Hp) *Hp = H > K ? H : K;
    if (Wp) *Wp = W > K ? W : K;
    if (items) *items = (int)n;
    return 1;
}

extern "C" int vip_nat_attn_fwd_f16(const void* qkv, const float* kv_pad, const float* table, void* out, int B, int H, int W, int C, int heads,
                                    int kernel_size, void* stream) {
    NatArgs a;
    const int st = na_prepare("vip_nat_attn_fwd_f16", a, qkv, kv_pad, table, out, B, H, W, C, heads, kernel_size, nullptr);
    if (st != VIP_OK) return st;
    hipLaunchKernelGGL(nat_attn_kernel, dim3(a.items), dim3(256), 0, (hipStream_t)stream, a);
    return vip_launch_status("vip_nat_attn_fwd_f16");
}

extern "C" int vip_nat_attn_fwd_s32(const float* qkv, const float* kv_pad, const float* table, float* out, int B, int H, int W, int C, int heads,
                                    int kernel_size, void* stream) {
    NatArgs a;
    const int st = na_prepare("vip_nat_attn_fwd_s32", a, qkv, kv_pad, table, out, B, H, W, C, heads, kernel_size, nullptr);
    if (st != VIP_OK) return st;
    hipLaunchKernelGGL(nat_attn_strict_kernel<NA32>, dim3(a.items), dim3(64), 0, (hipStream_t)stream, a);
    return vip_launch_status("vip_nat_attn_fwd_s32");
}

extern "C" int vip_nat_attn_fwd_h2(const void* qkv, const float* kv_pad, const float* table, void* out, int B, int H, int W, int C, int heads,
                                   int kernel_size, int* status, void* stream) {
    NatArgs a;
    const int st = na_prepare("vip_nat_attn_fwd_h2", a, qkv, kv_pad, table, out, B, H, W, C, heads, kernel_size, status);
    if (st != VIP_OK) return st;
    hipLaunchKernelGGL(nat_attn_strict_kernel<NAH2>, dim3(a.items), dim3(64), 0, (hipStream_t)stream, a);
    return vip_launch_status("vip_nat_attn_fwd_h2");
}
