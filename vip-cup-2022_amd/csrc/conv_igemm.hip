// Implicit-GEMM NHWC convolution / dense layer on CDNA4 matrix cores (v_mfma_f32_16x16x32_f16).
//
//   M = B*Ho*Wo output pixels, N = Cout_g, K = kh*kw*Cin_g  (k = (r*kw + s)*Cin_g + c)
//
// Block = 256 threads = 4 waves, tile BM x BN x 64.  Both operands are staged global -> VGPR ->
// LDS in 16-byte chunks (8 halfs of one filter tap), double-buffered so the loads of k-tile t+1
// are in flight while tile t is multiplied (one barrier per k-tile).  Out-of-image taps and the
// M/N/K tails are zero-filled at staging time, so the MFMA loop is branch-free.
//
// Orientation: the WEIGHT fragment is the MFMA "A" operand and the ACTIVATION fragment the "B"
// operand, so each lane ends up holding 4 consecutive output channels of one pixel per MFMA; the
// weight rows a wave feeds to its 4 n-tiles are interleaved (row r of n-tile t = channel
// (t>>1)*32 + (r>>2)*8 + (t&1)*4 + (r&3)) so that one lane owns two runs of 8 consecutive channels of a
// pixel, the epilogue (bias, activation, residual) runs on 16-byte vectors, and the four lanes of a
// pixel write 64 contiguous bytes per store instruction.
//
// LDS image: 128-byte rows (64 halfs), 16-byte chunks XOR-swizzled so that every ds_read_b128 of
// a fragment is bank-conflict free: activation rows use key row&7, weight rows (read in the
// interleaved order above) use key ((row>>3)&3)<<1 | ((row>>1)&1).
//
// Replaces Conv2D+BN+Activation(+Add) of the reference (resnet_rs_model.py:64-84,235-280;
// kecam common_layers.py:190-248; tfimm convnext.py:260-267,320-327) and every Dense layer.
#include "common.hpp"
#include <stdlib.h>
#include <string.h>
#include <type_traits>

// VIP_GEMM_H2 = 1 (conv_h2.hip includes this file a second time): the same kernels for the packed STRICT storage of common.hpp -
// every operand element is an fp16 (hi, lo) pair, 8 channels = [hi x 8][lo x 8] = two 16-byte MFMA fragments.  Seen as halfs, a packed
// tensor is an fp16 tensor with twice the channels, so all staging / addressing / tiling below is shared: ConvArgs carries the
// INPUT side (ldx, cin_off, Cin_g, K, ldw) in halfs (doubled), a 64-half k-chunk is 32 logical k whose eight 16-byte chunks are
// (hi, lo) x 4 k-groups, and LDS images hold them PERMUTED (h2_pos: the four hi chunks first, then the four lo chunks) so that the
// fragment reads are the fp16 kernels' own - "k-step 0" reads the hi plane, "k-step 1" the lo plane.  What differs: three MFMAs per
// fragment pair (w_lo x_hi + w_hi x_hi in k-step 0, w_hi x_lo in k-step 1), direct global fragment loads take chunk 2 lq + plane, and
// the epilogues (fp32 activations, the weights' power-of-two scale undone, packed residual / output, fp16 range check).
#ifndef VIP_GEMM_H2
#define VIP_GEMM_H2 0
#endif

#ifndef VIP_MFMA_PRIO
#define VIP_MFMA_PRIO 1
#endif
#ifndef VIP_MFMA_PRIO_TILE
#define VIP_MFMA_PRIO_TILE 1
#endif

namespace {

constexpr bool H2 = VIP_GEMM_H2;
// LDS position of logical 16-byte chunk c (0..7) of a 64-half row
__device__ __forceinline__ int h2_pos(int c) { return H2 ? (((c & 1) << 2) | (c >> 1)) : c; }
// masked lanes of a packed (32-byte) access: base and base + 16 both stay out of range (spans are checked < 0xFFFFFFE0)
constexpr unsigned OOB2 = 0xFFFFFFE0u;
constexpr int ESZ = H2 ? 4 : 2;          // bytes per output / residual element

struct ConvArgs {
    const f16* x;
    const f16* w;
    const float* bias;
    const f16* res;
    f16* y;
    int H, W, Ho, Wo;
    int Cin_g, Cout_g;
    int kh, kw, sh, sw, pt, pl;
    int ldx, ldy, ldr, ldw;
    int cin_off, cout_off, res_off;
    int M, K;
    long x_span_bytes;  // bytes from x (the tensor base) to the end of the input tensor
    long y_span_bytes, res_span_bytes;
    int bias_elems;
    int act_pre, act_post;
    int m_blocks, n_blocks;
    const f16* w_lo;   // optional low half of the weights, fp16(W32 - fp16(W32)), same layout as w; streaming kernel only
    const f16* gate;   // optional per-image input-channel gate [B][2][K] (hi, lo planes of a squeeze-excite scale, folded into the load); pwk only
    int y_lo_off;      // rows kernel: != 0 -> also write fp16(v - fp16(v)) this many halfs after each output (split gate)
    int gate_hw;       // pixels per image (image index of pixel m = m / gate_hw)
    const f16* ogate;  // optional per-image OUTPUT-channel gate [B][2][Cout] (hi, lo planes), applied to the accumulators in the epilogue
                       // (modes 7 / 8 of pw_gemm_kernel and pwk_direct_kernel; image index from gate_hw)
    int ogate_elems;   // halfs in ogate (buffer descriptor)
    unsigned hw_magic; // min(2^32 / gate_hw, 2^32 - 1): m / gate_hw = umulhi(m, hw_magic), + 1 when the remainder reaches gate_hw
    float out_scale;   // H2: 1 / (power-of-two scale folded into the weights AND the bias), applied to the accumulators
    int* status;       // H2: device word raised to VIP_H2_OVERFLOW when an output does not fit the fp16 range (may be NULL)
    const float* ln_g; // pwx_ln_kernel: LayerNorm scale / shift [K] fp32 over the input row, applied to the activation fragments (else NULL)
    const float* ln_b;
    float ln_eps;
};

// the arguments of the two-output instantiations of the output-gated epilogue (pw_gemm_kernel<.., OG, Y2>, pwk_direct_kernel<.., OG2>)
struct ConvArgs2 : ConvArgs {
    f16* y2;           // second output act2(y): the shape, span and leading dimension of y
};

// What one call launches.  plan() (below the kernels) fills it from the arguments alone - host code, no HIP call, so a dry run
// (vip_conv2d_kernel_name / _variant) is plan() without launch() - and launch() maps it to the instantiation.
enum Family { PW_GEMM, ROWS_GEMM, GEMM8P, PWX, PWK_DIRECT, PWK_GEMM, IM2COL, CONV_IGEMM };
// The epilogue a pointwise kernel carries (the kernels receive it as an int, pw_epilogue_mode below turns it into an instantiation of
// pw_epilogue): act_pre alone - the VIP_ACT_* code itself, 0..4 - or a residual with no act_pre, plain or followed by ReLU, and those
// two again with the output gate (a.ogate; fp16 storage only).  EPI_OTHER: none of these (an activation AND a residual, any other
// act_post) - conv_igemm_kernel's run-time epilogue.
enum EpiMode : int {
    EPI_OTHER = -1,
    EPI_NONE = VIP_ACT_NONE, EPI_RELU = VIP_ACT_RELU, EPI_SILU = VIP_ACT_SILU, EPI_GELU = VIP_ACT_GELU, EPI_SIGMOID = VIP_ACT_SIGMOID,
    EPI_RES = 5, EPI_RES_RELU = 6,
    EPI_OGATE_RES = 7, EPI_OGATE_RES_RELU = 8,
};
constexpr bool epi_out_gated(EpiMode m) { return m == EPI_OGATE_RES || m == EPI_OGATE_RES_RELU; }
struct Plan {
    Family family;
    EpiMode mode;
    int ng, pt, wn, ks, ksc, bm, bn;    // template arguments, those the family has
    bool gated, hilo, ln, xsplit, pipe;
    int m_blocks, n_blocks;             // -> ConvArgs (0 for the kernels that do not read them)
    int n_chunks, nb_ch, lds_stride;    // PW_GEMM: channel chunks (grid y), channels per chunk, LDS row stride in bytes
};

// f(std::integral_constant<int, V>) for the V among Vs that equals v: a plan's template argument back as a compile-time constant
template <int... Vs, class F>
int with_const(int v, F&& f) {
    int st = VIP_ERR_UNSUPPORTED;
    if (!((v == Vs && ((st = f(std::integral_constant<int, Vs>{})), true)) || ...)) vip_set_error("vip_conv2d_nhwc_f16: no instantiation for %d", v);
    return st;
}

// CU count of the device (256 where it cannot be asked): caps the persistent grids of pw_gemm_kernel and gemm8p_kernel
inline int device_cus() {
    static const int cus = [] {
        hipDeviceProp_t pr;
        int dev = 0;
        return (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0)
                   ? pr.multiProcessorCount : 256;
    }();
    return cus;
}

// ---- H2 epilogue core: 8 consecutive channels of one pixel (two accumulator quads) -> activation -> (+ residual) -> post -> packed
// store.  `off` = byte offset of the channel group in y, `roff` in the residual (OOB2 for masked lanes).
template <int ACT, bool RES, int POST>      // POST: 0 none, 1 ReLU, 2 run-time a.act_post
__device__ __forceinline__ void h2_store8(const ConvArgs& a, const f32x4& q0, const f32x4& q1, unsigned off, unsigned roff,
                                          const __amdgpu_buffer_rsrc_t& rb_res, const __amdgpu_buffer_rsrc_t& rb_y) {
    // two values per VALU slot (v_pk_mul / v_pk_fma / v_pk_add_f32): the GELU / swish epilogues of the many-pixel layers are VALU-bound
    // otherwise.  Activations: the packed forms of common.hpp (hardware exp2 / rcp, erfc polynomial: <= 7e-7 absolute).
    f32x2 p[4] = {{q0[0], q0[1]}, {q0[2], q0[3]}, {q1[0], q1[1]}, {q1[2], q1[3]}};
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = vip_act2<ACT>(p[e] * a.out_scale);
    if constexpr (RES) {
        // residual (hi, lo) pairs joined straight into the accumulators: v_fma_mix_f32 takes the fp16 half as an operand (p += hi; p += lo:
        // 4 instructions per pair against 4 conversions + 2 packed adds)
        const uint4 rh = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rb_res, roff, 0, 0));
        const uint4 rl = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rb_res, roff + 16u, 0, 0));
        const unsigned rhw[4] = {rh.x, rh.y, rh.z, rh.w}, rlw[4] = {rl.x, rl.y, rl.z, rl.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float px = p[e].x, py = p[e].y;
            asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel_hi:[1,0,0]" : "+v"(px) : "v"(rhw[e]));
            asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(py) : "v"(rhw[e]));
            asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel_hi:[1,0,0]" : "+v"(px) : "v"(rlw[e]));
            asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(py) : "v"(rlw[e]));
            p[e] = (f32x2){px, py};
        }
    }
    if constexpr (POST == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = (f32x2){fmaxf(p[e].x, 0.f), fmaxf(p[e].y, 0.f)};
    } else if constexpr (POST == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = (f32x2){vip_act_strict(p[e].x, a.act_post), vip_act_strict(p[e].y, a.act_post)};
    }
    // split: hi = rn16(v) (v_cvt_pk_f16_f32), lo = rn16(v - hi) as ONE v_fma_mixlo / mixhi_f16 per value (fma(hi, -1, v) is exact, so
    // this is the same single rounding as converting the fp32 difference).  Range check on the hi halves: a value beyond the fp16 range
    // (or a NaN) converts to an all-ones exponent, and as unsigned 16-bit integers |NaN| > |Inf| > every finite value - one packed
    // integer max per pair, one test per store
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    unsigned hw[4], lw[4];
    u16x2 mx = {0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        hw[e] = __builtin_bit_cast(unsigned, __builtin_convertvector(p[e], f16x2));
        const float px = p[e].x, py = p[e].y;
        asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lw[e]) : "v"(hw[e]), "v"(px));
        asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lw[e]) : "v"(hw[e]), "v"(py));
        mx = __builtin_elementwise_max(mx, __builtin_bit_cast(u16x2, hw[e] & 0x7FFF7FFFu));
    }
    typedef __attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned u32x4;
    const u32x4 oh = {hw[0], hw[1], hw[2], hw[3]}, ol = {lw[0], lw[1], lw[2], lw[3]};
    __builtin_amdgcn_raw_buffer_store_b128(oh, rb_y, off, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(ol, rb_y, off + 16u, 0, 0);
    if (a.status && off != OOB2 && (mx.x >= 0x7C00 || mx.y >= 0x7C00)) *a.status = VIP_H2_OVERFLOW;
}

__device__ __forceinline__ int swz_x(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }
__device__ __forceinline__ int swz_w(int row, int chunk) {
    const int key = (((row >> 3) & 3) << 1) | ((row >> 1) & 1);
    return row * 128 + ((chunk ^ key) << 4);
}

template <int ACT>
__device__ __forceinline__ float act_t(float v) {
    if constexpr (ACT == VIP_ACT_RELU) return v > 0.f ? v : 0.f;
    else if constexpr (ACT == VIP_ACT_SILU) return v * vip_sigmoid(v);
    else if constexpr (ACT == VIP_ACT_GELU) return 0.5f * v * (1.f + vip_erf(v * 0.70710678118654752f));
    else if constexpr (ACT == VIP_ACT_SIGMOID) return vip_sigmoid(v);
    else return v;
}

// Lane owns channels n_first + h*32 + (0..7), h = 0,1, of pixel rows m_base + mt*16.  Branch-free: bias /
// residual / output go through buffer descriptors; masked lanes use an out-of-range offset (loads return
// 0, stores are dropped).
template <int MT, int ACT>
__device__ __forceinline__ void epilogue(const ConvArgs& a, f32x4 (&acc)[MT][4], int m_base, int n_first, int group) {
    constexpr unsigned OOB = 0xFFFFFFF0u;
    const int ch_glob = group * a.Cout_g;
    const __amdgpu_buffer_rsrc_t rb_bias =
        __builtin_amdgcn_make_buffer_rsrc((void*)a.bias, 0, a.bias ? (unsigned)(a.bias_elems * 4) : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb_res =
        __builtin_amdgcn_make_buffer_rsrc((void*)a.res, 0, a.res ? (unsigned)a.res_span_bytes : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb_y = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, (unsigned)a.y_span_bytes, 0x00020000);
    f32x4 bv[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = n_first + h * 32;
        const unsigned off = (n < a.Cout_g) ? (unsigned)((ch_glob + n) * 4) : OOB;
        bv[h][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb_bias, off, 0, 0));
        bv[h][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb_bias, off, 16, 0));
    }
    if constexpr (H2) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int m = m_base + mt * 16;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = n_first + h * 32;
                const bool ok = (m < a.M) & (n < a.Cout_g);
                const unsigned off = ok ? (unsigned)(((long)m * a.ldy + a.cout_off + ch_glob + n) * 4) : OOB2;
                const unsigned roff = (ok && a.res) ? (unsigned)(((long)m * a.ldr + a.res_off + ch_glob + n) * 4) : OOB2;
                // the bias (pre-multiplied by the weights' scale on the host) joins the accumulators before the scale is undone
                const f32x4 q0 = acc[mt][h * 2] + bv[h][0], q1 = acc[mt][h * 2 + 1] + bv[h][1];
                if (a.res) h2_store8<ACT, true, 2>(a, q0, q1, off, roff, rb_res, rb_y);
                else h2_store8<ACT, false, 2>(a, q0, q1, off, roff, rb_res, rb_y);
            }
        }
        return;
    }
    const bool post_relu = a.act_post == VIP_ACT_RELU;
    const bool post_other = a.act_post != VIP_ACT_NONE && !post_relu;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = m_base + mt * 16;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = n_first + h * 32;
            const bool ok = (m < a.M) & (n < a.Cout_g);
            U4H8 r;
            r.u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                rb_res, ok ? (unsigned)((m * a.ldr + a.res_off + ch_glob + n) * 2) : OOB, 0, 0));
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; j += 2) {   // pairs: packed fp32 math (v_pk_add/fma/mul_f32)
                const f32x4 av = acc[mt][h * 2 + (j >> 2)], bb = bv[h][j >> 2];
                const f32x2 s = (f32x2){av[j & 3], av[(j & 3) + 1]} + (f32x2){bb[j & 3], bb[(j & 3) + 1]};
                const f32x2 t = vip_act2<ACT>(s) + (f32x2){(float)r.e[j], (float)r.e[j + 1]};
                v[j] = t.x;
                v[j + 1] = t.y;
                if (post_relu) {
                    v[j] = fmaxf(v[j], 0.f);
                    v[j + 1] = fmaxf(v[j + 1], 0.f);
                }
            }
            if (post_other) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = vip_act(v[j], a.act_post);
            }
            U4H8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o.e[j] = (f16)v[j];
            __builtin_amdgcn_raw_buffer_store_b128(
                __builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, o.u), rb_y,
                ok ? (unsigned)((m * a.ldy + a.cout_off + ch_glob + n) * 2) : OOB, 0, 0);
        }
    }
}

template <int BM, int BN>
__global__ __launch_bounds__(256) void conv_igemm_kernel(ConvArgs a) {
    constexpr int WAVES_N = BN / 64;
    constexpr int WAVES_M = 4 / WAVES_N;
    constexpr int WTM = BM / WAVES_M;  // rows of the block tile owned by one wave
    constexpr int MT = WTM / 16;       // 16-row MFMA tiles per wave
    constexpr int A_IT = BM / 32;      // 16-byte chunks of the activation tile per thread
    constexpr int B_IT = BN / 32;
    constexpr int A_BYTES = BM * 128;
    constexpr int STAGE_BYTES = (BM + BN) * 128;

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int group = blockIdx.z;

    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int mb = bid / a.n_blocks;
    const int nb = bid - mb * a.n_blocks;
    const int m0 = mb * BM;
    const int n0 = nb * BN;

    const f16* __restrict__ xg = a.x + a.cin_off + group * a.Cin_g;
    const f16* __restrict__ wg = a.w + (size_t)group * a.Cout_g * a.ldw;

    // ---- per-thread staging state -----------------------------------------------------------
    const int chunk = tid & 7;
    const int row0 = tid >> 3;  // + 32*i
    int hi0[A_IT], wi0[A_IT];
    int pix0[A_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int m = m0 + row0 + 32 * i;
        if (m < a.M) {
            const int hw = a.Ho * a.Wo;
            const int b = m / hw;
            const int rem = m - b * hw;
            const int ho = rem / a.Wo;
            const int wo = rem - ho * a.Wo;
            hi0[i] = ho * a.sh - a.pt;
            wi0[i] = wo * a.sw - a.pl;
            pix0[i] = b * a.H * a.W;
        } else {
            hi0[i] = -(1 << 28);
            wi0[i] = 0;
            pix0[i] = 0;
        }
    }
    // position of this thread's chunk inside the filter: (tap row r, tap col s, channel cc)
    int cc = chunk * 8, tr = 0, ts = 0;
    while (cc >= a.Cin_g) {
        cc -= a.Cin_g;
        if (++ts == a.kw) { ts = 0; ++tr; }
    }

    uint4 ra[A_IT], rb[B_IT];

    // Buffer descriptors: out-of-range offsets read as zero in hardware, so padding taps, the M/N/K
    // tails and masked rows cost no branch (a "cond ? load : 0" in HIP source compiles to a branch around
    // every load plus a vmcnt(0) per load — 8 dependent memory round trips per k-tile).
    const unsigned x_bytes = (unsigned)min((long)0xFFFFFFF0L, a.x_span_bytes - 2L * (a.cin_off + group * a.Cin_g));
    const unsigned w_bytes = (unsigned)min((long)0xFFFFFFF0L, 2L * a.Cout_g * a.ldw);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)xg, 0, x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)wg, 0, w_bytes, 0x00020000);
    constexpr unsigned OOB = 0xFFFFFFF0u;

    auto load_tiles = [&](int kt) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            const int hi = hi0[i] + tr, wi = wi0[i] + ts;
            const bool ok = (tr < a.kh) & ((unsigned)hi < (unsigned)a.H) & ((unsigned)wi < (unsigned)a.W);
            const unsigned off = (unsigned)(((pix0[i] + hi * a.W + wi) * a.ldx + cc) * 2);
            ra[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, ok ? off : OOB, 0, 0));
        }
        const int k = kt * 64 + chunk * 8;
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int n = n0 + row0 + 32 * i;
            const bool ok = (n < a.Cout_g) & (k < a.K);
            const unsigned off = (unsigned)((n * a.ldw + k) * 2);
            rb[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rw, ok ? off : OOB, 0, 0));
        }
        // advance the filter position by one k-tile (64 halfs)
        cc += 64;
        while (cc >= a.Cin_g) {
            cc -= a.Cin_g;
            if (++ts == a.kw) { ts = 0; ++tr; }
        }
    };
    auto store_tiles = [&](int buf) {
        char* sa = smem + buf * STAGE_BYTES;
        char* sb = sa + A_BYTES;
#pragma unroll
        for (int i = 0; i < A_IT; ++i) *reinterpret_cast<uint4*>(sa + swz_x(row0 + 32 * i, h2_pos(chunk))) = ra[i];
#pragma unroll
        for (int i = 0; i < B_IT; ++i) *reinterpret_cast<uint4*>(sb + swz_w(row0 + 32 * i, h2_pos(chunk))) = rb[i];
    };

    // ---- MFMA fragment addressing -------------------------------------------------------------
    const int wave_m0 = (wave / WAVES_N) * WTM;
    const int wave_n0 = (wave % WAVES_N) * 64;
    const int l15 = lane & 15, lq = lane >> 4;
    const int wrow_base = wave_n0 + (l15 >> 2) * 8 + (l15 & 3);  // + (nt>>1)*32 + (nt&1)*4
    const int xrow_base = wave_m0 + l15;                          // + mt*16

    f32x4 acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = (a.K + 63) >> 6;
    load_tiles(0);
    store_tiles(0);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tiles(kt + 1);
        const char* sa = smem + buf * STAGE_BYTES;
        const char* sb = sa + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int ch = ks * 4 + lq;
            U4H8 wf[4], xf[MT];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) wf[nt].u = *reinterpret_cast<const uint4*>(sb + swz_w(wrow_base + (nt >> 1) * 32 + (nt & 1) * 4, ch));
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) xf[mt].u = *reinterpret_cast<const uint4*>(sa + swz_x(xrow_base + mt * 16, ch));
            if constexpr (H2) {
                // ks = 0: x hi plane against BOTH weight planes; ks = 1: x lo plane against the weights' hi plane only
                U4H8 wl[4];
                if (ks == 0) {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) wl[nt].u = *reinterpret_cast<const uint4*>(sb + swz_w(wrow_base + (nt >> 1) * 32 + (nt & 1) * 4, 4 + lq));
                } else {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) wf[nt].u = *reinterpret_cast<const uint4*>(sb + swz_w(wrow_base + (nt >> 1) * 32 + (nt & 1) * 4, lq));
                }
                if (VIP_MFMA_PRIO_TILE) __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        if (ks == 0) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[nt].h, xf[mt].h, acc[mt][nt], 0, 0, 0);
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt].h, xf[mt].h, acc[mt][nt], 0, 0, 0);
                    }
                if (VIP_MFMA_PRIO_TILE) __builtin_amdgcn_s_setprio(0);
                continue;
            }
            if (VIP_MFMA_PRIO_TILE) __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt].h, xf[mt].h, acc[mt][nt], 0, 0, 0);
            if (VIP_MFMA_PRIO_TILE) __builtin_amdgcn_s_setprio(0);
        }
        if (kt + 1 < nk) store_tiles(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue (one instantiation per activation so the per-element code is straight-line) ----
    const int m_base = m0 + wave_m0 + l15;
    const int n_first = n0 + wave_n0 + lq * 8;
    switch (a.act_pre) {
        case VIP_ACT_RELU: epilogue<MT, VIP_ACT_RELU>(a, acc, m_base, n_first, group); break;
        case VIP_ACT_SILU: epilogue<MT, VIP_ACT_SILU>(a, acc, m_base, n_first, group); break;
        case VIP_ACT_GELU: epilogue<MT, VIP_ACT_GELU>(a, acc, m_base, n_first, group); break;
        case VIP_ACT_SIGMOID: epilogue<MT, VIP_ACT_SIGMOID>(a, acc, m_base, n_first, group); break;
        default: epilogue<MT, VIP_ACT_NONE>(a, acc, m_base, n_first, group); break;
    }
}

// ---- pointwise (1x1, stride 1) / dense layers with short K: weights-stationary streaming kernel -------------
// For K <= 256 the layer is a stream: read K halfs per pixel, write N.  The tile kernel above pays an LDS round
// trip + barrier per k-tile for BOTH operands and re-stages the weights for every 64..128 pixels.  Here:
//   * the block's weight slice [nb_ch x K] is staged into LDS ONCE (rows stored in MFMA-fragment order, row stride
//     32 (mod 64) bytes -> conflict-free ds_read_b128) and the block then walks pixel tiles with a
//     grid-stride loop;
//   * the activation fragment of v_mfma_f32_16x16x32_f16 (B operand: lane = pixel, 8 consecutive k) IS a 16-byte
//     run of an NHWC row, so it is loaded global -> VGPR directly (no LDS, no barrier in the loop) and kept in
//     registers while the wave sweeps all output-channel sub-tiles: every activation byte is read once;
//   * waves never synchronise after the weight staging, so one wave's epilogue (VALU + stores) overlaps the
//     others' loads and MFMAs.
// epilogue of the streaming kernel: the bias is already in the accumulators (it was the MFMA C operand), the
// activation runs two values per VALU slot, and residual / post-ReLU / output-gate code exists only in the variants that use it.
// OGATE: out = post(acc * g[image(m), n] + res) - the squeeze-excite multiply of a block tail whose gate was computed from the layer's
// INPUT (the layer is linear, so mean_hw(y) = W mean_hw(x) + b).  g = hi + lo of the split gate [B][2][Cout] (exact in fp32), the
// multiply is fp32 on the accumulators (bias included), before the residual add and the one fp16 rounding of the store.
// The gates come out of LDS (stage_out_gate below put the rows of the tile's few images there, joined to fp32): fetched from memory per
// pixel they were two more 16-byte loads and sixteen conversions next to every residual load (ResNet-RS stage 1: 193 -> 178 us).
struct GateLds {
    const float* g;     // [images][stride] fp32, image img0 first, channel n0 first
    int img0, stride, n0;
};

// m / gate_hw without a division (hw_magic = min(2^32 / gate_hw, 2^32 - 1): the estimate is at most one short)
__device__ __forceinline__ unsigned image_of(const ConvArgs& a, unsigned m) {
    unsigned img = __umulhi(m, a.hw_magic);
    if (m - img * (unsigned)a.gate_hw >= (unsigned)a.gate_hw) ++img;
    return img;
}

// rows [m_first, m_first + rows) of the output, channels [n0, n0 + nch): g[img - img0][n - n0] = hi + lo for their images, written by
// `nthreads` threads (a wave or the workgroup; the caller synchronises them) -> the first image.  Channels past Cout read as zero.
__device__ __forceinline__ int stage_out_gate(const ConvArgs& a, float* g_lds, int stride, int m_first, int rows, int n0, int nch, int t,
                                              int nthreads) {
    const __amdgpu_buffer_rsrc_t rb_g = __builtin_amdgcn_make_buffer_rsrc((void*)a.ogate, 0, (unsigned)a.ogate_elems * 2u, 0x00020000);
    const int img0 = (int)image_of(a, (unsigned)min(m_first, a.M - 1)), img1 = (int)image_of(a, (unsigned)min(m_first + rows - 1, a.M - 1));
    const int q = nch >> 2;                                  // 4-channel groups per image
    for (int i = t; i < (img1 - img0 + 1) * q; i += nthreads) {
        const int im = i / q, c = (i - im * q) * 4, n = n0 + c;
        const unsigned off = n < a.Cout_g ? ((unsigned)(img0 + im) * 2u * (unsigned)a.Cout_g + (unsigned)n) * 2u : 0xFFFFFFF0u;
        typedef __attribute__((__vector_size__(2 * sizeof(unsigned)))) unsigned u32x2;
        const u32x2 hv = __builtin_amdgcn_raw_buffer_load_b64(rb_g, off, 0, 0);
        const u32x2 lv = __builtin_amdgcn_raw_buffer_load_b64(rb_g, n < a.Cout_g ? off + (unsigned)a.Cout_g * 2u : 0xFFFFFFF0u, 0, 0);
        const f16x4 hh = __builtin_bit_cast(f16x4, hv), ll = __builtin_bit_cast(f16x4, lv);
        f32x4 gv;
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j] = (float)hh[j] + (float)ll[j];
        *reinterpret_cast<f32x4*>(g_lds + im * stride + c) = gv;
    }
    return img0;
}

// Y2 (with OGATE): a second output y2 = fp16(silu(float(y))) from the ROUNDED y, to rb_y2 at y's offsets - the expression of
// scale_add_act_kernel's second output (pointwise.hip), so y2 is bit for bit what that launch computes from y (the next block's act(x)
// of an ECA-NFNet block tail).
template <int PT, int ACT, bool RES, bool POST_RELU, bool OGATE = false, bool Y2 = false>
__device__ __forceinline__ void pw_epilogue(const ConvArgs& a, f32x4 (&acc)[PT][4], int m_base, int n_first,
                                            const __amdgpu_buffer_rsrc_t& rb_res, const __amdgpu_buffer_rsrc_t& rb_y, GateLds gl = GateLds{},
                                            const __amdgpu_buffer_rsrc_t* rb_y2 = nullptr) {
    constexpr unsigned OOB = 0xFFFFFFF0u;
    if constexpr (H2) {
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            const int m = m_base + p * 16;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = n_first + h * 32;
                const bool ok = (m < a.M) & (n < a.Cout_g);
                const unsigned off = ok ? (unsigned)(((long)m * a.ldy + a.cout_off + n) * 4) : OOB2;
                const unsigned roff = (RES && ok) ? (unsigned)(((long)m * a.ldr + a.res_off + n) * 4) : OOB2;
                h2_store8<ACT, RES, POST_RELU ? 1 : 0>(a, acc[p][h * 2], acc[p][h * 2 + 1], off, roff, rb_res, rb_y);
            }
        }
        return;
    }
    static_assert(!(OGATE && H2), "the output gate is carried by the fp16-storage build only");
    static_assert(OGATE || !Y2, "the second output belongs to the output-gated epilogue");
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        const int m = m_base + p * 16;
        int g_row = 0;           // the pixel's image row in the staged gates (rows past M: the first one, their stores are dropped)
        if constexpr (OGATE) g_row = m < a.M ? ((int)image_of(a, (unsigned)m) - gl.img0) * gl.stride - gl.n0 : -gl.n0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = n_first + h * 32;
            const bool ok = (m < a.M) & (n < a.Cout_g);
            U4H8 r;
            f32x4 g0, g1;
            if constexpr (RES)
                r.u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                                    rb_res, ok ? ((unsigned)m * (unsigned)a.ldr + (unsigned)(a.res_off + n)) * 2u : OOB, 0, 0));
            if constexpr (OGATE) {      // (n is inside the staged channel range for every lane: the range is whole 64-channel tiles)
                g0 = *reinterpret_cast<const f32x4*>(gl.g + g_row + n);
                g1 = *reinterpret_cast<const f32x4*>(gl.g + g_row + n + 4);
            }
            U4H8 o;
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const f32x4 av = acc[p][h * 2 + (j >> 2)];
                f32x2 t = vip_act2<ACT>((f32x2){av[j & 3], av[(j & 3) + 1]});
                if constexpr (OGATE) {
                    const f32x4 gq = j < 4 ? g0 : g1;
                    t = t * (f32x2){gq[j & 3], gq[(j & 3) + 1]};
                }
                if constexpr (RES) t = t + (f32x2){(float)r.e[j], (float)r.e[j + 1]};
                if constexpr (POST_RELU) t = (f32x2){fmaxf(t.x, 0.f), fmaxf(t.y, 0.f)};
                o.e[j] = (f16)t.x;
                o.e[j + 1] = (f16)t.y;
            }
            __builtin_amdgcn_raw_buffer_store_b128(
                __builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, o.u), rb_y,
                ok ? ((unsigned)m * (unsigned)a.ldy + (unsigned)(a.cout_off + n)) * 2u : OOB, 0, 0);      // (unsigned: spans < 4 GiB, m * ld * 2 may pass 2^31)
            if constexpr (Y2) {
                U4H8 o2;
#pragma unroll
                for (int j = 0; j < 8; ++j) o2.e[j] = (f16)vip_act((float)o.e[j], VIP_ACT_SILU);
                __builtin_amdgcn_raw_buffer_store_b128(
                    __builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, o2.u), *rb_y2,
                    ok ? ((unsigned)m * (unsigned)a.ldy + (unsigned)(a.cout_off + n)) * 2u : OOB, 0, 0);
            }
        }
    }
}

// The epilogue dispatch of every pointwise kernel: the run-time mode (EpiMode) -> the instantiation of pw_epilogue, for one 64-channel
// group of accumulators.  What an instantiation does with the two output-gated modes is a compile-time property of it (OG):
enum OutGateCases {
    OG_UNKNOWN,     // not cases of their own: like any number that is no mode they take the default (the packed build, and every kernel but
                    // the two below)
    OG_IGNORED,     // cases that do nothing: pwk_direct_kernel<.., GATED = true> of the fp16 build (plan() sends no output gate there)
    OG_CARRIED,     // carried beside the other modes: pwk_direct_kernel<.., GATED = false> (gl: the staged gate rows)
    OG_ALONE,       // nothing else is carried: the kernels of their own that plan() reaches in these modes alone, pw_gemm_kernel<.., OG>
                    // and, with Y2, the two-output form pwk_direct_kernel<.., OG2> (rb_y2: the descriptor of a.y2, made by the kernel from
                    // its own argument - the span of y)
};
template <int PT, OutGateCases OG = OG_UNKNOWN, bool Y2 = false, class Args>      // Args: ConvArgs, or ConvArgs2 as the kernel holds it
__device__ __forceinline__ void pw_epilogue_mode(int mode, const Args& a, f32x4 (&acc)[PT][4], int m_base, int n_first,
                                                 const __amdgpu_buffer_rsrc_t& rb_res, const __amdgpu_buffer_rsrc_t& rb_y, GateLds gl = GateLds{},
                                                 const __amdgpu_buffer_rsrc_t* rb_y2 = nullptr) {
    static_assert(!(H2 && OG != OG_UNKNOWN), "the output gate is carried by the fp16-storage build only");
    static_assert(OG == OG_ALONE || !Y2, "the second output belongs to the instantiations that carry the output gate alone");
    if constexpr (Y2) {
        if (mode == EPI_OGATE_RES_RELU) pw_epilogue<PT, VIP_ACT_NONE, true, true, true, true>(a, acc, m_base, n_first, rb_res, rb_y, gl, rb_y2);
        else pw_epilogue<PT, VIP_ACT_NONE, true, false, true, true>(a, acc, m_base, n_first, rb_res, rb_y, gl, rb_y2);
    } else if constexpr (OG == OG_ALONE) {
        if (mode == EPI_OGATE_RES_RELU) pw_epilogue<PT, VIP_ACT_NONE, true, true, true>(a, acc, m_base, n_first, rb_res, rb_y, gl);
        else pw_epilogue<PT, VIP_ACT_NONE, true, false, true>(a, acc, m_base, n_first, rb_res, rb_y, gl);
    } else {
        switch (mode) {
            case EPI_RELU: pw_epilogue<PT, VIP_ACT_RELU, false, false>(a, acc, m_base, n_first, rb_res, rb_y); break;
            case EPI_SILU: pw_epilogue<PT, VIP_ACT_SILU, false, false>(a, acc, m_base, n_first, rb_res, rb_y); break;
            case EPI_GELU: pw_epilogue<PT, VIP_ACT_GELU, false, false>(a, acc, m_base, n_first, rb_res, rb_y); break;
            case EPI_SIGMOID: pw_epilogue<PT, VIP_ACT_SIGMOID, false, false>(a, acc, m_base, n_first, rb_res, rb_y); break;
            case EPI_RES: pw_epilogue<PT, VIP_ACT_NONE, true, false>(a, acc, m_base, n_first, rb_res, rb_y); break;
            case EPI_RES_RELU: pw_epilogue<PT, VIP_ACT_NONE, true, true>(a, acc, m_base, n_first, rb_res, rb_y); break;
            // (OG_UNKNOWN: the two labels fall through to the default, i.e. are no cases)
            case EPI_OGATE_RES:
                if constexpr (OG != OG_UNKNOWN) {
                    if constexpr (OG == OG_CARRIED) pw_epilogue<PT, VIP_ACT_NONE, true, false, true>(a, acc, m_base, n_first, rb_res, rb_y, gl);
                    break;
                }
                [[fallthrough]];
            case EPI_OGATE_RES_RELU:
                if constexpr (OG != OG_UNKNOWN) {
                    if constexpr (OG == OG_CARRIED) pw_epilogue<PT, VIP_ACT_NONE, true, true, true>(a, acc, m_base, n_first, rb_res, rb_y, gl);
                    break;
                }
                [[fallthrough]];
            default: pw_epilogue<PT, VIP_ACT_NONE, false, false>(a, acc, m_base, n_first, rb_res, rb_y); break;
        }
    }
}

// ... for the NG 64-channel groups of a wave tile (n_lane: the lane's first channel in group 0).  One call per group, not a loop over
// g: with the packed-storage epilogue inlined seven times the unroller gives up and the accumulators would be indexed dynamically,
// i.e. live in scratch.
template <int NG, int PT>
__device__ __forceinline__ void pw_epilogue_groups(int mode, const ConvArgs& a, f32x4 (&acc)[NG][PT][4], int m_base, int n_lane,
                                                   const __amdgpu_buffer_rsrc_t& rb_res, const __amdgpu_buffer_rsrc_t& rb_y) {
    static_assert(NG == 1 || NG == 2, "one call per group below");
    pw_epilogue_mode<PT>(mode, a, acc[0], m_base, n_lane, rb_res, rb_y);
    if constexpr (NG > 1) pw_epilogue_mode<PT>(mode, a, acc[1], m_base, n_lane + 64, rb_res, rb_y);
}

// HILO: the LDS row of a channel holds its fp16 weights followed by their low halves (w_lo); every activation fragment is
// multiplied by both, so the layer computes with ~22-bit weights.  These layers are HBM-bound, the second MFMA is free.
// OG: the instantiations of the output-gated epilogue (modes 7 / 8, nothing else) - kernels of their own, so that the gate's registers
// (two more 16-byte loads per 8 channels, live next to the prefetched tile) cost the un-gated layers nothing.
// Y2 (with OG): the two-output form of the gated epilogue (vip_conv2d_out_gated2_nhwc_f16) - kernels of their own again, and the one
// argument they add (a.y2: ConvArgs2) is theirs alone, so the other instantiations keep their arguments, registers and code.
template <int KS, int PT, bool PRE, bool HILO, bool OG = false, bool Y2 = false>
__global__ __launch_bounds__(256, 2) void pw_gemm_kernel(std::conditional_t<Y2, ConvArgs2, ConvArgs> a, int nb_ch, int lds_stride, int n_tiles,
                                                         int mode) {
    static_assert(OG || !Y2, "the second output belongs to the output-gated instantiations");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int n_chunk0 = blockIdx.y * nb_ch;
    const int nch = min(nb_ch, ((a.Cout_g - n_chunk0) + 63) & ~63);   // channels computed by this block (x64)
    constexpr unsigned OOB = 0xFFFFFFF0u;
    float* bias_lds = reinterpret_cast<float*>(smem + nb_ch * lds_stride);
    // OG: each wave keeps the gate rows of its 64 pixels' images (at most OG_IMAGES: conv2d_plan) behind the bias, [image][nb_ch] fp32
    constexpr int OG_IMAGES = 4;
    float* g_lds = bias_lds + nb_ch + (tid >> 6) * (OG_IMAGES * nb_ch);

    {   // stage the weight slice: LDS row j <-> channel n_chunk0 + (j & ~63) + perm(j & 63) (fragment order)
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
            (void*)a.w, 0, (unsigned)min((long)0xFFFFFFF0L, 2L * a.Cout_g * a.ldw), 0x00020000);
        const __amdgpu_buffer_rsrc_t rwl = __builtin_amdgcn_make_buffer_rsrc(
            (void*)a.w_lo, 0, HILO ? (unsigned)min((long)0xFFFFFFF0L, 2L * a.Cout_g * a.ldw) : 0u, 0x00020000);
        const int cpr = KS * 4;                      // 16-byte chunks per (zero-padded) row
        constexpr int HALVES = HILO ? 2 : 1;
        for (int i = tid; i < nch * cpr * HALVES; i += 256) {
            const int j = i / (cpr * HALVES), c2 = i - j * (cpr * HALVES);
            const int c = c2 < cpr ? c2 : c2 - cpr;
            const int t = (j >> 4) & 3, r = j & 15;
            const int ch = n_chunk0 + (j & ~63) + (t >> 1) * 32 + (r >> 2) * 8 + (t & 1) * 4 + (r & 3);
            const bool ok = (ch < a.Cout_g) & (c * 8 < a.K);
            const unsigned off = ok ? (unsigned)((ch * a.ldw + c * 8) * 2) : OOB;
            const uint4 v = __builtin_bit_cast(uint4, c2 < cpr ? __builtin_amdgcn_raw_buffer_load_b128(rw, off, 0, 0)
                                                               : __builtin_amdgcn_raw_buffer_load_b128(rwl, off, 0, 0));
            // H2: logical chunk c of the row -> (64-half k-chunk c >> 3, permuted position of c & 7)
            *reinterpret_cast<uint4*>(smem + j * lds_stride + (H2 ? ((c2 & ~7) | h2_pos(c2 & 7)) : c2) * 16) = v;
        }
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
            (void*)a.bias, 0, a.bias ? (unsigned)(a.bias_elems * 4) : 0u, 0x00020000);
        for (int i = tid; i < nch; i += 256) {
            const int ch = n_chunk0 + i;
            bias_lds[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, ch < a.Cout_g ? (unsigned)(ch * 4) : OOB, 0, 0));
        }
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.x + a.cin_off), 0, (unsigned)min((long)0xFFFFFFF0L, a.x_span_bytes - 2L * a.cin_off), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb_res =
        __builtin_amdgcn_make_buffer_rsrc((void*)a.res, 0, a.res ? (unsigned)a.res_span_bytes : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb_y = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, (unsigned)a.y_span_bytes, 0x00020000);
    const char* wl = smem + l15 * lds_stride + lq * 16;

    auto load_x = [&](int tile, U4H8 (&xf)[KS][PT]) {
        const int m0 = tile * (64 * PT) + wave * (16 * PT);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                const int m = m0 + p * 16 + l15, k = H2 ? (ks >> 1) * 64 + lq * 16 + (ks & 1) * 8 : ks * 32 + lq * 8;
                const bool ok = (m < a.M) & (k < a.K);
                xf[ks][p].u = __builtin_bit_cast(
                    uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, ok ? (unsigned)((m * a.ldx + k) * 2) : OOB, 0, 0));
            }
    };

    U4H8 xf[KS][PT], xn[PRE ? KS : 1][PRE ? PT : 1];
    int tile = blockIdx.x;
    if (tile < n_tiles) load_x(tile, xf);
    for (; tile < n_tiles; tile += gridDim.x) {
        const int m0 = tile * (64 * PT) + wave * (16 * PT);
        if constexpr (PRE) {
            // next tile's activations: issued now, consumed after this tile's last epilogue (a tile past the end
            // is all out-of-range offsets: no memory traffic)
            load_x(tile + gridDim.x, xn);
        }
        GateLds gl{};
        if constexpr (OG) {     // wave-local: LDS operations of one wave complete in order, the fences keep the compiler to it
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int img0 = stage_out_gate(a, g_lds, nb_ch, __builtin_amdgcn_readfirstlane(m0), 16 * PT, n_chunk0, nch, lane, 64);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            gl = GateLds{g_lds, img0, nb_ch, n_chunk0};
        }
        for (int sub = 0; sub < nch; sub += 64) {
            f32x4 acc[PT][4];
            const char* ws = wl + sub * lds_stride;
            f32x4 bv[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                bv[nt] = *reinterpret_cast<const f32x4*>(bias_lds + sub + (nt >> 1) * 32 + lq * 8 + (nt & 1) * 4);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                U4H8 wf[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) wf[nt].u = *reinterpret_cast<const uint4*>(ws + nt * 16 * lds_stride + ks * 64);
                if constexpr (H2) {
                    // step ks = 2 c + plane of x: the hi plane (even ks) meets the weights' lo (step ks + 1) and hi (step ks) planes, the lo
                    // plane (odd ks) the weights' hi plane (step ks - 1)
                    if ((ks & 1) == 0) {
                        U4H8 wl[4];
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) wl[nt].u = *reinterpret_cast<const uint4*>(ws + nt * 16 * lds_stride + (ks + 1) * 64);
#pragma unroll
                        for (int p = 0; p < PT; ++p)
#pragma unroll
                            for (int nt = 0; nt < 4; ++nt) {
                                acc[p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[nt].h, xf[ks][p].h, ks == 0 ? bv[nt] : acc[p][nt], 0, 0, 0);
                                acc[p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt].h, xf[ks][p].h, acc[p][nt], 0, 0, 0);
                            }
                    } else {
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) wf[nt].u = *reinterpret_cast<const uint4*>(ws + nt * 16 * lds_stride + (ks - 1) * 64);
#pragma unroll
                        for (int p = 0; p < PT; ++p)
#pragma unroll
                            for (int nt = 0; nt < 4; ++nt)
                                acc[p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt].h, xf[ks][p].h, acc[p][nt], 0, 0, 0);
                    }
                    continue;
                }
#pragma unroll
                for (int p = 0; p < PT; ++p)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
                        acc[p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt].h, xf[ks][p].h, ks == 0 ? bv[nt] : acc[p][nt], 0, 0, 0);
                if constexpr (HILO) {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) wf[nt].u = *reinterpret_cast<const uint4*>(ws + nt * 16 * lds_stride + (KS + ks) * 64);
#pragma unroll
                    for (int p = 0; p < PT; ++p)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
                            acc[p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt].h, xf[ks][p].h, acc[p][nt], 0, 0, 0);
                }
            }
            const int m_base = m0 + l15, n_first = n_chunk0 + sub + lq * 8;
            if constexpr (Y2) {
                // (pw_gemm_kernel<.., Y2>: its two calls stay here - through pw_epilogue_mode<PT, OG_ALONE, true> these kernels allocate other registers)
                const __amdgpu_buffer_rsrc_t rb_y2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.y2, 0, (unsigned)a.y_span_bytes, 0x00020000);
                if (mode == EPI_OGATE_RES_RELU) pw_epilogue<PT, VIP_ACT_NONE, true, true, true, true>(a, acc, m_base, n_first, rb_res, rb_y, gl, &rb_y2);
                else pw_epilogue<PT, VIP_ACT_NONE, true, false, true, true>(a, acc, m_base, n_first, rb_res, rb_y, gl, &rb_y2);
            } else {
                pw_epilogue_mode<PT, OG ? OG_ALONE : OG_UNKNOWN>(mode, a, acc, m_base, n_first, rb_res, rb_y, gl);
            }
        }
        if constexpr (PRE) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int p = 0; p < PT; ++p) xf[ks][p] = xn[ks][p];
        } else {
            if (tile + (int)gridDim.x < n_tiles) load_x(tile + gridDim.x, xf);
        }
    }
}

// LDS of the output-gated streaming kernel's gate rows: 4 waves x OG_IMAGES images x nb_ch fp32
constexpr size_t pw_og_lds(int nb_ch) { return (size_t)4 * 4 * nb_ch * 4; }

// the kernel argument of a launch: ConvArgs, or for the two-output instantiations ConvArgs2 with the second output
template <bool Y2>
std::conditional_t<Y2, ConvArgs2, ConvArgs> kernel_args(const ConvArgs& a, f16* y2) {
    std::conditional_t<Y2, ConvArgs2, ConvArgs> ka;
    static_cast<ConvArgs&>(ka) = a;
    if constexpr (Y2) ka.y2 = y2;
    return ka;
}

// OG / Y2: the output-gated instantiations and their two-output form (y2) - the same grid, and the same LDS and prefetch rule for both
template <int KS, int PT, bool HILO, bool OG = false, bool Y2 = false>
int launch_pw(const ConvArgs& a, const Plan& p, hipStream_t s, f16* y2 = nullptr) {
    // (the gated epilogue holds two more 16-byte loads per 8 channels: at KS = 3 it does not fit next to a prefetched tile without scratch)
    constexpr bool PRE = OG ? KS <= 2 : KS <= 3;
    const int n_tiles = (a.M + 64 * PT - 1) / (64 * PT);
    int gx = (2 * device_cus() + p.n_chunks - 1) / p.n_chunks;      // two workgroups per CU
    if (gx > n_tiles) gx = n_tiles;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pw_gemm_kernel<KS, PT, PRE, HILO, OG, Y2>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    hipLaunchKernelGGL((pw_gemm_kernel<KS, PT, PRE, HILO, OG, Y2>), dim3((unsigned)gx, (unsigned)p.n_chunks), dim3(256),
                       (size_t)p.nb_ch * (p.lds_stride + 4) + (OG ? pw_og_lds(p.nb_ch) : 0), s, kernel_args<Y2>(a, y2), p.nb_ch, p.lds_stride,
                       n_tiles, (int)p.mode);
    return vip_launch_status(Y2 ? "vip_conv2d_out_gated2_nhwc_f16(pw)" : "vip_conv2d_nhwc_f16(pw)");
}

// ---- device code shared by the kernels that stream 64-k weight chunks through LDS (pwk_direct_kernel, pwx_body, pwk_gemm_kernel) and,
// where named, gemm8p_kernel ----
// The buffer descriptors of a pointwise kernel's operands: out-of-range offsets read as zero and drop stores, so tails and masked lanes
// cost no branch (see conv_igemm_kernel).
struct PwBuffers {
    __amdgpu_buffer_rsrc_t w, x, res, y, bias;
};
__device__ __forceinline__ PwBuffers pw_buffers(const ConvArgs& a) {
    PwBuffers b;
    b.w = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, (unsigned)min((long)0xFFFFFFF0L, 2L * a.Cout_g * a.ldw), 0x00020000);
    b.x = __builtin_amdgcn_make_buffer_rsrc((void*)(a.x + a.cin_off), 0, (unsigned)min((long)0xFFFFFFF0L, a.x_span_bytes - 2L * a.cin_off),
                                            0x00020000);
    b.res = __builtin_amdgcn_make_buffer_rsrc((void*)a.res, 0, a.res ? (unsigned)a.res_span_bytes : 0u, 0x00020000);
    b.y = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, (unsigned)a.y_span_bytes, 0x00020000);
    b.bias = __builtin_amdgcn_make_buffer_rsrc((void*)a.bias, 0, a.bias ? (unsigned)(a.bias_elems * 4) : 0u, 0x00020000);
    return b;
}

// One k-step (ks = 0 / 1: 32 k, or the hi / lo plane of the packed storage) of a wave's MFMAs: the activation fragments xf of its PT
// pixel tiles against the weight rows of its NG 64-channel groups in an LDS stage.  ws: the lane's fragment address in the first row
// (stage + l15 * ROWB + lq * 16 + ks * 64).
template <int NG, int PT, int ROWB>
__device__ __forceinline__ void pw_mfma_step(f32x4 (&acc)[NG][PT][4], const char* ws, const U4H8 (&xf)[PT], int ks) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        U4H8 wf[4];
        if constexpr (H2) {
            // ks = 0: the x hi fragments against the weights' lo plane (wh + 64) and hi plane (wh); ks = 1: x lo against the hi
            // plane (ws - 64: the caller's ks * 64 points at the lo plane)
            const char* wh = ws - ks * 64;
            U4H8 wl[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) wf[nt].u = *reinterpret_cast<const uint4*>(wh + (g * 64 + nt * 16) * ROWB);
            if (ks == 0) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) wl[nt].u = *reinterpret_cast<const uint4*>(wh + 64 + (g * 64 + nt * 16) * ROWB);
            }
            if (VIP_MFMA_PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int p = 0; p < PT; ++p) {
                    if (ks == 0) acc[g][p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[nt].h, xf[p].h, acc[g][p][nt], 0, 0, 0);
                    acc[g][p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt].h, xf[p].h, acc[g][p][nt], 0, 0, 0);
                }
            if (VIP_MFMA_PRIO) __builtin_amdgcn_s_setprio(0);
            continue;
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) wf[nt].u = *reinterpret_cast<const uint4*>(ws + (g * 64 + nt * 16) * ROWB);
        if (VIP_MFMA_PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int p = 0; p < PT; ++p)
                acc[g][p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt].h, xf[p].h, acc[g][p][nt], 0, 0, 0);
        if (VIP_MFMA_PRIO) __builtin_amdgcn_s_setprio(0);
    }
}

// ---- pointwise (1x1, stride 1) / dense layers, any K: activations direct to registers, weights through LDS ----
// Same operand routing as the streaming kernel, for K too large to keep the weight slice resident: the block's
// [64*NG channels] x 64-k weight chunk is double-buffered in LDS (shared by the 4 waves, one barrier per chunk);
// each wave owns 64 pixels and loads their activation fragments global -> VGPR one chunk ahead.  Against the
// im2col tile kernel this halves LDS traffic (no activation round trip), removes the per-k-tile im2col address
// arithmetic from the VALU (offsets here are linear in k) and gives each wave a 64 x 128 accumulator tile.
// Short-K variant of the kernel below: the activation fragments are fetched global -> VGPR directly (no LDS image,
// one barrier per chunk).  2-5 % faster than the LDS-staged form for K < 768, 5-10 % slower beyond (bench_gemm.py).
// PT = 16-pixel tiles per wave: 4 (256-pixel block tile) by default; 2 / 1 for layers whose 256-pixel grid would leave most of the
// chip idle (7x7 and 13x13 maps with narrow outputs: 98 workgroups for M = 12 544, N = 208) - more, smaller workgroups.
// OG2: the output-gated epilogue with the second output and nothing else (vip_conv2d_out_gated2_nhwc_f16: modes 7 / 8, a.y2 the second
// output's base with the span and leading dimension of y) - kernels of their own with an argument of their own (ConvArgs2): the shared
// kernel's loop sits at the register limit, and it keeps its arguments, registers and code.
template <int NG, bool GATED, int PT = 4, bool OG2 = false>
__global__ __launch_bounds__(256, 2) void pwk_direct_kernel(std::conditional_t<OG2, ConvArgs2, ConvArgs> a, int mode) {
    static_assert(!(OG2 && (GATED || H2)), "the second output: fp16 storage, no input gate");
    constexpr int NB = 64 * NG, ROWB = 160;                  // LDS row: 64 halfs + 32 B pad (stride = 32 mod 64: plan_pw)
    constexpr int STAGE = NB * ROWB;
    constexpr int W_IT = NB / 32;                            // 16-byte weight chunks staged per thread per k-chunk
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    constexpr unsigned OOB = 0xFFFFFFF0u;

    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int mb = bid / a.n_blocks, nb = bid - mb * a.n_blocks;
    const int m0 = mb * (64 * PT) + wave * (16 * PT);
    const int n0 = nb * NB;

    // (pwk_direct_kernel: the descriptors stay single variables - as a PwBuffers the gated instantiations allocate registers differently)
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.w, 0, (unsigned)min((long)0xFFFFFFF0L, 2L * a.Cout_g * a.ldw), 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.x + a.cin_off), 0, (unsigned)min((long)0xFFFFFFF0L, a.x_span_bytes - 2L * a.cin_off), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb_res =
        __builtin_amdgcn_make_buffer_rsrc((void*)a.res, 0, a.res ? (unsigned)a.res_span_bytes : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb_y = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, (unsigned)a.y_span_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb_bias =
        __builtin_amdgcn_make_buffer_rsrc((void*)a.bias, 0, a.bias ? (unsigned)(a.bias_elems * 4) : 0u, 0x00020000);

    // weight staging: thread -> (LDS row j = tid/8 + 32 i, 16-byte chunk c = tid%8); row j holds channel perm(j)
    // (pwk_direct_kernel: its own copy of the set-up it shares with pwk_gemm_kernel - as one struct with load / store members every
    // instantiation of both kernels changed)
    const int wc = tid & 7;
    unsigned w_off[W_IT];
    int w_lds[W_IT];
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
        const int j = (tid >> 3) + 32 * i;
        const int t = (j >> 4) & 3, r = j & 15;
        const int ch = n0 + (j & ~63) + (t >> 1) * 32 + (r >> 2) * 8 + (t & 1) * 4 + (r & 3);
        w_off[i] = ch < a.Cout_g ? (unsigned)((ch * a.ldw + wc * 8) * 2) : OOB;
        w_lds[i] = j * ROWB + h2_pos(wc) * 16;
    }
    // activation rows of this lane: pixel m0 + 16 p + l15, k offset lq*8 (+ 32 ks + 64 chunk)
    unsigned x_off[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        const int m = m0 + p * 16 + l15;
        // H2: the lane's k-group is the 32-byte (hi, lo) pair lq of the 64-half chunk; plane `ks` is 16 bytes further
        x_off[p] = m < a.M ? (unsigned)((m * a.ldx + lq * (H2 ? 16 : 8)) * 2) : 0xFFFF0000u;   // + k bytes stays out of range
    }
    // squeeze-excite gate folded into the activation operand: x[m, k] * (hi + lo)[image(m), k] as fma(x, hi, x * lo) in
    // packed fp16 - the product is rounded once, per element; the gate itself carries ~22 bits (see se_gate.hip)
    const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.gate, 0, GATED ? (unsigned)min((long)0xFFFFFFF0L, (H2 ? 2L : 4L) * ((a.M + a.gate_hw - 1) / a.gate_hw) * a.K) : 0u, 0x00020000);
    // H2: the gate is a packed [B][Cin] tensor (a.K = 2 Cin halfs per image); the lane's 8 channels are the 32-byte pair lq of the chunk
    unsigned g_off[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        const int m = m0 + p * 16 + l15;
        g_off[p] = (GATED && m < a.M) ? (H2 ? (unsigned)((m / a.gate_hw) * a.K * 2 + lq * 32) : (unsigned)(((m / a.gate_hw) * 2 * a.K + lq * 8) * 2))
                                      : 0xFFFF0000u;
    }
    const int nk = (a.K + 63) >> 6;

    uint4 wst[W_IT];
    auto load_w = [&](int kc) {
        const bool ok = kc * 64 + wc * 8 < a.K;
#pragma unroll
        for (int i = 0; i < W_IT; ++i)
            wst[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rw, ok ? w_off[i] + kc * 128 : OOB, 0, 0));
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int i = 0; i < W_IT; ++i) *reinterpret_cast<uint4*>(smem + buf * STAGE + w_lds[i]) = wst[i];
    };
    U4H8 xf[2][PT], gq[GATED ? 2 : 1][GATED ? PT : 1];      // gq: the gate planes (hi, lo) of ONE k-step
    auto load_x = [&](int kc, int ks) {
        // weights of the K tail are zero in LDS, but 0 * (Inf/NaN garbage of the next row) is NaN: mask the lanes
        const bool ok = kc * 64 + (H2 ? lq * 16 + ks * 8 : ks * 32 + lq * 8) < a.K;
#pragma unroll
        for (int p = 0; p < PT; ++p)
            xf[ks][p].u = __builtin_bit_cast(
                uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, ok ? x_off[p] + kc * 128 + ks * (H2 ? 16 : 64) : OOB, 0, 0));
    };
    // Gate fragments run one k-step ahead of their use in ONE register set (a second prefetched set does not fit next to
    // the accumulators): gate_x(ks) folds them into xf[ks] - fma(x, hi, x * lo) in packed fp16 - and the set is
    // re-requested at once for the following k-step, landing under the MFMAs in between.  The buffer is [B][2][K]
    // halfs, L1/L2-resident.
    auto load_g = [&](int kc, int ks) {
        if constexpr (GATED && H2) {         // both planes of the chunk's gate values, once per chunk (ks unused)
            const bool ok = kc * 64 + lq * 16 < a.K;
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                gq[0][p].u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rg, ok ? g_off[p] + kc * 128 : OOB, 0, 0));
                gq[1][p].u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rg, ok ? g_off[p] + kc * 128 + 16 : OOB, 0, 0));
            }
        } else if constexpr (GATED) {
            const bool ok = kc * 64 + ks * 32 + lq * 8 < a.K;
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                gq[0][p].u = __builtin_bit_cast(
                    uint4, __builtin_amdgcn_raw_buffer_load_b128(rg, ok ? g_off[p] + kc * 128 + ks * 64 : OOB, 0, 0));
                gq[1][p].u = __builtin_bit_cast(
                    uint4, __builtin_amdgcn_raw_buffer_load_b128(rg, ok ? g_off[p] + kc * 128 + ks * 64 + 2 * a.K : OOB, 0, 0));
            }
        }
    };
    auto gate_x = [&](int ks) {
        if constexpr (GATED && H2) {         // (x_hi + x_lo) * (g_hi + g_lo) in fp32, split again: both planes of the chunk at once
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                float xv[8], gv[8];
                h2_join8(xf[0][p], xf[1][p], xv);
                h2_join8(gq[0][p], gq[1][p], gv);
#pragma unroll
                for (int j = 0; j < 8; ++j) xv[j] *= gv[j];
                h2_split8(xv, xf[0][p], xf[1][p]);
            }
        } else if constexpr (GATED) {
#pragma unroll
            for (int p = 0; p < PT; ++p)                                              // 4 x (v_pk_mul_f16 + v_pk_fma_f16)
                xf[ks][p].h = __builtin_elementwise_fma(xf[ks][p].h, gq[0][p].h, xf[ks][p].h * gq[1][p].h);
        }
    };

    f32x4 acc[NG][PT][4];
    {   // bias is the C operand of the first MFMA of every accumulator  (pwk_direct_kernel: the loop stays a copy here, in pwx_body,
        // pwk_gemm_kernel and gemm8p_kernel - as one function, forced inline or not, it changed the code of all four)
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = n0 + g * 64 + (nt >> 1) * 32 + lq * 8 + (nt & 1) * 4;
                const f32x4 bv = __builtin_bit_cast(
                    f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb_bias, n < a.Cout_g ? (unsigned)(n * 4) : OOB, 0, 0));
#pragma unroll
                for (int p = 0; p < PT; ++p) acc[g][p][nt] = bv;
            }
    }

    load_w(0);
    load_x(0, 0);
    load_x(0, 1);
    load_g(0, 0);
    store_w(0);
    __syncthreads();

    auto compute = [&](int buf, int ks) {
        pw_mfma_step<NG, PT, ROWB>(acc, smem + buf * STAGE + l15 * ROWB + lq * 16 + ks * 64, xf[ks], ks);
    };

    // One activation register set: the fragments of k-step ks are re-loaded for the NEXT chunk as soon as this
    // chunk's MFMAs on them are issued, so each load has the other k-step's 32 MFMAs (plus the second resident
    // wave) to land.  Everything in the loop is unconditional (a chunk past the end is all out-of-range offsets:
    // zeros, no memory traffic): a branch around a prefetch makes hipcc fold the "loads skipped" path into its
    // vmcnt bookkeeping and the next MFMA then waits for loads that were only just issued.
    for (int kc = 0; kc < nk; ++kc) {
        const int buf = kc & 1;
        load_w(kc + 1);
        __builtin_amdgcn_sched_barrier(0);   // pin the issue points: the scheduler otherwise sinks every load below
        if constexpr (GATED && H2) {         // the MFMAs, right in front of its wait
            gate_x(0);                       // both planes of chunk kc
            __builtin_amdgcn_sched_barrier(0);
            load_g(kc + 1, 0);
            __builtin_amdgcn_sched_barrier(0);
        } else if constexpr (GATED) {
            gate_x(0);
            __builtin_amdgcn_sched_barrier(0);
            load_g(kc, 1);
            __builtin_amdgcn_sched_barrier(0);
        }
        compute(buf, 0);
        __builtin_amdgcn_sched_barrier(0);
        load_x(kc + 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (GATED && !H2) {
            gate_x(1);
            __builtin_amdgcn_sched_barrier(0);
            load_g(kc + 1, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        compute(buf, 1);
        __builtin_amdgcn_sched_barrier(0);
        load_x(kc + 1, 1);
        store_w(buf ^ 1);
        __syncthreads();
    }

    // opaque to the optimiser: otherwise the epilogue's address arithmetic is hoisted above the k-loop and its
    // ~20 registers stay live through it (the loop is at the 256-VGPR limit of two waves per SIMD)
    int m_base = m0 + l15, n_lane = n0 + lq * 8;
    asm volatile("" : "+v"(m_base), "+v"(n_lane));
    // output gate: the instantiations without the INPUT gate alone (plan() sends no other one here with an output gate)
    constexpr OutGateCases OG = OG2 ? OG_ALONE : H2 ? OG_UNKNOWN : GATED ? OG_IGNORED : OG_CARRIED;
    GateLds gl{};
    if constexpr (OG == OG_CARRIED || OG == OG_ALONE) {
        if (mode >= EPI_OGATE_RES) {    // the weight stages are free after the loop's last barrier - the gate rows of the block's images go there
            float* g_lds = reinterpret_cast<float*>(smem);
            const int img0 = stage_out_gate(a, g_lds, NB, mb * (64 * PT), 64 * PT, n0, NB, (int)threadIdx.x, 256);
            __syncthreads();
            gl = GateLds{g_lds, img0, NB, n0};
        }
    }
    // (pwk_direct_kernel: the per-group call keeps its lambda - called through pw_epilogue_groups the gated instantiations allocate other
    // registers in the k-loop)
    auto epi = [&](auto gtag) {
        constexpr int G_ = decltype(gtag)::value;
        const int n_first = n_lane + G_ * 64;
        if constexpr (OG2) {
            const __amdgpu_buffer_rsrc_t rb_y2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.y2, 0, (unsigned)a.y_span_bytes, 0x00020000);
            pw_epilogue_mode<PT, OG, true>(mode, a, acc[G_], m_base, n_first, rb_res, rb_y, gl, &rb_y2);
        } else {
            pw_epilogue_mode<PT, OG>(mode, a, acc[G_], m_base, n_first, rb_res, rb_y, gl);
        }
    };
    epi(std::integral_constant<int, 0>{});
    if constexpr (NG > 1) epi(std::integral_constant<int, 1>{});
}


// ---- pointwise / dense layers with SHORT K and WIDE N: activations resident in registers, weights streamed over all of N ----
// pwk_direct_kernel gives every 128-channel slice of the output its own workgroup: with K <= 256 that workgroup runs 2-4 k-chunks, so its
// life is one pipeline fill (the first weight chunk and activation fragments: ~2 us of L2 / HBM latency) and one drain (the epilogue)
// around ~1 us of MFMAs, and each of the N / 128 workgroups of a pixel tile fetches the same activations again (PMC, round 3: matrix
// pipe 30 % busy, half of a wave's life in s_waitcnt).  Here a workgroup keeps the activation fragments of ALL of K in registers
// (KSC 64-half chunks: <= 64 VGPRs at 32 pixels per wave) and walks over every 128-channel tile of N: the weight chunks of
// (tile, chunk) pairs stream through the same double-buffered LDS image back to back - the prefetch of tile t+1's first chunk is issued
// under tile t's last MFMAs, so there is one fill per workgroup instead of one per 128 channels - and the activations are read once.
//
// LN = true (pwx_ln_kernel, vip_ln_gemm_bias_act_f16): the rows are LayerNorm-ed over K on their way in.  A row's K channels sit in the
// four lanes (l15, lq = 0..3) of its pixel, so once the fragments have landed the statistics are in-lane sums over the lane's 8-channel
// groups plus two lane exchanges (as ln_fragments of mlp_fused.hip): fp32 two-pass mean / variance and the expression of layernorm_kernel
// (pointwise.hip), and the normalised row is rounded to fp16 IN PLACE - the MFMA operand is what the stand-alone launch would have
// stored, without its write and the read back (2 x M x K x 2 bytes per layer).  Replaces LayerNormalization -> Dense of the reference
// (tfimm vit.py:170-227 norm1 -> qkv and norm2 -> fc1, convnext.py:220-229 norm -> fc1, gcvit/layers/block.py:60-81).
template <int KSC, int PT, bool LN>
__device__ __forceinline__ void pwx_body(const ConvArgs& a, int mode) {
    constexpr int NG = 2, NB = 64 * NG, ROWB = 160;
    constexpr int STAGE = NB * ROWB;
    constexpr int W_IT = NB / 32;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    constexpr unsigned OOB = 0xFFFFFFF0u;

    const int bid = xcd_remap(blockIdx.x, gridDim.x);    // XCD-contiguous pixel tiles
    const int m0 = bid * (64 * PT) + wave * (16 * PT);

    const PwBuffers rb = pw_buffers(a);

    // weight staging: thread -> (LDS row j = tid/8 + 32 i, 16-byte chunk c = tid%8); row j holds channel n0 + perm(j)
    const int wc = tid & 7;
    int w_ch[W_IT], w_lds[W_IT];
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
        const int j = (tid >> 3) + 32 * i;
        const int t = (j >> 4) & 3, r = j & 15;
        w_ch[i] = (j & ~63) + (t >> 1) * 32 + (r >> 2) * 8 + (t & 1) * 4 + (r & 3);
        w_lds[i] = j * ROWB + h2_pos(wc) * 16;
    }
    uint4 wst[W_IT];
    auto load_w = [&](int n0, int kc) {
        const bool okk = kc * 64 + wc * 8 < a.K;
#pragma unroll
        for (int i = 0; i < W_IT; ++i) {
            const int ch = n0 + w_ch[i];
            wst[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                                   rb.w, (okk && ch < a.Cout_g) ? (unsigned)((ch * a.ldw + wc * 8) * 2) + kc * 128 : OOB, 0, 0));
        }
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int i = 0; i < W_IT; ++i) *reinterpret_cast<uint4*>(smem + buf * STAGE + w_lds[i]) = wst[i];
    };

    // the activation fragments of the whole K axis (masked beyond K: the weights there are zero in LDS, but 0 * garbage may be NaN)
    U4H8 xf[2 * KSC][PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        const int m = m0 + p * 16 + l15;
        // (unsigned: m * ldx * 2 passes 2^31 on the large maps; the span is checked < 4 GiB by the host)
        const unsigned xo = m < a.M ? ((unsigned)m * (unsigned)a.ldx + (unsigned)(lq * (H2 ? 16 : 8))) * 2u : 0xFFFF0000u;
#pragma unroll
        for (int kc = 0; kc < KSC; ++kc)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bool ok = kc * 64 + (H2 ? lq * 16 + ks * 8 : ks * 32 + lq * 8) < a.K;
                xf[2 * kc + ks][p].u = __builtin_bit_cast(
                    uint4, __builtin_amdgcn_raw_buffer_load_b128(rb.x, ok ? xo + kc * 128 + ks * (H2 ? 16 : 64) : OOB, 0, 0));
            }
    }
    if constexpr (LN && !H2) {
        // fragment i = 2 kc + ks of a lane holds channels 64 kc + 32 ks + 8 lq + 0..7.  Channels beyond K (the K tail, and whole
        // chunks when K < 64 KSC) were loaded as zeros: they add nothing to the sum, are left out of the squared deviations, and
        // must STAY zero - their gamma and beta are staged as zeros, so a masked channel gets d * 0 + 0 = 0 (d is finite)
        // (beta must not leak into a channel whose weights are only zero in LDS: see the note at xf).  Rows beyond M are all
        // zeros: mean 0, rstd = rsqrt(eps), finite, and never stored.
        // gamma / beta: staged once per workgroup (zeros beyond K), read back per fragment with the lane's own 8-channel offsets
        __shared__ __attribute__((aligned(16))) float lnp[2][64 * KSC];
        for (int c = tid; c < 64 * KSC; c += 256) {
            lnp[0][c] = c < a.K ? a.ln_g[c] : 0.f;
            lnp[1][c] = c < a.K ? a.ln_b[c] : 0.f;
        }
        __syncthreads();
        const float fk = (float)a.K;
        float mean[PT], rstd[PT];
        // the fp16 fragments are converted again in every pass: opaque between the passes, or the compiler keeps the fp32 copies of the
        // whole tile live (2 x 8 KSC x PT registers) and spills
        auto pin = [&]() {
#pragma unroll
            for (int i = 0; i < 2 * KSC; ++i)
#pragma unroll
                for (int p = 0; p < PT; ++p) {
                    unsigned t0 = xf[i][p].u.x, t1 = xf[i][p].u.y, t2 = xf[i][p].u.z, t3 = xf[i][p].u.w;
                    asm volatile("" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3));
                    xf[i][p].u = make_uint4(t0, t1, t2, t3);
                }
        };
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 2 * KSC; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) sum += (float)xf[i][p].e[j];
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            mean[p] = sum / fk;
            pin();
            float sq = 0.f;
#pragma unroll
            for (int i = 0; i < 2 * KSC; ++i) {
                const bool ok = (i >> 1) * 64 + (i & 1) * 32 + lq * 8 < a.K;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float d = ok ? (float)xf[i][p].e[j] - mean[p] : 0.f;
                    sq += d * d;
                }
            }
            sq += __shfl_xor(sq, 16, 64);
            sq += __shfl_xor(sq, 32, 64);
            rstd[p] = rsqrtf(sq / fk + a.ln_eps);
            pin();
        }
#pragma unroll
        for (int i = 0; i < 2 * KSC; ++i) {
            const int c0 = (i >> 1) * 64 + (i & 1) * 32 + lq * 8;
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(&lnp[0][c0]), g1 = *reinterpret_cast<const f32x4*>(&lnp[0][c0 + 4]);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(&lnp[1][c0]), b1 = *reinterpret_cast<const f32x4*>(&lnp[1][c0 + 4]);
#pragma unroll
            for (int p = 0; p < PT; ++p)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float gg = j < 4 ? g0[j & 3] : g1[j & 3], bb = j < 4 ? b0[j & 3] : b1[j & 3];
                    xf[i][p].e[j] = (f16)(((float)xf[i][p].e[j] - mean[p]) * rstd[p] * gg + bb);
                }
            // one fragment pair at a time: left alone, every gamma / beta read (16 registers per pair) is hoisted above the arithmetic
            // and spills.  The finished fragments are operands of an opaque statement the next pair's LDS reads cannot cross.
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                unsigned t0 = xf[i][p].u.x, t1 = xf[i][p].u.y, t2 = xf[i][p].u.z, t3 = xf[i][p].u.w;
                asm volatile("" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3) : : "memory");
                xf[i][p].u = make_uint4(t0, t1, t2, t3);
            }
        }
        __builtin_amdgcn_sched_barrier(0);      // the prologue is over before the weight pipeline starts
    }

    f32x4 acc[NG][PT][4];
    auto init_acc = [&](int n0) {     // bias is the C operand of the first MFMA of every accumulator  (pwx_body: a copy, see pwk_direct_kernel)
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = n0 + g * 64 + (nt >> 1) * 32 + lq * 8 + (nt & 1) * 4;
                const f32x4 bv = __builtin_bit_cast(
                    f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb.bias, n < a.Cout_g ? (unsigned)(n * 4) : OOB, 0, 0));
#pragma unroll
                for (int p = 0; p < PT; ++p) acc[g][p][nt] = bv;
            }
    };
    // (pwx_body: its own copy of pw_mfma_step - with the shared one the packed build's pwx_kernel allocates other registers)
    auto compute = [&](int buf, int ks, const U4H8 (&xk)[2][PT]) {
        const char* ws = smem + buf * STAGE + l15 * ROWB + lq * 16 + ks * 64;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            U4H8 wf[4];
            if constexpr (H2) {      // ks = 0: x hi against the weights' lo and hi planes; ks = 1: x lo against the hi plane
                const char* wh = ws - ks * 64;
                U4H8 wl[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) wf[nt].u = *reinterpret_cast<const uint4*>(wh + (g * 64 + nt * 16) * ROWB);
                if (ks == 0) {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) wl[nt].u = *reinterpret_cast<const uint4*>(wh + 64 + (g * 64 + nt * 16) * ROWB);
                }
                if (VIP_MFMA_PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int p = 0; p < PT; ++p) {
                        if (ks == 0) acc[g][p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[nt].h, xk[0][p].h, acc[g][p][nt], 0, 0, 0);
                        acc[g][p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt].h, xk[ks][p].h, acc[g][p][nt], 0, 0, 0);
                    }
                if (VIP_MFMA_PRIO) __builtin_amdgcn_s_setprio(0);
                continue;
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) wf[nt].u = *reinterpret_cast<const uint4*>(ws + (g * 64 + nt * 16) * ROWB);
            if (VIP_MFMA_PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int p = 0; p < PT; ++p) acc[g][p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt].h, xk[ks][p].h, acc[g][p][nt], 0, 0, 0);
            if (VIP_MFMA_PRIO) __builtin_amdgcn_s_setprio(0);
        }
    };

    const int n_tiles = (a.Cout_g + NB - 1) / NB;
    load_w(0, 0);
    store_w(0);
    __syncthreads();
    int buf = 0;
#pragma unroll 1
    for (int t = 0; t < n_tiles; ++t) {
        const int n0 = t * NB;
        init_acc(n0);
#pragma unroll
        for (int kc = 0; kc < KSC; ++kc) {
            // next (tile, chunk) pair; past the last tile every offset is out of range (zeros, no traffic)
            if (kc + 1 < KSC) load_w(n0, kc + 1);
            else load_w(n0 + NB, 0);
            __builtin_amdgcn_sched_barrier(0);
            U4H8 xk[2][PT];
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                xk[0][p] = xf[2 * kc][p];
                xk[1][p] = xf[2 * kc + 1][p];
            }
            compute(buf, 0, xk);
            compute(buf, 1, xk);
            __builtin_amdgcn_sched_barrier(0);
            store_w(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
        int m_base = m0 + l15, n_lane = n0 + lq * 8;
        asm volatile("" : "+v"(m_base), "+v"(n_lane));      // (as in pwk_direct_kernel)
        pw_epilogue_groups<NG, PT>(mode, a, acc, m_base, n_lane, rb.res, rb.y);
    }
}

template <int KSC, int PT>
__global__ __launch_bounds__(256, 2) void pwx_kernel(ConvArgs a, int mode) {
    pwx_body<KSC, PT, false>(a, mode);
}

template <int KSC, int PT>
__global__ __launch_bounds__(256, 2) void pwx_ln_kernel(ConvArgs a, int mode) {
    pwx_body<KSC, PT, true>(a, mode);
}

template <int KSC, int PT, bool LN>
int launch_pwx(const ConvArgs& a, int mode, hipStream_t s) {
    if constexpr (LN) hipLaunchKernelGGL((pwx_ln_kernel<KSC, PT>), dim3((unsigned)a.m_blocks), dim3(256), 0, s, a, mode);
    else hipLaunchKernelGGL((pwx_kernel<KSC, PT>), dim3((unsigned)a.m_blocks), dim3(256), 0, s, a, mode);
    return vip_launch_status(LN ? "vip_ln_gemm_bias_act_f16" : "vip_conv2d_nhwc_f16(pwx)");
}

template <int NG, int WN, bool IM2COL>
__global__ __launch_bounds__(256 * WN, WN == 1 ? 2 : 1) void pwk_gemm_kernel(ConvArgs a, int mode) {
    // IM2COL: the same kernel for k x k / strided / grouped convolutions - only the activation staging changes (each
    // 16-byte chunk of a k-chunk belongs to one filter tap: the lane's tap and channel come from one division per
    // chunk, the pixel coordinates of its rows are precomputed); group = blockIdx.y.
    if constexpr (IM2COL) {
        const int group = blockIdx.y;
        a.x += group * a.Cin_g;
        a.w += (size_t)group * a.Cout_g * a.ldw;
        if (a.bias) a.bias += group * a.Cout_g;
        a.bias_elems -= group * a.Cout_g;
        a.cout_off += group * a.Cout_g;
        a.res_off += group * a.Cout_g;
        a.x_span_bytes -= 2L * group * a.Cin_g;
    }
    // 4 x WN waves: wave (wm, wn) owns pixels 64 wm .. +63 and channels (64 NG) wn .. of the 256 x (64 NG WN) block tile.
    // WN = 2 halves the L2 traffic of the activations (each activation image feeds two waves) at the same number of
    // resident waves per CU (one 8-wave workgroup instead of two 4-wave ones).
    constexpr int PT = 4, NB = 64 * NG, NBLK = NB * WN, ROWB = 160;   // LDS row: 64 halfs + 32 B pad (32 mod 64: plan_pw)
    constexpr int NTHR = 256 * WN;
    constexpr int STAGE = NBLK * ROWB;
    constexpr int W_IT = NBLK * 8 / NTHR;                    // 16-byte weight chunks staged per thread per k-chunk (4)
    constexpr int X_IT = 256 * 8 / NTHR;                     // 16-byte activation chunks per thread per k-chunk (8 / WN)
    constexpr int XS = 64 * ROWB;                            // one activation image: 64 pixels x 64 k
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 weight stages][4 activation images]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 3, wn = wave >> 2;
    const int l15 = lane & 15, lq = lane >> 4;
    constexpr unsigned OOB = 0xFFFFFFF0u;

    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int mb = bid / a.n_blocks, nb = bid - mb * a.n_blocks;
    const int mblk = mb * 256;                               // first pixel of the block tile
    const int m0 = mblk + wm * 64;                           // first pixel of this wave
    const int nblk = nb * NBLK;
    const int n0 = nblk + wn * NB;

    const PwBuffers rb = pw_buffers(a);

    // weight staging: thread -> (LDS row j = tid/8 + (NTHR/8) i, 16-byte chunk c = tid%8); row j holds channel perm(j)
    // (pwk_gemm_kernel: pwk_direct_kernel's set-up with NTHR / 8 for 32 and nblk for n0, a copy for the reason given there)
    const int wc = tid & 7;
    unsigned w_off[W_IT];
    int w_lds[W_IT];
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
        const int j = (tid >> 3) + (NTHR / 8) * i;
        const int t = (j >> 4) & 3, r = j & 15;
        const int ch = nblk + (j & ~63) + (t >> 1) * 32 + (r >> 2) * 8 + (t & 1) * 4 + (r & 3);
        w_off[i] = ch < a.Cout_g ? (unsigned)((ch * a.ldw + wc * 8) * 2) : OOB;
        w_lds[i] = j * ROWB + h2_pos(wc) * 16;
    }
    // Activation staging: the block's 256 pixels x 64 k of a chunk are fetched in FULL 128-byte lines (8 consecutive
    // lanes = one pixel row's 64 halfs, 8 rows per wave-instruction), parked in four 64-pixel LDS images and read back
    // as MFMA fragments.  Fetching the fragments directly (16 rows x 64 B per instruction) costs the texture path two
    // half-used lines per row; and with the activation descriptor zero-sized (timing-only build) the K = 3072 GEMM ran
    // 1.84x faster: the activation fetch, not the matrix core, sets this kernel's pace.
    // WN = 1: every wave stages its OWN image (rows 64 wm + lane/8 + 8 i), so rewriting it needs no workgroup barrier -
    // LDS executes one wave's accesses in order; WN = 2: the images are shared, all threads stage all of them.
    constexpr int XROWS = WN == 1 ? 8 : NTHR / 8;            // rows covered by one staging pass of this thread's group
    const int xr = WN == 1 ? wm * 64 + (lane >> 3) : (tid >> 3);
    const int xc = tid & 7;                                  // 16-byte chunk
    char* ximg = smem + 2 * STAGE;
    const unsigned x_base = (unsigned)(((mblk + xr) * a.ldx + xc * 8) * 2);
    const unsigned x_rstep = (unsigned)(XROWS * a.ldx * 2);
    int pix0[IM2COL ? X_IT : 1], hw0[IM2COL ? X_IT : 1];     // image base pixel, packed (hi0, wi0) of this lane's rows
    if constexpr (IM2COL) {
#pragma unroll
        for (int i = 0; i < X_IT; ++i) {
            const int m = mblk + xr + XROWS * i;
            int hi0 = -30000, wi0 = 0, pb = 0;
            if (m < a.M) {
                const int hw = a.Ho * a.Wo;
                const int b = m / hw, rem = m - b * hw;
                const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
                hi0 = ho * a.sh - a.pt;
                wi0 = wo * a.sw - a.pl;
                pb = b * a.H * a.W;
            }
            pix0[i] = pb;
            hw0[i] = hi0 * 65536 + (wi0 & 0xFFFF);
        }
    }
    const int nk = (a.K + 63) >> 6;

    uint4 wst[W_IT];
    auto load_w = [&](int kc) {
        const bool ok = kc * 64 + wc * 8 < a.K;
#pragma unroll
        for (int i = 0; i < W_IT; ++i)
            wst[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rb.w, ok ? w_off[i] + kc * 128 : OOB, 0, 0));
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int i = 0; i < W_IT; ++i) *reinterpret_cast<uint4*>(smem + buf * STAGE + w_lds[i]) = wst[i];
    };
    U4H8 xst[X_IT];
    auto load_x = [&](int kc) {
        // weights of the K tail are zero in LDS, but 0 * (Inf/NaN garbage of the next row) is NaN: mask the lanes
        const bool kok = kc * 64 + xc * 8 < a.K;
        if constexpr (IM2COL) {
            const int k0 = kc * 64 + xc * 8;
            const int tap = k0 / a.Cin_g, c = k0 - tap * a.Cin_g;
            const int tr = tap / a.kw, ts = tap - tr * a.kw;
#pragma unroll
            for (int i = 0; i < X_IT; ++i) {
                const int hi = (hw0[i] >> 16) + tr, wi = (int)(short)(hw0[i] & 0xFFFF) + ts;
                const bool ok = kok & ((unsigned)hi < (unsigned)a.H) & ((unsigned)wi < (unsigned)a.W);
                const unsigned off = (unsigned)(((pix0[i] + hi * a.W + wi) * a.ldx + c) * 2);
                xst[i].u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rb.x, ok ? off : OOB, 0, 0));
            }
        } else {
#pragma unroll
            for (int i = 0; i < X_IT; ++i) {
                const bool ok = kok & (mblk + xr + XROWS * i < a.M);
                xst[i].u = __builtin_bit_cast(
                    uint4, __builtin_amdgcn_raw_buffer_load_b128(rb.x, ok ? x_base + i * x_rstep + kc * 128 : OOB, 0, 0));
            }
        }
    };
    auto store_x = [&]() {
#pragma unroll
        for (int i = 0; i < X_IT; ++i) {
            *reinterpret_cast<uint4*>(ximg + (xr + XROWS * i) * ROWB + h2_pos(xc) * 16) = xst[i].u;   // image r/64, row r%64
        }
    };
    const char* xs = ximg + wm * XS;

    f32x4 acc[NG][PT][4];
    {   // bias is the C operand of the first MFMA of every accumulator  (pwk_gemm_kernel: a copy, see pwk_direct_kernel)
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = n0 + g * 64 + (nt >> 1) * 32 + lq * 8 + (nt & 1) * 4;
                const f32x4 bv = __builtin_bit_cast(
                    f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb.bias, n < a.Cout_g ? (unsigned)(n * 4) : OOB, 0, 0));
#pragma unroll
                for (int p = 0; p < PT; ++p) acc[g][p][nt] = bv;
            }
    }

    load_w(0);
    load_x(0);
    store_w(0);
    store_x();
    __syncthreads();

    auto compute = [&](int buf, int ks) {
        // (wave column wn reads ITS NB weight rows of the stage: without the offset the upper half of every 256-channel tile was
        // computed from the lower half's weights - WN = 2 only, a shape gemm8p has taken since it exists unless K % 64 != 0)
        const char* ws = smem + buf * STAGE + (WN > 1 ? wn * NB * ROWB : 0) + l15 * ROWB + lq * 16 + ks * 64;
        const char* xl = xs + l15 * ROWB + lq * 16 + ks * 64;
        U4H8 xf[PT];     // the fragments of the wave's activation image: the hi (ks = 0) / lo (ks = 1) plane of x on the packed storage
#pragma unroll
        for (int p = 0; p < PT; ++p) xf[p].u = *reinterpret_cast<const uint4*>(xl + p * 16 * ROWB);
        pw_mfma_step<NG, PT, ROWB>(acc, ws, xf, ks);
    };

    // The next chunk's weights and activations are requested (global -> VGPR) before this chunk's math and written to
    // LDS after it; the weight image is double-buffered, the activation images are single-buffered (LDS budget) and
    // rewritten between two barriers.  Everything in the loop is
    // unconditional (a chunk past the end is all out-of-range offsets: zeros, no memory traffic): a branch around a
    // prefetch makes hipcc fold the "loads skipped" path into its vmcnt bookkeeping, and without the sched_barriers
    // it sinks every load below the MFMAs, right in front of its wait - both silently serialise the pipeline.
    for (int kc = 0; kc < nk; ++kc) {
        const int buf = kc & 1;
        load_w(kc + 1);
        load_x(kc + 1);
        __builtin_amdgcn_sched_barrier(0);
        compute(buf, 0);
        compute(buf, 1);
        __builtin_amdgcn_sched_barrier(0);
        store_w(buf ^ 1);
        if constexpr (WN > 1) __syncthreads();   // every wave is done reading the (single-buffered, shared) activation images
        store_x();
        __syncthreads();
    }

    int m_base = m0 + l15, n_lane = n0 + lq * 8;
    asm volatile("" : "+v"(m_base), "+v"(n_lane));      // (as in pwk_direct_kernel)
    pw_epilogue_groups<NG, PT>(mode, a, acc, m_base, n_lane, rb.res, rb.y);
}

// Y2: the two-output instantiations of the output-gated epilogue (y2: the second output)
template <int NG, bool Y2 = false>
int launch_pwk_direct(const ConvArgs& a, const Plan& p, hipStream_t s, f16* y2 = nullptr) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)(a.m_blocks * a.n_blocks)), dim3(256), 0, s, kernel_args<Y2>(a, y2), (int)p.mode);
    };
    if constexpr (Y2) {
        if (p.pt == 1) go(pwk_direct_kernel<NG, false, 1, true>);
        else go(pwk_direct_kernel<NG, false, 4, true>);
    } else {
        if (p.pt == 1) p.gated ? go(pwk_direct_kernel<NG, true, 1>) : go(pwk_direct_kernel<NG, false, 1>);
        else p.gated ? go(pwk_direct_kernel<NG, true, 4>) : go(pwk_direct_kernel<NG, false, 4>);
    }
    return vip_launch_status(Y2 ? "vip_conv2d_out_gated2_nhwc_f16(pwk-direct)" : "vip_conv2d_nhwc_f16(pwk-direct)");
}

// IM2COL: the k x k form, one grid plane per group (the pointwise form is ungrouped)
template <int NG, int WN, bool IM2COL>
int launch_pwk(const ConvArgs& a, int mode, int groups, hipStream_t s) {
    constexpr size_t smem = (2 * 64 * NG * WN + 4 * 64) * 160;     // 2 weight stages + 4 activation images
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pwk_gemm_kernel<NG, WN, IM2COL>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        attr_set = true;
    }
    const dim3 grid((unsigned)(a.m_blocks * a.n_blocks), (unsigned)groups);
    hipLaunchKernelGGL((pwk_gemm_kernel<NG, WN, IM2COL>), grid, dim3(256 * WN), smem, s, a, mode);
    return vip_launch_status(IM2COL ? "vip_conv2d_nhwc_f16(pwk-im2col)" : "vip_conv2d_nhwc_f16(pwk)");
}

#include "gemm8p.hpp"

// ---- Dense / 1x1 layers with at most 256 rows (the squeeze-excite and ECA layers: M = batch) ------------------------
// On the tile kernels such a layer is ONE m-block: 2..16 workgroups walk K chunk by chunk behind a barrier each, 30-100
// us of pure latency while the chip idles.  Here a workgroup owns 16 output channels for all rows, both MFMA operands
// are loaded global -> VGPR directly (no LDS staging, no barrier in the loop), K is split over the workgroup's four
// waves whose partial sums meet in LDS once, and (N/16) x (M/64) workgroups run side by side.
// XSPLIT: the rows are [M][2][K] - a hi and a lo fp16 plane (what gap_kernel / this kernel write with y_lo_off) - and every weight
// fragment meets both: the vector keeps ~22 bits through the squeeze-excite / ECA / split-attention chains.
// WLO (with XSPLIT, fp16 storage): two-term weights - a.w_lo, fp16(W32 - w) in the layout of w, meets the hi plane of the rows (the
// product of the two lo terms is below the fp32 sum's own rounding)
template <bool XSPLIT, bool WLO = false>
__global__ __launch_bounds__(256) void rows_gemm_kernel(ConvArgs a) {
    // workgroup = (16 channels, 64 rows): blockIdx.y = row quarter; its 4 waves split K and meet in LDS.  (One workgroup
    // per channel slab streaming ALL rows was bound by a single CU's L2 bandwidth: 1 MB of activations per workgroup.)
    constexpr unsigned OOB = 0xFFFFFFF0u;
    __shared__ float red[3][1][16][64];                      // [kq-1][.][acc register][lane]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = 0, kq = wave;
    const int l15 = lane & 15, lq = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int m0 = blockIdx.y * 64;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.w, 0, (unsigned)min((long)0xFFFFFFF0L, 2L * a.Cout_g * a.ldw), 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.x + a.cin_off), 0, (unsigned)min((long)0xFFFFFFF0L, a.x_span_bytes - 2L * a.cin_off), 0x00020000);
    // H2: k-step u = 2 c + plane of the 64-half chunk c; the lane's k-group is the 32-byte (hi, lo) pair lq of the chunk
    const unsigned w_off = (n0 + l15 < a.Cout_g) ? (unsigned)(((n0 + l15) * a.ldw + lq * (H2 ? 16 : 8)) * 2) : 0xFFFF0000u;
    unsigned x_off[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int m = m0 + p * 16 + l15;
        x_off[p] = m < a.M ? (unsigned)((m * a.ldx + lq * (H2 ? 16 : 8)) * 2) : 0xFFFF0000u;
    }
    f32x4 acc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nks = H2 ? 2 * ((a.K + 63) >> 6) : (a.K + 31) >> 5;
    const int per = ((nks + 3) / 4 + 3) & ~3;                // k-steps per K quarter, multiple of the unroll
    const int ks_lo = kq * per, ks_hi = min(nks, ks_lo + per);
    if (m0 < a.M) {
        for (int ks0 = ks_lo; ks0 < ks_hi; ks0 += 4) {
            U4H8 wf[4], xf[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kst = ks0 + u;
                const bool ok = (kst < ks_hi) & ((H2 ? (kst >> 1) * 64 + lq * 16 + (kst & 1) * 8 : kst * 32 + lq * 8) < a.K);
                const unsigned kb = H2 ? (unsigned)((kst >> 1) * 128 + (kst & 1) * 16) : (unsigned)(kst * 64);
                wf[u].u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rw, ok ? w_off + kb : OOB, 0, 0));
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    xf[u][p].u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, ok ? x_off[p] + kb : OOB, 0, 0));
            }
            if constexpr (H2) {     // (ks0, per: multiples of 4, so u = 0 / 2 are hi planes and u + 1 their lo planes)
#pragma unroll
                for (int u = 0; u < 4; u += 2)
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u + 1].h, xf[u][p].h, acc[p], 0, 0, 0);
                        acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u].h, xf[u + 1][p].h, acc[p], 0, 0, 0);
                        acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u].h, xf[u][p].h, acc[p], 0, 0, 0);
                    }
                continue;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u].h, xf[u][p].h, acc[p], 0, 0, 0);
            if constexpr (WLO) {
                const __amdgpu_buffer_rsrc_t rwl = __builtin_amdgcn_make_buffer_rsrc(
                    (void*)a.w_lo, 0, (unsigned)min((long)0xFFFFFFF0L, 2L * a.Cout_g * a.ldw), 0x00020000);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool ok = (ks0 + u < ks_hi) & ((ks0 + u) * 32 + lq * 8 < a.K);
                    wf[u].u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rwl, ok ? w_off + (ks0 + u) * 64 : OOB, 0, 0));
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int p = 0; p < 4; ++p) acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u].h, xf[u][p].h, acc[p], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 4; ++u) {       // the weights' first term again, for the rows' lo plane
                    const bool ok = (ks0 + u < ks_hi) & ((ks0 + u) * 32 + lq * 8 < a.K);
                    wf[u].u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rw, ok ? w_off + (ks0 + u) * 64 : OOB, 0, 0));
                }
            }
            if constexpr (XSPLIT) {     // the lo plane: K halfs further in the same row
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool ok = (ks0 + u < ks_hi) & ((ks0 + u) * 32 + lq * 8 < a.K);
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        xf[u][p].u = __builtin_bit_cast(
                            uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, ok ? x_off[p] + (ks0 + u) * 64 + 2 * a.K : OOB, 0, 0));
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int p = 0; p < 4; ++p) acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u].h, xf[u][p].h, acc[p], 0, 0, 0);
            }
        }
    }
    if (kq > 0) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[kq - 1][mw][p * 4 + r][lane] = acc[p][r];
    }
    __syncthreads();
    if (kq > 0 || m0 >= a.M) return;
    // lane: row m0 + 16 p + l15, channels n0 + 4 lq + (0..3)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int m = m0 + p * 16 + l15;
        if (m >= a.M) continue;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + lq * 4 + r;
            v[r] = acc[p][r] + red[0][mw][p * 4 + r][lane] + red[1][mw][p * 4 + r][lane] + red[2][mw][p * 4 + r][lane] +
                   ((a.bias && n < a.Cout_g) ? a.bias[n] : 0.f);
        }
        if constexpr (H2) {     // 4 consecutive channels of a packed row (Cout % 8 == 0, so the quad is whole or absent)
            if (n0 + lq * 4 < a.Cout_g) {
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = vip_act_strict(v[r] * a.out_scale, a.act_pre);
                h2_st4(a.y, (long)m * a.ldy + a.cout_off + n0 + lq * 4, o, a.status);
            }
            continue;
        }
        f16* dst = a.y + (long)m * a.ldy + a.cout_off + n0 + lq * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = vip_act(v[r], a.act_pre);
        if (n0 + lq * 4 + 3 < a.Cout_g) {
            f16x4 o, ol;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o[r] = (f16)v[r];
                ol[r] = (f16)(v[r] - (float)o[r]);
            }
            *reinterpret_cast<f16x4*>(dst) = o;
            if (a.y_lo_off) *reinterpret_cast<f16x4*>(dst + a.y_lo_off) = ol;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n0 + lq * 4 + r < a.Cout_g) {
                    const f16 o = (f16)v[r];
                    dst[r] = o;
                    if (a.y_lo_off) dst[a.y_lo_off + r] = (f16)(v[r] - (float)o);
                }
        }
    }
}

template <bool XSPLIT, bool WLO = false>
int launch_rows(const ConvArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((rows_gemm_kernel<XSPLIT, WLO>), dim3((unsigned)((a.Cout_g + 15) / 16), (unsigned)((a.M + 63) / 64)), dim3(256), 0, s, a);
    return vip_launch_status("vip_conv2d_nhwc_f16(rows)");
}

template <int BM, int BN>
int launch_igemm(const ConvArgs& a, int groups, hipStream_t s) {
    const int nk = (a.K + 63) >> 6;
    const size_t smem = (nk == 1 ? 1 : 2) * (BM + BN) * 128;  // a single k-tile needs no second stage
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_igemm_kernel<BM, BN>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (BM + BN) * 128);
        attr_set = true;
    }
    dim3 grid((unsigned)(a.m_blocks * a.n_blocks), 1, (unsigned)groups);
    hipLaunchKernelGGL((conv_igemm_kernel<BM, BN>), grid, dim3(256), smem, s, a);
    return vip_launch_status("vip_conv2d_nhwc_f16");
}

}  // namespace

// ---- selection: which kernel, which template arguments, which tile grid.  Host code alone - every threshold and every selection
// switch of the environment is read here (static: once per process; VIP_G8P_MINK, VIP_PWX and VIP_LN_GEMM_ALL per call:
// their tests set them mid-process), and the selection's VIP_ERR_UNSUPPORTED exits are here (those of the argument checks stay in front).
static void plan_blocks(Plan& p, const ConvArgs& a, int bm, int bn) {
    p.m_blocks = (a.M + bm - 1) / bm;
    p.n_blocks = (a.Cout_g + bn - 1) / bn;
}

static int plan_pw(Plan& p, const ConvArgs& a) {
    p.family = PW_GEMM; p.pt = 4; p.hilo = a.w_lo != nullptr;
    const int ks = H2 ? 2 * ((a.K + 63) >> 6) : (a.K + 31) >> 5;     // H2: whole 64-half chunks (hi and lo planes of 32 logical k)
    p.ks = ks <= 4 ? ks : ks <= 6 ? 6 : 8;
    // two workgroups per CU.  H2: a packed weight slice is twice as large, so the same budget cuts N into more channel chunks and
    // every chunk re-reads the activations; with >= 512K rows that traffic costs more than the second resident workgroup gains
    // (M=2.5M N=384 K=96: 1.71 -> 1.23 ms), below that the shorter launch prefers the two workgroups (M=160K N=512 K=128:
    // 0.16 vs 0.20 ms) - profiles/r04_ab_pw_h2_lds.log.  VIP_PW_H2_LDS_KB overrides.
    static const int h2_lds_kb = getenv("VIP_PW_H2_LDS_KB") ? atoi(getenv("VIP_PW_H2_LDS_KB")) : 0;
    const int LDS_MAX = (H2 ? (h2_lds_kb ? h2_lds_kb : (a.M >= (1 << 19) ? 156 : 72)) : 72) * 1024;
    // row stride in 16-byte chunks == 2 (mod 4), i.e. 32 (mod 64) bytes: ds_read_b128 is serviced in the lane groups
    // {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... over 64 banks, and with the fragment pattern (lane&15 = row, lane>>4 =
    // chunk) that stride puts each group's 16 chunks on 16 distinct 16-byte slots (an ODD chunk stride does not: 46 %
    // conflict cycles measured)
    int s16 = p.ks * 4 * (p.hilo ? 2 : 1);
    while ((s16 & 3) != 2) ++s16;
    p.lds_stride = s16 * 16;
    const int cout64 = (a.Cout_g + 63) & ~63;
    const int max_rows = (LDS_MAX / (p.lds_stride + 4)) & ~63;
    p.n_chunks = (cout64 + max_rows - 1) / max_rows;
    p.nb_ch = (((cout64 / 64 + p.n_chunks - 1) / p.n_chunks)) * 64;
    return VIP_OK;
}

static int plan_pwx(Plan& p, const ConvArgs& a, int ksc, int pt, bool ln) {
    p.family = PWX; p.ksc = ksc; p.pt = pt; p.ln = ln;
    p.m_blocks = (a.M + 64 * pt - 1) / (64 * pt); p.n_blocks = 1;
    return VIP_OK;
}

static int plan_pwk_direct(Plan& p, const ConvArgs& a) {
    p.family = PWK_DIRECT; p.ng = a.Cout_g <= 64 ? 1 : 2; p.gated = a.gate != nullptr;
    // fewer 256-pixel workgroups than CUs (7x7 / 13x13 maps with narrow outputs): 64-pixel tiles instead - measured 48 -> 29 us on
    // M = 12 544, N = 208, K = 1 248 (98 -> 392 workgroups), 35 -> 28 us on 43 264 x 128 x 768; 128-pixel tiles in the band up to
    // 2 x CUs measured no gain and are not instantiated (tools/bench_pwk_fill.py, profiles/r02_pwk_small_tiles_ab.log)
    static const int fill = getenv("VIP_PWK_FILL") ? atoi(getenv("VIP_PWK_FILL")) : 256;
    const long wg256 = (long)((a.M + 255) / 256) * ((a.Cout_g + 64 * p.ng - 1) / (64 * p.ng));
    p.pt = wg256 < fill ? 1 : 4;
    plan_blocks(p, a, 64 * p.pt, 64 * p.ng);
    return VIP_OK;
}

static int plan_pwk(Plan& p, const ConvArgs& a, int ng, int wn) {
    p.family = PWK_GEMM; p.ng = ng; p.wn = wn;
    plan_blocks(p, a, 256, 64 * ng * wn);
    return VIP_OK;
}

static int plan(const ConvArgs& a, const vip_conv_desc* d, bool x_split, Plan* out) {
    Plan& p = *out = Plan{};
    const long M = a.M;
    const int cin_g = d->Cin / d->groups, cout_g = a.Cout_g;
    const bool residual = a.res, gate = a.gate, w_lo = a.w_lo;
    EpiMode mode = EPI_OTHER;
    if (!residual && d->act_post == VIP_ACT_NONE) mode = (EpiMode)d->act_pre;
    else if (residual && d->act_pre == VIP_ACT_NONE && d->act_post == VIP_ACT_NONE) mode = EPI_RES;
    else if (residual && d->act_pre == VIP_ACT_NONE && d->act_post == VIP_ACT_RELU) mode = EPI_RES_RELU;
    p.mode = mode;
#if !VIP_GEMM_H2
    if (a.ln_g) {     // vip_ln_gemm_bias_act_f16: the one kernel with the LayerNorm prologue, no fall-back (a missing kernel is an error)
        VIP_REQUIRE(mode != EPI_OTHER && a.ln_b && !w_lo && !gate && !a.y_lo_off && !x_split && d->groups == 1 && d->kh == 1 && d->kw == 1 && d->sh == 1 &&
                        d->sw == 1 && d->pt == 0 && d->pl == 0 && d->Ho == d->H && d->Wo == d->W && d->cin_off == 0 &&
                        vip_ln_gemm_supported((int)M, a.K, cout_g, d->act_pre) && a.x_span_bytes < 0xFFFF0000L - 2L * a.K,
                    VIP_ERR_UNSUPPORTED,
                    "vip_ln_gemm_bias_act_f16: M=%ld K=%d N=%d act=%d/%d%s not taken (vip_ln_gemm_supported; (activation) or "
                    "(residual [+ReLU]) epilogue)", M, a.K, cout_g, d->act_pre, d->act_post, residual ? " +res" : "");
        const int ksc = (a.K + 63) >> 6;
        return plan_pwx(p, a, ksc <= 2 ? 2 : ksc <= 3 ? 3 : ksc <= 4 ? 4 : 6, 2, true);
    }
#endif
    // HBM-bound shapes (short K): a smaller M tile -> 24-48 KB LDS and half the accumulators -> 3-5 workgroups per
    // CU in flight instead of 2, which is what hides the load -> MFMA -> store latency chain of a 1-4 k-tile block.
    // (Tried and measured SLOWER on these shapes: a two-deep register prefetch (+40 VGPRs), an LDS-transposed
    // "fully coalesced" epilogue, and a persistent tile loop that prefetches the next tile under the epilogue
    // (+60 VGPRs): all three trade resident workgroups for in-workgroup overlap, and residency wins.)
    const bool short_k = a.K <= 256;
    static const int pw_mode = getenv("VIP_PW") ? atoi(getenv("VIP_PW")) : 3;
    if (pw_mode && d->groups == 1 && d->kh == 1 && d->kw == 1 && d->sh == 1 && d->sw == 1 && d->pt == 0 && d->pl == 0 &&
        d->Ho == d->H && d->Wo == d->W) {
        if (w_lo && x_split) {      // vip_gemm_split2_hilo_f16: a few split rows against two-term weights
            VIP_REQUIRE(!H2 && M <= 256 && !residual && !gate && a.y_lo_off && d->act_post == VIP_ACT_NONE && d->ldy % 4 == 0 &&
                            d->cout_off % 4 == 0 && a.x_span_bytes < 0xFFFF0000L - 2L * a.K && 2L * cout_g * d->ldw < 0xFFFF0000L - 2L * a.K,
                        VIP_ERR_UNSUPPORTED, "vip_gemm_split2_hilo_f16: at most 256 rows, N %% 4 == 0");
            p.family = ROWS_GEMM; p.xsplit = true; p.hilo = true;
            return VIP_OK;
        }
        if (w_lo) {     // hi + lo weights: the streaming kernel is the one that carries them (any M)
            VIP_REQUIRE(mode != EPI_OTHER && short_k && !gate && !a.y_lo_off, VIP_ERR_UNSUPPORTED,
                        "vip_conv2d_hilo_nhwc_f16: 1x1 stride-1 ungrouped, K <= 256, (activation) or (residual [+ReLU]) epilogue");
            return plan_pw(p, a);
        }
        if (M <= 256 && !residual && !gate && d->act_post == VIP_ACT_NONE && d->ldy % 4 == 0 && d->cout_off % 4 == 0 &&
            a.x_span_bytes < 0xFFFF0000L - 2L * a.K && 2L * cout_g * d->ldw < 0xFFFF0000L - 2L * a.K) {
            p.family = ROWS_GEMM; p.xsplit = x_split;
            return VIP_OK;
        }
        VIP_REQUIRE(!a.y_lo_off && !x_split, VIP_ERR_UNSUPPORTED, "vip_gemm_split_f16: at most 256 rows, N %% 4 == 0");
        if (mode != EPI_OTHER && (pw_mode & 1) && short_k && M >= 65536 && !gate) return plan_pw(p, a);
        // deep K, wide N: the LDS-DMA kernel (gemm8p.hpp).  VIP_G8P_MINK: smallest K it takes (0 = never).  1024: in isolation it
        // wins from K = 256 up (+6..+27 %), but it owns a CU (128 KB of LDS, 8 waves x 256 VGPRs, persistent) and the ensemble step
        // runs three member streams - with the K = 256-768 layers on it the STEP was 1.5-2 % slower (58.2 ms vs 57.1-57.4,
        // alternating runs on one box, profiles/r02_gemm8p_mink_streams_ab.log) and a single stream gained nothing either.
        const char* g8_env = getenv("VIP_G8P_MINK");     // read per call: the kernel's own tests lower it
        const int g8_min_k = g8_env ? atoi(g8_env) : 1024;
        if (mode != EPI_OTHER && g8_min_k > 0 && !gate && a.K >= g8_min_k && gemm8p_eligible(a) && cout_g % 256 == 0 &&
            (long)((M + 255) / 256) * (cout_g / 256) >= 128) {
            p.family = GEMM8P; p.pipe = a.K % 128 == 0;
            plan_blocks(p, a, 256, 256);
            return VIP_OK;
        }
        if (mode != EPI_OTHER && (pw_mode & 2) && a.x_span_bytes < 0xFFFFFFF0L) {
            // (a 64 x 256 wave tile at one wave per SIMD - NG = 4 - measured 15-40 % slower than NG = 2 at two)
            static const int xl_min_k = getenv("VIP_PWK_XLK") ? atoi(getenv("VIP_PWK_XLK")) : 768;
            // (gated convolutions: only the direct kernel carries the gate pipeline - their deep-K cases are small launches)
            // short K, wide N: the activation-resident kernel (pwx_kernel) - an EXPERIMENT, off unless VIP_PWX=1 (read per call: its tests
            // set it).  Measured per shape against pwk_direct_kernel (profiles/r04_pwx_vs_pwk_direct.log): a wash on the fp16 storage
            // (sum of ten ensemble shapes 566 vs 564 us) and 7-35 % slower on the packed storage, where K = 256 needs 128 fragment
            // registers, leaves 16 pixels per wave and makes every 64-pixel workgroup stream all of W out of L2.  The K <= 256 layers are
            // not bound by the fill / drain this kernel removes: their GELU / residual epilogues issue 7 VALU instructions per MFMA.
            const char* pwx_env = getenv("VIP_PWX");
            const int pwx_on = pwx_env ? atoi(pwx_env) : 0;
            if (pwx_on && !gate && cout_g >= 256 && a.K <= (H2 ? 512 : 256) && a.K > 64 && M >= 16384 && a.x_span_bytes < 0xFFFF0000L - 2L * a.K) {
                const int ksc = (a.K + 63) >> 6;
                if (H2) {
                    if (ksc <= 4) return plan_pwx(p, a, 4, 2, false);
                    return plan_pwx(p, a, ksc <= 6 ? 6 : 8, 1, false);      // (32 pixels per wave spill at 96 fragment registers)
                }
                return plan_pwx(p, a, ksc <= 2 ? 2 : ksc <= 3 ? 3 : 4, 2, false);
            }
            if ((a.K < xl_min_k || gate) && a.x_span_bytes < 0xFFFF0000L - 2L * a.K) return plan_pwk_direct(p, a);
            VIP_REQUIRE(!gate, VIP_ERR_UNSUPPORTED, "vip_conv2d_gated_nhwc_f16: input tensor too large (4 GB - 2K)");
            if (cout_g <= 64) return plan_pwk(p, a, 1, 1);
            // 256 x 256 block tiles (8 waves): 5 % on deep-K layers whose N is a multiple of 256; slower whenever the last
            // 256-channel tile is half empty (N = 384: 258 -> 346 us) or K is short
            static const int wn2_min_k = getenv("VIP_PWK_WN2K") ? atoi(getenv("VIP_PWK_WN2K")) : 1024;
            if (cout_g % 256 == 0 && a.K >= wn2_min_k && (long)((M + 255) / 256) * (cout_g / 256) >= 256) return plan_pwk(p, a, 2, 2);
            return plan_pwk(p, a, 2, 1);
        }
    }
    {   // k x k convolutions on the pointwise kernel with im2col staging (64 px x 128 ch wave tiles, half the LDS fragment
        // reads per MFMA of the 64 x 64 tiles below): stems (Cin <= 16: 277 vs 385 us on the EfficientNet stems) and every
        // layer with at least 32 K pixels - measured per shape on the ensemble after the MFMA-priority change: +3..+25 %
        // (ResNeSt's grouped 3x3: 585 -> 726, 721 -> 853 TF), except the 7 x 7-pixel stages (M = 12 544: 637 -> 497 TF),
        // which keep the tile kernel.  VIP_PWK_CONV: 1 = every eligible conv (tests), -1 = stems only.
        static const int im2col_all = getenv("VIP_PWK_CONV") ? atoi(getenv("VIP_PWK_CONV")) : 0;
        if ((cin_g <= 16 || im2col_all > 0 || (im2col_all == 0 && M >= 32768)) && mode != EPI_OTHER && !gate && a.x_span_bytes < 0xFFFFFFF0L && d->H < 30000 &&
            d->W < 30000 && d->pt < 16 && d->pl < 16) {
            p.family = IM2COL; p.ng = cout_g <= 64 ? 1 : 2;
            plan_blocks(p, a, 256, 64 * p.ng);
            return VIP_OK;
        }
    }
    VIP_REQUIRE(!w_lo, VIP_ERR_UNSUPPORTED, "vip_conv2d_hilo_nhwc_f16: only 1x1 stride-1 ungrouped convolutions with K <= 256");
    VIP_REQUIRE(!gate, VIP_ERR_UNSUPPORTED,
                "vip_conv2d_gated_nhwc_f16: only 1x1 stride-1 ungrouped convolutions with (activation) or (residual [+ReLU]) "
                "epilogues take a gate; apply vip_scale_add_act_f16 first");
    p.family = CONV_IGEMM; p.bm = short_k ? 64 : 128; p.bn = cout_g <= 64 ? 64 : 128;
    plan_blocks(p, a, p.bm, p.bn);
    return VIP_OK;
}

// ---- launch: the plan's instantiation.  What is read here depends on the device or changes nothing in the selection: the CU count that
// caps the persistent grids, VIP_G8P_PERSIST, the once-per-kernel dynamic-LDS attributes.
// y2: the second output of vip_conv2d_out_gated2_nhwc_f16, else NULL - it exists in the output-gated instantiations of two families alone
static int launch(const Plan& p, ConvArgs a, int groups, hipStream_t s, f16* y2 = nullptr) {
    a.m_blocks = p.m_blocks; a.n_blocks = p.n_blocks;
    const bool og = epi_out_gated(p.mode);
    if (y2 && !(og && (p.family == PW_GEMM || p.family == PWK_DIRECT))) return VIP_ERR_UNSUPPORTED;
    switch (p.family) {
        case PW_GEMM:
            return with_const<1, 2, 3, 4, 6, 8>(p.ks, [&](auto ks) {
                constexpr int KS = decltype(ks)::value;
                if constexpr (!H2 && KS <= 4)       // (K > 128: the gated epilogue would spill - conv2d_plan declines)
                    if (og) {
                        if (y2) return p.hilo ? launch_pw<KS, 4, true, true, true>(a, p, s, y2) : launch_pw<KS, 4, false, true, true>(a, p, s, y2);
                        return p.hilo ? launch_pw<KS, 4, true, true>(a, p, s) : launch_pw<KS, 4, false, true>(a, p, s);
                    }
                if (og) return (int)VIP_ERR_UNSUPPORTED;
                return p.hilo ? launch_pw<KS, 4, true>(a, p, s) : launch_pw<KS, 4, false>(a, p, s);
            });
        case ROWS_GEMM:
            if constexpr (!H2)
                if (p.hilo) return launch_rows<true, true>(a, s);
            return p.xsplit ? launch_rows<true>(a, s) : launch_rows<false>(a, s);
        case GEMM8P: return launch_gemm8p(a, p.mode, p.pipe, s);
        case PWX:
#if !VIP_GEMM_H2
            if (p.ln) return with_const<2, 3, 4, 6>(p.ksc, [&](auto ksc) { return launch_pwx<decltype(ksc)::value, 2, true>(a, p.mode, s); });
#endif
            if (p.pt == 2) return with_const<2, 3, 4>(p.ksc, [&](auto ksc) { return launch_pwx<decltype(ksc)::value, 2, false>(a, p.mode, s); });
            return with_const<6, 8>(p.ksc, [&](auto ksc) { return launch_pwx<decltype(ksc)::value, 1, false>(a, p.mode, s); });
        case PWK_DIRECT:
#if !VIP_GEMM_H2
            if (y2) return p.ng == 1 ? launch_pwk_direct<1, true>(a, p, s, y2) : launch_pwk_direct<2, true>(a, p, s, y2);
#endif
            return p.ng == 1 ? launch_pwk_direct<1>(a, p, s) : launch_pwk_direct<2>(a, p, s);
        case PWK_GEMM:
            if (p.ng == 1) return launch_pwk<1, 1, false>(a, p.mode, groups, s);
            return p.wn == 1 ? launch_pwk<2, 1, false>(a, p.mode, groups, s) : launch_pwk<2, 2, false>(a, p.mode, groups, s);
        case IM2COL: return p.ng == 1 ? launch_pwk<1, 1, true>(a, p.mode, groups, s) : launch_pwk<2, 1, true>(a, p.mode, groups, s);
        case CONV_IGEMM:
            if (p.bn == 64) return p.bm == 64 ? launch_igemm<64, 64>(a, groups, s) : launch_igemm<128, 64>(a, groups, s);
            return p.bm == 64 ? launch_igemm<64, 128>(a, groups, s) : launch_igemm<128, 128>(a, groups, s);
    }
    return VIP_ERR_UNSUPPORTED;
}

// One call as its entry point states it: the operands every call has, and whatever else that entry point means (the rest keeps its default)
struct ConvCall {
    const void* x = nullptr;
    const void* w = nullptr;
    const float* bias = nullptr;
    const void* residual = nullptr;
    void* y = nullptr;
    const vip_conv_desc* d = nullptr;
    const void* gate = nullptr;         // per-image input-channel gate (ConvArgs::gate)
    int y_lo_off = 0;                   // split output (ConvArgs::y_lo_off)
    const void* w_lo = nullptr;         // second weight term
    bool x_split = false;               // the rows are [M][2][K]: a hi and a lo plane
    float out_scale = 1.f;              // packed storage: 1 / the weights' scale
    int* status = nullptr;              // packed storage: the overflow word
    const float* ln_g = nullptr;        // LayerNorm over the input row (pwx_ln_kernel)
    const float* ln_b = nullptr;
    float ln_eps = 0.f;
    const void* out_gate = nullptr;     // per-image output-channel gate (ConvArgs::ogate)
    void* y2 = nullptr;                 // second output of the output-gated epilogue
};
static ConvCall conv_call(const void* x, const void* w, const float* bias, const void* residual, void* y, const vip_conv_desc* d) {
    ConvCall c;
    c.x = x; c.w = w; c.bias = bias; c.residual = residual; c.y = y; c.d = d;
    return c;
}

// the argument checks, the kernel arguments and the plan of one call
static int conv2d_plan(const ConvCall& c, ConvArgs* args, Plan* p) {
    const void *x = c.x, *w = c.w, *residual = c.residual, *gate = c.gate, *w_lo = c.w_lo, *out_gate = c.out_gate;
    void* y = c.y;
    const vip_conv_desc* d = c.d;
    const int y_lo_off = c.y_lo_off;
    const bool x_split = c.x_split;
    const float* ln_g = c.ln_g;
    VIP_REQUIRE(x && w && y && d, VIP_ERR_BAD_ARG, "vip_conv2d_nhwc_f16: null pointer");
    VIP_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0 && d->kh > 0 && d->kw > 0 &&
                    d->sh > 0 && d->sw > 0 && d->Ho > 0 && d->Wo > 0 && d->groups > 0 && d->pt >= 0 && d->pl >= 0,
                VIP_ERR_BAD_ARG, "vip_conv2d_nhwc_f16: non-positive dimension");
    VIP_REQUIRE(d->Cin % d->groups == 0 && d->Cout % d->groups == 0, VIP_ERR_BAD_ARG,
                "vip_conv2d_nhwc_f16: channels (%d,%d) not divisible by groups %d", d->Cin, d->Cout, d->groups);
    const int cin_g = d->Cin / d->groups, cout_g = d->Cout / d->groups;
    VIP_REQUIRE(cin_g % 8 == 0 && cout_g % 8 == 0, VIP_ERR_ALIGNMENT,
                "vip_conv2d_nhwc_f16: Cin/groups=%d and Cout/groups=%d must be multiples of 8", cin_g, cout_g);
    VIP_REQUIRE(d->ldx % 8 == 0 && d->ldy % 8 == 0 && d->ldw % 8 == 0 && d->cin_off % 8 == 0 &&
                    d->cout_off % 8 == 0 && (!residual || (d->ldr % 8 == 0 && d->res_off % 8 == 0)),
                VIP_ERR_ALIGNMENT, "vip_conv2d_nhwc_f16: strides/offsets must be multiples of 8 halfs");
    constexpr int IN = H2 ? 2 : 1;       // halfs per input element (H2: an (hi, lo) pair)
    VIP_REQUIRE(d->ldx >= d->cin_off + d->Cin && d->ldy >= d->cout_off + d->Cout && d->ldw >= IN * d->kh * d->kw * cin_g,
                VIP_ERR_BAD_ARG, "vip_conv2d_nhwc_f16: leading dimension smaller than the channel extent");
    VIP_REQUIRE(!H2 || (d->ldw % 16 == 0 && !w_lo && !y_lo_off && !x_split), VIP_ERR_BAD_ARG,
                "vip_conv2d_nhwc_h2: ldw must be a multiple of 16 halfs; no split variants");
    VIP_REQUIRE((unsigned)d->act_pre <= 4u && (unsigned)d->act_post <= 4u, VIP_ERR_BAD_ARG,
                "vip_conv2d_nhwc_f16: unknown activation code");
    // the caller's Ho/Wo must not read past what padding+kernel imply on the top/left; bottom/right
    // overhang is zero-filled, so any Ho/Wo is memory-safe.
    const long M = (long)d->B * d->Ho * d->Wo;
    VIP_REQUIRE(M < (1L << 31) - 256, VIP_ERR_UNSUPPORTED, "vip_conv2d_nhwc_f16: B*Ho*Wo too large");

    ConvArgs& a = *args;
    a.x = (const f16*)x; a.w = (const f16*)w; a.bias = c.bias; a.res = (const f16*)residual; a.y = (f16*)y;
    a.H = d->H; a.W = d->W; a.Ho = d->Ho; a.Wo = d->Wo;
    // the INPUT side in halfs (H2: twice the logical channels - see the head of this file), the output side in logical channels
    a.Cin_g = cin_g * IN; a.Cout_g = cout_g;
    a.kh = d->kh; a.kw = d->kw; a.sh = d->sh; a.sw = d->sw; a.pt = d->pt; a.pl = d->pl;
    a.ldx = d->ldx * IN; a.ldy = d->ldy; a.ldr = d->ldr; a.ldw = d->ldw;
    a.cin_off = d->cin_off * IN; a.cout_off = d->cout_off; a.res_off = d->res_off;
    a.M = (int)M; a.K = d->kh * d->kw * cin_g * IN;
    a.x_span_bytes = 2L * IN * d->B * d->H * d->W * d->ldx;
    a.y_span_bytes = (long)ESZ * M * d->ldy;
    a.res_span_bytes = (long)ESZ * M * d->ldr;
    a.bias_elems = d->Cout;
    a.out_scale = c.out_scale;
    a.status = c.status;
    VIP_REQUIRE(a.y_span_bytes < 0xFFFFFFE0L && a.res_span_bytes < 0xFFFFFFE0L, VIP_ERR_UNSUPPORTED,
                "vip_conv2d_nhwc_f16: output or residual tensor exceeds the 4 GiB buffer-addressing range");
    VIP_REQUIRE(a.x_span_bytes < 0xFFFFFFF0L && 2L * d->Cout * d->ldw < 0xFFFFFFF0L, VIP_ERR_UNSUPPORTED,
                "vip_conv2d_nhwc_f16: input or weight tensor exceeds the 4 GiB buffer-addressing range");
    a.act_pre = d->act_pre; a.act_post = d->act_post;
    a.m_blocks = a.n_blocks = 0;
    a.w_lo = (const f16*)w_lo;
    a.gate = (const f16*)gate;
    a.gate_hw = d->Ho * d->Wo;
    a.y_lo_off = y_lo_off;
    a.ln_g = ln_g; a.ln_b = c.ln_b; a.ln_eps = c.ln_eps;
    a.ogate = (const f16*)out_gate;
    a.ogate_elems = 0;
    a.hw_magic = a.gate_hw > 1 ? (unsigned)((1L << 32) / a.gate_hw) : 0xFFFFFFFFu;
    if (!out_gate) return plan(a, d, x_split, p);
    // Output gate: the selection is the residual call's own (the plan below does not see the gate); only the two kernel families that
    // serve the block-final 1x1 layers carry the gated epilogue, everything else declines and the caller runs its two launches.
    VIP_REQUIRE(!H2 && residual && !gate && !y_lo_off && !x_split && !ln_g && d->groups == 1 && d->cout_off == 0 && d->act_pre == VIP_ACT_NONE &&
                    (d->act_post == VIP_ACT_NONE || d->act_post == VIP_ACT_RELU) && 4L * d->B * d->Cout < 0xFFFFFFF0L,
                VIP_ERR_UNSUPPORTED, "vip_conv2d_out_gated_nhwc_f16: ungrouped, residual [+ReLU] epilogue, no input gate, cout_off = 0");
    a.ogate_elems = 2 * d->B * d->Cout;
    const int st = plan(a, d, x_split, p);
    if (st != VIP_OK) return st;
    // (pw_gemm_kernel up to K = 128: with six or eight k-steps of activation fragments resident the gated epilogue goes to scratch.
    // The gate rows of a tile's images are staged in LDS: a wave's 64 pixels may span four images there - maps of 32 pixels and more -
    // next to a weight slice that still leaves room for two workgroups per CU; the direct kernel has its 256 pixels' images in the
    // weight stages, 80 of them.)
    const bool pw_ok = p->family == PW_GEMM && p->ks <= 4 && 63 / a.gate_hw + 2 <= 4 &&
                       (size_t)p->nb_ch * (p->lds_stride + 4) + pw_og_lds(p->nb_ch) <= 80 * 1024;
    const bool pwk_ok = p->family == PWK_DIRECT && !p->gated && (64 * p->pt - 1) / a.gate_hw + 2 <= 80;
    VIP_REQUIRE((p->mode == EPI_RES || p->mode == EPI_RES_RELU) && (pw_ok || pwk_ok), VIP_ERR_UNSUPPORTED,
                "vip_conv2d_out_gated_nhwc_f16: this shape's kernel carries no output gate (pw_gemm_kernel up to K = 128 and "
                "pwk_direct_kernel do)");
    p->mode = p->mode == EPI_RES ? EPI_OGATE_RES : EPI_OGATE_RES_RELU;
    return VIP_OK;
}

static int conv2d_impl(const ConvCall& c, void* stream) {
    ConvArgs a;
    Plan p;
    const int st = conv2d_plan(c, &a, &p);
    return st != VIP_OK ? st : launch(p, a, c.d->groups, (hipStream_t)stream, (f16*)c.y2);
}

// vip_conv2d_kernel_name[_h2] / vip_conv2d_kernel_variant[_h2]: a dry run - the checks and the plan of the call the flags describe, and
// no launch.  The name is the kernel family (profile labels), the variant the instantiation and its tile grid.
static int kernel_query(const char* who, bool variant, const vip_conv_desc* d, int has_residual, int has_gate, int has_w_lo, char* out,
                        size_t cap, bool out_gate = false) {
    VIP_REQUIRE(d && out && cap > 0, VIP_ERR_BAD_ARG, "%s: null pointer", who);
    static const char dummy[16] = {0};     // non-null stand-ins: nothing is dereferenced or launched in a dry run
    ConvArgs a;
    Plan p;
    ConvCall c = conv_call(dummy, dummy, nullptr, has_residual ? dummy : nullptr, const_cast<char*>(dummy), d);
    if (has_gate) c.gate = dummy;
    if (has_w_lo) c.w_lo = dummy;
    if (out_gate) c.out_gate = dummy;
    const int st = conv2d_plan(c, &a, &p);
    if (st != VIP_OK) return st;
    static const char* const kernel[] = {"pw_gemm_kernel",    "rows_gemm_kernel", "gemm8p_kernel",           "pwx_kernel",
                                         "pwk_direct_kernel", "pwk_gemm_kernel",  "pwk_gemm_kernel(im2col)", "conv_igemm_kernel"};
    if (!variant) {
        snprintf(out, cap, "%s", p.family == PWX && p.ln ? "pwx_ln_kernel" : kernel[p.family]);
        return VIP_OK;
    }
    switch (p.family) {
        case PW_GEMM: snprintf(out, cap, "pw_gemm<KS=%d%s> %d x %d%s", p.ks, p.hilo ? ",hilo" : "", p.n_chunks, p.nb_ch, epi_out_gated(p.mode) ? " ogate" : ""); break;
        case ROWS_GEMM: snprintf(out, cap, "rows_gemm%s", p.xsplit ? "<xsplit>" : ""); break;
        case GEMM8P: snprintf(out, cap, "gemm8p<%s> %d x %d", p.pipe ? "pipe" : "basic", p.m_blocks, p.n_blocks); break;
        case PWX: snprintf(out, cap, "%s<%d,%d>", p.ln ? "pwx_ln" : "pwx", p.ksc, p.pt); break;
        case PWK_DIRECT:
            snprintf(out, cap, "pwk_direct<%d%s> PT=%d%s", p.ng, p.gated ? ",gated" : "", p.pt, epi_out_gated(p.mode) ? " ogate" : "");
            break;
        case PWK_GEMM: snprintf(out, cap, "pwk_gemm<%d,%d> %d x %d", p.ng, p.wn, p.m_blocks, p.n_blocks); break;
        case IM2COL: snprintf(out, cap, "im2col<%d>", p.ng); break;
        case CONV_IGEMM: snprintf(out, cap, "conv_igemm<%d,%d>", p.bm, p.bn); break;
    }
    return VIP_OK;
}

#if VIP_GEMM_H2
/* Conv2D / Dense on the packed STRICT storage (include/vipcup_hip.h): x, residual, y packed [.., C] (4 bytes per element), w packed
 * rows [Cout][ldw halfs] = per 8 k: [hi x 8][lo x 8] of (W * w_scale), bias = b * w_scale (fp32), out_scale = 1 / w_scale. */
extern "C" int vip_conv2d_nhwc_h2(const void* x, const void* w, const float* bias, const void* residual, void* y, const vip_conv_desc* d,
                                  float out_scale, int* status, void* stream) {
    VIP_REQUIRE(out_scale > 0.f, VIP_ERR_BAD_ARG, "vip_conv2d_nhwc_h2: out_scale must be positive");
    ConvCall c = conv_call(x, w, bias, residual, y, d);
    c.out_scale = out_scale; c.status = status;
    return conv2d_impl(c, stream);
}

/* The same with a squeeze-excite gate folded into the activation operand: gate packed [B][Cin]; the product (x_hi + x_lo)(g_hi + g_lo) is
 * formed in fp32 per element and split again in registers (pwk_direct_kernel) - only 1x1 stride-1 ungrouped convolutions with an
 * (activation) or (residual [+ReLU]) epilogue, cin_off = 0, ldx = Cin; anything else returns VIP_ERR_UNSUPPORTED. */
extern "C" int vip_conv2d_gated_nhwc_h2(const void* x, const void* gate, const void* w, const float* bias, const void* residual, void* y,
                                        const vip_conv_desc* d, float out_scale, int* status, void* stream) {
    VIP_REQUIRE(gate, VIP_ERR_BAD_ARG, "vip_conv2d_gated_nhwc_h2: null gate");
    VIP_REQUIRE(out_scale > 0.f, VIP_ERR_BAD_ARG, "vip_conv2d_gated_nhwc_h2: out_scale must be positive");
    VIP_REQUIRE(d && d->cin_off == 0 && d->ldx == d->Cin, VIP_ERR_UNSUPPORTED,
                "vip_conv2d_gated_nhwc_h2: the gate indexes the whole input channel axis (cin_off = 0, ldx = Cin)");
    ConvCall c = conv_call(x, w, bias, residual, y, d);
    c.gate = gate; c.out_scale = out_scale; c.status = status;
    return conv2d_impl(c, stream);
}

extern "C" int vip_conv2d_kernel_name_h2(const vip_conv_desc* d, int has_residual, char* name, size_t cap) {
    return kernel_query("vip_conv2d_kernel_name_h2", false, d, has_residual, 0, 0, name, cap);
}

extern "C" int vip_conv2d_kernel_variant_h2(const vip_conv_desc* d, int has_residual, char* variant, size_t cap) {
    return kernel_query("vip_conv2d_kernel_variant_h2", true, d, has_residual, 0, 0, variant, cap);
}
#else
extern "C" int vip_conv2d_nhwc_f16(const void* x, const void* w, const float* bias, const void* residual, void* y,
                                   const vip_conv_desc* d, void* stream) {
    return conv2d_impl(conv_call(x, w, bias, residual, y, d), stream);
}

extern "C" int vip_conv2d_gated_nhwc_f16(const void* x, const void* gate, const void* w, const float* bias,
                                         const void* residual, void* y, const vip_conv_desc* d, void* stream) {
    VIP_REQUIRE(gate, VIP_ERR_BAD_ARG, "vip_conv2d_gated_nhwc_f16: null gate");
    VIP_REQUIRE(d && d->cin_off == 0 && d->ldx == d->Cin, VIP_ERR_UNSUPPORTED,
                "vip_conv2d_gated_nhwc_f16: the gate indexes the whole input channel axis (cin_off = 0, ldx = Cin)");
    ConvCall c = conv_call(x, w, bias, residual, y, d);
    c.gate = gate;
    return conv2d_impl(c, stream);
}

extern "C" int vip_conv2d_hilo_nhwc_f16(const void* x, const void* w_hi, const void* w_lo, const float* bias,
                                        const void* residual, void* y, const vip_conv_desc* d, void* stream) {
    VIP_REQUIRE(w_lo, VIP_ERR_BAD_ARG, "vip_conv2d_hilo_nhwc_f16: null w_lo");
    ConvCall c = conv_call(x, w_hi, bias, residual, y, d);
    c.w_lo = w_lo;
    return conv2d_impl(c, stream);
}

/* y = act_post(conv(x) * g + residual), g = hi + lo of out_gate [B][2][Cout] fp16 (vip_se_gate_f16 with split): the squeeze-excite
 * multiply, the shortcut add and the block's ReLU in the epilogue of the block-final 1x1 layer.  w_lo: the layer's second weight term
 * or NULL.  Only where the same call with a residual selects pw_gemm_kernel or pwk_direct_kernel; VIP_ERR_UNSUPPORTED otherwise. */
extern "C" int vip_conv2d_out_gated_nhwc_f16(const void* x, const void* w, const void* w_lo, const float* bias, const void* out_gate,
                                             const void* residual, void* y, const vip_conv_desc* d, void* stream) {
    VIP_REQUIRE(out_gate && residual, VIP_ERR_BAD_ARG, "vip_conv2d_out_gated_nhwc_f16: null gate or residual");
    ConvCall c = conv_call(x, w, bias, residual, y, d);
    c.w_lo = w_lo; c.out_gate = out_gate;
    return conv2d_impl(c, stream);
}

/* dry run of vip_conv2d_out_gated_nhwc_f16: VIP_OK and the instantiation ("pw_gemm<KS=2,hilo> 1 x 256 ogate") where the call is taken */
extern "C" int vip_conv2d_out_gated_variant(const vip_conv_desc* d, int has_w_lo, char* variant, size_t cap) {
    return kernel_query("vip_conv2d_out_gated_variant", true, d, 1, 0, has_w_lo, variant, cap, true);
}

/* The same with a second output y2 = act2(y), computed from the ROUNDED y by the expression of vip_scale_add_act_f16's second output (bit
 * for bit what that launch gives on y): the tail of an ECA-NFNet block, whose next block reads act(x).  y2: the shape, span and leading
 * dimension of y.  act2: VIP_ACT_SILU is what is built; the selection and what declines are those of the one-output call. */
extern "C" int vip_conv2d_out_gated2_nhwc_f16(const void* x, const void* w, const void* w_lo, const float* bias, const void* out_gate,
                                              const void* residual, void* y, void* y2, int act2, const vip_conv_desc* d, void* stream) {
    VIP_REQUIRE(out_gate && residual && y2, VIP_ERR_BAD_ARG, "vip_conv2d_out_gated2_nhwc_f16: null gate, residual or second output");
    VIP_REQUIRE(act2 == VIP_ACT_SILU, VIP_ERR_UNSUPPORTED, "vip_conv2d_out_gated2_nhwc_f16: act2=%d (the second output is built for SiLU)", act2);
    ConvCall c = conv_call(x, w, bias, residual, y, d);
    c.w_lo = w_lo; c.out_gate = out_gate; c.y2 = y2;
    return conv2d_impl(c, stream);
}

/* dry run of vip_conv2d_out_gated2_nhwc_f16: the one-output call's selection with " y2" behind it ("pwk_direct<2> PT=4 ogate y2") */
extern "C" int vip_conv2d_out_gated2_variant(const vip_conv_desc* d, int has_w_lo, int act2, char* variant, size_t cap) {
    VIP_REQUIRE(act2 == VIP_ACT_SILU, VIP_ERR_UNSUPPORTED, "vip_conv2d_out_gated2_variant: act2=%d (the second output is built for SiLU)", act2);
    const int st = kernel_query("vip_conv2d_out_gated2_variant", true, d, 1, 0, has_w_lo, variant, cap, true);
    if (st != VIP_OK) return st;
    const size_t n = strlen(variant);
    if (n + 4 <= cap) memcpy(variant + n, " y2", 4);
    return VIP_OK;
}

extern "C" int vip_conv2d_kernel_name(const vip_conv_desc* d, int has_residual, int has_gate, int has_w_lo, char* name,
                                      size_t cap) {
    return kernel_query("vip_conv2d_kernel_name", false, d, has_residual, has_gate, has_w_lo, name, cap);
}

extern "C" int vip_conv2d_kernel_variant(const vip_conv_desc* d, int has_residual, int has_gate, int has_w_lo, char* variant,
                                         size_t cap) {
    return kernel_query("vip_conv2d_kernel_variant", true, d, has_residual, has_gate, has_w_lo, variant, cap);
}

// the descriptor of a plain GEMM [M, K] x [K, N]: M images of one pixel, a 1 x 1 ungrouped convolution
static vip_conv_desc gemm_desc(int M, int N, int K, int lda, int ldw, int ldc, int ldr, int act_pre, int act_post) {
    vip_conv_desc d;
    d.B = M; d.H = 1; d.W = 1; d.Cin = K; d.Cout = N; d.kh = d.kw = 1; d.sh = d.sw = 1; d.pt = d.pl = 0;
    d.Ho = d.Wo = 1; d.groups = 1; d.ldx = lda; d.cin_off = 0; d.ldy = ldc; d.cout_off = 0; d.ldr = ldr;
    d.res_off = 0; d.ldw = ldw; d.act_pre = act_pre; d.act_post = act_post;
    return d;
}

extern "C" int vip_gemm_bias_act_f16(const void* A, const void* W, const float* bias, const void* residual,
                                     void* C, int M, int N, int K, int lda, int ldw, int ldc, int ldr,
                                     int act_pre, int act_post, void* stream) {
    const vip_conv_desc d = gemm_desc(M, N, K, lda, ldw, ldc, ldr, act_pre, act_post);
    return vip_conv2d_nhwc_f16(A, W, bias, residual, C, &d, stream);
}

/* LayerNorm folded into the GEMM that consumes it (pwx_ln_kernel).  Shapes: the row must fit the kernel's resident fragments
 * (K <= 384: 96 fragment + 64 accumulator registers at 32 pixels per wave, no scratch; K = 512 would leave 16 pixels per wave and has
 * no call site with M >= 16384 in the ensemble), and the activation-resident form needs enough rows and channel tiles to pay
 * (M >= 16384, N >= 256: the limits of pwx_kernel). */
extern "C" int vip_ln_gemm_supported(int M, int K, int N, int act) {
    if (M < 16384 || N < 256 || N % 8 != 0 || K % 8 != 0 || K <= 64 || K > 384 || (unsigned)act > 4u) return 0;
    // what follows is POLICY, not capability: call sites that measured no faster than the two launches.  VIP_LN_GEMM_ALL=1 (read per
    // call: the A/B driver and the kernel's tests set it) lifts it, so that every shape the kernel can run stays measurable and tested.
    const char* all = getenv("VIP_LN_GEMM_ALL");
    if (all && atoi(all)) return 1;
    // Measured per call site against layernorm_kernel + the GEMM ops.dense picks (tools/bench_ln_gemm.py, eight rounds per side,
    // profiles/ln_gemm_per_site_ab.log).  A workgroup owns 128 rows and every channel tile of N, so M / 128 workgroups run on the chip's
    // 512 slots (256 CUs x 2).  Where they fill them the fused launch wins outside the spread of the rounds - ConvNeXt-T stage 2 fc1
    // (147456 x 384 x 1536 gelu), GCViT-T level 1 fc1 (200704 x 128 x 384 gelu) - and so does the one under-filled site with few
    // channel tiles, GCViT-T level 2 qkv with a global query (50176 x 256 x 512).  With ~50 000 rows (392-394 workgroups) and N >= 768 -
    // ViT-S qkv / fc1 (50432 x 384 x 1152 / 1536), GCViT-T level 2 qkv / fc1 (50176 x 256 x 768) - the direct kernel's split over N
    // makes up for the LayerNorm pass it cannot fold: fused and two launches overlap, no gain shown, they keep the two launches.
    if (M < 65536 && N > 512) return 0;
    return 1;
}

extern "C" int vip_ln_gemm_bias_act_f16(const void* A, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* W,
                                        const float* bias, const void* residual, void* C, int M, int N, int K, int lda, int ldw,
                                        int ldc, int ldr, int act_pre, int act_post, void* stream) {
    VIP_REQUIRE(ln_gamma && ln_beta, VIP_ERR_BAD_ARG, "vip_ln_gemm_bias_act_f16: null LayerNorm parameters");
    VIP_REQUIRE(ln_eps > 0.f, VIP_ERR_BAD_ARG, "vip_ln_gemm_bias_act_f16: eps must be positive");
    const vip_conv_desc d = gemm_desc(M, N, K, lda, ldw, ldc, ldr, act_pre, act_post);
    ConvCall c = conv_call(A, W, bias, residual, C, &d);
    c.ln_g = ln_gamma; c.ln_b = ln_beta; c.ln_eps = ln_eps;
    return conv2d_impl(c, stream);
}

extern "C" int vip_gemm_split_f16(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int lda,
                                  int ldw, int act, void* stream) {
    VIP_REQUIRE(M > 0 && M <= 256, VIP_ERR_UNSUPPORTED, "vip_gemm_split_f16: M=%d (1..256 rows)", M);
    const vip_conv_desc d = gemm_desc(M, N, K, lda, ldw, 2 * N, 0, act, VIP_ACT_NONE);
    ConvCall c = conv_call(A, W, bias, nullptr, C, &d);
    c.y_lo_off = N;
    return conv2d_impl(c, stream);
}

extern "C" int vip_gemm_split2_hilo_f16(const void* A, const void* W, const void* W_lo, const float* bias, void* C, int M, int N, int K,
                                        int ldw, int act, void* stream) {
    VIP_REQUIRE(W_lo, VIP_ERR_BAD_ARG, "vip_gemm_split2_hilo_f16: null W_lo");
    VIP_REQUIRE(M > 0 && M <= 256, VIP_ERR_UNSUPPORTED, "vip_gemm_split2_hilo_f16: M=%d (1..256 rows)", M);
    VIP_REQUIRE(K % 8 == 0, VIP_ERR_ALIGNMENT, "vip_gemm_split2_hilo_f16: K must be a multiple of 8");
    const vip_conv_desc d = gemm_desc(M, N, K, 2 * K, ldw, 2 * N, 0, act, VIP_ACT_NONE);
    ConvCall c = conv_call(A, W, bias, nullptr, C, &d);
    c.y_lo_off = N; c.w_lo = W_lo; c.x_split = true;
    return conv2d_impl(c, stream);
}

extern "C" int vip_gemm_split2_f16(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int ldw, int act,
                                   void* stream) {
    VIP_REQUIRE(M > 0 && M <= 256, VIP_ERR_UNSUPPORTED, "vip_gemm_split2_f16: M=%d (1..256 rows)", M);
    VIP_REQUIRE(K % 8 == 0, VIP_ERR_ALIGNMENT, "vip_gemm_split2_f16: K must be a multiple of 8");
    const vip_conv_desc d = gemm_desc(M, N, K, 2 * K, ldw, 2 * N, 0, act, VIP_ACT_NONE);
    ConvCall c = conv_call(A, W, bias, nullptr, C, &d);
    c.y_lo_off = N; c.x_split = true;
    return conv2d_impl(c, stream);
}
#endif  // VIP_GEMM_H2
