/*
 * vipcup_hip.h — C ABI of libvipcup_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the per-image scoring path of awsaf49/vip-cup-2022
 * (reference main.py:58-149 -> model.predict).  The reference has no FFI of its
 * own (it is 100 % Python on TensorFlow); every entry point below replaces the
 * TensorFlow/Keras op group named in its comment (reference file:line), i.e. it
 * is what a ctypes binding on the reference side would call instead of the Keras
 * layer.  See INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *   - return 0 on success, negative vip_status on error; nothing throws or
 *     aborts across the ABI; no hidden allocation, no hidden synchronisation;
 *   - pointers are DEVICE pointers unless the name ends in _h (host);
 *   - activations are NHWC / row-major fp16 ("f16"), accumulation is fp32;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - all functions are stateless and thread-safe.
 */
#ifndef VIPCUP_HIP_H
#define VIPCUP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vip_status {
    VIP_OK = 0,
    VIP_ERR_BAD_ARG = -1,      /* null pointer, non-positive dim, unsupported value  */
    VIP_ERR_ALIGNMENT = -2,    /* channel count / stride not a multiple of 8 halfs   */
    VIP_ERR_UNSUPPORTED = -3,  /* shape outside what the kernel family implements    */
    VIP_ERR_LAUNCH = -4,       /* hipGetLastError() != hipSuccess after the launch   */
    VIP_ERR_JPEG = -5,         /* stream is not a baseline JPEG this decoder accepts */
    VIP_ERR_PNG = -6,          /* stream is not a PNG this decoder accepts           */
    VIP_ERR_WEBP = -7          /* stream is not a WebP this decoder accepts          */
} vip_status;

/* activation codes shared by every epilogue */
enum { VIP_ACT_NONE = 0, VIP_ACT_RELU = 1, VIP_ACT_SILU = 2, VIP_ACT_GELU = 3, VIP_ACT_SIGMOID = 4 };

/* ABI version: major*1000 + minor. */
int vip_version(void);
/* Human-readable description of the last failing argument check on this thread. */
const char* vip_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Conv2D (+ folded BatchNorm) (+ activation) (+ residual) — implicit GEMM on MFMA.
 * Replaces: tf.keras.layers.Conv2D + BatchNormalization + Activation (+ Add) chains, e.g.
 *   models/resnet_rs/resnet_rs_model.py:64-84,97-139,235-280 ; kecam common_layers.py:190-248 ;
 *   models/tfimm/architectures/convnext.py:320-327 ; and every Dense layer (kh=kw=1, H=W=1).
 *
 *   y[b,ho,wo,co] = act_post( act_pre( sum_{r,s,ci} x[b,ho*sh+r-pt, wo*sw+s-pl, ci] * w[co,r,s,ci]
 *                                       + bias[co] ) + residual[b,ho,wo,co] )
 *
 *   x        [B,H,W,*]   f16, pixel stride ldx (>= cin_off + groups*cin_g), channels cin_off.. used
 *   w        [Cout][kh][kw][Cin_g] f16, row stride ldw halfs (ldw >= kh*kw*Cin_g, ldw % 8 == 0)
 *   bias     [Cout] f32 or NULL
 *   residual [B,Ho,Wo,*] f16 pixel stride ldr, or NULL
 *   y        [B,Ho,Wo,*] f16 pixel stride ldy, channels cout_off.. written
 *   groups   grouped convolution: Cin_g = Cin/groups inputs feed Cout/groups outputs.
 *   Out-of-image taps read as zero (explicit ZeroPadding2D / SAME semantics are expressed by pt/pl).
 *   Requirements: Cin_g % 8 == 0, Cout_g % 8 == 0, every ld* and channel offset % 8 == 0.
 * ------------------------------------------------------------------------------------------ */
typedef struct vip_conv_desc {
    int B, H, W;            /* input batch / spatial size                      */
    int Cin, Cout;          /* total input / output channels (all groups)      */
    int kh, kw, sh, sw;     /* kernel and stride                               */
    int pt, pl;             /* zero padding before (top / left)                */
    int Ho, Wo;             /* output spatial size (caller computes)           */
    int groups;
    int ldx, cin_off;       /* input pixel stride / first channel (halfs)      */
    int ldy, cout_off;      /* output pixel stride / first channel             */
    int ldr, res_off;       /* residual pixel stride / first channel           */
    int ldw;                /* weight row stride (halfs)                       */
    int act_pre, act_post;  /* VIP_ACT_*                                       */
} vip_conv_desc;

int vip_conv2d_nhwc_f16(const void* x, const void* w, const float* bias, const void* residual,
                        void* y, const vip_conv_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * vip_conv2d_nhwc_f16 with a squeeze-excite gate folded into the activation load:
 *   y = epilogue( conv1x1( x[b,h,w,c] * gate[b,c] ) )
 * gate [B][2][Cin] f16: the split output of vip_se_gate_f16 / vip_gemm_split_f16 (hi = fp16(g), lo = fp16(g - hi)).
 * The operand is fma(x, hi, x * lo) in packed fp16 - one rounding per element.  vip_scale_add_act3_f16 with two scale
 * planes followed by vip_conv2d_nhwc_f16 computes the same thing with x * (hi + lo) rounded from fp32: the two agree
 * except where the inner rounding of x * lo tips the final one (rare, one ulp of one operand), and are bit-identical
 * when lo = 0.  What the gated form saves is the read+write of the expanded tensor.  Replaces `Multiply()([inputs, se])` + the projection Conv2D of kecam se_module
 * (common_layers.py:328-332 with efficientnet_v2.py:97-101) and of gcvit/layers/feature.py:66-70,135-137.
 * Only 1x1 stride-1 ungrouped convolutions whose epilogue is (activation) or (residual [+ReLU]) are accepted
 * (VIP_ERR_UNSUPPORTED otherwise: scale with vip_scale_add_act_f16, then vip_conv2d_nhwc_f16).
 * ------------------------------------------------------------------------------------------ */
int vip_conv2d_gated_nhwc_f16(const void* x, const void* gate, const void* w, const float* bias, const void* residual,
                              void* y, const vip_conv_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * vip_conv2d_nhwc_f16 with two-term weights:  y = epilogue( (w_hi + w_lo) * x ),  w_lo = fp16(W32 - fp16(W32)) in the layout
 * of w_hi - the layer computes with ~22-bit weights.  For the short-K, many-pixel 1x1 convolutions (EfficientNet expand
 * convolutions, kecam efficientnet_v2.py:63-66): they are HBM-bound, so the second MFMA per fragment is free, and their
 * fp16 weight rounding is what dominates EfficientNetV1-B4's logit error (Numerics).
 * Only 1x1 stride-1 ungrouped convolutions with K <= 256 and an (activation) or (residual [+ReLU]) epilogue.
 * ------------------------------------------------------------------------------------------ */
int vip_conv2d_hilo_nhwc_f16(const void* x, const void* w_hi, const void* w_lo, const float* bias, const void* residual,
                             void* y, const vip_conv_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Block-final 1x1 convolution of a squeeze-excite bottleneck with the block tail in its epilogue:
 *   y[m, n] = act_post( (conv(x)[m, n] + bias[n]) * g[image(m), n] + residual[m, n] ),   g = hi + lo of out_gate
 * out_gate [B][2][Cout] fp16 is the split gate of vip_se_gate_f16 / vip_gemm_split_f16.  The layer is linear, so the gate's
 * pooled input mean_hw(conv(x)) = W mean_hw(x) + b can be formed from x BEFORE this launch (reduce weights folded with W): the
 * un-gated map is never written, and the pooling read and the vip_scale_add_act_f16 launch go (ResNet-RS `SE`,
 * resnet_rs_model.py:145-183,262-280).  The multiply is fp32 on the accumulators, before the residual add and the single fp16
 * rounding of the store.  w_lo: the second weight term (vip_conv2d_hilo_nhwc_f16) or NULL.  act_pre none, act_post none / ReLU,
 * ungrouped, cout_off = 0, and only where the same call with a residual selects pw_gemm_kernel or pwk_direct_kernel - the
 * selection is that call's own; everything else returns VIP_ERR_UNSUPPORTED and the caller runs conv + vip_scale_add_act_f16.
 * vip_conv2d_out_gated_variant: the dry run - VIP_OK and the instantiation ("pwk_direct<2> PT=4 ogate") where the call is taken.
 * ------------------------------------------------------------------------------------------ */
int vip_conv2d_out_gated_nhwc_f16(const void* x, const void* w, const void* w_lo, const float* bias, const void* out_gate,
                                  const void* residual, void* y, const vip_conv_desc* d, void* stream);
int vip_conv2d_out_gated_variant(const vip_conv_desc* d, int has_w_lo, char* variant, size_t cap);
/* The two-output form: also y2[m, n] = act2(y[m, n]), from the ROUNDED y by the expression of vip_scale_add_act_f16's second output, so
 * y2 is bit for bit what that launch gives on y.  The tail of an ECA-NFNet block (nfnets.py:116-168): deep_4 is linear, its ECA gate is
 * formed from its pooled INPUT, and the next block reads act(x) - the un-gated map, the pool over it and the elementwise launch go.
 * y2: the shape, span and leading dimension of y.  act2: VIP_ACT_SILU (anything else VIP_ERR_UNSUPPORTED).  Kernels of their own
 * (pw_gemm_kernel<.., OG, Y2>, pwk_direct_kernel<.., OG2>); the selection and what declines are the one-output call's.
 * vip_conv2d_out_gated2_variant: the dry run - the one-output variant with " y2" behind it. */
int vip_conv2d_out_gated2_nhwc_f16(const void* x, const void* w, const void* w_lo, const float* bias, const void* out_gate,
                                   const void* residual, void* y, void* y2, int act2, const vip_conv_desc* d, void* stream);
int vip_conv2d_out_gated2_variant(const vip_conv_desc* d, int has_w_lo, int act2, char* variant, size_t cap);

/* Dense / 1x1 convenience wrapper: C[M,N] = act_post(act_pre(A[M,K] @ W[N,K]^T + bias) + residual).
 * Replaces tf.keras.layers.Dense (gcvit/layers/attention.py:25,33, feature.py:20-22;
 * tfimm/layers/transformers.py:192-205; all classifier heads). */
int vip_gemm_bias_act_f16(const void* A, const void* W, const float* bias, const void* residual,
                          void* C, int M, int N, int K, int lda, int ldw, int ldc, int ldr,
                          int act_pre, int act_post, void* stream);

/* The same with a LayerNorm over K folded into the activation operand:
 *   C[M,N] = act_post(act_pre(LN(A[M,K]; gamma, beta, eps) @ W[N,K]^T + bias) + residual)
 * in ONE launch: the row is normalised in the registers of the GEMM that consumes it (fp32 two-pass statistics, the normalised
 * operand rounded to fp16 exactly where vip_layernorm_f16 would have stored it), so LN(A) is neither written nor read back.
 * ln_gamma, ln_beta [K] f32; the other arguments and the epilogue modes ((activation) or (residual [+ post-ReLU])) as
 * vip_gemm_bias_act_f16.  vip_ln_gemm_supported(M, K, N, act_pre) != 0 for the shapes it takes: what the kernel can run (64 < K <= 384,
 * K % 8 == 0, M >= 16384, N >= 256) less the shapes that measured no faster than the two launches (M < 65536 with N > 512: too few
 * workgroups for the chip; VIP_LN_GEMM_ALL=1 lifts this for A/B runs and tests).  Anything else returns VIP_ERR_UNSUPPORTED - use
 * vip_layernorm_f16 + vip_gemm_bias_act_f16.
 * Replaces LayerNormalization -> Dense of models/tfimm/architectures/convnext.py:220-229 (norm -> fc1, stage 2) and
 * models/gcvit/layers/block.py:60-81 (level 1 norm2 -> fc1, level 2 norm1 -> qkv with a global query); the same pattern of
 * vit.py:170-227 (norm1 -> qkv, norm2 -> fc1) and the other level 2 layers of GCViT are shapes the policy leaves on two launches. */
int vip_ln_gemm_supported(int M, int K, int N, int act);
int vip_ln_gemm_bias_act_f16(const void* A, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* W,
                             const float* bias, const void* residual, void* C, int M, int N, int K, int lda, int ldw,
                             int ldc, int ldr, int act_pre, int act_post, void* stream);

/* Few-row Dense with a SPLIT fp16 output:  v = act(A[M,K] @ W[N,K]^T + bias);  C[m][0][n] = fp16(v), C[m][1][n] =
 * fp16(v - fp16(v)), C is [M][2][N] f16.  For the last layer of a squeeze-excite block whose matrices are too large for
 * vip_se_gate_f16 (resnet_rs_model.py:167-180 at 1024/2048 channels): the gate keeps ~22 bits.  M <= 256, N % 4 == 0. */
int vip_gemm_split_f16(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int lda,
                       int ldw, int act, void* stream);

/* vip_gemm_split_f16 whose INPUT rows are split too: A is [M][2][K] f16 (hi plane, lo plane - what
 * vip_global_avgpool_split_f16 or a previous split Dense wrote), v = act((A_hi + A_lo) @ W^T + bias), C [M][2][N] as above.
 * For the chains of Dense layers on pooled vectors (the first squeeze-excite layer at 1024/2048 channels,
 * resnet_rs_model.py:150-166; kecam resnest.py:44-57; the ECA Conv1D of kecam attention_layers `eca_module`): a pooled vector's
 * rounding error is the same for every pixel the gate later scales, so it is not averaged away.  M <= 256, N % 4 == 0, K % 8 == 0. */
int vip_gemm_split2_f16(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int ldw, int act,
                        void* stream);
/* vip_gemm_split2_f16 with two-term weights: v = act((A_hi + A_lo) @ W^T + A_hi @ W_lo^T + bias), W_lo = fp16(W32 - W) in the layout
 * of W.  For a first squeeze-excite layer that is the PRODUCT of two layers (the reduce layer folded with the linear layer in front of
 * the pool, see vip_conv2d_out_gated_nhwc_f16): its elements are not fp16 values. */
int vip_gemm_split2_hilo_f16(const void* A, const void* W, const void* W_lo, const float* bias, void* C, int M, int N, int K, int ldw,
                             int act, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused two-layer MLP:  y[M,C] = W2 . act(W1 . LN(x) + b1) + b2 (+ residual), hidden tensor never written to memory.
 * LN = the LayerNormalization in front of the MLP (convnext.py:199 `norm`, gcvit block `norm2`, ViT `norm2`) when
 * ln_gamma/ln_beta [C] f32 are given (both NULL: x is used as is).
 * Replaces Dense -> GELU -> Dense (-> layer-scale, folded by the caller) -> Add of
 *   tfimm/architectures/convnext.py:200-229, gcvit/layers/feature.py:20-22 (Mlp),
 *   tfimm/layers/transformers.py:192-205 (MLP)
 * for narrow token widths whose two weight matrices fit in LDS together.
 *   x [M][ldx] f16 ; w1 [hidden][ldw1] f16 (rows = hidden channels, C contiguous) ; b1 [hidden] f32 or NULL ;
 *   w2 [C][ldw2] f16 (rows = output channels, hidden contiguous) ; b2 [C] f32 or NULL ; residual [M][ldr] or NULL.
 * vip_mlp_fused_supported() says whether a shape is handled (C in {64, 96} with both matrices <= 160 KB of LDS, or C = 192
 * with streamed weights; act = GELU, hidden % 32 == 0, M >= 8192); otherwise use two vip_gemm_bias_act_f16 calls.
 * ------------------------------------------------------------------------------------------ */
int vip_mlp_fused_supported(int M, int C, int hidden, int act);
/* Dry run of that launch (nothing is launched; the launcher calls the same function): returns the number of token tiles the kernel
 * walks (0: shape not supported), *workgroups = the workgroups that walk them (tile += workgroups: min(tiles, CUs) - asks the current
 * device for its CU count), *tile_rows = tokens per tile (512 with LDS-resident weights, 256 with streamed ones).  Either pointer may
 * be NULL.  More tiles than workgroups means a workgroup runs several passes of its tile loop. */
int vip_mlp_fused_plan(int M, int C, int hidden, int act, int* workgroups, int* tile_rows);
int vip_mlp_fused_f16(const void* x, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* w1,
                      const float* b1, const void* w2, const float* b2, const void* residual, void* y, int M, int C,
                      int hidden, int ldx, int ldw1, int ldw2, int ldy, int ldr, int act, void* stream);

/* ------------------------------------------------------------------------------------------
 * Squeeze-excite gate in one launch:  gate[b,:] = act2(W2 . act1(W1 . mean_hw(x[b]) + b1) + b2).
 * Replaces GlobalAveragePooling2D -> Conv1x1/Dense(+act) -> Conv1x1/Dense(+sigmoid) of
 *   kecam common_layers.py:311-332 (se_module), resnet_rs_model.py:145-183 (SE),
 *   gcvit/layers/feature.py:46-70 (SE), kecam resnest/resnest.py:44-57 (split-attention gate).
 *   x [B][HW][ldx] f16 ; w1 [Cr][ldw1] f16, b1 [Cr] f32 or NULL ; w2 [Cout][ldw2] f16, b2 [Cout] f32 or NULL ;
 *   gate [B][Cout] f16 (split = 0) or [B][2][Cout] f16 (split = 1: hi = fp16(g), lo = fp16(g - hi)).  C, Cr multiples
 *   of 8 (pad with zero weights).  The pooled and hidden vectors stay fp32.  A gate multiplies a whole channel map, so
 *   its rounding error does not average out over pixels the way an activation's does: the split form is what
 *   vip_conv2d_gated_nhwc_f16 and vip_scale_add_act3_f16 consume.
 * ------------------------------------------------------------------------------------------ */
int vip_se_gate_f16(const void* x, const void* w1, const float* b1, const void* w2, const float* b2, void* gate,
                    int B, int HW, int C, int ldx, int Cr, int ldw1, int Cout, int ldw2, int act1, int act2,
                    int split, void* stream);
/* The same with a two-term first matrix, w1_lo = fp16(W32 - w1) in the layout of w1, joined with it in fp32 (~22-bit weights): for a
 * reduce layer folded with the linear layer in front of the pool (see vip_conv2d_out_gated_nhwc_f16). */
int vip_se_gate_hilo_f16(const void* x, const void* w1, const void* w1_lo, const float* b1, const void* w2, const float* b2, void* gate,
                         int B, int HW, int C, int ldx, int Cr, int ldw1, int Cout, int ldw2, int act1, int act2, int split,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Depthwise Conv2D k x k (+bias)(+act).  Replaces tf.keras.layers.DepthwiseConv2D:
 *   gcvit/layers/feature.py:93,133 ; tfimm/architectures/convnext.py:192-198 ;
 *   kecam efficientnet_v2.py:85 (common_layers.py:251-265).
 *   w [kh][kw][C] f32 (k*k taps per channel: there is no K-long sum for rounding errors to average out in, and the
 *   filter is a few KB, so it stays in full precision) ; bias [C] f32 or NULL ; C % 8 == 0.
 * ------------------------------------------------------------------------------------------ */
int vip_dwconv2d_nhwc_f16(const void* x, const float* w, const float* bias, void* y,
                          int B, int H, int W, int C, int k, int stride, int pt, int pl,
                          int Ho, int Wo, int act, void* stream);

/* Depthwise Conv2D that also leaves the sums a following squeeze-excite pool needs (the `DepthwiseConv2D -> activation ->
 * se_module` run of kecam efficientnet_v2.py:85-97 and `conv = [dw3x3, gelu, SE, ...]` of gcvit/layers/feature.py:46-70,93-96):
 * every workgroup adds up the activated fp32 outputs of its tiles and writes one row of partial sums,
 *   partials [B][parts][C] f32,  parts = vip_dwconv2d_pool_parts(...)  (0: shape not handled - use the plain call),
 * in a fixed order (no atomics: bit-reproducible).  vip_se_gate_pooled_f16 finishes the mean from them instead of reading
 * the whole map again. */
int vip_dwconv2d_pool_parts(int B, int H, int W, int C, int k, int stride, int Ho, int Wo);
/* Dry run of the stride-1 register-tiled depthwise launch (plain form, or with pooled != 0 the pooling form): returns the number of
 * tile groups a channel block's workgroups walk (0: the tile kernel does not take the shape), *workgroups = those workgroups
 * (gridDim.x; at the cap each XCD walks one band of groups), geom[4] = {channel chunks per block, tiles per block, channel blocks
 * (gridDim.y), workgroup cap}.  workgroups / geom may be NULL.  Pure host arithmetic: no device is needed. */
long vip_dwconv2d_tile_plan(int B, int H, int W, int C, int k, int stride, int Ho, int Wo, int pooled, int* workgroups, int* geom);
int vip_dwconv2d_pool_nhwc_f16(const void* x, const float* w, const float* bias, void* y, float* partials, int parts,
                               int B, int H, int W, int C, int k, int stride, int pt, int pl, int Ho, int Wo, int act,
                               void* stream);
/* vip_se_gate_f16 whose pool arrives as partial sums: mean[b,c] = sum_g partials[b][g][c] / HW (fp32), then the same two
 * matrix-vector products and output forms. */
int vip_se_gate_pooled_f16(const float* partials, int parts, const void* w1, const float* b1, const void* w2,
                           const float* b2, void* gate, int B, int HW, int C, int Cr, int ldw1, int Cout, int ldw2,
                           int act1, int act2, int split, void* stream);

/* LayerNormalization over the last axis (rows x C), fp32 statistics.
 * Replaces tf.keras.layers.LayerNormalization (gcvit/layers/block.py:28,39; tfimm/layers/factory.py:37-45).
 * gamma/beta f32 [C]. */
int vip_layernorm_f16(const void* x, const float* gamma, const float* beta, void* y,
                      int rows, int C, float eps, void* stream);

/* 2-D pooling, NHWC. mode 0: max over a ZERO-padded input (gcvit/layers/feature.py:151-152,
 * kecam aotnet.py:329-330); mode 1: average dividing by the number of VALID taps (Keras
 * AveragePooling2D padding="same", resnet_rs_model.py:207-212); mode 2: average dividing by k*k
 * (explicit ZeroPadding2D followed by VALID AvgPool, kecam resnest.py:63-65). */
int vip_pool2d_nhwc_f16(const void* x, void* y, int B, int H, int W, int C, int ldx, int ldy,
                        int k, int stride, int pt, int pl, int Ho, int Wo, int mode, void* stream);

/* Global average pool [B,HW,C] -> [B,C] (f16 out, fp32 accumulate).
 * Replaces GlobalAveragePooling2D (resnet_rs_model.py:150,468) / tfa AdaptiveAveragePooling2D(1). */
int vip_global_avgpool_f16(const void* x, void* y, int B, int HW, int C, int ldx, void* stream);

/* The same pool with the mean written as two fp16 planes: y [B][2][C], y[b][0][c] = fp16(mean), y[b][1][c] = fp16(mean - hi). */
int vip_global_avgpool_split_f16(const void* x, void* y, int B, int HW, int C, int ldx, void* stream);

/* Classifier head with fp32 output: out[b,n] = bias[n] + sum_c mean_p(x[b,p,c]) * W[n,c].
 * Replaces GlobalAveragePooling2D + Dense(classes) (resnet_rs_model.py:468-476; gcvit models/gcvit.py:104-113;
 * tfimm convnext.py:432-436) — with HW = 1 it is a plain Dense on [B,C] vectors (vit.py:441-461).
 * x f16 [B,HW,*] pixel stride ldx; W f32 [N][C]; bias f32 [N] or NULL; out f32 [B][N]. C <= 4096. */
int vip_gap_dense_f32(const void* x, const float* W, const float* bias, float* out, int B, int HW, int C,
                      int ldx, int N, void* stream);

/* The head with a LayerNorm between the pool and the Dense, all fp32:
 *   out[b,n] = bias[n] + sum_c LN_c(mean_p x[b,p,c]; gamma, beta, eps) * W[n,c]
 * Replaces GlobalAveragePooling2D -> LayerNormalization -> Dense of tfimm convnext.py:432-436 and kecam hornet.py:166-171.
 * gamma, beta f32 [C]; the rest as vip_gap_dense_f32. */
int vip_gap_ln_dense_f32(const void* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias,
                         float* out, int B, int HW, int C, int ldx, int N, void* stream);

/* y = act( x * scale[b,c] + residual ) — the SE "excite" multiply fused with the block's Add+act.
 * Replaces layers.multiply + Add + Activation (resnet_rs_model.py:183,278-280; gcvit feature.py:70).
 * scale [B,C] f16 or NULL (=1); residual f16 or NULL. */
int vip_scale_add_act_f16(const void* x, const void* scale, const void* residual, void* y,
                          int B, int HW, int C, int act, void* stream);
/* Same with a second output  y2 = act2(y)  computed from the fp16-rounded y (bit-identical to a second launch reading y
 * back): NormFreeNet's block needs both x_{l+1} and act(x_{l+1}) (kecam nfnets.py:116-168).  y2 may be NULL. */
int vip_scale_add_act2_f16(const void* x, const void* scale, const void* residual, void* y, void* y2,
                           int B, int HW, int C, int act, int act2, void* stream);
/* Same with the scale as scale_planes fp16 planes [B][scale_planes][C] that are summed in fp32 (2 = a split gate). */
int vip_scale_add_act3_f16(const void* x, const void* scale, int scale_planes, const void* residual, void* y, void* y2,
                           int B, int HW, int C, int act, int act2, void* stream);

/* Elementwise product of channel slices of two row-major tensors:  y[m, y_off + c] = a[m, a_off + c] * b[m, b_off + c],
 * c < C (fp32 product, one rounding).  Replaces the `pw * dw` gating products of kecam hornet.py:104-107 (gnconv), whose
 * operands are slices of wider tensors (tf.split).  Everything a multiple of 8 halfs. */
int vip_mul_f16(const void* a, const void* b, void* y, long rows, int C, int lda, int a_off, int ldb, int b_off,
                int ldy, int y_off, void* stream);

/* ResNeSt split-attention combine (kecam resnest/resnest.py:57-61): out[b,p,c] = sum_r x[b,p,r*C+c] *
 * scale[b,r*C+c].  x f16 [B,HW,radix*C]; scale f16 [B,radix*C] (the r-softmax weights); out [B,HW,C]. */
int vip_radix_combine_f16(const void* x, const void* scale, void* y, int B, int HW, int C, int radix,
                          void* stream);
/* Same with the weights as scale_planes fp16 planes [B][scale_planes][radix*C] summed in fp32 (2 = split, see vip_se_gate_f16). */
int vip_radix_combine2_f16(const void* x, const void* scale, int scale_planes, void* y, int B, int HW, int C, int radix,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * GCViT attention half of a block in ONE launch - the fused form of the north-star path:
 *   y = x + proj( window_attention( qkv( LayerNorm(x) ) ) )       gcvit/layers/block.py:58-79, attention.py:52-83
 * for the level-0 and level-1 configurations - 7 x 7 windows, C = 64 with 2 heads of 32 or C = 128 with 4
 * (vip_gcvit_attn_block_supported; other levels run vip_layernorm_f16 -> vip_gemm_bias_act_f16 -> vip_window_attn_fwd_f16 ->
 * vip_gemm_bias_act_f16).
 *   x, y [B][Hp][Wp][C] f16, Hp and Wp multiples of 7, y must not alias x ; q_global [B][49][C] f16 or NULL ;
 *   wqkv [nq*C][ldwq] f16 (nq = 3: q, k, v rows; nq = 2 with q_global: k, v), bqkv [nq*C] f32 or NULL ;
 *   wproj [C][ldwp] f16 (layer scale folded in by the caller), bproj [C] f32 or NULL ; ln_gamma, ln_beta [C] f32 ;
 *   table [(2 ws - 1)^2][heads] f32 ; scale = head_dim^-0.5.
 * Same roundings as the four launches (LayerNorm output, q / k / v, attention output and y are rounded to fp16 at the same
 * points); the proj sum runs over the head channels in another order, so y agrees to fp32 summation order, not bitwise.
 * ------------------------------------------------------------------------------------------ */
int vip_gcvit_attn_block_supported(int C, int heads, int ws);
int vip_gcvit_attn_block_f16(const void* x, const void* q_global, const float* ln_gamma, const float* ln_beta, float ln_eps,
                             const void* wqkv, int ldwq, const float* bqkv, const void* wproj, int ldwp, const float* bproj,
                             const float* table, void* y, int B, int Hp, int Wp, int C, int heads, int ws, float scale,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * GCViT window attention core (gcvit/layers/attention.py:52-83, window.py:3-15):
 *   out = softmax( (q*scale) k^T + rel_bias ) v     per (image, window, head)
 * qkv        [B, Hp, Wp, nq*C] f16, feature-map layout (NOT window-partitioned): the window
 *            partition / reverse permutation is folded into the kernel's addressing.
 *            nq = 3: channels = (q|k|v, head, hd);  nq = 2 (global query): (k|v, head, hd).
 * q_global   [B, ws*ws, C] f16 when nq == 2 (channels = (head, hd)), else NULL.
 * bias_table [(2ws-1)^2, heads] f32 — the raw relative_position_bias_table; the index
 *            (dh+ws-1)*(2ws-1)+(dw+ws-1) (attention.py:39-50) is computed in-kernel.
 * out        [B, Hp, Wp, C] f16 feature-map layout, channels = (head, hd).
 * Hp, Wp multiples of ws; hd = C/heads must be 32.
 * ------------------------------------------------------------------------------------------ */
int vip_window_attn_fwd_f16(const void* qkv, const void* q_global, const float* bias_table,
                            void* out, int B, int Hp, int Wp, int C, int heads, int ws, int nq,
                            float scale, void* stream);

/* Plain multi-head self-attention core (tfimm/architectures/vit.py:148-167):
 * out = softmax(scale * q k^T) v per (image, head).  qkv [B,N,3*D] f16 (channels = (q|k|v, head, hd));
 * out [B,N,D].  head_dim = D/heads must be 64, N <= 224. */
int vip_mhsa_fwd_f16(const void* qkv, void* out, int B, int N, int D, int heads, float scale,
                     void* stream);

/* ViT token assembly (tfimm/architectures/vit.py:419-426): out[b,0,:] = cls_token + pos_embed[0];
 * out[b,1+i,:] = patches[b,i,:] + pos_embed[1+i].  patches [B,n_patches,D], cls [D], pos [n_patches+1,D],
 * out [B,n_patches+1,D], all f16. */
int vip_vit_tokens_f16(const void* patches, const void* cls_token, const void* pos_embed, void* out,
                       int B, int n_patches, int D, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input pipeline (dataset/dataset.py:22-39): decode_jpeg -> cast f32 -> bicubic resize -> /255,
 * and the TTA ops of dataset/augment.py:115-120,142-146.
 * ------------------------------------------------------------------------------------------ */
typedef struct vip_jpeg_desc {
    int32_t width, height;            /* image size                                             */
    int32_t ncomp;                    /* 1 or 3                                                 */
    int32_t hsamp[3], vsamp[3];       /* sampling factors                                       */
    int32_t blocks_w[3], blocks_h[3]; /* coefficient-plane size in 8x8 blocks (padded to MCUs)  */
    int64_t coef_off[3];              /* offset (int16 elements) of each component's blocks     */
    uint16_t qt[3][64];               /* dequantisation tables, natural (row-major) order       */
    int32_t rgb_coded;                /* 3 components that ARE R,G,B (Adobe APP14 transform 0 / ids 'R','G','B',
                                         libjpeg jdapimin.c default_decompress_parms): no YCbCr->RGB conversion   */
} vip_jpeg_desc;

/* Host: parse headers only (fills the descriptor; coef_off relative to 0) and report how many int16
 * coefficients the image needs. */
int vip_jpeg_probe_h(const uint8_t* jpeg_h, size_t len, vip_jpeg_desc* desc_h, size_t* coef_elems_h);

/* Host, multithreaded: Huffman decode - sequential (ITU-T T.81 Annex F) and progressive (Annex G) - of n JPEG byte streams into
 * quantised DCT coefficients (natural order, int16, block-major per component) packed back to back in
 * coef_h; desc_h[i].coef_off are offsets into coef_h.  Replaces the entropy-decoding half of
 * tf.image.decode_jpeg (dataset/dataset.py:28).  Arithmetic / lossless / 12-bit / CMYK -> VIP_ERR_JPEG. */
int vip_jpeg_entropy_decode_h(const uint8_t* const* jpeg_h, const size_t* len_h, int n,
                              vip_jpeg_desc* desc_h, int16_t* coef_h, size_t coef_cap,
                              size_t* coef_used_h, int threads);

/* Device: dequantise + 8x8 ISLOW IDCT (libjpeg jidctint.c) into component planes (planes_ws: one byte per
 * coefficient, same offsets), then h2v1/h2v2/h1v2 "fancy" chroma upsampling (jdsample.c) + YCbCr->RGB
 * (jdcolor.c): the same uint8 pixels as libjpeg-turbo, the decoder inside tf.image.decode_jpeg.
 * coef/desc are DEVICE copies of what vip_jpeg_entropy_decode_h produced; max_blocks = the largest
 * per-image block count (all components); rgb_u8 [n][maxH][maxW][3] (pixels beyond an image's size are
 * left untouched). */
int vip_jpeg_idct_rgb_u8(const int16_t* coef, const vip_jpeg_desc* desc, int n, int max_blocks,
                         uint8_t* planes_ws, uint8_t* rgb_u8, int maxH, int maxW, void* stream);

/* ------------------------------------------------------------------------------------------
 * JPEG re-save (dataset/augment.py:110-113, JpegCompress -> tf.image.random_jpeg_quality: an encode -> decode round trip) without the
 * entropy coder, which is lossless: RGB -> quantised DCT coefficients in the layout above, which vip_jpeg_idct_rgb_u8 then turns into
 * the pixels the re-saved file would decode to.  The arithmetic is libjpeg's baseline compressor with its defaults (what
 * tf.image.encode_jpeg and Pillow run), all of it in integers, so coefficients and pixels are bit-exact against libjpeg-turbo.
 *
 * vip_jpeg_quality_tables_h (host): jpeg_set_quality(quality, force_baseline) of jcparam.c - scale = 5000 / q below 50, 200 - 2 q from
 *   50; entry = (base * scale + 50) / 100 clamped to 1..255 over the luminance / chrominance tables of ITU-T T.81 Annex K.
 *   luma_h, chroma_h: uint16 [64], natural (row-major) order.  quality outside 1..100 -> VIP_ERR_BAD_ARG.
 * vip_jpeg_encode_layout_h (host): the descriptor vip_jpeg_probe_h reads from a file written at this size, subsampling (420 or 444;
 *   anything else -> VIP_ERR_BAD_ARG) and quality: ncomp = 3, rgb_coded = 0, sampling 2x2,1x1,1x1 or 1x1 three times, blocks_* padded
 *   to whole MCUs, qt rows 0 / 1 / 2 = luma / chroma / chroma, coef_off relative to 0; *coef_elems_h = int16 coefficients the image
 *   needs.  A side outside 1..65535 or more than VIP_MAX_JPEG_PIXELS (environment, default 64 Mi) pixels -> VIP_ERR_BAD_ARG.
 * vip_jpeg_fdct_quant_u8 (device): rgb_u8 [n][maxH][maxW][3] (image i in the top-left height x width corner of its slot, the layout
 *   vip_jpeg_idct_rgb_u8 writes) -> YCbCr (jccolor.c: 16 fractional bits) -> 4:2:0 chroma by h2v2_downsample (jcsample.c: four-sample
 *   sum + bias 1, 2, 1, 2 along the row, >> 2) or none -> component planes in planes_ws (one byte per coefficient, same offsets) ->
 *   level shift, ISLOW forward DCT (jfdctint.c), quantisation (jcdctmgr.c: divisor 8 x table entry, magnitude rounded to nearest) ->
 *   coef (int16, natural order, block-major per component, at desc[i].coef_off).  Edges as libjpeg pads them: last column / row
 *   replicated out to whole blocks (for 4:2:0 chroma the columns before the downsampling, the rows after it); the blocks that only
 *   fill the last MCU column / row are jccoefct.c's dummy blocks (AC zero, DC of the block before them in the MCU).
 *   desc: DEVICE copy of n vip_jpeg_encode_layout_h descriptors with coef_off made absolute; max_blocks = the largest per-image block
 *   count (all components); planes_ws and coef hold the sum of the images' coefficient counts and are 16-byte aligned
 *   (VIP_ERR_ALIGNMENT otherwise).  An image whose descriptor is all zero is skipped.  No allocation, no atomics: bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
int vip_jpeg_quality_tables_h(int quality, uint16_t* luma_h, uint16_t* chroma_h);
int vip_jpeg_encode_layout_h(int width, int height, int subsampling, int quality, vip_jpeg_desc* desc_h, size_t* coef_elems_h);
int vip_jpeg_fdct_quant_u8(const uint8_t* rgb_u8, const vip_jpeg_desc* desc, int n, int max_blocks, uint8_t* planes_ws,
                           int16_t* coef, int maxH, int maxW, void* stream);

/* ------------------------------------------------------------------------------------------
 * Antialiased resampling of decoded u8 RGB to a new size: what an image editor or an upload does before it re-saves (the first half of
 * the challenge's "resized and then JPEG-compressed").  NOT the network-input resize below, which stays TensorFlow's non-antialiased
 * bicubic.  The operation is Pillow's 8-bit Image.resize, bit for bit: integer tables from the host, integer passes on the device.
 *
 * vip_resample_coeffs_h (host, double precision): the tables of ONE axis for in_size -> out_size samples and a filter
 *   (VIP_RESAMPLE_BILINEAR support 1, _BICUBIC Keys a = -0.5 support 2, _LANCZOS support 3).  scale = in / out, fscale = max(scale, 1),
 *   support = filter support * fscale, *ksize_h = 2 ceil(support) + 1.  Per output index x: center = (x + 0.5) scale,
 *   xmin = max(int(center - support + 0.5), 0), count = min(int(center + support + 0.5), in) - xmin,
 *   w_j = f((j + xmin - center + 0.5) * (1 / fscale)); the weights are summed left to right and divided by the sum when it is not 0;
 *   k = int(w * 2^22 +- 0.5), the sign of the 0.5 that of w; unused slots 0.
 *   bounds_h int32 [out][2] = (xmin, count), k_h int32 [out][ksize]; bounds_cap / k_cap = the buffers' sizes in int32.  With both
 *   buffers NULL only *ksize_h is written (a size query).  Sizes outside 1..2^20, an unknown filter, one buffer NULL or a buffer too
 *   short -> VIP_ERR_BAD_ARG with a message, before anything is written.
 * vip_resample_rgb_u8 (device, caller's stream, one launch per batch): src_u8 [n][maxH][maxW][3] with image i in the top-left
 *   src_sizes_hw[i] = (h, w) corner of its slot -> dst_u8 [n][maxHo][maxWo][3], image i at dst_sizes_hw[i] = (h', w').  Per channel:
 *   horizontal pass to u8 = clamp((2^21 + sum px * k) >> 22, 0, 255) with a 32-bit accumulator and an arithmetic shift, then the same
 *   formula vertically over the ROUNDED u8 rows; a pass whose sizes are equal is skipped.  Only the h' x w' pixels of an image are
 *   written: the rest of dst_u8 keeps what the caller put there.
 *   image_tab int32 [n][8]: first tile of the image (prefix sum over the batch), tiles per tile row, then horizontal and vertical
 *   (bounds offset, coefficient offset, ksize) into `tables`, the concatenated vip_resample_coeffs_h outputs (device copies; the
 *   offsets of a skipped pass are unused).  A tile is rows x bytes of vip_resample_tile_shape over the interleaved output row:
 *   tiles per row = ceil(3 w' / bytes), tile rows = ceil(h' / rows); total_tiles = their sum over the batch.
 *   A workgroup resamples the input rows its tile's vertical window needs horizontally into LDS and runs the vertical pass from there;
 *   a window taller than window_rows is worked through in groups of output rows inside the same launch, with the same arithmetic.
 *   max_window = the largest tap count of one output row over the batch (min(vertical ksize, h)); beyond window_rows (a shrink
 *   past ~25x) the call is refused with VIP_ERR_UNSUPPORTED - there is no two-launch fallback.  No allocation, no atomics:
 *   bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
enum { VIP_RESAMPLE_BILINEAR = 0, VIP_RESAMPLE_BICUBIC = 1, VIP_RESAMPLE_LANCZOS = 2 };
int vip_resample_coeffs_h(int in_size, int out_size, int filter, int32_t* bounds_h, size_t bounds_cap, int32_t* k_h, size_t k_cap,
                          int* ksize_h);
int vip_resample_tile_shape(int* rows_h, int* bytes_h, int* window_rows_h);
int vip_resample_rgb_u8(const uint8_t* src_u8, const int32_t* src_sizes_hw, int maxH, int maxW, uint8_t* dst_u8,
                        const int32_t* dst_sizes_hw, int maxHo, int maxWo, const int32_t* image_tab, const int32_t* tables, int n,
                        int total_tiles, int max_window, void* stream);

/* ------------------------------------------------------------------------------------------
 * Smoothing of decoded u8 RGB at the image's own size: a Gaussian blur and a K x K median, the two filters of dataset/augment.py:131-140
 * (`Blur`: tfa.image.gaussian_filter2d / median_filter2d) as stress perturbations.  Each image of the batch is filtered on its own and
 * each channel separately; the output has the size of the input.
 *
 * Edges are REFLECT without repeating the edge sample (tfa's default, scipy's mode='mirror').  Sample i of an axis of n samples:
 *   n == 1: 0;  otherwise p = 2 (n - 1), i = i mod p (non-negative), i = p - i if i >= n.
 *   The formula reflects repeatedly, so a side shorter than the radius needs no special case.
 *
 * vip_blur_weights_h (host, double precision, no FP contraction): the 2 radius + 1 integer weights of one axis, w_h[j + radius] for
 *   j = -radius..radius.  g[j] = exp(-j^2 / (2 sigma^2)), summed left to right and divided by the sum; w[j] = floor(g[j] * 65536 + 0.5);
 *   then the centre takes the rounding, w[0] += 65536 - sum(w): the weights are non-negative and sum to exactly 65536.
 *   cap = the buffer's size in int32.  sigma outside 0.3..5.0, radius outside 1..15 or a buffer shorter than 2 radius + 1
 *   -> VIP_ERR_BAD_ARG with a message, before anything is written.
 * vip_blur_gauss_rgb_u8 (device, caller's stream, one launch per batch): src_u8 [n][maxH][maxW][3] with image i in the top-left
 *   sizes_hw[i] = (h, w) corner of its slot -> dst_u8 [n][dstMaxH][dstMaxW][3], image i in the same corner of its slot (a pitch of its
 *   own, at least the image's size).  weights_d: a device copy of vip_blur_weights_h's output for `radius` (1..15).  Per channel, in
 *   UNSIGNED 32-bit integers:
 *     horizontal pass   t   = (sum_j w[j] * px[mirror(x + j)] + 128) >> 8              8.8 fixed point, <= 65280, held as u16
 *     vertical pass     out = min((sum_j w[j] * t[mirror(y + j)] + 2^23) >> 24, 255)   the sum is <= 65536 * 65280 + 2^23 < 2^32
 *   The intermediate is rounded once to 1 / 256 level and a weight is off by at most 2^-17: the result is within 0.75 level of the
 *   exact convolution and at most one level from its rounded value.  Only the h x w pixels of an image are written: the rest of dst_u8
 *   keeps what the caller put there.  An image larger than a source or destination slot is skipped.  src_u8 and dst_u8 overlapping
 *   -> VIP_ERR_BAD_ARG (the filter cannot run in place).
 *   A workgroup owns 16 rows x 256 bytes of the interleaved output row; it stages the tile and its halo once into LDS as u8, mirroring
 *   on the pixel index, runs the horizontal pass into a u16 LDS plane and the vertical pass from there (40 KiB of LDS at any radius).
 *   The grid is (tiles of a maxH x maxW image) x n; a tile outside its image returns at once.  No allocation, no atomics: bit-reproducible.
 * vip_median_rgb_u8: the same conventions; per channel the element of rank k * k / 2 (0-based) of the mirrored k x k window, exact.
 *   k = 3: sorted columns, then med3(max of the minima, median of the medians, min of the maxima); k = 5: a 99-exchange selection
 *   network; both on packed 16-bit min / max, no data-dependent control flow.  k not 3 or 5 -> VIP_ERR_BAD_ARG.
 * vip_sharpen_rgb_u8 (device, caller's stream, one launch per batch): an unsharp mask, the sharpening a platform adds after a downscale;
 *   the conventions, argument checks and weights of vip_blur_gauss_rgb_u8.  Integers only, per byte of the interleaved RGB image, each
 *   image of the batch on its own:
 *     B   = vip_blur_gauss_rgb_u8's u8 result for (weights_d, radius), bit for bit
 *     d   = X - B                                            (-255..255)
 *     out = X                                                if |d| <= threshold
 *     out = clamp(X + ((amount_q8 * d + 128) >> 8), 0, 255)  otherwise; >> is an arithmetic shift (floor)
 *   amount_q8 = round(256 * P / 100) for a gain of P percent, 1..1280 (P = 1..500 gives 3..1280); threshold 0..255; either outside its
 *   range -> VIP_ERR_BAD_ARG.  Because |amount_q8 / 256 - P / 100| <= 1 / 512 and |d| <= 255, the result is at most one level from
 *   round(X + P / 100 * (X - B)) clamped.  The Gaussian's kernel with one more epilogue: the vertical pass takes the centre bytes from the
 *   staged u8 tile, so B never reaches global memory; amount_q8 and threshold travel as kernel arguments.  No extra LDS, no atomics, no
 *   allocation: bit-reproducible.  (Pillow's UnsharpMask blurs with a box approximation of the Gaussian: close, not a bit-exact yardstick.)
 * ------------------------------------------------------------------------------------------ */
int vip_blur_weights_h(double sigma, int radius, int32_t* w_h, size_t cap);
int vip_blur_gauss_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH, int dstMaxW,
                          const int32_t* weights_d, int radius, int n, void* stream);
int vip_median_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH, int dstMaxW, int k,
                      int n, void* stream);
int vip_sharpen_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH, int dstMaxW,
                       const int32_t* weights_d, int radius, int amount_q8, int threshold, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Geometry of decoded u8 RGB: an inverse affine warp with bilinear taps in integer arithmetic, the one kernel under the flip, crop and
 * rotate stress perturbations (dataset/augment.py:115-120 `RandomFlip`, :68-107 `ShiftScaleShearRotate` through tfa.image.rotate /
 * transform).  Each image of the batch has its own transform and its own output size.
 *
 * vip_warp_affine_rgb_u8 (device, caller's stream, one launch per batch): src_u8 [n][maxH][maxW][3] with image i in the top-left
 *   sizes_hw[i] = (h, w) corner of its slot -> dst_u8 [n][dstMaxH][dstMaxW][3], image i in the top-left dst_sizes_hw[i] = (h', w')
 *   corner of its slot.  xform_d: int64 [n][6] on the device, (A, B, TX, C, D, TY) per image: A..D the coefficients of the INVERSE map
 *   (output -> source) in Q24, TX, TY its offsets in Q25, in pixel-edge coordinates (pixel x covers [x, x + 1)).  For output pixel
 *   (x, y), with u = 2 x + 1 and v = 2 y + 1, in int64 throughout:
 *     SX = A u + B v + TX - 2^24,  SY = C u + D v + TY - 2^24       the source sample-centre coordinate in Q25
 *     ix = SX >> 25 (arithmetic shift),  wx = (SX >> 15) & 1023      and the same for y
 *     per channel  top = p[iy][ix] (1024 - wx) + p[iy][ix + 1] wx,  bot likewise on row iy + 1
 *                  out = (top (1024 - wy) + bot wy + 2^19) >> 20
 *   Taps by `fill`: VIP_WARP_FILL_BLACK - a tap outside the source image is 0 (tfa's `constant`, the reference's CFG.fill_mode);
 *   VIP_WARP_FILL_MIRROR - reflect without repeating the edge sample (the formula of the smoothing filters above; every tap of a
 *   1-pixel axis is index 0).  With A = D = +-2^24, B = C = 0 and whole-pixel offsets both weights are 0: flips and crops are exact
 *   copies.  Otherwise the result is within 0.5 (rounding) + 2 * 255 / 1024 (the truncated 10-bit weights) + about 0.02 (coefficient
 *   rounding at sides up to 200) < 1.02 levels of the exact bilinear value; 16-bit coefficients with 8-bit weights were off by 2.
 *   Only the h' x w' pixels of an image are written: the rest of dst_u8 keeps what the caller put there.  An image whose source or
 *   output size is not positive or exceeds its slot is skipped.  Null pointer, n or a slot side not positive, fill not 0 or 1, src_u8
 *   and dst_u8 overlapping -> VIP_ERR_BAD_ARG; sizes not 4-byte or xform_d not 8-byte aligned -> VIP_ERR_ALIGNMENT; all before any work.
 *   A workgroup owns 64 pixels x 16 rows of the output - a compact tile, so that the source footprint of a rotated tile stays in the
 *   CU's cache - with one wave per output row; results pass through an LDS image of the tile and leave as whole dwords.  The grid is
 *   (tiles of a dstMaxH x dstMaxW image) x n; a tile outside its image returns at once.  No allocation, no atomics: bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
#define VIP_WARP_FILL_BLACK 0
#define VIP_WARP_FILL_MIRROR 1
int vip_warp_affine_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, const int32_t* dst_sizes_hw,
                           int dstMaxH, int dstMaxW, const int64_t* xform_d, int fill, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Colour of decoded u8 RGB: a 3 x 3 matrix, a per-image mean term, an offset and a look-up table in integer arithmetic, the one kernel
 * under the gray, BGR, hue, saturation, contrast, brightness and gamma stress perturbations (dataset/augment.py:142-146 `RandomGray`,
 * :148-151 `RandomBGR`, :122-129 `RandomJitter`).  Every image keeps its size.
 *
 * vip_colour_rgb_u8 (device, caller's stream, one launch per batch): src_u8 [n][maxH][maxW][3] with image i in the top-left
 *   sizes_hw[i] = (h, w) corner of its slot -> dst_u8 [n][dstMaxH][dstMaxW][3], image i in the same corner of its slot (a pitch of its
 *   own).  coef_h: int32 [15] on the HOST, M[3][3] (row c = output channel c), K[3], O[3], all Q16; they are copied into the kernel's
 *   arguments, so a variant costs no host-to-device copy and no synchronisation.  mean_u8: uint8 [n][4] on the device, (r, g, b, 0)
 *   per image as vip_image_mean_u8 writes it, or NULL when every K is 0.  lut_d: uint8 [256] on the device, or NULL.  Per pixel
 *   (R, G, B) of image i and output channel c, in signed 32-bit integers:
 *     s_c   = M[c][0] R + M[c][1] G + M[c][2] B + K[c] mean_u8[i][c] + O[c] + 32768
 *     v_c   = clamp(s_c >> 16, 0, 255)          arithmetic shift: floor, also for a negative sum
 *     out_c = lut_d ? lut_d[v_c] : v_c
 *   Admitted: |M[c][k]| <= 2^18 and |K[c]| <= 2^18 (4.0 in Q16), |O[c]| <= 2^25 (512 levels).  With samples and means of at most 255
 *   |s_c| <= 3 * 255 * 2^18 + 255 * 2^18 + 2^25 + 2^15 = (1020 + 128) * 2^18 + 2^15 = 300 974 080 < 2^31: no sum leaves 32 bits.
 *   Only the h x w pixels of an image are written: the rest of dst_u8 keeps what the caller put there, and nothing but the images'
 *   pixels is read.  An image whose size is not positive or exceeds the source or the destination slot is skipped.  Null src_u8,
 *   sizes_hw, dst_u8 or coef_h, n or a slot side not positive, src_u8 and dst_u8 overlapping, a coefficient outside the bounds above,
 *   mean_u8 == NULL while some K[c] != 0 -> VIP_ERR_BAD_ARG; sizes_hw or mean_u8 not 4-byte aligned -> VIP_ERR_ALIGNMENT; all before
 *   any work.
 *   A workgroup owns 128 pixels x 8 rows.  A slot row starts at (i maxH + y) maxW 3 bytes, dword-aligned only by accident, and the two
 *   pitches differ, so a tile row is fetched as the aligned dwords of the source that cover it into an LDS image that keeps the row's
 *   phase, a lane converts one pixel from there into a second LDS image at the destination row's phase, and that image leaves as the
 *   aligned dwords of the destination; the head and the tail of a row, where a dword also holds a neighbour's bytes, move byte by
 *   byte.  lut_d is copied into LDS once per workgroup.  The grid is (tiles of the smaller slot) x n; a tile outside its image
 *   returns at once.  No allocation, no atomics: bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
int vip_colour_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH, int dstMaxW,
                      const int32_t* coef_h, const uint8_t* mean_u8, const uint8_t* lut_d, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Noise on decoded u8 RGB: additive Gaussian (per channel, or one sample on all three channels), multiplicative speckle and
 * salt-and-pepper impulses, in integer arithmetic from a counter-based generator - the one kernel under the noise stress perturbations.
 * dataset/augment.py has no noise augmentation; this goes beyond the reference.  Every image keeps its size.
 *
 * vip_noise_rgb_u8 (device, caller's stream, one launch per batch): src_u8 [n][maxH][maxW][3] with image i in the top-left
 *   sizes_hw[i] = (h, w) corner of its slot -> dst_u8 [n][dstMaxH][dstMaxW][3], image i in the same corner of its slot (a pitch of its
 *   own); the two must not overlap.  mode 0 gaussian, 1 mono, 2 speckle, 3 impulse; amount: the integer a (modes 0..2) or thr (mode 3)
 *   below; seed: one word for the run; keys_u32: uint32 [n] on the device, one word per image (the tools use zlib's crc32 of the file's
 *   basename); table_i32: int32 [4097] on the device, the table T below (NULL is admitted in mode 3, which reads none).
 *   Random words.  Philox4x32-10: multipliers 0xD2511F53 and 0xCD9E8D57, Weyl constants 0x9E3779B9 and 0xBB67AE85, ten rounds, the key
 *   bumped between rounds.  Pixel (x, y) of image i, IN THE IMAGE'S OWN COORDINATES, has the counter (x, y, 0, 0) and the key
 *   (seed, keys_u32[i]); the four output words are w0..w3.  The field depends on seed, key and pixel position only - not on mode,
 *   amount, batch index, slot pitch or batch size: two amounts see the same field at two gains, and an image keeps its noise wherever
 *   it sits in whatever batch.
 *   Standard normal, Q12.  T[i] = round(4096 Phi^-1(i / 4096)) for 0 < i < 4096, T[0] = -16384, T[4096] = 16384, built by the caller in
 *   float64 (odd-symmetric, increasing, largest step 2101), and
 *     z(w) = T[w >> 20] + (((T[(w >> 20) + 1] - T[w >> 20]) * ((w >> 5) & 0x7FFF) + 16384) >> 15)
 *   the inverse CDF, linear inside each of the 4096 bins and cut at +-4 (std of the law 1.000034, kurtosis 2.9998); the product is
 *   below 2101 * 32767 + 16384 < 2^27.
 *   Modes.  Signed 32-bit integers, arithmetic shifts (floor, also for a negative sum), X the input sample:
 *     0 gaussian  out_c = clamp(X_c + ((a z(w_c) + 2^19) >> 20), 0, 255), c = 0, 1, 2
 *                 a = round(256 sigma), sigma 0.5..50.0 levels in steps of 0.1: 128 <= a <= 12800; |a z| <= 12800 * 16384 < 2^28
 *     1 mono      mode 0 with z(w0) on all three channels (luminance noise); a as in mode 0
 *     2 speckle   out_c = clamp(X_c + ((X_c a z(w_c) + 2^19) >> 20), 0, 255)
 *                 a = round(256 P / 100), P = 1..50 percent: 3 <= a <= 128; |X a z| <= 255 * 128 * 16384 < 2^29
 *     3 impulse   if w3 < thr (unsigned) all three channels become (w2 & 1) ? 255 : 0, otherwise the pixel is copied
 *                 thr = round(P / 100 * 2^32), P = 0.1..50.0 percent in steps of 0.1: 4294967 <= thr <= 2^31
 *   No sum leaves 32 bits.
 *   Only the h x w pixels of an image are written: the rest of dst_u8 keeps what the caller put there, and nothing but the images'
 *   pixels is read.  An image whose size is not positive or exceeds the source or the destination slot is skipped.  Null src_u8,
 *   sizes_hw, dst_u8 or keys_u32, null table_i32 in modes 0..2, n or a slot side not positive, src_u8 and dst_u8 overlapping, a mode
 *   outside 0..3, an amount outside its mode's range -> VIP_ERR_BAD_ARG; sizes_hw, keys_u32 or table_i32 not 4-byte aligned ->
 *   VIP_ERR_ALIGNMENT; all before any work: a refused call launches nothing.
 *   A workgroup owns 128 pixels x 8 rows and moves them as vip_colour_rgb_u8 does: aligned dwords of the source into an LDS image that
 *   keeps each row's byte phase, one pixel per lane into a second LDS image at the destination row's phase, aligned dwords out; heads
 *   and tails of rows byte by byte.  T is either gathered from global memory through the vector L1, one tile per workgroup, or copied
 *   into LDS by a workgroup that then loops over 8 consecutive tiles; vip_noise_rgb_u8 uses the gathers, which measured faster
 *   (README.md).  Mode 3 reads no table and copies none.  No allocation, no atomics: bit-reproducible.
 * vip_noise_rgb_u8_placed: the same with the table's placement chosen by the caller (0: global gathers, 1: the LDS copy; anything
 *   else -> VIP_ERR_BAD_ARG), for the benchmark (tools/bench_noise.py) and the tests; both placements write the same bytes.
 * ------------------------------------------------------------------------------------------ */
int vip_noise_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH, int dstMaxW,
                     int mode, int64_t amount, uint32_t seed, const uint32_t* keys_u32, const int32_t* table_i32, int n, void* stream);
int vip_noise_rgb_u8_placed(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH, int dstMaxW,
                            int mode, int64_t amount, uint32_t seed, const uint32_t* keys_u32, const int32_t* table_i32, int placement,
                            int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tone of decoded u8 RGB: curves MEASURED from the picture's histogram - auto-contrast, equalisation and contrast-limited adaptive
 * equalisation (CLAHE) - the kernels under the tone stress perturbations.  dataset/augment.py has nothing of the kind; this goes beyond
 * the reference.  Every image keeps its size.  A variant is three launches on the caller's stream, without a host round trip:
 * vip_tone_hist_u8 -> vip_tone_lut_u8 -> vip_tone_apply_rgb_u8.  All arithmetic is integer except the one float64 expression below.
 *
 * Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Pillow's convert("L").
 * Modes: VIP_TONE_AC 0 (auto-contrast per channel), VIP_TONE_ACL 1 (auto-contrast, one table from Y on all three channels),
 *   VIP_TONE_EQ 2 (equalisation per channel), VIP_TONE_CLAHE 3.  Histogram channels C: 3 in modes 0 and 2 (R, G, B), 1 in modes 1 and
 *   3 (Y).  Parameter: the cutoff C% in 0..49 (modes 0, 1), 0 (mode 2), TT = ten times the clip limit in 10..99 (mode 3).
 * Grid (per axis of `side` pixels, G = grid in 1..16): g = min(G, max(1, side / 16)); tile k covers [b[k], b[k + 1]) with b[k] =
 *   (k side) / g; every tile is at least 16 pixels wide unless g = 1.  Tile (ky, kx) of an image with gy x gx tiles is slot
 *   ky gx + kx of that image.
 *
 * vip_tone_hist_u8: src_u8 [n][maxH][maxW][3], sizes_hw[i] = (h, w) -> hist_i32 int32 [n][slots][channels][256], per image and tile
 *   the histogram of its pixels' R, G and B (channels = 3) or Y (channels = 1).  EVERY slot is written, one without a tile (slot >= gy
 *   gx; an image whose size is not positive or exceeds the slot, or whose gy gx exceeds `slots`) with zeros: the buffer need not be
 *   cleared, and the sum over an image's slots is the histogram of the whole image whatever `grid` is.  Nothing but the images' pixels
 *   is read.  One workgroup per slot, LDS atomics on integer counts: the result does not depend on the order.
 * vip_tone_lut_u8: hist_i32 [n][slots][C][256] (C by mode) -> lut_u8 uint8 [n][C][256] (modes 0..2, from the SUM h of the image's
 *   slots) or [n][slots][256] (mode 3, one table per slot).  One workgroup per table.  With N = sum h:
 *   modes 0, 1   cut = (N * cutoff) / 100 in 64 bits; lo = the smallest i with sum(h[0..i]) > cut, hi = the largest i with
 *                sum(h[i..255]) > cut; hi <= lo (or N = 0): lut[i] = i; otherwise
 *                  lut[i] = clamp(trunc(i * scale + offset), 0, 255), scale = 255.0 / (hi - lo), offset = -lo * scale
 *                in IEEE float64, the division, the two products and the sum each rounded to nearest on its own (no fused
 *                multiply-add), trunc towards zero: Pillow's ImageOps.autocontrast(cutoff) bit for bit.
 *   mode 2       fewer than two non-zero bins: lut[i] = i; otherwise step = (N - (the last non-zero bin)) / 255; step = 0: lut[i] =
 *                i; otherwise lut[i] = min((step / 2 + sum(h[0..i-1])) / step, 255): Pillow's ImageOps.equalize bit for bit.
 *   mode 3       A = N (the tile's area; A = 0: lut[i] = i), clip = max(1, (TT * A) / 2560) in 64 bits, h'[i] = min(h[i], clip),
 *                E = A - sum h', h''[i] = h'[i] + E / 256 + [(i (E % 256)) / 256 != ((i + 1) (E % 256)) / 256]  (sum h'' = A),
 *                T[i] = (sum(h''[0..i]) * 255 + A / 2) / A in 64 bits.
 * vip_tone_apply_rgb_u8: src_u8 -> dst_u8 [n][dstMaxH][dstMaxW][3] (a pitch of its own; the two must not overlap) through lut_u8 as
 *   vip_tone_lut_u8 wrote it for `mode`.  Modes 0, 2: out_c = lut[i][c][X_c]; mode 1: out_c = lut[i][0][X_c].  Mode 3, per axis with
 *   pixel x, X2 = 2 x + 1 and c2[k] = b[k] + b[k + 1]: X2 < c2[0] -> both neighbours tile 0; X2 >= c2[g - 1] -> both g - 1; otherwise k
 *   with c2[k] <= X2 < c2[k + 1], neighbours k and k + 1, wq = ((X2 - c2[k]) << 8) / (c2[k + 1] - c2[k]) in 0..255; then
 *     V     = ((256 - wyq) ((256 - wxq) T00[Y] + wxq T01[Y]) + wyq ((256 - wxq) T10[Y] + wxq T11[Y]) + 32768) >> 16
 *     out_c = clamp(X_c + V - Y, 0, 255)
 *   (CLAHE of the Y of YCbCr with the chroma kept).  `grid` and `slots` are those of the histogram call (read in mode 3 only; an image
 *   whose gy gx exceeds `slots` is skipped).  Only the h x w pixels of an image are written and nothing but the images' pixels is read;
 *   an image whose size is not positive or exceeds the source or the destination slot is skipped.  A workgroup owns 128 pixels x 8 rows
 *   and moves them as vip_colour_rgb_u8 does.  The image's table(s) are copied into LDS; in mode 3 the four tile tables are gathered
 *   from global memory through the vector L1 (README.md has the measurement against an LDS copy).
 * vip_tone_apply_rgb_u8_placed: the same with the placement of mode 3's tables chosen by the caller (0: global gathers, 1: the at
 *   most 3 x 10 tables a workgroup's pixels touch copied into LDS), for tools/bench_tone.py and the tests; both write the same bytes.
 * All three: a null pointer, n or a slot side not positive or above 2^26, a mode, parameter, grid (1..16), channels, placement or
 *   slots (1..256) out of range, src_u8 and dst_u8 overlapping -> VIP_ERR_BAD_ARG; sizes_hw, hist_i32 or lut_u8 not 4-byte aligned ->
 *   VIP_ERR_ALIGNMENT; all before any work: a refused call launches nothing.  No allocation, no global atomics: bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
enum { VIP_TONE_AC = 0, VIP_TONE_ACL = 1, VIP_TONE_EQ = 2, VIP_TONE_CLAHE = 3 };
int vip_tone_hist_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int n, int maxH, int maxW, int grid, int channels, int32_t* hist_i32,
                     int slots, void* stream);
int vip_tone_lut_u8(const int32_t* hist_i32, int n, int slots, int mode, int param, uint8_t* lut_u8, void* stream);
int vip_tone_apply_rgb_u8(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH, int dstMaxW,
                          const uint8_t* lut_u8, int mode, int grid, int slots, int n, void* stream);
int vip_tone_apply_rgb_u8_placed(const uint8_t* src_u8, const int32_t* sizes_hw, int maxH, int maxW, uint8_t* dst_u8, int dstMaxH, int dstMaxW,
                                 const uint8_t* lut_u8, int mode, int grid, int slots, int placement, int n, void* stream);

/* PNG (dataset/dataset.py:22-30, build_decoder(ext='png') -> tf.image.decode_png(channels=3)): the host inflates, the
 * GPU undoes the scanline filters and expands to 8-bit RGB.  Same output as vip_jpeg_idct_rgb_u8. */
typedef struct vip_png_desc {
    int32_t width, height;            /* image size                                                      */
    int32_t bit_depth;                /* 1, 2, 4, 8 or 16                                                */
    int32_t color_type;               /* 0 gray, 2 RGB, 3 palette, 4 gray+alpha, 6 RGBA                  */
    int32_t interlace;                /* 0 none, 1 Adam7                                                 */
    int32_t channels;                 /* samples per pixel (1, 3, 1, 2, 4)                               */
    int32_t bpp;                      /* filter distance in bytes: max(1, channels * bit_depth / 8)      */
    int32_t palette_size;             /* PLTE entries (0 when the image has no palette)                  */
    int64_t stream_off;               /* byte offset of the image's filtered scanlines in the batch buffer */
    int64_t pass_off[7];              /* offset of each pass relative to stream_off (pass 0 only when not
                                         interlaced; an empty Adam7 pass has no bytes)                   */
    int32_t pass_w[7], pass_h[7];     /* pixels per row / rows of each pass (0 = empty or absent pass)   */
    uint8_t palette[256][3];          /* PLTE entries as RGB, unused entries zero                         */
} vip_png_desc;

/* Host: walk the chunks (signature, critical-chunk CRCs are checked by vip_png_inflate_h), validate IHDR and fill the
 * descriptor (stream_off = 0); *stream_bytes_h = the size of the filtered scanline stream, (1 + rowbytes) per row of every
 * pass.  The per-image pixel cap VIP_MAX_JPEG_PIXELS (environment, default 64 Mi) applies: larger -> VIP_ERR_PNG. */
int vip_png_probe_h(const uint8_t* png_h, size_t len, vip_png_desc* desc_h, size_t* stream_bytes_h);

/* Host, multithreaded: check critical-chunk CRCs, inflate (RFC 1950/1951) the concatenated IDAT data of n PNG byte streams
 * and pack the still-filtered scanlines back to back in stream_h; desc_h[i].stream_off are offsets into stream_h.  Filter
 * types are validated (0..4).  Replaces the zlib half of tf.image.decode_png (dataset/dataset.py:30). */
int vip_png_inflate_h(const uint8_t* const* png_h, const size_t* len_h, int n, vip_png_desc* desc_h, uint8_t* stream_h,
                      size_t stream_cap, size_t* stream_used_h, int threads);

/* Device: undo the scanline filters (None, Sub, Up, Average, Paeth) IN PLACE in `filtered` (a device copy of what
 * vip_png_inflate_h produced) and expand to 8-bit RGB like libpng for channels=3: gray 1/2/4 bits by bit replication,
 * palette by PLTE lookup (an index past the palette is black), alpha dropped, 16-bit samples reduced to round(v / 257)
 * (png_set_scale_16).  Adam7 passes are scattered to their pixel positions.  rgb_u8 [n][maxH][maxW][3]; pixels beyond an
 * image's size are left untouched. */
int vip_png_unfilter_rgb_u8(uint8_t* filtered, const vip_png_desc* desc, int n, uint8_t* rgb_u8, int maxH, int maxW,
                            void* stream);

/* Lossless WebP (RIFF container, VP8L bitstream): the host decodes everything that is serial (prefix codes, LZ77, colour
 * cache, the transforms' sub-images), the GPU undoes the transforms and writes 8-bit RGB.  Same output as
 * vip_jpeg_idct_rgb_u8.  Lossy (VP8) and animated files are refused. */
#define VIP_WEBP_PREDICTOR 0
#define VIP_WEBP_CROSS_COLOR 1
#define VIP_WEBP_SUBTRACT_GREEN 2
#define VIP_WEBP_COLOR_INDEXING 3
/* vip_webp_desc.stats: what the host decoder met in the stream (coverage word for the tests) */
#define VIP_WEBP_STAT_CACHE 1         /* a colour cache was used                    */
#define VIP_WEBP_STAT_META 2          /* a meta prefix image was used               */
#define VIP_WEBP_STAT_SIMPLE 4        /* a simple prefix code was read              */
#define VIP_WEBP_STAT_MAX_SYMBOL 8    /* a normal code with max_symbol was read     */
#define VIP_WEBP_STAT_REP16 16        /* code-length repeat codes 16, 17, 18        */
#define VIP_WEBP_STAT_REP17 32
#define VIP_WEBP_STAT_REP18 64
#define VIP_WEBP_STAT_PLANE 128       /* a backward reference with a plane code (<= 120) */
#define VIP_WEBP_STAT_LINEAR 256      /* a backward reference with a linear distance     */
typedef struct vip_webp_desc {
    int32_t width, height;            /* image size                                                          */
    int32_t has_alpha;                /* the header's alpha hint (alpha is dropped either way)               */
    int32_t coded_width;              /* width of the entropy-coded main image: < width when colour indexing
                                         bundles 2, 4 or 8 pixels per coded pixel                            */
    int32_t n_transforms;             /* 0..4                                                                */
    int32_t stats;                    /* VIP_WEBP_STAT_* bits, filled by vip_webp_entropy_h                  */
    int32_t type[4];                  /* per transform, in the order read: VIP_WEBP_*                        */
    int32_t bits[4];                  /* block size bits (predictor, cross-colour) / pixel bundling bits     */
    int32_t xsize[4];                 /* the image width the transform works at                              */
    int64_t stream_off;               /* byte offset of the image's words in the batch buffer                */
    int64_t data_off[4];              /* sub-image / 256-entry table of the transform, relative to stream_off */
    int64_t argb_off;                 /* the main image's 32-bit ARGB words, relative to stream_off; width * height
                                         words are reserved (coded_width * height are written by the host)   */
} vip_webp_desc;

/* Host: walk the RIFF container (VP8L, or VP8X followed by VP8L), read the VP8L header and fill width, height and
 * has_alpha (everything else zero); *stream_bytes_h = an upper bound of the image's share of the batch buffer:
 * width * height words for the main image, ceil(w/4) * ceil(h/4) words for each of a predictor and a cross-colour
 * sub-image, 256 words of palette.  VIP_MAX_JPEG_PIXELS applies as for PNG: larger -> VIP_ERR_WEBP. */
int vip_webp_probe_h(const uint8_t* webp_h, size_t len, vip_webp_desc* desc_h, size_t* stream_bytes_h);

/* Host, multithreaded: decode the VP8L streams of n WebP files - transform headers and their sub-images, colour cache,
 * meta prefix image, prefix codes, LZ77 - and write per image the still-transformed ARGB words and the transforms' data
 * back to back in stream_h (each image takes its probe bound); the palette is delta-decoded and zero-padded to 256
 * entries.  No transform is undone.  Errors name the image ("webp image K: ..."). */
int vip_webp_entropy_h(const uint8_t* const* webp_h, const size_t* len_h, int n, vip_webp_desc* desc_h, uint8_t* stream_h,
                       size_t stream_cap, size_t* stream_used_h, int threads);

/* Device: undo the transforms in the reverse of the order read, IN PLACE in `words` (a device copy of what
 * vip_webp_entropy_h produced), drop alpha and write rgb_u8 [n][maxH][maxW][3]; pixels beyond an image's size are left
 * untouched and an all-zero descriptor writes nothing.  A palette index past the table is transparent black. */
int vip_webp_inverse_rgb_u8(uint8_t* words, const vip_webp_desc* desc, int n, uint8_t* rgb_u8, int maxH, int maxW,
                            void* stream);

/* Lossy WebP (RIFF container, a VP8 key frame, RFC 6386): the host reads everything the boolean decoder carries - frame
 * header, per-macroblock modes, residual tokens - and dequantises; the GPU predicts, adds the residuals, runs the in-loop
 * filter, upsamples the chroma planes ("fancy" 9-3-3-1) and converts to 8-bit RGB: libwebp's decoder, bit for bit.  Alpha
 * (an ALPH chunk) is dropped.  Opt-in: vip_webp_probe_h / vip_webp_entropy_h keep refusing a `VP8 ` chunk. */
/* vip_vp8_desc.stats: what the host decoder met in the stream (coverage word for the tests) */
#define VIP_VP8_STAT_SEGMENTS (1ll << 0)        /* segmentation enabled                                   */
#define VIP_VP8_STAT_MAP_UPDATE (1ll << 1)      /* a segment map was read                                 */
#define VIP_VP8_STAT_SEG_DELTA (1ll << 2)       /* segment data in delta mode                             */
#define VIP_VP8_STAT_SIMPLE_FILTER (1ll << 3)
#define VIP_VP8_STAT_NORMAL_FILTER (1ll << 4)
#define VIP_VP8_STAT_SHARPNESS (1ll << 5)       /* sharpness > 0 with a filter on                         */
#define VIP_VP8_STAT_LEVEL0_MB (1ll << 6)       /* a macroblock at filter level 0 in a filtered frame     */
#define VIP_VP8_STAT_LF_DELTA (1ll << 7)        /* loop-filter deltas enabled                             */
#define VIP_VP8_STAT_PARTS2 (1ll << 8)          /* 2, 4, 8 token partitions                               */
#define VIP_VP8_STAT_PARTS4 (1ll << 9)
#define VIP_VP8_STAT_PARTS8 (1ll << 10)
#define VIP_VP8_STAT_BPRED (1ll << 11)          /* a macroblock with 16 sub-block modes                   */
#define VIP_VP8_STAT_BMODE0 (1ll << 12)         /* .. << 21: one bit per sub-block mode (VIP_VP8_B_*)     */
#define VIP_VP8_STAT_YMODE0 (1ll << 22)         /* .. << 25: one bit per 16x16 mode (DC, TM, V, H)        */
#define VIP_VP8_STAT_UVMODE0 (1ll << 26)        /* .. << 29: one bit per chroma mode (DC, TM, V, H)       */
#define VIP_VP8_STAT_SKIP (1ll << 30)           /* a macroblock with its skip flag set                    */
#define VIP_VP8_STAT_PROBA_UPDATE (1ll << 31)   /* a coefficient probability update was read              */
#define VIP_VP8_STAT_CAT6 (1ll << 32)           /* a token of the largest category                        */
#define VIP_VP8_STAT_Y2_AC (1ll << 33)          /* a Y2 block with more than its DC                       */
#define VIP_VP8_STAT_DC_ONLY (1ll << 34)        /* a coded block with only its DC                         */
#define VIP_VP8_STAT_FULL_BLOCK (1ll << 35)     /* a coded block with AC coefficients                     */
#define VIP_VP8_STAT_ALL ((1ll << 36) - 1)
/* modes, in libwebp's numbering; DC, TM, V, H double as the 16x16 and chroma modes */
#define VIP_VP8_B_DC 0
#define VIP_VP8_B_TM 1
#define VIP_VP8_B_VE 2
#define VIP_VP8_B_HE 3
#define VIP_VP8_B_RD 4
#define VIP_VP8_B_VR 5
#define VIP_VP8_B_LD 6
#define VIP_VP8_B_VL 7
#define VIP_VP8_B_HD 8
#define VIP_VP8_B_HU 9
#define VIP_VP8_B_PRED 4                        /* vip_vp8_mb.ymode of a macroblock with sub-block modes   */
/* one macroblock, everything resolved on the host.  Coded blocks are numbered Y 0..15 (raster), U 16..19, V 20..23,
 * Y2 24; their 16 dequantised int16 coefficients (raster order) lie back to back, in that order, from block coef_idx of
 * the image's coefficient area.  A luma block of a 16x16-predicted macroblock takes its DC from the inverse WHT of Y2
 * (when Y2 is coded) and its stored [0] is 0. */
typedef struct vip_vp8_mb {
    uint8_t ymode;                    /* VIP_VP8_B_DC / TM / VE / HE for 16x16 prediction, VIP_VP8_B_PRED             */
    uint8_t uvmode;                   /* VIP_VP8_B_DC / TM / VE / HE                                                  */
    uint8_t flevel;                   /* loop filter level 0..63, 0 = not filtered                                    */
    uint8_t ilevel;                   /* interior limit                                                               */
    uint8_t hev;                      /* high edge variance threshold                                                 */
    uint8_t inner;                    /* 1: the inner edges are filtered too                                          */
    uint8_t segment, skip;            /* as read (not used by the device)                                             */
    uint8_t bmodes[16];               /* sub-block modes of a VIP_VP8_B_PRED macroblock                               */
    uint32_t nz;                      /* bit b: block b is coded (25 bits)                                            */
    uint32_t dc_only;                 /* bit b: only [0] of coded block b is non-zero                                 */
    uint32_t coef_idx;                /* first coded block of the macroblock, in blocks of 16 coefficients            */
    uint32_t reserved;
} vip_vp8_mb;
typedef struct vip_vp8_desc {
    int32_t width, height;            /* image size                                                                   */
    int32_t mb_w, mb_h;               /* in macroblocks                                                               */
    int32_t has_alpha;                /* the VP8X alpha flag (alpha is dropped either way)                            */
    int32_t filter_type;              /* 0 none, 1 simple, 2 normal                                                   */
    int64_t stats;                    /* VIP_VP8_STAT_* bits, filled by vip_vp8_entropy_h                             */
    int64_t stream_off;               /* byte offset of the image's data in the batch buffer (8-byte aligned)         */
    int64_t mb_off;                   /* mb_w * mb_h vip_vp8_mb records, relative to stream_off                       */
    int64_t coef_off;                 /* the coded blocks' int16 coefficients, relative to stream_off                 */
    int64_t coef_blocks;              /* how many blocks of 16 coefficients                                           */
    int64_t plane_off;                /* byte offset of the image's Y / U / V planes in the device scratch buffer:
                                         mb_w * mb_h * 384 bytes, Y [16 mb_h][16 mb_w] then U and V [8 mb_h][8 mb_w]  */
} vip_vp8_desc;

/* Host: walk the RIFF container (a `VP8 ` chunk, alone or behind VP8X; ALPH, ICCP, EXIF, XMP and unknown chunks are
 * skipped), read the frame tag and the key-frame start code and fill width, height, mb_w, mb_h and has_alpha (everything
 * else zero); *stream_bytes_h = an upper bound of the image's share of the batch buffer (every block of every macroblock
 * coded).  Refused with VIP_ERR_WEBP: animation, an inter frame, a frame not shown, profile > 3, a first partition past
 * the chunk, a VP8X canvas that differs from the frame, zero sizes, sizes beyond VIP_MAX_JPEG_PIXELS; a VP8L file too
 * (that is vip_webp_probe_h's). */
int vip_vp8_probe_h(const uint8_t* webp_h, size_t len, vip_vp8_desc* desc_h, size_t* stream_bytes_h);

/* Host, multithreaded (images over up to `threads` workers): decode the frame header, the macroblock modes and the
 * residual tokens of n lossy WebP files, dequantise as libwebp does, and write per image the macroblock records and the
 * coded blocks' coefficients back to back in stream_h (8-byte aligned; only what is used: *stream_used_h <= the sum of
 * the probe bounds, and the same bytes whatever `threads` is).  plane_off is filled for a scratch buffer that holds the
 * batch's planes back to back (vip_vp8_scratch_bytes).  Errors name the image ("webp image K: ..."). */
int vip_vp8_entropy_h(const uint8_t* const* webp_h, const size_t* len_h, int n, vip_vp8_desc* desc_h, uint8_t* stream_h,
                      size_t stream_cap, size_t* stream_used_h, int threads);

/* Host: *bytes_h = the size of the device scratch buffer the descriptors' planes need (at least 16). */
int vip_vp8_scratch_bytes(const vip_vp8_desc* desc_h, int n, size_t* bytes_h);

/* Device: from a device copy of what vip_vp8_entropy_h produced (stream, stream_bytes of it) reconstruct every image -
 * intra prediction + inverse WHT / DCT into the planes in `scratch`, then the in-loop filter in place, then chroma
 * upsampling and YUV -> RGB - and write rgb_u8 [n][maxH][maxW][3], cropped to the image's size; pixels beyond it are
 * left untouched and an all-zero descriptor writes nothing.  A descriptor whose records or planes do not fit
 * stream_bytes / scratch_bytes is skipped. */
int vip_vp8_reconstruct_rgb_u8(const uint8_t* stream_d, size_t stream_bytes, const vip_vp8_desc* desc, int n, uint8_t* scratch,
                               size_t scratch_bytes, uint8_t* rgb_u8, int maxH, int maxW, void* stream);

/* The same with a choice of stages, for measurements (tools/bench_webp_lossy.py): reconstruction and filter are one
 * launch, the output another; a stage left out leaves the planes in `scratch` as the call found them. */
#define VIP_VP8_STAGE_RECON 1
#define VIP_VP8_STAGE_FILTER 2
#define VIP_VP8_STAGE_OUTPUT 4
#define VIP_VP8_STAGE_LDS_PLANES 8    /* with RECON: images of up to 13 x 13 macroblocks keep their planes in LDS until the end */
int vip_vp8_default_stages(void);      /* the mask vip_vp8_reconstruct_rgb_u8 runs */
int vip_vp8_reconstruct_stages_rgb_u8(const uint8_t* stream_d, size_t stream_bytes, const vip_vp8_desc* desc, int n, uint8_t* scratch,
                                      size_t scratch_bytes, uint8_t* rgb_u8, int maxH, int maxW, int stages, void* stream);

/* Lossy WebP re-save (the stress test's `w<Q>` step): the project's own VP8 key-frame encoder up to the entropy coder,
 * which is lossless and skipped - forward colour conversion, mode decision, forward transforms and quantisation on the
 * GPU, then the decoder's own in-loop filter and RGB output.  The decisions are the project's, not libwebp's; the result
 * is a valid key frame: written out as a file (tests/_vp8.py does that), libwebp decodes it to the same pixels, bit for bit.
 * The rules, all integer and deterministic:
 *  - RGB -> YUV 4:2:0 as libwebp's plain integer path: Y = (16839 R + 33059 G + 6420 B + (16 << 16) + 32768) >> 16; with
 *    R, G, B summed over a 2 x 2 block, U = clip8((-9719 R - 19081 G + 28800 B + (128 << 18) + (1 << 17)) >> 18) and
 *    V = clip8((28800 R - 24116 G - 4684 B + (128 << 18) + (1 << 17)) >> 18).  The last column and row are replicated for odd
 *    sizes and out to the macroblock grid.
 *  - One quantiser index for the frame, base_q = clamp(int(127 (1 - l^(1/3))), 0, 127) with c = quality / 100 and
 *    l = 2 c / 3 below c = 0.75, 2 c - 1 from there (libwebp's quality curve, float64 on the host); no segments, no deltas;
 *    the six steps as a decoder derives them from base_q.
 *  - level = sign(c) min(2047, (|c| + ((3 q) >> 3)) / q); the decoder sees level * q.
 *  - Forward 4 x 4 DCT and WHT in the published integer forms of VP8 encoders.
 *  - Chroma: of DC, TM, VE, HE the mode with the smallest sum of squared errors between source and prediction over U and V
 *    together, ties to the first in that order.
 *  - Luma: S16 = the smallest prediction SSE of the four 16 x 16 modes (ties as for chroma).  Sub-blocks in raster order take
 *    the best of the ten modes by prediction SSE, ties to the lowest VIP_VP8_B_* number, and are transformed, quantised and
 *    reconstructed in place before the next one predicts; S4 = the sum of their SSEs.  Sub-block modes are used when
 *    S4 + i4_bias < S16, i4_bias = (k * q * q) >> 4 with q the luma AC step (k: DESIGN.md).  A 16 x 16 macroblock sends its
 *    sixteen luma DCs through the forward WHT as Y2.
 *  - A macroblock without a non-zero level is skipped.
 *  - Normal loop filter, sharpness 0, one level = clamp((a * base_q + b) >> 4, 0, 63) (a, b: DESIGN.md), no deltas. */
typedef struct vip_vp8_enc_params {
    int32_t quality, base_q;
    int32_t y1[2], y2[2], uv[2];      /* [0] DC step, [1] AC step                                                      */
    int32_t filter_level;             /* the frame header's level; 0: no filter                                        */
    int32_t flevel, ilevel, hev;      /* what every macroblock record gets                                             */
    int32_t i4_bias;
    int32_t reserved;
    uint32_t y1_inv[2], y2_inv[2], uv_inv[2];   /* ceil(2^32 / step): (x * inv) >> 32 == x / step for 0 <= x < 65536  */
} vip_vp8_enc_params;

/* Host: the numbers above for `quality` (1..100). */
int vip_vp8_encode_params_h(int quality, vip_vp8_enc_params* params_h);

/* Host: the descriptors of n images re-saved as lossy WebP, sizes_hw_h int32 [n][2] = (h, w), in the layout
 * vip_vp8_entropy_h produces, every macroblock with room for 25 coded blocks (coef_idx = 25 * macroblock index), stream_off and coef_off
 * 16-byte aligned; filter_type
 * from `quality`.  *stream_bytes_h / *scratch_bytes_h = the sizes of the device buffers they address.  Sizes beyond
 * VIP_MAX_JPEG_PIXELS are refused. */
int vip_vp8_encode_layout_h(const int32_t* sizes_hw_h, int n, int quality, vip_vp8_desc* desc_h, size_t* stream_bytes_h,
                            size_t* scratch_bytes_h);

/* Device: encode rgb_u8 [n][maxH][maxW][3] (image i at its descriptor's size, a device copy of vip_vp8_encode_layout_h's)
 * at `quality`: per image the macroblock records and the dequantised coefficients of the coded blocks into stream_d (coded
 * blocks back to back from block coef_idx), the quantised levels into levels_d (int16 [macroblock][25][16], raster order,
 * macroblocks of the batch back to back in image order - for tests) and the unfiltered reconstruction into the planes in
 * `scratch`.  vip_vp8_reconstruct_stages_rgb_u8 with VIP_VP8_STAGE_FILTER | VIP_VP8_STAGE_OUTPUT then gives the pixels of
 * the re-saved file.  No atomics: the output does not depend on the batch around an image; every byte of an image's share
 * of stream_d's coefficient area and of levels_d is written.  A descriptor that does not fit the buffers or the slots is
 * skipped.  Null pointers, a quality outside 1..100 and slots beyond VIP_MAX_JPEG_PIXELS are refused before any HIP call. */
int vip_vp8_encode_rgb_u8(const uint8_t* rgb_u8, const vip_vp8_desc* desc, int n, int maxH, int maxW, int quality, uint8_t* stream_d,
                          size_t stream_bytes, int16_t* levels_d, size_t levels_elems, uint8_t* scratch, size_t scratch_bytes,
                          void* stream);

/* Host: the 1025x2 coefficient table of TensorFlow's legacy bicubic kernel (Keys a = -0.5). */
int vip_bicubic_table_f32(float* table_h);

/* Device: uint8 RGB -> float -> bicubic resize (Keys a=-0.5, half-pixel centres, offset quantised to the
 * 1024-entry table, out-of-image taps dropped and weights renormalised = tf.image.resize(method="bicubic",
 * antialias=False)) -> /255 -> f16 NHWC with the channel axis zero-padded to c_out.
 * Replaces dataset/dataset.py:31-38.  sizes_hw int32 [n][2] = (h,w) of each image inside its
 * maxH x maxW slot; table = device copy of vip_bicubic_table_f32. */
int vip_resize_bicubic_norm_f16(const uint8_t* rgb_u8, const int32_t* sizes_hw, const float* table,
                                int n, int maxH, int maxW, void* out, int outH, int outW, int c_out,
                                void* stream);

/* Native-resolution tiles (main.py --tiles-out): tile t of tile_tab int32 [n_tiles][4] = (image, y0, x0, 0) is the tile x tile
 * pixels at (y0, x0) of that image's slot in rgb_u8 [n][maxH][maxW][3], scored as an image of its own.  out [n_tiles][outH][outW]
 * [c_out] holds exactly what vip_resize_bicubic_norm_f16 / _s32 gives for the same pixels held as a stand-alone tile x tile image -
 * dataset/dataset.py:31-38 applied to the crop: p / 255 when out == tile, else the legacy bicubic with the same table and order
 * of operations, its taps clamped at the TILE's edge (no neighbouring pixel of the large image and no slot padding is read).
 * One launch per call, n_tiles <= 65535, out 16-byte aligned; a row of tile_tab that does not lie inside a slot yields a zero
 * tile.  _f16: fp16 output; _s32: the unrounded fp32 values (STRICT path). */
int vip_tile_resize_bicubic_norm_f16(const uint8_t* rgb_u8, const int32_t* tile_tab, const float* table, int n_tiles, int maxH,
                                     int maxW, int tile, void* out, int outH, int outW, int c_out, void* stream);
int vip_tile_resize_bicubic_norm_s32(const uint8_t* rgb_u8, const int32_t* tile_tab, const float* table, int n_tiles, int maxH,
                                     int maxW, int tile, float* out, int outH, int outW, int c_out, void* stream);

/* Occlusion variants (main.py --occlusion): variant v of occ_tab int32 [V][8] = (image, y0, x0, y1, x1, 0, 0, 0) is that image with
 * the pixels y0 <= y < y1, x0 <= x < x1 replaced by fill_u8[image] (uint8 [n][4] = r, g, b, 0; 4-byte aligned), sent through
 * dataset/dataset.py:31-38.  out [V][outH][outW][c_out] holds exactly what vip_resize_bicubic_norm_f16 / _s32 gives for an occluded
 * uint8 copy of the image: the same taps on the image's own size, the same order of operations, the identity branch when
 * h == outH && w == outW.  The replacement is applied per tap as the byte is read: one launch per call, V <= 65535, no intermediate
 * uint8 batch, out 16-byte aligned.  n = the number of images in rgb_u8 / sizes_hw / fill_u8: a row whose image index is not in
 * 0 .. n-1 or whose rectangle does not lie inside its image (0 <= y0 <= y1 <= h, 0 <= x0 <= x1 <= w) yields a zero output and
 * reads nothing.  _f16: fp16 output; _s32: the unrounded fp32 values (STRICT path; packed storage = vip_pack_h2 of them).
 * vip_image_mean_u8: fill_u8[i] = the mean colour of image i over its own h x w pixels (the slot's padding is never read), per
 * channel (sum + h w / 2) / (h w) in 64-bit integers - exact, halves up; byte 3 is 0. */
int vip_image_mean_u8(const uint8_t* rgb_u8, const int32_t* sizes_hw, int n, int maxH, int maxW, uint8_t* fill_u8, void* stream);
int vip_occlude_resize_bicubic_norm_f16(const uint8_t* rgb_u8, const int32_t* sizes_hw, const uint8_t* fill_u8, const int32_t* occ_tab,
                                        const float* table, int n, int V, int maxH, int maxW, void* out, int outH, int outW, int c_out,
                                        void* stream);
int vip_occlude_resize_bicubic_norm_s32(const uint8_t* rgb_u8, const int32_t* sizes_hw, const uint8_t* fill_u8, const int32_t* occ_tab,
                                        const float* table, int n, int V, int maxH, int maxW, float* out, int outH, int outW, int c_out,
                                        void* stream);

/* TTA ops (dataset/augment.py:115-120,142-146) on f16 NHWC batches: flags int32 [B]: bit0 horizontal flip,
 * bit1 vertical flip, bit2 RGB->gray->RGB (0.2989, 0.5870, 0.1140). */
int vip_tta_augment_f16(const void* x, void* y, const int32_t* flags, int B, int H, int W, int C,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * MBConv front half in one launch:  z = act_d( dwconv_kxk,stride( zero_pad( act_e( conv1x1(x; we) + be ) ) ) + bd ).
 * Replaces the expand Conv2D(1x1)+BN+swish and the DepthwiseConv2D(k, strides)+BN+swish of kecam's inverted residual block
 * (efficientnet_v2.py:63-66,85-90): the expanded tensor stays in LDS.  Same rounding points as vip_conv2d_nhwc_f16 /
 * vip_conv2d_hilo_nhwc_f16 followed by vip_dwconv2d_nhwc_f16 (the expanded activations are rounded to fp16 before the filter).
 * x f16 [B,H,W,Cin]; we f16 [Ce][ldw] (+ optional we_lo, the low halves of two-term weights); be, bd f32 [Ce] or NULL;
 * wd f32 [k][k][Ce]; z f16 [B,Ho,Wo,Ce]; (pt, pl) = zero padding of the depthwise input.  vip_mbconv_expand_dw_supported:
 * Cin % 8 == 0, Cin <= 128, Ce % 32 == 0, k in {3, 5}, stride in {1, 2}.
 * ------------------------------------------------------------------------------------------ */
/* EXPERIMENT (measured 0.4-0.8x the speed of the two launches it replaces): compiled only with VIP_BUILD_EXPERIMENTS=1; in the default
 * library vip_mbconv_expand_dw_supported() is 0 for every shape and vip_mbconv_expand_dw_f16 returns VIP_ERR_UNSUPPORTED.
 * vip_experiments_built() = 1 when the experimental kernels (this one, the depthwise convolution on the matrix cores behind
 * VIP_DW_MFMA=1, the pipelined window attention behind VIP_ATTN_PIPE=1) are in the library. */
int vip_experiments_built(void);
int vip_mbconv_expand_dw_supported(int Cin, int Ce, int k, int stride);
int vip_mbconv_expand_dw_f16(const void* x, const void* we, const void* we_lo, const float* be, const float* wd, const float* bd,
                             void* z, int B, int H, int W, int Cin, int Ce, int ldw, int k, int stride, int pt, int pl, int Ho,
                             int Wo, int act_e, int act_d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scores.
 * vip_head_prob_f32: what `model.predict` applies to the logits - sigmoid for one class, softmax otherwise (the Dense(classes,
 *   activation=...) heads of resnet_rs_model.py:474-476, gcvit models/gcvit.py:109-113, tfimm / kecam classifiers) -> prob [B][N]
 *   (may be NULL), and main.py:113-114's multi-class -> binary map -> score [B] = N == 1 ? p : 1 - p[:, 0] (may be NULL).
 * vip_ensemble_mean_f32: mean over the M members of scores [M][ld] -> mean [n] (pd.concat + groupby('filename').mean(),
 *   main.py:142-143, for images that appear once per member).  All fp32.
 * vip_prob_to_score_f32: the same map applied to probabilities a model's predict() already returned (prob [B][N] -> score [B]).
 * ------------------------------------------------------------------------------------------ */
int vip_head_prob_f32(const float* logits, float* prob, float* score, int B, int N, void* stream);
/* The classifier activation a checkpoint's model_config names when it is not the default pairing above (Dense(classes,
 * activation=classifier_activation | head_act), resnet_rs_model.py:474-476, gcvit models/gcvit.py:113): act 0 = linear (the logits),
 * 1 = element-wise sigmoid for any N, 2 = softmax for any N (N = 1 -> 1.0, as Keras computes it). */
int vip_head_act_f32(const float* logits, float* prob, int B, int N, int act, void* stream);
int vip_prob_to_score_f32(const float* prob, float* score, int B, int N, void* stream);
int vip_ensemble_mean_f32(const float* scores, float* mean, int M, int n, long ld, void* stream);
/* Tile report: scores f32 [rows][T] (rows = members + 1, the last row the per-tile ensemble mean), seg int32 [n + 1] with the
 * tiles of image i at columns seg[i] .. seg[i+1]-1 -> out f32 [3][rows][n] = per row and image the mean of its tile scores (fp32,
 * summed sequentially in tile order: independent of the launch shape), their max, and the fraction of tiles > thr.  An image
 * without tiles gets NaN in all three. */
int vip_tile_aggregate_f32(const float* scores, const int32_t* seg, int n, int rows, int T, float thr, float* out, void* stream);
/* Occlusion report: scores f32 [rows][V] (rows = members + 1, the last row the per-variant ensemble mean), plain f32 [rows][n] the
 * scores of the images as they are, seg int32 [n + 1] with the variants of image i at columns seg[i] .. seg[i+1]-1: the
 * (G - K + 1)^2 windows of K x K cells on its G x G grid, row-major (2 <= G <= 32, 1 <= K <= G).  delta = plain - score.
 * cells f32 [rows][n][G][G]: per cell the mean of delta over the windows that cover it (fp32, summed sequentially in variant order,
 * one division: independent of the launch shape).  stats f32 [rows][n][4] = (max delta, min delta, index of the first variant with
 * the max delta, number of variants whose (score > thr) differs from (plain > thr)).  An image without variants (seg[i] ==
 * seg[i+1]) gets NaN in all of them.  seg is device memory, so a count that is neither 0 nor (G - K + 1)^2 cannot be refused here:
 * such an image reads nothing and gets NaN too; the caller checks its host copy of seg (ops.occlusion_cells raises). */
int vip_occlusion_cells_f32(const float* scores, const float* plain, const int32_t* seg, int n, int rows, int V, int G, int K, float thr,
                            float* cells, float* stats, void* stream);
/* Full-size map of one row: cells_row f32 [n][G][G], sizes_hw int32 [n][2] -> out [n][maxH][maxW]: pixel (y, x) of image i takes
 * the value of the cell whose range [(g L) / G, ((g + 1) L) / G) holds it on each axis - the occluder's own edges; 0 outside the
 * image.  out_u8 = 0: f32, the values as they are.  out_u8 = 1: uint8 round(255 (0.5 + 0.5 v / peak)), peak = max |cell| of the
 * image; 128 (= no effect) everywhere in an image whose peak is 0 or whose cells are NaN - a map vip_cam_overlay_u8 blends. */
int vip_occlusion_map(const float* cells_row, const int32_t* sizes_hw, int n, int maxH, int maxW, int G, void* out, int out_u8,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * STRICT precision path, packed storage (entry points ending in _h2) - the default of `--precision strict` since round 4.
 * An activation or weight value v is TWO fp16 terms, hi = rn16(v) and lo = rn16(v - hi): 2^-22 relative for |v| >= 2^-3, 2^-25
 * absolute below, |v| <= 65504.  Layout: 8 consecutive channels c0..c0+7 (c0 % 8 == 0) of a row = 32 bytes [hi x 8][lo x 8] - four
 * bytes per element like fp32; every channel count, stride and offset is a multiple of 8 and is given in ELEMENTS.  Contractions run
 * on v_mfma_f32_16x16x32_f16, three per fragment pair (w_lo x_hi + w_hi x_lo + w_hi x_hi; w_lo x_lo, 2^-22 of the product, is dropped)
 * with fp32 accumulation: fp32-quality results at 1/3 of the fp16 matrix rate instead of 1/6 (the bf16 x 3 splits of _s32x) or 1/16
 * (_s32), and producers store the split ONCE so that consumers load MFMA fragments with no conversion.  Everything else (LayerNorm,
 * pooling, depthwise filters, softmax, activations) is fp32 arithmetic on the joined value.
 * `status`: optional device word; a producer that meets a value outside the fp16 range (or a NaN) stores VIP_H2_OVERFLOW there -
 * the caller checks it after the forward pass and falls back to the fp32-storage path (_s32).  Same reference call sites as _s32.
 * vip_pack_h2 / vip_unpack_h2 convert fp32 rows <-> packed rows (n elements, n % 8 == 0).
 * ------------------------------------------------------------------------------------------ */
#define VIP_H2_OVERFLOW 1
int vip_pack_h2(const float* x, void* y, long n, int* status, void* stream);
int vip_unpack_h2(const void* x, float* y, long n, void* stream);
/* w: packed rows [Cout][ldw halfs] of (W * w_scale) ([kh][kw][Cin_g] order, 8 k = [hi x 8][lo x 8]; ldw % 16 == 0, zero padded),
 * bias = b * w_scale (fp32), out_scale = 1 / w_scale (a power of two chosen by the caller so that the low halves are fp16 normals). */
int vip_conv2d_nhwc_h2(const void* x, const void* w, const float* bias, const void* residual, void* y, const vip_conv_desc* d,
                       float out_scale, int* status, void* stream);
int vip_conv2d_kernel_name_h2(const vip_conv_desc* d, int has_residual, char* name, size_t cap);
int vip_conv2d_kernel_variant_h2(const vip_conv_desc* d, int has_residual, char* variant, size_t cap);   /* see vip_conv2d_kernel_variant */
/* vip_conv2d_gated_nhwc_f16 on the packed storage: gate packed [B][Cin] (vip_se_gate_h2), multiplied into the activation operand in fp32
 * and split again in registers; 1x1 stride-1 ungrouped, (activation) or (residual [+ReLU]) epilogue, cin_off = 0, ldx = Cin. */
int vip_conv2d_gated_nhwc_h2(const void* x, const void* gate, const void* w, const float* bias, const void* residual, void* y,
                             const vip_conv_desc* d, float out_scale, int* status, void* stream);
/* every other operator, arguments as the _s32 form (strict_ops.hip: one kernel template, two storages); fp32 parameters (LayerNorm
 * gamma / beta, depthwise filters, head matrices, relative-position table) and fp32 head outputs as there */
int vip_dwconv2d_nhwc_h2(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int C, int k, int stride,
                         int pt, int pl, int Ho, int Wo, int act, int* status, void* stream);
/* Dry run of the stride-1 register-tiled launch vip_dwconv2d_nhwc_h2 makes (dwconv_tile_h2_kernel), as vip_dwconv2d_tile_plan: returns
 * the tile groups a channel block's workgroups walk (0: that kernel does not take the call), *workgroups = gridDim.x, geom[4] =
 * {4-channel chunks per block, tiles per block, channel blocks (gridDim.y), workgroup cap}.  Pure host arithmetic: no device is needed. */
long vip_dwconv2d_tile_plan_h2(int B, int H, int W, int C, int k, int stride, int pt, int pl, int Ho, int Wo, int* workgroups, int* geom);
/* Stride-1 k = 3 / 5 / 7 DepthwiseConv2D on the packed storage, staged through LDS (dwconv_lds_h2.hip) - the Keras DepthwiseConv2D of
 * tfimm's ConvNeXtBlock (/root/reference/models/tfimm/architectures/convnext.py:200-229) and of the MBConv blocks in strict mode.
 * w_quad: the filter QUAD-MAJOR, fp32 [C/4][k*k][4] (vip_dw_filter_quad_major converts the [k*k][C] layout of vip_dwconv2d_nhwc_h2).
 * vip_dwconv2d_s1_supported_h2 != 0 for the shapes it takes; others return VIP_ERR_UNSUPPORTED (use vip_dwconv2d_nhwc_h2). */
/* Fused  y = W2 . gelu(W1 . LN(x) + b1) + b2 (+ residual)  on the packed storage (mlp_h2.hip; C = 64 / 96 / 128, hidden % 32 == 0,
 * M >= 8192 - vip_mlp_fused_supported_h2): the strict form of vip_mlp_fused_f16, same call sites.  x, residual, y packed rows (ldx, ldy,
 * ldr in logical elements), w1 [hidden][ldw1 halfs] and w2 [C][ldw2 halfs] packed and pre-scaled as for vip_conv2d_nhwc_h2 (b = bias *
 * scale, out_scale = 1 / scale); ln_gamma / ln_beta NULL: no LayerNorm. */
int vip_mlp_fused_supported_h2(int M, int C, int hidden, int act);
/* dry run, as vip_mlp_fused_plan: tiles (0: unsupported), *workgroups (CUs x workgroups per CU, at most), *tile_rows (32 per wave of the
 * instantiation the host picks: 128 or 256) */
int vip_mlp_fused_plan_h2(int M, int C, int hidden, int act, int* workgroups, int* tile_rows);
int vip_mlp_fused_h2(const void* x, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* w1, const float* b1, float out_scale1,
                     const void* w2, const float* b2, float out_scale2, const void* residual, void* y, int M, int C, int hidden, int ldx,
                     int ldw1, int ldw2, int ldy, int ldr, int act, int* status, void* stream);
int vip_dw_filter_quad_major(const float* w, float* w_quad, int k, int C, void* stream);
int vip_dwconv2d_s1_supported_h2(int B, int H, int W, int C, int k, int Ho, int Wo);
/* dry run of vip_dwconv2d_s1_h2 / _pool_h2: returns the work items (region group x 16-channel block; 0: shape not taken), *workgroups =
 * the workgroups that share them as contiguous runs (min(2 x CUs, items) - asks the current device), geom[6] = {sub-regions per wave,
 * tile rows, tile columns of a sub-region, sub-regions per image in y, in x, 16-channel blocks}.  workgroups / geom may be NULL. */
long vip_dwconv2d_s1_plan_h2(int B, int H, int W, int C, int k, int Ho, int Wo, int* workgroups, int* geom);
int vip_dwconv2d_s1_h2(const void* x, const float* w_quad, const float* bias, void* y, int B, int H, int W, int C, int k, int pt, int pl,
                       int Ho, int Wo, int act, int* status, void* stream);
/* The pooling form (strict counterpart of vip_dwconv2d_pool_nhwc_f16 + vip_se_gate_pooled_f16): also leaves partials[B][parts][C] fp32,
 * the sums of the activated outputs over `parts` = vip_dwconv2d_s1_pool_parts_h2(...) blocks of each image (0: shape not taken), from
 * which vip_se_gate_pooled_h2 finishes the squeeze-excite mean without reading the map again; fixed summation order. */
int vip_dwconv2d_s1_pool_parts_h2(int B, int H, int W, int C, int k, int Ho, int Wo);
int vip_dwconv2d_s1_pool_h2(const void* x, const float* w_quad, const float* bias, void* y, float* partials, int parts, int B, int H, int W, int C,
                            int k, int pt, int pl, int Ho, int Wo, int act, int* status, void* stream);
int vip_se_gate_pooled_h2(const float* partials, int parts, const void* w1, const float* b1, float s1, const void* w2, const float* b2, float s2,
                          void* gate, int B, int HW, int C, int Cr, int ldw1, int Cout, int ldw2, int act1, int act2, int* status, void* stream);
/* vip_se_gate_f16 on the packed storage: gate [B][Cout] packed; w1 / w2 packed rows of W * scale (ldw in halfs), b = bias * scale,
 * s1 / s2 = 1 / scale */
int vip_se_gate_h2(const void* x, const void* w1, const float* b1, float s1, const void* w2, const float* b2, float s2, void* gate,
                   int B, int HW, int C, int ldx, int Cr, int ldw1, int Cout, int ldw2, int act1, int act2, int* status, void* stream);
int vip_layernorm_h2(const void* x, const float* gamma, const float* beta, void* y, int rows, int C, float eps, int* status, void* stream);
int vip_pool2d_nhwc_h2(const void* x, void* y, int B, int H, int W, int C, int ldx, int ldy, int k, int stride, int pt, int pl, int Ho,
                       int Wo, int mode, int* status, void* stream);
int vip_global_avgpool_h2(const void* x, void* y, int B, int HW, int C, int ldx, int* status, void* stream);
int vip_scale_add_act_h2(const void* x, const void* scale, const void* residual, void* y, void* y2, int B, int HW, int C, int act,
                         int act2, int* status, void* stream);
int vip_radix_combine_h2(const void* x, const void* scale, void* y, int B, int HW, int C, int radix, int* status, void* stream);
int vip_mul_h2(const void* a, const void* b, void* y, long rows, int C, int lda, int a_off, int ldb, int b_off, int ldy, int y_off,
               int* status, void* stream);
int vip_vit_tokens_h2(const void* patches, const void* cls, const void* pos, void* out, int B, int NP, int D, int* status, void* stream);
int vip_gap_ln_dense_h2(const void* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias, float* out,
                        int B, int HW, int C, int ldx, long img_stride, int N, void* stream);
int vip_window_attn_fwd_h2(const void* qkv, const void* q_global, const float* bias_table, void* out, int B, int Hp, int Wp, int C,
                           int heads, int ws, int nq, float scale, int* status, void* stream);
int vip_mhsa_fwd_h2(const void* qkv, void* out, int B, int N, int D, int heads, float scale, int* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * STRICT precision path (entry points ending in _s32): the same operators with fp32 storage and fp32 arithmetic.
 *
 * The reference computes in fp32 (main.py:107-109: tf.keras.models.load_model(...).predict, no mixed-precision policy anywhere)
 * and BASELINE.json's tolerance is |dz| <= 1e-3 on every member's sigmoid logit.  The fp16-storage entry points above sit at the
 * fp16 storage floor of each graph (7e-4 ... 8e-3 with the amplifying synthetic heads); these entry points are
 * the mode in which the tolerance is met member by member.  Activations, weights, biases, gates: fp32, NHWC / row-major, every
 * channel count, stride and offset a multiple of 4 floats; strides in vip_conv_desc are in FLOATS.  Contractions run on
 * v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulate: 157 TFLOP/s on MI355X, 1/16 of the fp16 rate); activations are evaluated
 * in fp32 to 3e-7 absolute (v_exp_f32 / v_rcp_f32, Abramowitz-Stegun 7.1.26 erf), the attention softmax with libm expf and true
 * divisions.  Each entry point replaces the same reference call sites as its _f16 counterpart:
 *   vip_conv2d_nhwc_s32        Conv2D / Dense (+ folded BN) (+ act) (+ residual): resnet_rs_model.py:64-84, kecam common_layers.py:190-248,
 *                              gcvit/layers/attention.py:25,33, tfimm/layers/transformers.py:192-205 (w [Cout][kh][kw][Cin_g] f32)
 *   vip_dwconv2d_nhwc_s32      DepthwiseConv2D: gcvit/layers/feature.py:93,133, tfimm convnext.py:192-198, kecam efficientnet_v2.py:85
 *   vip_layernorm_s32          LayerNormalization: gcvit/layers/block.py:28,39, tfimm/layers/factory.py:37-45
 *   vip_pool2d_nhwc_s32        Average / Max pooling (modes as vip_pool2d_nhwc_f16): resnet_rs_model.py:207-212, aotnet.py:105,329-330
 *   vip_global_avgpool_s32     GlobalAveragePooling2D -> [B][C]
 *   vip_scale_add_act_s32      y = act(x * scale[b,c] + residual), y2 = act2(y) (SE excite + Add + activation): resnet_rs_model.py:269-280
 *   vip_radix_combine_s32      ResNeSt split-attention combine: kecam resnest/resnest.py:57-61
 *   vip_mul_s32                product of channel slices (HorNet gated convolution)
 *   vip_vit_tokens_s32         cls token + position embedding: tfimm vit.py:419-426
 *   vip_gap_ln_dense_s32       classifier heads: (mean over HW rows | token 0) [-> LayerNorm] -> Dense: resnet_rs_model.py:468-476,
 *                              convnext.py:432-436, vit.py:441-461
 *   vip_window_attn_fwd_s32    GCViT WindowAttention core: gcvit/layers/attention.py:52-83 (head_dim 32, <= 256 tokens per window)
 *   vip_mhsa_fwd_s32           ViT MHSA core: tfimm vit.py:148-167 (head_dim 64, N <= 256)
 *   vip_resize_bicubic_norm_s32 / vip_tta_augment_s32   dataset/dataset.py:31-38 / dataset/augment.py:115-120,142-146 with fp32 output
 * ------------------------------------------------------------------------------------------ */
int vip_conv2d_nhwc_s32(const float* x, const float* w, const float* bias, const float* residual, float* y,
                        const vip_conv_desc* d, void* stream);
/* vip_conv2d_nhwc_s32 at 2.7x the matrix rate: every f32 operand is the sum of three bf16 terms (exact: 8 + 8 + 8 bits, f32's exponent
 * range) and the product keeps the six partial products down to 2^-16 of the leading one on v_mfma_f32_16x16x32_bf16 with f32
 * accumulation - what is dropped is <= 3 * 2^-24 of each product, the same results as the f32-MFMA entry point to f32 round-off.
 * w_planes = the weights pre-split: three bf16 planes [3][Cout][ldwp] (ldwp % 8 == 0, zero padded), w = p0 + p1 + p2; activations are
 * split inside the kernel.  d->ldw is ignored; everything else as vip_conv2d_nhwc_s32.  The default of the STRICT path. */
int vip_conv2d_nhwc_s32x(const float* x, const void* w_planes, int ldwp, const float* bias, const float* residual, float* y,
                         const vip_conv_desc* d, void* stream);
/* The same with TWO bf16 terms per operand (planes 0 and 1 of the same w_planes tensor; three MFMAs per block: b0 c0 + b0 c1 + b1 c0):
 * 2^-17 of each product is dropped - 64x finer than fp16 storage, not f32 quality; twice the matrix rate of vip_conv2d_nhwc_s32x.
 * Opt-in (VIP_STRICT_GEMM=bf16x2). */
int vip_conv2d_nhwc_s32x2(const float* x, const void* w_planes, int ldwp, const float* bias, const float* residual, float* y,
                          const vip_conv_desc* d, void* stream);
int vip_dwconv2d_nhwc_s32(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int C, int k,
                          int stride, int pt, int pl, int Ho, int Wo, int act, void* stream);
int vip_layernorm_s32(const float* x, const float* gamma, const float* beta, float* y, int rows, int C, float eps, void* stream);
int vip_pool2d_nhwc_s32(const float* x, float* y, int B, int H, int W, int C, int ldx, int ldy, int k, int stride, int pt,
                        int pl, int Ho, int Wo, int mode, void* stream);
int vip_global_avgpool_s32(const float* x, float* y, int B, int HW, int C, int ldx, void* stream);
int vip_scale_add_act_s32(const float* x, const float* scale, const float* residual, float* y, float* y2, int B, int HW, int C,
                          int act, int act2, void* stream);
int vip_radix_combine_s32(const float* x, const float* scale, float* y, int B, int HW, int C, int radix, void* stream);
int vip_mul_s32(const float* a, const float* b, float* y, long rows, int C, int lda, int a_off, int ldb, int b_off, int ldy,
                int y_off, void* stream);
int vip_vit_tokens_s32(const float* patches, const float* cls, const float* pos, float* out, int B, int NP, int D, void* stream);
int vip_gap_ln_dense_s32(const float* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias,
                         float* out, int B, int HW, int C, int ldx, long img_stride, int N, void* stream);
int vip_window_attn_fwd_s32(const float* qkv, const float* q_global, const float* bias_table, float* out, int B, int Hp, int Wp,
                            int C, int heads, int ws, int nq, float scale, void* stream);
int vip_mhsa_fwd_s32(const float* qkv, float* out, int B, int N, int D, int heads, float scale, void* stream);
int vip_resize_bicubic_norm_s32(const uint8_t* rgb_u8, const int32_t* sizes_hw, const float* table, int n, int maxH, int maxW,
                                float* out, int outH, int outW, int c_out, void* stream);
int vip_tta_augment_s32(const float* x, float* y, const int32_t* flags, int B, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Introspection and measurement support (no reference counterpart: the reference leaves kernel choice to cuDNN and
 * has no roofline measurement; SURVEY.md section 8(b) / 8(d) ask for these).
 * ------------------------------------------------------------------------------------------ */

/* ------------------------------------------------------------------------------------------
 * Evidence maps (Grad-CAM) for heads of the form GlobalAveragePooling -> [LayerNormalization] -> Dense -> activation (csrc/cam.hip).
 * With v = mean_hw F, u = LN(v) | v, z = W u + b, p = act(z) the gradient Grad-CAM pools has a closed form, so the map comes out of
 * the forward pass:  dz = d target / d z,  a = W^T dz,  [LayerNorm head, uh = (v - mean v) / sd:  a <- gamma a,
 * a <- (a - mean a - uh mean(a uh)) / sd],  g = a / HW = mean_hw d target / d F,  cam[h,w] = max(0, sum_c F[h,w,c] g[c]).
 * Replaces tape.gradient + reduce_mean + feats @ pooled_grads + maximum of models/gcvit/utils/gradcam.py:44-55 and
 * keras_cv_attention_models/visualizing/visualizing.py:186-245 (use_v2=False), with the gradient mean taken PER IMAGE.
 * vip_cam_f32 / _s32 / _h2: F in fp16 / fp32 / packed fp16-pair storage; the other arguments as vip_gap_ln_dense_s32 (gamma = beta =
 *   NULL: no LayerNorm; W f32 [N][C]; bias f32 [N] or NULL; C <= 4096, N <= 64).  act: 0 linear, 1 element-wise sigmoid, 2 softmax
 *   (vip_head_act_f32).  target: -1 = the score vip_prob_to_score_f32 forms (p[0] for N = 1, else 1 - p[0]), k >= 0 = p[k]
 *   (`class_channel = preds[:, pred_index]`, gradcam.py:48).  Outputs, all f32: cam [B][HW] (after the max with 0, NOT normalised),
 *   peak [B] = max_hw cam (0 for an all-zero map; NaN when a position is not finite - the caller's error), z [B][N] the logits.
 * vip_cam_compose_f32: `members` (1 .. 16) low-resolution maps - host arrays of device pointers maps_h[m] -> [n][gh*gw] f32 and
 *   peaks_h[m] -> [n] f32, grids grid_h_h / grid_w_h, weights weights_h - -> sum_m weight[m] * resize(map_m / peak_m) per image at
 *   its own size (sizes_hw, slot layout [n][maxH][maxW] as vip_resize_bicubic_norm_f16; outside the image 0).  Bilinear, half-pixel
 *   centres, edge clamp (tf.image.resize(..., "bilinear"), visualizing.py:305); a member whose peak is 0 contributes 0, not NaN.
 *   out: f32, or with out_u8 = 1 uint8 round(255 * map).
 * vip_cam_overlay_u8: out = clip(round(rgb + alpha * table[map]), 0, 255): the colour table [256][3] uint8 applied to the uint8 map and
 *   blended over the decoded pixels (gradcam.py:57-65); rgb / out [n][maxH][maxW][3], map [n][maxH][maxW].
 * ------------------------------------------------------------------------------------------ */
int vip_cam_f32(const void* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias, float* cam,
                float* peak, float* z, int B, int HW, int C, int ldx, long img_stride, int N, int act, int target, void* stream);
int vip_cam_s32(const float* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias, float* cam,
                float* peak, float* z, int B, int HW, int C, int ldx, long img_stride, int N, int act, int target, void* stream);
int vip_cam_h2(const void* x, const float* gamma, const float* beta, float eps, const float* W, const float* bias, float* cam,
               float* peak, float* z, int B, int HW, int C, int ldx, long img_stride, int N, int act, int target, void* stream);
int vip_cam_compose_f32(const float* const* maps_h, const int* grid_h_h, const int* grid_w_h, const float* const* peaks_h,
                        const float* weights_h, int members, const int32_t* sizes_hw, int n, int maxH, int maxW, void* out,
                        int out_u8, void* stream);
int vip_cam_overlay_u8(const uint8_t* rgb_u8, const uint8_t* map_u8, const uint8_t* table_u8, float alpha, int n, int maxH,
                       int maxW, uint8_t* out_u8, void* stream);

/* ---- HorNet global-local filter (csrc/global_filter.hip) ------------------------------------------------------------------------
 * Everything between the two LayerNorms of kecam hornet/hornet.py:53-81 `global_local_filter` in one launch, on the three storages
 * (_f16: fp16, _s32: fp32, _h2: packed (hi, lo) pairs with the status word of the other packed producers).  x, y [B][H][W][S],
 * half = S / 2; w3 [3][3][half] and g [H][W][half] are fp32 parameters:
 *   y[b,h,w,2i]   = sum_{dy,dx in -1..1} w3[dy+1][dx+1][i] * x[b,h+dy,w+dx,i]               (DepthwiseConv2D 3x3, SAME, no bias;
 *                                                                                             pixels outside the map count as zero)
 *   y[b,h,w,2i+1] = sum_{a<H, c<W} g[a][c][i] * x[b,(h-a) mod H,(w-c) mod W,half+i]
 * The second line is irfft2(rfft2(x[..., half+i]) * Wc[..., i], s=(H,W)) with g = irfft2(Wc, s=(H,W)) (numpy / pocketfft semantics:
 * the imaginary parts of the k = 0 column, and of the Nyquist column for even W, do not reach the output) - the `ComplexDense`
 * weight as a circular depthwise filter, built on the host in float64.  Channels 2i / 2i+1 are the reference's concat on a new last
 * axis + reshape.  fp32 products and sums in an order fixed by (H, W), one rounding on the store; no atomics: bit-reproducible and
 * independent of the batch.  The whole map is held in LDS: 2 <= H, W <= 16 and S % 16 == 0, anything else is VIP_ERR_UNSUPPORTED.
 * W = 14 / 12 / 7 / 6 (the maps of 224 and 200 pixel inputs) run register-blocked, the other widths a generic form. */
int vip_global_local_filter_supported(int H, int W, int S);
/* dry run: workgroups per image (0: unsupported); *block_channels = channels of S one workgroup owns, *lds_bytes = its LDS */
int vip_global_local_filter_plan(int H, int W, int S, int* block_channels, int* lds_bytes);
int vip_global_local_filter_nhwc_f16(const void* x, const float* w3, const float* g, void* y, int B, int H, int W, int S, void* stream);
int vip_global_local_filter_nhwc_s32(const float* x, const float* w3, const float* g, float* y, int B, int H, int W, int S, void* stream);
int vip_global_local_filter_nhwc_h2(const void* x, const float* w3, const float* g, void* y, int B, int H, int W, int S, int* status,
                                    void* stream);

/* ---- Swin Transformer V2 shifted cosine window attention (csrc/swin_attn.hip) -----------------------------------------------------
 * Everything between the `qkv` Dense and the `output` Dense of kecam swin_transformer_v2.py:164-262 (`shifted_window_attention` with
 * `window_mhsa_with_pair_wise_positional_embedding`) in one launch on the UNPADDED map, on the three storages (_f16: fp16, _s32: fp32,
 * _h2: packed (hi, lo) pairs with the status word of the other packed producers).
 *   qkv [B][H][W][3C], channels (q|k|v, head, 32) - query_bias and value_bias already added by the producing Dense; out [B][H][W][C];
 *   v_bias fp32 [C] or NULL (the layer has no qv_bias): the value row of a padded token;
 *   tau fp32 [heads] = exp(min(scale_weight, ln 100)); bias_table fp32 [(2ws-1)^2][heads] = 16 sigmoid(meta MLP of the log-spaced
 *   offsets), built on the host; ws in 2 .. 8 (the caller clamps it to the map); shift 0 or ws / 2 rounded down.
 * Hp = ceil(H / ws) ws, Wp likewise.  The token at ROLLED position (Y, X) of window (Y / ws, X / ws) is the map's token at
 * y = (Y + shift) mod Hp, x = (X + shift) mod Wp; with y >= H or x >= W it is PADDED: key 0, value v_bias, never a query, never stored.
 * Padded keys are not masked: they take part in the softmax of their window with the logit 0 + table.
 *   qn = q rsqrt(max(sum q^2, 1e-6)), kn likewise (fp32; a maximum under the root, tf.nn.l2_normalize)
 *   logit = tau[head] qn.kn + bias_table[(qr - kr + ws - 1)(2ws - 1) + (qc - kc + ws - 1)][head]
 *           + (shift > 0 and region(q) != region(k) ? -100 : 0)
 *   region(Y, X) = 3 r(Y, Hp) + r(X, Wp), r(t, L) = [t >= L - ws] + [t >= L - shift]   (rolled, padded coordinates)
 *   out[b, y, x, head 32 + :] = softmax over the ws^2 keys of the window (logit) . v, at the query's unrolled position.
 * No atomics: bit-reproducible, independent of the batch.  Anything else (head_dim != 32, ws > 8, another shift): VIP_ERR_UNSUPPORTED. */
int vip_swin_attn_supported(int C, int heads, int ws, int shift);
/* dry run on the host, nothing is launched: 1 and *Hp, *Wp (the padded map), *items = B * windows * heads (the work items of a
 * launch), or 0 when the launch would be refused */
int vip_swin_attn_plan(int B, int H, int W, int heads, int ws, int shift, int* Hp, int* Wp, int* items);
int vip_swin_attn_fwd_f16(const void* qkv, const float* v_bias, const float* tau, const float* bias_table, void* out, int B, int H, int W,
                          int C, int heads, int ws, int shift, void* stream);
int vip_swin_attn_fwd_s32(const float* qkv, const float* v_bias, const float* tau, const float* bias_table, float* out, int B, int H,
                          int W, int C, int heads, int ws, int shift, void* stream);
int vip_swin_attn_fwd_h2(const void* qkv, const float* v_bias, const float* tau, const float* bias_table, void* out, int B, int H, int W,
                         int C, int heads, int ws, int shift, int* status, void* stream);

/* ---- Neighbourhood attention (csrc/nat_attn.hip) ------------------------------------------------------------------------------------
 * Everything between the `qkv` Dense and the `output` Dense of kecam nat/nat.py:65-116 (`neighborhood_attention` with
 * `MultiHeadRelativePositionalKernelBias`) in one launch on the UNPADDED map, on the three storages (_f16: fp16, _s32: fp32, _h2: packed
 * (hi, lo) pairs with the status word of the other packed producers).
 *   qkv [B][H][W][3C], channels (q|k|v, head, 32) - the output of the layer's qkv Dense as it stands; out [B][H][W][C];
 *   kv_pad fp32 [2C] (k | v) or NULL (zeros): the key and value of a PADDED token - the k | v part of the qkv Dense's bias, since the
 *   layer zero-pads a map below the kernel BEFORE that Dense;
 *   table fp32 [heads][(2K-1)^2]: the layer's `positional_embedding`; K = kernel_size in {3, 5, 7}.
 * With r = K / 2, Hp = max(H, K), Wp = max(W, K) the query at (y, x), y < H, x < W, attends to the K x K block with the origin
 *   sy = clamp(y - r, 0, Hp - K), sx = clamp(x - r, 0, Wp - K):
 *   logit(ky, kx) = 2^-2.5 q . k[ky, kx] + table[head][(ky - y + K - 1)(2K - 1) + (kx - x + K - 1)]     (ky, kx) in [sy, sy+K) x [sx, sx+K)
 *   out[b, y, x, head 32 + :] = softmax over the K^2 keys of the block (logit) . v
 * The table index is the absolute key-minus-query offset, not the key's position inside the clamped block.  A token with ky >= H or
 * kx >= W (only when the map is below the kernel) is padded: k | v = kv_pad, it is a key of every block that holds it, never a query,
 * never stored.  No atomics: bit-reproducible, independent of the batch.  K outside {3, 5, 7}, C != 32 heads, sizes beyond the plan's
 * range: VIP_ERR_UNSUPPORTED. */
/* dry run on the host, nothing is launched: 1 and *Hp, *Wp (the padded map), *items = B * ceil(H / 8) * ceil(W / 8) * heads (the work
 * items of a launch: 8 x 8 query tiles per head), or 0 when the launch would be refused */
int vip_nat_attn_plan(int B, int H, int W, int heads, int kernel_size, int* Hp, int* Wp, int* items);
int vip_nat_attn_fwd_f16(const void* qkv, const float* kv_pad, const float* table, void* out, int B, int H, int W, int C, int heads,
                         int kernel_size, void* stream);
int vip_nat_attn_fwd_s32(const float* qkv, const float* kv_pad, const float* table, float* out, int B, int H, int W, int C, int heads,
                         int kernel_size, void* stream);
int vip_nat_attn_fwd_h2(const void* qkv, const float* kv_pad, const float* table, void* out, int B, int H, int W, int C, int heads,
                        int kernel_size, int* status, void* stream);

/* Which kernel vip_conv2d_nhwc_f16 / _gated_ / _hilo_ would launch for this descriptor ("pw_gemm_kernel",
 * "pwk_direct_kernel", "pwk_gemm_kernel", "pwk_gemm_kernel(im2col)", "rows_gemm_kernel", "conv_igemm_kernel"):
 * the dispatcher itself in a dry run, nothing is launched.  Used to label profiler records (bench.py roofline). */
int vip_conv2d_kernel_name(const vip_conv_desc* d, int has_residual, int has_gate, int has_w_lo, char* name_h,
                           size_t cap);
/* The same dry run, down to the instantiation: template arguments and, where the kernel tiles M x N, the tile grid - "rows_gemm",
 * "pw_gemm<KS=8> 2 x 128" (channel chunks x channels per chunk), "pw_gemm<KS=4,hilo> 1 x 256", "pwk_direct<2,gated> PT=4",
 * "pwk_gemm<2,2> 65 x 4", "gemm8p<pipe> 34 x 4", "im2col<2>", "conv_igemm<128,128>", "pwx<4,2>", "pwx_ln<6,2>" (KSC, PT). */
int vip_conv2d_kernel_variant(const vip_conv_desc* d, int has_residual, int has_gate, int has_w_lo, char* variant_h,
                              size_t cap);

/* Scratch memory an entry point needs from its caller (bytes); 0 for every operator that works in place on its
 * operands.  op = one of VIP_OP_*; dims as documented per op. */
enum { VIP_OP_CONV2D = 0, VIP_OP_MLP_FUSED = 1, VIP_OP_WINDOW_ATTN = 2, VIP_OP_MHSA = 3,
       VIP_OP_JPEG_IDCT_RGB = 4 /* dims[0] = total int16 coefficients of the batch -> planes_ws bytes */ };
size_t vip_workspace_bytes(int op, const int64_t* dims, int ndims);

/* On-box peak probes for the roofline denominators ("measured on-box, never hard-coded").
 * vip_microbench_copy: dst[i] = src[i] over `bytes` bytes (16 B per lane, grid-stride) - 2*bytes of HBM traffic.
 * vip_microbench_mfma_f16: every wave of a chip-filling grid issues `iters` rounds of 16 independent
 * v_mfma_f32_16x16x32_f16; *flops_h receives the FLOPs of the launch; sink = >= 4 device bytes. */
int vip_microbench_copy(const void* src, void* dst, size_t bytes, void* stream);
/* the same probe in two more access shapes; bench.py reports the best of the three as `peak_measured`:
 * variant 0 = vip_microbench_copy, 1 = flat float4 copy (one 16-byte element per thread), 2 = one contiguous 64 KiB span per workgroup */
int vip_microbench_copy_variant(const void* src, void* dst, size_t bytes, int variant, void* stream);
int vip_microbench_mfma_f16(void* sink, int iters, double* flops_h, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIPCUP_HIP_H */
