"""Rows and operands of the output-gated epilogue (vip_conv2d_out_gated_nhwc_f16: modes 7 / 8 of pw_gemm_kernel and pwk_direct_kernel,
csrc/conv_igemm.hip), shared by tests/test_gpu_out_gate.py and tests/test_se_tail_cpu.py.

One row per instantiation the mode is built for.  The shapes are those of tests/_f16_gemm_cases.py moved onto 7 x 7 maps (its GATE_HW:
hw = 49 is no multiple of the 16-row MFMA tile, so tiles straddle image boundaries, and no B x 49 is a multiple of the 256-row block
tile, so the last tile is ragged): pwk_direct<2> PT=4 at the 256 workgroups of its (7937, 264, 1024) row, pwk_direct<1> PT=4 at the
1333 images of its gated 64-channel row, pw_gemm without a second weight term one image past M = 65 536; the instantiations the table
reaches only at larger shapes than they need (64-pixel tiles, two-term weights at any M) run on 11 images, three block tiles."""
import torch

from tests._f16_gemm_cases import GATE_HW, conv_desc, gated_case, instantiation  # noqa: F401

# (B, K, N, two-term weights, instantiation, what it hits)
ROWS = [
    (11, 24, 64, True, "pw_gemm<KS=1,hilo>", "one k-step with a K tail; 3 block tiles, 27 rows in the last"),
    (11, 56, 136, True, "pw_gemm<KS=2,hilo>", "ResNet-RS stage 1's kernel; ragged last channel tile (8 of 64)"),
    (11, 88, 64, True, "pw_gemm<KS=3,hilo>", "three k-steps: the gated form runs without the next-tile prefetch"),
    (11, 120, 72, True, "pw_gemm<KS=4,hilo>", "ResNet-RS stage 2's kernel; 8 channels in the second sub-tile"),
    (1338, 24, 40, False, "pw_gemm<KS=1>", "M = 65 562: 26 rows past the pw_gemm switch, 257 tiles on a persistent grid"),
    (1338, 56, 64, False, "pw_gemm<KS=2>", "the stage-1 layer without its second weight term"),
    (1338, 88, 40, False, "pw_gemm<KS=3>", "three k-steps, one weight term"),
    (1338, 120, 72, False, "pw_gemm<KS=4>", "the largest K the gated streaming kernel takes (128)"),
    (11, 72, 40, False, "pwk_direct<1> PT=1", "64-channel tile on 64-pixel workgroups, 24 empty channels, K tail"),
    (11, 264, 200, False, "pwk_direct<2> PT=1", "ragged last channel tile (72 of 128), K tail inside the fifth chunk"),
    (1333, 72, 40, False, "pwk_direct<1> PT=4", "M = 65 317: 256 m tiles of 256 pixels, five image boundaries per tile"),
    (162, 264, 1024, False, "pwk_direct<2> PT=4", "ResNet-RS stage 3 / 4's kernel: exactly 256 workgroups (32 x 8), XCD swizzle"),
]
IDS = [f"{r[0]}x7x7x{r[1]}-{r[2]}{'-hilo' if r[3] else ''}" for r in ROWS]

# what declines (the caller then runs conv2d + scale_add_act): (B, H, W, K, N, k, two-term weights, reason)
DECLINED = [
    (11, 7, 7, 184, 64, 1, True, "pw_gemm KS = 6: K > 128 on the streaming kernel"),
    (11, 7, 7, 256, 64, 1, True, "pw_gemm KS = 8"),
    (1338, 7, 7, 256, 192, 1, False, "pw_gemm KS = 8 by row count"),
    (11, 7, 7, 768, 208, 1, False, "pwk_gemm_kernel (K >= 768)"),
    (700, 7, 7, 1024, 256, 1, False, "gemm8p_kernel"),
    (2, 130, 127, 64, 128, 3, False, "k x k: im2col staging"),
    (2, 13, 13, 64, 64, 3, False, "k x k: the tile kernel"),
]


def desc(B, K, N, relu, ldw, k=1, H=GATE_HW[0], W=GATE_HW[1]):
    """the ConvDesc of the gated launch: a residual of the output's own width, act_post none / ReLU"""
    from vipcup_amd import ops
    d, _ = conv_desc((B, H, W, K, N, k, 1, ((k - 1) // 2,) * 4, 1, None, True), ldw)
    d.act_post = ops._act("relu" if relu else None)
    return d


def exact_operands(B, K, N, hilo):
    """Operands for which every partial sum of ``(x . W + b) * g + r`` is exact in fp32 (and so the fp16 result is ONE rounding of the
    exact value, whatever the summation order): x in {-2..2}, r in {-8..8}, b in {-3..3}, and
      * two-term rows: W = i + j 2^-12, i in {-2..2}, j in {-1, 0, 1} (hi = fp16(W) and lo = fp16(W - hi) carry it exactly), the gate a
        power of two 2^a: sums are multiples of 2^-12 below 2^11 (23 bits), scaled exactly;
      * one-term rows: W = i, the gate 2^a (1 + 2^-12) on BOTH planes (hi = 2^a, lo = 2^(a-12)): integer sums below 2^11 times a
        13-bit gate (24 bits).
    a = -2..3 varies with image and channel (neighbouring images and neighbouring channels never share a gate).
    -> fp32 tensors x [B,7,7,K], w [1,1,K,N], b [N], gate planes [B,2,N], r [B,7,7,N]"""
    H, W = GATE_HW
    g = torch.Generator().manual_seed(B * 100003 + K * 1009 + N)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()
    x = ints(-2, 2, B, H, W, K)
    w = ints(-2, 2, 1, 1, K, N)
    if hilo:
        w = w + ints(-1, 1, 1, 1, K, N) * 2.0 ** -12
    b = ints(-3, 3, N)
    r = ints(-8, 8, B, H, W, N)
    a = ((torch.arange(B)[:, None] * 5 + torch.arange(N)[None, :] * 3) % 6 - 2).float()
    hi = torch.pow(2.0, a)
    lo = torch.zeros_like(hi) if hilo else hi * 2.0 ** -12
    return x, w, b, torch.stack([hi, lo], 1), r


def random_operands(B, K, N, hilo=False):
    """seeded fp16-representable operands at the scales of tests/test_gpu_ops.py's rows (two-term rows: the weights as fp16(w) +
    fp16(w - fp16(w)), what ``make_conv_weight(hilo=True)`` stores), the gate an fp32 value in (0, 1) as two planes"""
    H, W = GATE_HW
    g = torch.Generator().manual_seed(B + K + N)

    def h16(t):
        return t.to(torch.float16).to(torch.float32)
    x = h16(torch.randn(B, H, W, K, generator=g))
    w = torch.randn(1, 1, K, N, generator=g) / K ** 0.5
    w = h16(w) + h16(w - h16(w)) if hilo else h16(w)
    b = torch.randn(N, generator=g) * 0.1
    r = h16(torch.randn(B, H, W, N, generator=g))
    gate = torch.rand(B, N, generator=g)
    hi = h16(gate)
    lo = h16(gate - hi)
    return x, w, b, torch.stack([hi, lo], 1), r


def reference(x, w, b, planes, r, relu):
    """fp64: post((x . W + b) * (hi + lo) + r)"""
    y = x.double().reshape(-1, x.shape[-1]) @ w.double()[0, 0] + b.double()
    y = y.reshape(*x.shape[:3], -1) * (planes[:, 0].double() + planes[:, 1].double())[:, None, None, :] + r.double()
    return y.clamp_min(0) if relu else y
