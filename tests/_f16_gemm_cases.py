"""Shapes that select each GEMM and convolution kernel of the fp16 storage (csrc/conv_igemm.hip; the default precision, the one bench.py
times) under DEFAULT dispatch - no environment switch.  The fp16 twin of tests/_h2_gemm_cases.py: here a.K is the logical K, so short_k
is K <= 256, pwk_direct ends below K = 768 (gated launches stay on it at any K), the 256 x 256 pwk tiles and gemm8p start at K = 1024,
plan_pw picks KS = ceil(K / 32) of {1, 2, 3, 4, 6, 8}.

The dry run confirms every row in tests/test_f16_dispatch_cpu.py, before any GPU time is spent: vip_conv2d_kernel_name the kernel,
vip_conv2d_kernel_variant the instantiation and its tile grid (`variant`) - both are plan() of csrc/conv_igemm.hip, the code that the
launch goes through.  A change of its rules fails that test: re-derive the shapes then, never the expected kernel.  The GPU tests
(test_f16_dense_kernels, test_f16_gated_conv_kernels, test_f16_conv_kernels in tests/test_gpu_ops.py) run every row against the
oracle."""
import re

from tests._h2_gemm_cases import ALL, EPILOGUE, NONE  # noqa: F401  (the epilogue families are those of the packed table)

# (M, K, N, epilogues, expected kernel, variant, what it hits)
_DENSE_ROWS = [
    (7937, 264, 1024, ALL, "pwk_direct_kernel", "pwk_direct<2> PT=4",
     "exactly the 256 workgroups (32 x 8) that switch to 256-pixel tiles; one row in the last m tile; K tail inside the fifth chunk"),
    (65300, 72, 40, NONE, "pwk_direct_kernel", "pwk_direct<1> PT=4",
     "N <= 64 needs 256 m tiles for the 256-pixel form and M stays below the pw_gemm switch; 20 rows in the last tile, 24 empty channels"),
    (65535, 256, 192, NONE, "pwk_direct_kernel", "pwk_direct<2> PT=4",
     "largest short K, one row short of pw_gemm_kernel; 512 workgroups, a half-empty channel tile"),
    (65536, 256, 192, NONE, "pw_gemm_kernel", "pw_gemm<KS=8> 2 x 128", "the other side of that switch: channel chunks of 128 + 64"),
    (9217, 264, 840, NONE, "pwk_direct_kernel", "pwk_direct<2> PT=4",
     "37 x 7 = 259 workgroups: the XCD block swizzle with remainder 3; ragged last channel tile (72 of 128); one row in the last m tile"),
    (12549, 760, 208, NONE, "pwk_direct_kernel", "pwk_direct<2> PT=1",
     "largest K below the 768 switch (tail inside the 12th chunk), 100 workgroups of 256 pixels: 64-pixel tiles"),
    (12549, 768, 208, NONE, "pwk_gemm_kernel", "pwk_gemm<2,1> 50 x 2", "the other side of the K = 768 switch"),
    (16400, 1032, 1024, ALL, "pwk_gemm_kernel", "pwk_gemm<2,2> 65 x 4",
     "K = 1032 is no multiple of 64, so gemm8p declines; 260 >= 256 tiles of 256 x 256; K tail inside a chunk; 16 rows in the last m tile"),
    (32512, 1024, 256, NONE, "pwk_gemm_kernel", "pwk_gemm<2,1> 127 x 2", "127 tiles of 256 x 256: one short of gemm8p's 128"),
    (32513, 1024, 256, NONE, "gemm8p_kernel", "gemm8p<pipe> 128 x 1",
     "shortest K loop default dispatch sends here, exactly the 128 tiles it asks for, last m tile holds 1 row"),
    (33000, 1088, 256, NONE, "gemm8p_kernel", "gemm8p<basic> 129 x 1", "K = 1088 is a multiple of 64 but not of 128: the basic schedule"),
    (8500, 1536, 1024, ALL, "gemm8p_kernel", "gemm8p<pipe> 34 x 4", "four channel tiles, long K loop, ragged last m tile (52 rows)"),
    (257, 2048, 512, NONE, "pwk_gemm_kernel", "pwk_gemm<2,1> 2 x 4",
     "one row above rows_gemm_kernel (M <= 256): a second m tile with a single row"),
    (3000, 1240, 56, NONE, "pwk_gemm_kernel", "pwk_gemm<1,1> 12 x 1", "N <= 64: the 64-channel tile, 8 of them empty; K tail (19.375 chunks)"),
    (2500, 1536, 384, NONE, "pwk_gemm_kernel", "pwk_gemm<2,1> 10 x 3",
     "N = 384 is no multiple of 256, so it stays on 128-channel tiles; ragged M"),
]

DENSE_CASES = [(M, K, N, epi, kernel, variant, what) for M, K, N, epis, kernel, variant, what in _DENSE_ROWS for epi in epis]
DENSE_IDS = [f"{c[0]}x{c[1]}x{c[2]}-{c[3]}" for c in DENSE_CASES]

# boundary pairs of the dense dispatch: (M, K, N, expected kernel) on both sides of each switch, no epilogue
DENSE_BOUNDARIES = [
    ((256, 2048, 512, "rows_gemm_kernel"), (257, 2048, 512, "pwk_gemm_kernel")),
    ((65535, 256, 192, "pwk_direct_kernel"), (65536, 256, 192, "pw_gemm_kernel")),
    ((12549, 760, 208, "pwk_direct_kernel"), (12549, 768, 208, "pwk_gemm_kernel")),
    ((32512, 1024, 256, "pwk_gemm_kernel"), (32513, 1024, 256, "gemm8p_kernel")),
]

# squeeze-excite gated 1 x 1 convolutions on 7 x 7 maps (gate_hw = 49: a 256-pixel tile spans six images), each run without and with a
# residual: (B, K, N, expected kernel, variant, what it hits)
GATE_HW = (7, 7)
_GATED_ROWS = [
    (163, 672, 1024, "pwk_direct_kernel", "pwk_direct<2,gated> PT=4",
     "M = 7987: exactly 256 workgroups (32 x 8); 51 rows in the last m tile; K tail inside the 11th chunk"),
    (445, 1632, 272, "pwk_direct_kernel", "pwk_direct<2,gated> PT=4",
     "M = 21805: the gated deep-K loop (K >= 768 reaches this kernel only with a gate), 86 x 3 = 258 workgroups, 16 of 128 channels in "
     "the last channel tile"),
    (1333, 72, 40, "pwk_direct_kernel", "pwk_direct<1,gated> PT=4",
     "M = 65317: the 64-channel gated form on 256-pixel tiles (the ensemble's first MBConv projections), 256 m tiles, K tail"),
]
GATED_CASES = [(B, K, N, res, kernel, variant, what) for B, K, N, kernel, variant, what in _GATED_ROWS for res in (False, True)]
GATED_IDS = [f"{c[0]}x7x7x{c[1]}-{c[2]}{'-res' if c[3] else ''}" for c in GATED_CASES]


def gated_case(B, K, N, res):
    """a gated row as a CONV_CASES tuple"""
    return (B, GATE_HW[0], GATE_HW[1], K, N, 1, 1, (0, 0, 0, 0), 1, None, res)


# k x k convolutions: tests/test_gpu_ops.py's CONV_CASES tuple (B, H, W, Cin, Cout, k, stride, pad(t,b,l,r), groups, act, residual),
# then the expected kernel, the variant and the reason
CONV_F16_CASES = [
    ((2, 130, 127, 32, 96, 3, 1, (1, 1, 1, 1), 1, "silu", False), "pwk_gemm_kernel(im2col)", "im2col<2>",
     "im2col staging by row count (M = 33 020 >= 32 768), not by cin_g <= 16; 96 of 128 channels; 252 rows in the last m tile"),
    # (the pointwise epilogues carry a residual only without a pre-activation, so this one has none: with one it is conv_igemm_kernel)
    ((2, 130, 127, 64, 128, 3, 1, (1, 1, 1, 1), 2, None, True), "pwk_gemm_kernel(im2col)", "im2col<1>",
     "the same map grouped (2 x 32 -> 64): the group axis of the grid over 129 m blocks, 64-channel tiles, residual epilogue"),
    ((2, 128, 127, 32, 96, 3, 1, (1, 1, 1, 1), 1, "silu", False), "conv_igemm_kernel", "conv_igemm<128,128>",
     "M = 32 512: 256 rows under the im2col switch, the tile kernel's largest default-dispatch launch without a residual"),
    ((2, 15, 15, 64, 256, 1, 2, (0, 0, 0, 0), 1, None, False), "conv_igemm_kernel", "conv_igemm<64,128>",
     "stride-2 1 x 1 shortcut: short K (64) and Cout > 64"),
    ((2, 258, 256, 24, 96, 2, 2, (0, 0, 0, 0), 1, None, False), "pwk_gemm_kernel(im2col)", "im2col<2>",
     "2 x 2 / 2 downsample, M = 33 024, cin_g = 24: K = 96: taps of 24 channels that do not line up with the 64-k chunks, K tail"),
    ((2, 130, 127, 32, 96, 3, 1, (1, 1, 1, 1), 1, "silu", True), "conv_igemm_kernel", "conv_igemm<128,128>",
     "activation + residual, the one epilogue the pointwise kernels do not carry: the tile kernel at 33 020 rows, past the im2col switch"),
    ((2, 259, 257, 64, 192, 3, 2, (0, 1, 0, 1), 2, "silu", False), "pwk_gemm_kernel(im2col)", "im2col<2>",
     "grouped (2 x 32 -> 96), stride 2, TF SAME padding on an odd map (bottom / right only), M = 33 024 with cin_g = 32: the row count and "
     "not the stem rule selects it; group axis x 129 m blocks, 96 of 128 channels"),
]
CONV_F16_IDS = ["x".join(str(v) for v in c[0][:9]) + ("-res" if c[0][10] else "") for c in CONV_F16_CASES]

# M = 32 512 / 33 020 for the 3 x 3 case, as a pair
CONV_BOUNDARY = (CONV_F16_CASES[2], CONV_F16_CASES[0])

# the four tile shapes of conv_igemm_kernel: reached jointly by test_gpu_ops.CONV_CASES and by test_dense (GELU AND a residual, which no
# pointwise kernel carries) - the existing case that reaches each, as a CONV_CASES tuple, for the dry run
IGEMM_ROWS = [
    ((1, 20, 20, 24, 40, 3, 1, (1, 1, 1, 1), 1, "gelu", False), "conv_igemm<64,64>", "CONV_CASES"),
    ((2, 12, 10, 32, 64, 3, 1, (1, 1, 1, 1), 1, "relu", False), "conv_igemm<128,64>", "CONV_CASES"),
    ((1000, 1, 1, 256, 768, 1, 1, (0, 0, 0, 0), 1, "gelu", True), "conv_igemm<64,128>", "DENSE_SHAPES"),
    ((2, 13, 13, 128, 128, 3, 2, (1, 1, 1, 1), 1, "silu", False), "conv_igemm<128,128>", "CONV_CASES"),
]

# every instantiation the fp16 hot path reaches: what the rows above, with the existing case lists of tests/test_gpu_ops.py (PW_CASES,
# FEW_ROWS_SHAPES, GATED_CASES, IGEMM_ROWS), must cover
INSTANTIATIONS = {
    "rows_gemm", "pw_gemm<KS=1>", "pw_gemm<KS=2>", "pw_gemm<KS=3>", "pw_gemm<KS=4>", "pw_gemm<KS=6>", "pw_gemm<KS=8>",
    "gemm8p<pipe>", "gemm8p<basic>", "pwk_direct<1> PT=4", "pwk_direct<2> PT=4", "pwk_direct<2> PT=1", "pwk_direct<1,gated> PT=1",
    "pwk_direct<2,gated> PT=1", "pwk_direct<1,gated> PT=4", "pwk_direct<2,gated> PT=4", "pwk_gemm<1,1>", "pwk_gemm<2,1>", "pwk_gemm<2,2>",
    "im2col<1>", "im2col<2>", "conv_igemm<64,64>", "conv_igemm<128,64>", "conv_igemm<64,128>", "conv_igemm<128,128>",
}


def dense_desc(M, K, N, epi, ldw):
    """(ConvDesc, has_residual) of the launch ops.dense makes for fp16 [M, K] rows: what vip_conv2d_kernel_name is asked"""
    from vipcup_amd import _abi, ops
    act, post, res = EPILOGUE[epi]
    return _abi.ConvDesc(B=M, H=1, W=1, Cin=K, Cout=N, kh=1, kw=1, sh=1, sw=1, pt=0, pl=0, Ho=1, Wo=1, groups=1, ldx=K, cin_off=0, ldy=N,
                         cout_off=0, ldr=N if res else 0, res_off=0, ldw=ldw, act_pre=ops._act(act), act_post=ops._act(post)), res


def conv_desc(case, ldw):
    """the same for a CONV_CASES tuple (ops.conv2d: act is the pre-activation, the residual is added after it)"""
    from vipcup_amd import _abi, ops
    B, H, W, Cin, Cout, k, s, pad, groups, act, use_res = case
    Ho, Wo = ops._out_hw(H, W, k, k, s, s, pad)
    return _abi.ConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, kh=k, kw=k, sh=s, sw=s, pt=pad[0], pl=pad[2], Ho=Ho, Wo=Wo, groups=groups,
                         ldx=Cin, cin_off=0, ldy=Cout, cout_off=0, ldr=Cout if use_res else 0, res_off=0, ldw=ldw, act_pre=ops._act(act),
                         act_post=0), use_res


def instantiation(variant):
    """a variant string without its tile grid: 'pwk_gemm<2,2> 65 x 4' -> 'pwk_gemm<2,2>'; 'pwk_direct<2> PT=4' stays (PT is a template
    argument)"""
    return re.sub(r" \d+ x \d+$", "", variant)


def same_kernel(name, variant):
    """do the name query and the variant query speak of one kernel?  'gemm8p_kernel' and 'gemm8p<pipe> 34 x 4', 'pwk_gemm_kernel(im2col)'
    and 'im2col<2>'"""
    family = re.match(r"\w+", variant).group(0)
    return name == ("pwk_gemm_kernel(im2col)" if family == "im2col" else family + "_kernel")
