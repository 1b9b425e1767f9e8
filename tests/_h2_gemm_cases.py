"""Shapes that select each GEMM kernel of the packed strict storage (csrc/conv_h2.hip = conv_igemm.hip with VIP_GEMM_H2) under DEFAULT
dispatch - no environment switch.  In that build a.K, a.ldx and a.Cin_g are in halfs, so every K threshold of plan() / plan_pw() /
gemm8p_eligible applies to 2 K: short_k is K <= 128, pwk_direct ends below K = 384, the 256 x 256 pwk tiles and gemm8p start
at K = 512, plan_pw picks KS = 2 ceil(K / 32) of 8.

The dry run confirms every row in tests/test_h2_dispatch_cpu.py, before any GPU time is spent: vip_conv2d_kernel_name_h2 the kernel,
vip_conv2d_kernel_variant_h2 the instantiation and its tile grid (`variant`) - both are plan() of csrc/conv_igemm.hip, the code that the
launch goes through.  A change of its rules fails that test: re-derive the shapes then, never the expected kernel."""

ALL = ("none", "gelu", "res", "res_relu")      # the epilogue families of the pointwise kernels: plain, activation, residual, residual + ReLU
NONE = ("none",)

# (M, K, N, epilogues, expected kernel, variant, what it hits)
_DENSE_ROWS = [
    (32513, 512, 256, ALL, "gemm8p_kernel", "gemm8p<pipe> 128 x 1",
     "shortest K loop the packed build sends here (2 K = 1024), exactly the 128 tiles it asks for, last m tile holds 1 row"),
    (8500, 1536, 1024, ALL, "gemm8p_kernel", "gemm8p<pipe> 34 x 4",
     "four channel tiles, long K loop, ragged last m tile (52 rows)"),
    (33000, 544, 256, NONE, "gemm8p_kernel", "gemm8p<basic> 129 x 1",
     "2 K = 1088 is a multiple of 64 but not of 128: the basic schedule, which no fp16-twin shape reaches on this storage"),
    (16400, 520, 1024, ALL, "pwk_gemm_kernel", "pwk_gemm<2,2> 65 x 4",
     "2 K = 1040 is no multiple of 64, so gemm8p declines; 260 >= 256 tiles of 256 x 256; K tail inside a chunk; 16 rows in the last m tile"),
    (257, 2048, 512, NONE, "pwk_gemm_kernel", "pwk_gemm<2,1> 2 x 4",
     "one row above rows_gemm_kernel (M <= 256): a second m tile with a single row"),
    (2500, 1536, 384, NONE, "pwk_gemm_kernel", "pwk_gemm<2,1> 10 x 3",
     "N = 384 is no multiple of 256, so it stays on 128-channel tiles; ragged M"),
    (3000, 1240, 56, NONE, "pwk_gemm_kernel", "pwk_gemm<1,1> 12 x 1",
     "N <= 64: the 64-channel tile, 8 of them empty; K tail (2 K = 2480 = 38.75 chunks; at K = 1248 the packed build has none)"),
    (12544 + 5, 376, 208, ALL, "pwk_direct_kernel", "pwk_direct<2> PT=1",
     "largest K below the 384 switch (2 K = 752, tail inside the 12th chunk), ragged N, fewer than 256 workgroups: 64-pixel tiles"),
    (777, 72, 40, NONE, "pwk_direct_kernel", "pwk_direct<1> PT=1", "N <= 64, K tail inside a chunk, 9 rows in the last tile"),
    (65535, 128, 192, NONE, "pwk_direct_kernel", "pwk_direct<2> PT=4",
     "short K, one row short of pw_gemm_kernel; 512 workgroups: 256-pixel tiles, the last one row short, a half-empty channel tile"),
    (65536 + 37, 32, 64, NONE, "pw_gemm_kernel", "pw_gemm<KS=2> 1 x 64", "the only PRE (prefetch-in-registers) instantiation"),
    (66000, 64, 136, NONE, "pw_gemm_kernel", "pw_gemm<KS=4> 1 x 192", "ragged N inside a 64-channel tile"),
    (65600, 88, 320, NONE, "pw_gemm_kernel", "pw_gemm<KS=6> 3 x 128", "K tail inside the sixth half-chunk; three channel chunks (128 + 128 + 64)"),
    (65536 + 64 * 3 + 1, 128, 192, ALL, "pw_gemm_kernel", "pw_gemm<KS=8> 2 x 128",
     "the 72 KB weight slice holds 128 rows: channel chunks of 128 + 64; one row in the last 256-pixel tile"),
    ((1 << 19) + 37, 128, 384, ("gelu",), "pw_gemm_kernel", "pw_gemm<KS=8> 2 x 192",
     "M >= 2^19 switches to the 156 KB slice: two chunks of 192 where 72 KB would give three of 128"),
]

DENSE_CASES = [(M, K, N, epi, kernel, variant, what) for M, K, N, epis, kernel, variant, what in _DENSE_ROWS for epi in epis]
DENSE_IDS = [f"{c[0]}x{c[1]}x{c[2]}-{c[3]}" for c in DENSE_CASES]

# boundary pairs of the dense dispatch: (M, K, N, expected kernel) on both sides of each switch, no epilogue
DENSE_BOUNDARIES = [
    ((256, 2048, 512, "rows_gemm_kernel"), (257, 2048, 512, "pwk_gemm_kernel")),
    ((65535, 128, 192, "pwk_direct_kernel"), (65536, 128, 192, "pw_gemm_kernel")),
    ((12549, 376, 208, "pwk_direct_kernel"), (12549, 384, 208, "pwk_gemm_kernel")),
    ((32513, 504, 256, "pwk_gemm_kernel"), (32513, 512, 256, "gemm8p_kernel")),
]

# k x k convolutions: tests/test_gpu_strict.py's CONV_CASES tuple (B, H, W, Cin, Cout, k, stride, pad(t,b,l,r), groups, act, residual),
# then the expected kernel, the variant and the reason
CONV_H2_CASES = [
    ((2, 130, 127, 32, 96, 3, 1, (1, 1, 1, 1), 1, "silu", False), "pwk_gemm_kernel(im2col)", "im2col<2>",
     "im2col staging by row count (M = 33 020 >= 32 768), not by cin_g <= 16; 96 of 128 channels; 252 rows in the last m tile"),
    # (the pointwise epilogues carry a residual only without a pre-activation, so this one has none: with one it is conv_igemm_kernel)
    ((2, 130, 127, 64, 128, 3, 1, (1, 1, 1, 1), 2, None, True), "pwk_gemm_kernel(im2col)", "im2col<1>",
     "the same map grouped (2 x 32 -> 64): the group axis of the grid, 64-channel tiles, residual epilogue"),
    ((2, 15, 15, 64, 256, 1, 2, (0, 0, 0, 0), 1, None, False), "conv_igemm_kernel", "conv_igemm<64,128>",
     "stride-2 1 x 1 shortcut: short K (2 K = 128) and Cout > 64"),
    ((2, 128, 127, 32, 96, 3, 1, (1, 1, 1, 1), 1, "silu", False), "conv_igemm_kernel", "conv_igemm<128,128>",
     "M = 32 512: 256 rows under the im2col switch, the tile kernel's largest default-dispatch launch"),
]

CONV_H2_IDS = ["x".join(str(v) for v in c[0][:9]) for c in CONV_H2_CASES]

# M = 32 512 / 33 020 for the 3 x 3 case: the first and the last row above, as a pair
CONV_BOUNDARY = (CONV_H2_CASES[3], CONV_H2_CASES[0])


# epilogue family -> (act, act_post, residual) of ops.dense / ops.conv2d
EPILOGUE = {"none": (None, None, False), "gelu": ("gelu", None, False), "res": (None, None, True), "res_relu": (None, "relu", True)}


def dense_desc(M, K, N, epi, ldw):
    """(ConvDesc, has_residual) of the launch ops.dense makes for packed [M, K] rows: what vip_conv2d_kernel_name_h2 is asked"""
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
