"""Results must not depend on what else the chip is running.  Round 2's window-attention kernel was bit-exact alone and wrong (|d| up to
1.0 on a few 16-query blocks, deterministic values) whenever waves of another MFMA-heavy kernel shared its SIMDs - which is what the
ensemble's three member streams do all the time, and what made pipelined and joined bench steps differ (DESIGN.md section 8.6 of round 2;
found with tools/stress_determinism.py -> tools/bisect_determinism.py -> tools/race_matrix.py).  Every MFMA kernel family of the
library is launched here on one stream while a second stream keeps the matrix pipes busy, and compared BIT FOR BIT with its solo result."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tools.make_synth import synth_jpeg  # noqa: E402


# launches per kernel family next to the co-runner (round 3 sampled 12; the wrong tiles of the old window-attention kernel showed up in
# 39 of 40 launches, a rarer failure needs more)
N_CO = int(os.environ.get("VIP_CONCURRENCY_ITERS", "200"))


def _victims():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    g = torch.Generator().manual_seed(3)

    def r(*shape):
        return torch.randn(*shape, generator=g).to(torch.float16).cuda()

    qkv14, tab14 = r(64, 14, 14, 768), (torch.randn(27 * 27, 8, generator=g) * 0.5).cuda()
    qkv14g, qg14 = r(64, 14, 14, 512), r(64, 196, 256)
    qkv7, tab7 = r(16, 56, 56, 192), (torch.randn(13 * 13, 2, generator=g) * 0.5).cuda()
    qkvm = r(32, 197, 3 * 384)
    xm = r(64 * 56 * 56, 96)
    f1 = ops.make_dense_weight(torch.randn(96, 384, generator=g) / 10, torch.zeros(384))
    f2 = ops.make_dense_weight(torch.randn(384, 96, generator=g) / 20, torch.zeros(96))
    xg = r(50176, 256)
    cw = ops.make_dense_weight(torch.randn(256, 768, generator=g) / 16, torch.zeros(768))
    xc3 = r(64, 50, 50, 64)
    cw3 = ops.make_conv_weight(torch.randn(3, 3, 64, 64, generator=g) / 24, torch.zeros(64))
    wsk = torch.randn(1, 1, 256, 256, generator=g) / 16
    with ops.precision("f32"):
        cws = ops.make_conv_weight(wsk, torch.zeros(256))
    with ops.precision("strict"):
        cwh = ops.make_conv_weight(wsk, torch.zeros(256))
        f1h = ops.make_dense_weight(torch.randn(96, 384, generator=g) / 10, torch.zeros(384))
        f2h = ops.make_dense_weight(torch.randn(384, 96, generator=g) / 20, torch.zeros(96))
        cw8h = ops.make_dense_weight(torch.randn(768, 256, generator=g) / 28, torch.zeros(256))
    lnh = (torch.ones(96).cuda(), torch.zeros(96).cuda(), 1e-6)
    gateh = ops.pack_h2(torch.rand(64, 256, generator=g).cuda())
    dw7 = ops.make_dw_weight(torch.randn(7, 7, 256, 1, generator=g) / 7)
    x8h = ops.pack_h2(torch.randn(36864, 768, generator=g).cuda())
    xs32 = torch.randn(64, 14, 14, 256, generator=g).cuda()
    xsh = ops.pack_h2(xs32)
    xmh = ops.pack_h2(torch.randn(64 * 56 * 56, 96, generator=g).cuda())
    qkv14h, qkv7h, qkvmh = ops.pack_h2(qkv14.float()), ops.pack_h2(qkv7.float()), ops.pack_h2(qkvm.float())
    xb = r(16, 56, 56, 64)
    lnb = (torch.ones(64).cuda(), torch.zeros(64).cuda(), 1e-5)
    cq3 = ops.make_dense_weight(torch.randn(64, 192, generator=g) / 8, torch.zeros(192))
    cq2 = ops.make_dense_weight(torch.randn(64, 128, generator=g) / 8, torch.zeros(128))
    cpj = ops.make_dense_weight(torch.randn(64, 64, generator=g) / 8, torch.zeros(64))
    qgb = r(16, 49, 64)
    xb1, tab7b = r(16, 28, 28, 128), (torch.randn(13 * 13, 4, generator=g) * 0.5).cuda()
    lnb1 = (torch.ones(128).cuda(), torch.zeros(128).cuda(), 1e-5)
    cq31 = ops.make_dense_weight(torch.randn(128, 384, generator=g) / 11, torch.zeros(384))
    cpj1 = ops.make_dense_weight(torch.randn(128, 128, generator=g) / 11, torch.zeros(128))
    xb2 = r(24, 14, 14, 256)
    lnb2 = (torch.ones(256).cuda(), torch.zeros(256).cuda(), 1e-5)
    cq32 = ops.make_dense_weight(torch.randn(256, 768, generator=g) / 16, torch.zeros(768))
    cq22 = ops.make_dense_weight(torch.randn(256, 512, generator=g) / 16, torch.zeros(512))
    cpj2 = ops.make_dense_weight(torch.randn(256, 256, generator=g) / 16, torch.zeros(256))
    qgb2 = r(24, 196, 256)
    # packed instantiations with no other entry here, at their rows of tests/_h2_gemm_cases.py: 256 x 256 pwk tiles, and the direct
    # kernel on 256-pixel tiles ("strict conv (h2 pwk)" above is its 64-pixel form)
    with ops.precision("strict"):
        cw22h = ops.make_dense_weight(torch.randn(520, 1024, generator=g) / 23, torch.zeros(1024))
        cwd2h = ops.make_dense_weight(torch.randn(128, 192, generator=g) / 11, torch.zeros(192))
    x22h = ops.pack_h2(torch.randn(16400, 520, generator=g).cuda())
    xd2h = ops.pack_h2(torch.randn(65535, 128, generator=g).cuda())
    from vipcup_amd import _abi
    exp = {}
    if _abi.lib().vip_experiments_built():          # the opt-in 14 x 14-window fused block (experiments build)
        exp = {"gcvit_attn_block ws14": lambda: ops.gcvit_attn_block(xb2, None, lnb2, cq32, cpj2, tab14, 8, 14, 32 ** -0.5),
               "gcvit_attn_block ws14 gq": lambda: ops.gcvit_attn_block(xb2, qgb2, lnb2, cq22, cpj2, tab14, 8, 14, 32 ** -0.5)}
    return {
        **exp,
        "gcvit_attn_block C128": lambda: ops.gcvit_attn_block(xb1, None, lnb1, cq31, cpj1, tab7b, 4, 7, 32 ** -0.5),
        "gcvit_attn_block (fused)": lambda: ops.gcvit_attn_block(xb, None, lnb, cq3, cpj, tab7, 2, 7, 32 ** -0.5),
        "gcvit_attn_block global q": lambda: ops.gcvit_attn_block(xb, qgb, lnb, cq2, cpj, tab7, 2, 7, 32 ** -0.5),
        "window_attn ws14": lambda: ops.window_attention(qkv14, None, tab14, 8, 14, 32 ** -0.5),
        "window_attn ws14 global": lambda: ops.window_attention(qkv14g, qg14, tab14, 8, 14, 32 ** -0.5),
        "window_attn ws7": lambda: ops.window_attention(qkv7, None, tab7, 2, 7, 32 ** -0.5),
        "mhsa": lambda: ops.mhsa(qkvm, 6, 0.125),
        "mlp_fused": lambda: ops.mlp(xm, f1, f2, act="gelu", residual=xm),
        "pwk gemm + gelu": lambda: ops.dense(xg, cw, act="gelu"),
        "conv3x3": lambda: ops.conv2d(xc3, cw3, pad=(1, 1, 1, 1), act="relu"),
        "f32 conv": lambda: ops.conv2d(xs32, cws, act="gelu"),
        # the packed strict storage: the same GEMM kernel family with three MFMAs per fragment pair, and its MFMA attention cores
        "strict conv (h2 pwk)": lambda: ops.conv2d(xsh, cwh, act="gelu"),
        "strict dense (h2 pw_gemm)": lambda: ops.dense(xmh, f1h, act="gelu"),
        "strict window_attn ws14 (h2)": lambda: ops.window_attention(qkv14h, None, tab14, 8, 14, 32 ** -0.5),
        "strict window_attn ws7 (h2)": lambda: ops.window_attention(qkv7h, None, tab7, 2, 7, 32 ** -0.5),
        "strict mhsa (h2)": lambda: ops.mhsa(qkvmh, 6, 0.125),
        # round 4: the fused LayerNorm-MLP, the gate inside the GEMM operand, the LDS-staged depthwise kernel, gemm8p on the packed storage
        "strict mlp fused (h2)": lambda: ops.mlp(xmh, f1h, f2h, act="gelu", residual=xmh, ln=lnh),
        "strict gated conv (h2)": lambda: ops.conv2d(xsh, cwh, gate=gateh),
        "strict dwconv 7x7 (h2 lds)": lambda: ops.dwconv2d(xsh, dw7, None, 7, 1, (3, 3, 3, 3)),
        "strict dense (h2 gemm8p)": lambda: ops.dense(x8h, cw8h),
        "strict dense (h2 pwk_gemm<2,2>)": lambda: ops.dense(x22h, cw22h, act="gelu"),
        "strict dense (h2 pwk_direct<2>)": lambda: ops.dense(xd2h, cwd2h),
    }


def test_kernels_are_bit_exact_next_to_a_busy_matrix_pipe(report, monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, ops
    monkeypatch.setattr(ops, "_GCVIT_BLOCK14", True)          # the opt-in ws 14 fused block is a victim too
    lib = _abi.lib()
    sink = torch.zeros((16,), dtype=torch.float32, device="cuda")
    flops = C.c_double(0.0)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    bad = {}
    for name, fn in _victims().items():
        ref = fn().clone()
        torch.cuda.synchronize()
        n_bad, worst = 0, 0.0
        for _ in range(N_CO):
            with torch.cuda.stream(sb):      # 4 waves per SIMD of back-to-back v_mfma_f32_16x16x32_f16, nothing else
                _abi.check(lib.vip_microbench_mfma_f16(sink.data_ptr(), 300, C.byref(flops), sb.cuda_stream), "vip_microbench_mfma_f16")
            with torch.cuda.stream(sa):
                out = fn()
            torch.cuda.synchronize()
            if not torch.equal(out, ref):
                n_bad += 1
                worst = max(worst, float((out.float() - ref.float()).abs().max()))
        report(f"[concurrency] {name:30s} next to an MFMA-saturating kernel: {n_bad} of {N_CO} launches differ from the solo result"
               + (f" (max |d| {worst:.2e})" if n_bad else ""))
        if n_bad:
            bad[name] = (n_bad, worst)
    assert not bad, f"results depend on the co-running kernel: {bad}"


def test_pipelined_bench_steps_are_bit_reproducible(report):
    """30 pipelined steps of the config-4 workload (three member streams, next step forked before the previous one is joined, mixed-size
    batch): every member's scores bit-identical to a joined reference step"""
    import vipcup_amd  # noqa: F401
    from tests import _parity as P
    from vipcup_amd import workloads
    raws = [synth_jpeg(100 + i) for i in range(15)] + [synth_jpeg(149)]
    wl = workloads.build("ensemble4", batch=16, jpegs=raws, models=[P.gpu_member(k) for k in workloads.member_list("ensemble4")])
    wl.step()
    wl.step()
    ref = wl.member_scores.clone()
    diffs = 0
    for _ in range(30):
        if wl.step(pipelined=True) is not None:
            diffs += int(not torch.equal(wl.member_scores, ref))
    wl.flush()
    diffs += int(not torch.equal(wl.member_scores, ref))
    report(f"[concurrency] ensemble4, 30 pipelined steps vs a joined step: {diffs} differ")
    wl.close()
    assert diffs == 0
