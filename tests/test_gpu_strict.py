"""GPU parity of the two STRICT precision modes against the fp32 CPU oracle - every operator at fp32 round-off, every ensemble member's
CALIBRATED logit within BASELINE.json's 1e-3 (the fp16 path sits at its storage floor, tests/_parity.py):
  "strict": packed fp16 (hi, lo) pair storage, three fp16 MFMAs per fragment pair (csrc/conv_h2.hip = the fast path's GEMM kernels
            instantiated for this storage, csrc/strict_ops.hip<SH2>) - the default of --precision strict since round 4;
  "f32":    fp32 storage, f32-quality matrix arithmetic (csrc/strict_conv.hip, strict_ops.hip<SF32>) - round 3's strict mode."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gcvit_ref  # noqa: E402
from oracle import ops_ref as R  # noqa: E402
from tests import _h2_gemm_cases as T  # noqa: E402
from tests import _parity as P  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402

N_IMG = int(os.environ.get("VIP_E2E_N", "16"))   # as tests/test_gpu_e2e.py
TOL_OP = 2e-5        # relative to the output scale: fp32 summation order over K <= 4608 terms, 3e-7 absolute in exp / erf against torch's


def _ops():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    return ops


MODES = ["strict", "f32"]


def dev(t):
    """a PARAMETER (fp32 in both modes)"""
    return t.to(torch.float32).cuda().contiguous()


def A(t, mode):
    """an ACTIVATION in the mode's storage"""
    d = dev(t)
    return _ops().pack_h2(d) if mode == "strict" else d


def check(report, name, got, ref, tol=TOL_OP):
    if got.dtype == torch.int32:
        got = _ops().unpack_h2(got)
        _ops().h2_check(name)
    got = got.float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = ref.abs().max().item() + 1e-6
    err = (got - ref).abs().max().item()
    report(f"[strict-ops] {name}: max_abs_err={err:.3e} ref_absmax={scale:.3e} rel={err / scale:.3e}")
    assert torch.isfinite(got).all(), name
    assert err <= tol * scale, f"{name}: err {err} > {tol}*{scale}"


CONV_CASES = [
    # B, H, W, Cin, Cout, k, stride, pad(t,b,l,r), groups, act, residual
    (2, 9, 9, 8, 32, 3, 2, (1, 1, 1, 1), 1, "relu", False),       # stem-like: Cin=8, K=72 (partial k chunk), 32-channel tile
    (2, 12, 10, 32, 64, 3, 1, (1, 1, 1, 1), 1, "relu", False),    # 3x3 same, 64-channel tile
    (3, 7, 7, 64, 256, 1, 1, (0, 0, 0, 0), 1, None, True),        # 1x1 + residual, 128-channel tile x 2
    (2, 13, 13, 128, 128, 3, 2, (1, 1, 1, 1), 1, "silu", False),  # stride 2 odd size
    (1, 20, 20, 24, 40, 3, 1, (1, 1, 1, 1), 1, "gelu", False),    # ragged channels (40 of a 64 tile), K = 216
    (2, 8, 8, 128, 128, 3, 1, (1, 1, 1, 1), 2, "relu", False),    # grouped (NFNet / ResNeSt style)
    (2, 10, 10, 16, 200, 4, 2, (0, 0, 0, 0), 1, None, False),     # 4x4/2 VALID patchify, Cout = 200 (128 + 72)
    (2, 6, 6, 512, 72, 1, 1, (0, 0, 0, 0), 1, "sigmoid", False),  # deep K, narrow N
    (1, 33, 31, 64, 64, 3, 1, (1, 1, 1, 1), 1, "relu", True),     # M tail (1023 pixels)
    (2, 9, 9, 64, 64, 5, 1, (2, 2, 2, 2), 1, None, False),        # 5x5
    (2, 9, 9, 96, 96, 2, 2, (0, 0, 0, 0), 1, None, False),        # 2x2/2 downsample (ConvNeXt)
    (2, 9, 9, 32, 32, 3, 2, (0, 1, 0, 1), 1, "silu", False),      # TF SAME asymmetric pad (EffNetV1)
    (256, 1, 1, 2048, 512, 1, 1, (0, 0, 0, 0), 1, "relu", False),  # squeeze-excite Dense: M = batch
    (2, 16, 16, 12, 8, 1, 1, (0, 0, 0, 0), 1, None, False),       # Cin = 12 (K tail inside a float4 group of the chunk), Cout 8
]


@pytest.mark.parametrize("gemm", ["h2", "bf16x3", "f32", "bf16x2"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(v) for v in c[:9]))
def test_conv2d_strict(case, gemm, report, monkeypatch):
    """the STRICT GEMM arithmetics: "h2" = packed fp16 pairs, three fp16 MFMAs (precision "strict"); in precision "f32": three-term bf16
    splits on six bf16 MFMAs (the default there) and the f32-input MFMA - all f32 quality, 2e-5 - and the opt-in two-term bf16 split
    (three MFMAs, 2^-17 of each product dropped: held to 1e-4 of the output scale)"""
    ops = _ops()
    mode = "strict" if gemm == "h2" else "f32"
    if gemm != "h2":
        monkeypatch.setattr(ops, "STRICT_GEMM", gemm)
    B, H, W, Cin, Cout, k, s, pad, groups, act, use_res = case
    if mode == "strict" and ((Cin // groups) % 8 or (Cout // groups) % 8):
        pytest.skip("packed storage: channel counts are multiples of 8 (models pad, as on the fp16 path)")
    g = torch.Generator().manual_seed(hash(case[:9]) % (2 ** 31))
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(k, k, Cin // groups, Cout, generator=g) / math.sqrt(k * k * Cin / groups)
    bias = torch.randn(Cout, generator=g) * 0.1
    ref = R.act(R.conv2d(x, w, bias, s, pad, groups), act)
    res = None
    if use_res:
        res = torch.randn(*ref.shape, generator=g)
        ref = ref + res
    with ops.precision(mode):
        cw = ops.make_conv_weight(w, bias, groups=groups)
    assert cw.kind == ("h2" if mode == "strict" else "s32")
    got = ops.conv2d(A(x, mode), cw, stride=s, pad=pad, act=act, residual=None if res is None else A(res, mode))
    torch.cuda.synchronize()
    assert got.dtype == ops.act_dtype(mode)
    check(report, f"conv2d[{gemm}] {case}", got, ref, tol=1e-4 if gemm == "bf16x2" else TOL_OP)


@pytest.mark.parametrize("mode", MODES)
def test_conv2d_strict_channel_slices_and_gate(mode, report):
    """cin_off / cout_off (concat-free splits and joins), act_post after the residual, and a squeeze-excite gate"""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 11, 9, 96, generator=g)
    w = torch.randn(1, 1, 32, 48, generator=g) / math.sqrt(32)
    b = torch.randn(48, generator=g) * 0.1
    res = torch.randn(2, 11, 9, 48, generator=g)
    with ops.precision(mode):
        cw = ops.make_conv_weight(w, b)
    out = torch.zeros((2, 11, 9, 112), dtype=ops.act_dtype(mode), device="cuda")       # all-zero bits are 0.0 in both storages
    ops.conv2d(A(x, mode), cw, residual=A(res, mode), act_post="relu", out=out, cin_off=32, cout_off=64)
    ref = torch.relu(R.conv2d(x[..., 32:64], w, b) + res)
    full = ops.unpack_h2(out) if mode == "strict" else out
    check(report, "conv2d slices", full[..., 64:112].contiguous(), ref)
    assert float(full[..., :64].abs().max()) == 0.0
    gate = torch.rand(2, 32, generator=g)
    x2 = torch.randn(2, 5, 5, 32, generator=g)
    got = ops.conv2d(A(x2, mode), cw, gate=A(gate, mode))
    check(report, "conv2d gate", got, R.conv2d(x2 * gate[:, None, None, :], w, b))


@pytest.mark.parametrize("M,K,N,act,res", [(16384 + 37, 256, 768, "gelu", False), (20000, 192, 320, None, True), (16500, 128, 256, None, False),
                                           (17000, 200, 1024, "silu", False), (16384, 72, 384, None, True)])
def test_dense_pwx_h2(M, K, N, act, res, report, monkeypatch):
    """the activation-resident short-K / wide-N kernel on the packed storage (pwx_kernel: 4 / 6 / 8 half-chunks of K, 32 or 16 pixels per
    wave), K tails, a half-empty last channel tile, ragged M"""
    monkeypatch.setenv("VIP_PWX", "1")          # an experiment, off by default; read per call
    ops = _ops()
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g)
    w, b = torch.randn(K, N, generator=g) / math.sqrt(K), torch.randn(N, generator=g) * 0.1
    r = torch.randn(M, N, generator=g) if res else None
    with ops.precision("strict"):
        cw = ops.make_dense_weight(w, b)
    d = ops._abi.ConvDesc(B=M, H=1, W=1, Cin=K, Cout=N, kh=1, kw=1, sh=1, sw=1, pt=0, pl=0, Ho=1, Wo=1, groups=1, ldx=K, cin_off=0, ldy=N,
                          cout_off=0, ldr=N if res else 0, res_off=0, ldw=cw.ldw, act_pre=ops._act(act), act_post=0)
    assert ops.conv_kernel_name_h2(d, res) == "pwx_kernel"
    got = ops.dense(A(x, "strict"), cw, act=act, residual=A(r, "strict") if res else None)
    check(report, f"dense pwx {M}x{K}x{N}", got, R.act(R.dense(x, w, b), act) + (r if res else 0))


def check_worst(report, name, got, ref, tol=TOL_OP):
    """check() for a packed result that also names the row and channel of its worst element, so that a failure points at its tile"""
    ops = _ops()
    assert got.dtype == torch.int32 and tuple(got.shape) == tuple(ref.shape), (name, got.dtype, got.shape, ref.shape)
    ops.h2_check(name)
    d = ops.unpack_h2(got).cpu().reshape(-1, got.shape[-1])
    finite = bool(torch.isfinite(d).all())
    ref = ref.reshape(-1, ref.shape[-1])
    scale = ref.abs().max().item() + 1e-6
    d.sub_(ref).abs_()
    row, ch = divmod(int(d.argmax()), d.shape[1])
    err = d[row, ch].item()
    report(f"[strict-ops] {name}: max_abs_err={err:.3e} at row {row} of {d.shape[0]} (256-row tile {row // 256}), channel {ch} "
           f"ref_absmax={scale:.3e} rel={err / scale:.3e}")
    assert finite, name
    assert err <= tol * scale, f"{name}: err {err} > {tol}*{scale} at row {row}, channel {ch}"


@pytest.mark.parametrize("M,K,N,epi,kernel,variant,what", T.DENSE_CASES, ids=T.DENSE_IDS)
def test_dense_h2_kernels(M, K, N, epi, kernel, variant, what, report):
    """every GEMM kernel of the packed storage at the smallest shapes that select it under default dispatch (tests/_h2_gemm_cases.py; the
    table itself is held against the dispatcher in tests/test_h2_dispatch_cpu.py): the dispatcher really picks it, the WHOLE output
    against the fp32 oracle at TOL_OP, and a second launch bit for bit.  The 2^19-row case (the 156 KB weight slice) is compared in full
    as well: its fp32 CPU reference takes 2-3 s on 16 threads."""
    ops = _ops()
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g)
    w, b = torch.randn(K, N, generator=g) / math.sqrt(K), torch.randn(N, generator=g) * 0.1
    act, post, has_res = T.EPILOGUE[epi]
    r = torch.randn(M, N, generator=g) if has_res else None         # the scale of the product: a dropped residual is 1e5 tolerances
    with ops.precision("strict"):
        cw = ops.make_dense_weight(w, b)
    d, _ = T.dense_desc(M, K, N, epi, cw.ldw)
    assert ops.conv_kernel_name_h2(d, has_res) == kernel, what
    xa, ra = A(x, "strict"), (A(r, "strict") if has_res else None)
    got = ops.dense(xa, cw, act=act, act_post=post, residual=ra)
    ref = R.act(R.dense(x, w, b), act)
    if has_res:
        ref = R.act(ref.add_(r), post)
    check_worst(report, f"dense h2 {variant.split(' ')[0]} {M}x{K}x{N} {epi}", got, ref)
    again = ops.dense(xa, cw, act=act, act_post=post, residual=ra)
    assert torch.equal(got, again), "two launches on the same operands must agree bit for bit"


@pytest.mark.parametrize("case,kernel,variant,what", T.CONV_H2_CASES, ids=T.CONV_H2_IDS)
def test_conv2d_h2_kernels(case, kernel, variant, what, report):
    """k x k convolutions of the packed storage beyond CONV_CASES' 1 023 rows: im2col staging selected by the row count (plain and
    grouped), the tile kernel just under that switch, and its <64,128> instantiation"""
    ops = _ops()
    B, H, W, Cin, Cout, k, s, pad, groups, act, use_res = case
    g = torch.Generator().manual_seed(hash(case[:9]) % (2 ** 31))
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(k, k, Cin // groups, Cout, generator=g) / math.sqrt(k * k * Cin / groups)
    bias = torch.randn(Cout, generator=g) * 0.1
    ref = R.act(R.conv2d(x, w, bias, s, pad, groups), act)
    res = None
    if use_res:
        res = torch.randn(*ref.shape, generator=g)
        ref = ref + res
    with ops.precision("strict"):
        cw = ops.make_conv_weight(w, bias, groups=groups)
    d, _ = T.conv_desc(case, cw.ldw)
    assert ops.conv_kernel_name_h2(d, use_res) == kernel, what
    xa, ra = A(x, "strict"), (A(res, "strict") if use_res else None)
    got = ops.conv2d(xa, cw, stride=s, pad=pad, act=act, residual=ra)
    check_worst(report, f"conv2d h2 {variant} {case}", got, ref)
    again = ops.conv2d(xa, cw, stride=s, pad=pad, act=act, residual=ra)
    assert torch.equal(got, again), "two launches on the same operands must agree bit for bit"


@pytest.mark.parametrize("B,HW,Cin,Cout,act,res", [(4, 14, 96, 40, None, False), (3, 14, 96, 160, None, True), (2, 7, 24, 72, "silu", False),
                                                   (5, 13, 416, 112, None, False), (70, 28, 48, 24, None, True), (2, 7, 1248, 208, None, True)])
def test_conv2d_gated_h2(B, HW, Cin, Cout, act, res, report):
    """the squeeze-excite gate inside the GEMM's activation operand (vip_conv2d_gated_nhwc_h2): one or several k chunks, a partial chunk,
    64- and 128-channel tiles, 16- and 64-pixel wave tiles, and the same values as the separate multiply pass"""
    ops = _ops()
    g = torch.Generator().manual_seed(B + Cin + Cout)
    x = torch.randn(B, HW, HW, Cin, generator=g)
    gate = torch.rand(B, Cin, generator=g) * 1.2
    w = torch.randn(1, 1, Cin, Cout, generator=g) / math.sqrt(Cin)
    b = torch.randn(Cout, generator=g) * 0.1
    r = torch.randn(B, HW, HW, Cout, generator=g) if res else None
    with ops.precision("strict"):
        cw = ops.make_conv_weight(w, b)
    xa, ga, ra = A(x, "strict"), A(gate, "strict"), (A(r, "strict") if res else None)
    got = ops.conv2d(xa, cw, act=act, gate=ga, residual=ra)
    ref = R.act(R.conv2d(x * gate[:, None, None, :], w, b), act) + (r if res else 0)
    check(report, f"conv2d gated {B}x{HW}x{HW}x{Cin}->{Cout}", got, ref)
    with ops.unfused():
        two = ops.conv2d(xa, cw, act=act, gate=ga, residual=ra)
    d = (ops.unpack_h2(got) - ops.unpack_h2(two)).abs().max().item()
    report(f"[strict-ops] gated conv vs multiply + conv: max_abs_diff={d:.3e}")
    assert d <= 2e-5 * (ref.abs().max().item() + 1e-6)


@pytest.mark.parametrize("C,hidden,M,ln,res", [(96, 384, 9216 + 37, True, True), (64, 256, 8192, True, True), (128, 384, 8192 + 255, True, True),
                                               (96, 384, 8200, False, False), (128, 512, 8192 + 1, True, False), (64, 192, 12000, False, True)])
def test_mlp_fused_h2(C, hidden, M, ln, res, report):
    """the one-launch MLP of the packed storage (csrc/mlp_h2.hip): ragged last tile, with / without LayerNorm and residual, and the same
    arithmetic as the three-launch form (VIP_MLP_H2_FUSED=0) to fp32 round-off"""
    ops = _ops()
    g = torch.Generator().manual_seed(C + hidden)
    x = torch.randn(M, C, generator=g) * 1.5
    k1, b1 = torch.randn(C, hidden, generator=g) / math.sqrt(C), torch.randn(hidden, generator=g) * 0.1
    k2, b2 = torch.randn(hidden, C, generator=g) / math.sqrt(hidden), torch.randn(C, generator=g) * 0.1
    gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    with ops.precision("strict"):
        fc1, fc2 = ops.make_dense_weight(k1, b1), ops.make_dense_weight(k2, b2)
    assert _ops()._abi.lib().vip_mlp_fused_supported_h2(M, C, hidden, 3)
    xa = A(x, "strict")
    got = ops.mlp(xa, fc1, fc2, act="gelu", residual=xa if res else None, ln=(dev(gam), dev(bet), 1e-5) if ln else None)
    h = R.layernorm(x, gam, bet, 1e-5) if ln else x
    ref = R.dense(R.act(R.dense(h, k1, b1), "gelu"), k2, b2) + (x if res else 0)
    check(report, f"mlp fused C{C} hidden{hidden} M{M}", got, ref)
    with ops.unfused():
        three = ops.mlp(xa, fc1, fc2, act="gelu", residual=xa if res else None, ln=(dev(gam), dev(bet), 1e-5) if ln else None)
    d = (ops.unpack_h2(got) - ops.unpack_h2(three)).abs().max().item()
    report(f"[strict-ops] mlp fused vs three launches C{C}: max_abs_diff={d:.3e}")
    assert d <= 2e-5 * (ref.abs().max().item() + 1e-6)


@pytest.mark.parametrize("mode", MODES)
def test_dense_mlp_se_strict(mode, report):
    ops = _ops()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, 50, 96, generator=g)
    k1, b1 = torch.randn(96, 384, generator=g) / math.sqrt(96), torch.randn(384, generator=g) * 0.1
    k2, b2 = torch.randn(384, 96, generator=g) / math.sqrt(384), torch.randn(96, generator=g) * 0.1
    gam, bet = 1 + 0.1 * torch.randn(96, generator=g), 0.1 * torch.randn(96, generator=g)
    with ops.precision(mode):
        fc1, fc2 = ops.make_dense_weight(k1, b1), ops.make_dense_weight(k2, b2)
    got = ops.mlp(A(x, mode), fc1, fc2, act="gelu", residual=A(x, mode), ln=(dev(gam), dev(bet), 1e-5))
    ref = x + R.dense(R.act(R.dense(R.layernorm(x, gam, bet, 1e-5), k1, b1), "gelu"), k2, b2)
    check(report, "mlp", got, ref)
    xs = torch.randn(4, 7, 7, 96, generator=g)
    s = ops.se_gate(A(xs, mode), fc1, fc2, "silu", "sigmoid")
    assert s.shape == (4, 96) and s.dtype == ops.act_dtype(mode)
    sref = torch.sigmoid(R.dense(R.act(R.dense(xs.mean((1, 2)), k1, b1), "silu"), k2, b2))
    check(report, "se_gate", s, sref)
    y = ops.scale_add_act(A(xs, mode), s, A(xs, mode), "relu")
    check(report, "scale_add_act", y, torch.relu(xs * sref[:, None, None, :] + xs))
    y1, y2 = ops.scale_add_act(A(xs, mode), None, None, None, act2="silu")
    check(report, "scale_add_act second output", y2, R.act(xs, "silu"))
    if mode == "f32":
        assert torch.equal(y1.cpu(), xs)
    else:
        check(report, "scale_add_act identity", y1, xs, tol=3e-7)


@pytest.mark.parametrize("k,s,pad,act", [(3, 1, (1, 1, 1, 1), "gelu"), (3, 2, (0, 1, 0, 1), "silu"), (5, 1, (2, 2, 2, 2), "silu"),
                                         (5, 2, (1, 2, 1, 2), None), (7, 1, (3, 3, 3, 3), None)])
@pytest.mark.parametrize("mode", MODES)
def test_dwconv_strict(k, s, pad, act, mode, report):
    ops = _ops()
    g = torch.Generator().manual_seed(k * 10 + s)
    x = torch.randn(2, 15, 13, 40, generator=g)
    w = torch.randn(k, k, 40, 1, generator=g) / k
    b = torch.randn(40, generator=g) * 0.1
    got = ops.dwconv2d(A(x, mode), ops.make_dw_weight(w), dev(b), k, s, pad, act=act)
    check(report, f"dwconv k{k} s{s}", got, R.act(R.dwconv2d(x, w, b, s, pad), act))


# the LDS-staged stride-1 kernel (csrc/dwconv_lds_h2.hip): its lane packings (several images per wave on 7 x 7 / 14 x 14 maps, several
# regions per image on large ones), partial 16-channel blocks (C = 24, 40, 72), asymmetric padding, maps smaller than the filter
DW_LDS_CASES = [
    # B, H, W, C, k, pad(t,b,l,r), act
    (11, 7, 7, 48, 3, (1, 1, 1, 1), "silu"),
    (9, 7, 7, 40, 5, (2, 2, 2, 2), "silu"),
    (3, 14, 14, 72, 5, (2, 2, 2, 2), "silu"),
    (3, 13, 13, 32, 3, (1, 1, 1, 1), "gelu"),
    (2, 24, 24, 96, 7, (3, 3, 3, 3), None),
    (2, 12, 12, 64, 7, (3, 3, 3, 3), None),
    (1, 99, 99, 24, 7, (3, 3, 3, 3), None),
    (1, 49, 49, 16, 7, (3, 3, 3, 3), "relu"),
    (2, 56, 56, 24, 3, (1, 1, 1, 1), "silu"),
    (1, 112, 112, 8, 3, (1, 1, 1, 1), "silu"),
    (2, 28, 28, 16, 5, (2, 2, 2, 2), "silu"),
    (2, 5, 4, 16, 7, (3, 3, 3, 3), None),
    (2, 17, 19, 16, 3, (0, 0, 0, 0), None),          # VALID: Ho = H - 2
    (2, 16, 16, 16, 5, (1, 2, 2, 1), "gelu"),
]


@pytest.mark.parametrize("B,H,W,C,k,pad,act", DW_LDS_CASES)
def test_dwconv_lds_h2(B, H, W, C, k, pad, act, report):
    ops = _ops()
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + k)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(k, k, C, 1, generator=g) / k
    b = torch.randn(C, generator=g) * 0.1
    got = ops.dwconv2d(A(x, "strict"), ops.make_dw_weight(w), dev(b), k, 1, pad, act=act)
    check(report, f"dwconv(lds) {B}x{H}x{W}x{C} k{k}", got, R.act(R.dwconv2d(x, w, b, 1, pad), act))


@pytest.mark.parametrize("B,H,W,C,k,act", [(5, 14, 14, 96, 5, "silu"), (9, 7, 7, 40, 3, "silu"), (3, 24, 20, 64, 3, "gelu"), (2, 56, 56, 24, 3, "silu"),
                                           (2, 99, 99, 16, 7, None), (17, 13, 13, 72, 3, "silu")])
def test_dwconv_se_pooled_h2(B, H, W, C, k, act, report):
    """DepthwiseConv2D -> activation -> se_module with the pool's partial sums left by the depthwise kernel (vip_dwconv2d_s1_pool_h2 +
    vip_se_gate_pooled_h2): the map and the gate against the oracle, against the two plain launches, and bit-reproducible"""
    ops = _ops()
    g = torch.Generator().manual_seed(B + H + C + k)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(k, k, C, 1, generator=g) / k
    b = torch.randn(C, generator=g) * 0.1
    Cr = max(8, C // 4 // 8 * 8)
    k1, b1 = torch.randn(C, Cr, generator=g) / math.sqrt(C), torch.randn(Cr, generator=g) * 0.1
    k2, b2 = torch.randn(Cr, C, generator=g) / math.sqrt(Cr), torch.randn(C, generator=g) * 0.1
    with ops.precision("strict"):
        fc1, fc2 = ops.make_dense_weight(k1, b1), ops.make_dense_weight(k2, b2)
    p = k // 2
    xa, dw, bb = A(x, "strict"), ops.make_dw_weight(w), dev(b)
    assert ops._abi.lib().vip_dwconv2d_s1_pool_parts_h2(B, H, W, C, k, H, W) > 0
    h, gate = ops.dwconv2d_se(xa, dw, bb, k, 1, (p, p, p, p), act, fc1, fc2, "silu", "sigmoid")
    ops.h2_check("dwconv2d_se")
    href = R.act(R.dwconv2d(x, w, b, 1, (p, p, p, p)), act)
    gref = torch.sigmoid(R.dense(R.act(R.dense(href.mean((1, 2)), k1, b1), "silu"), k2, b2))
    check(report, f"dwconv_se map {B}x{H}x{W}x{C} k{k}", h, href)
    check(report, f"dwconv_se gate {B}x{H}x{W}x{C} k{k}", gate, gref)
    with ops.unfused():
        h2, gate2 = ops.dwconv2d_se(xa, dw, bb, k, 1, (p, p, p, p), act, fc1, fc2, "silu", "sigmoid")
    assert torch.equal(h.cpu(), h2.cpu()), "the pooling form must not change the map"
    d = (ops.unpack_h2(gate) - ops.unpack_h2(gate2)).abs().max().item()
    report(f"[strict-ops] pooled gate vs plain gate: max_abs_diff={d:.3e}")
    assert d <= 2e-6
    h3, gate3 = ops.dwconv2d_se(xa, dw, bb, k, 1, (p, p, p, p), act, fc1, fc2, "silu", "sigmoid")
    assert torch.equal(gate.cpu(), gate3.cpu()) and torch.equal(h.cpu(), h3.cpu()), "bit-reproducible"


def test_dwconv_lds_h2_fuzz(report):
    """60 random shapes (maps from 1 x 1 to 130 x 70, 8 ... 200 channels, ragged batches, every padding up to k - 1) through the LDS-staged
    kernel's own entry point against the plain strict kernel (vip_dwconv2d_nhwc_h2 with the tile / LDS paths bypassed is not reachable
    per call, so the reference here is the fp32 oracle on the unpacked input) - the lane packings the host picks are data-dependent"""
    import random
    ops = _ops()
    lib = ops._abi.lib()
    rnd = random.Random(1234)
    worst = 0.0
    for it in range(60):
        k = rnd.choice([3, 5, 7])
        H, W = rnd.choice([(1, 1), (2, 3), (7, 7), (5, 19), (14, 14), (13, 29), (33, 17), (64, 9), (130, 70), (49, 49)])
        C = 8 * rnd.randint(1, 25)
        B = rnd.choice([1, 2, 3, 5, 17])
        pt, pl = rnd.randint(0, k - 1), rnd.randint(0, k - 1)
        pb, pr = rnd.randint(0, k - 1), rnd.randint(0, k - 1)
        Ho, Wo = H + pt + pb - k + 1, W + pl + pr - k + 1
        if Ho <= 0 or Wo <= 0:
            continue
        g = torch.Generator().manual_seed(it)
        x = torch.randn(B, H, W, C, generator=g)
        w = torch.randn(k, k, C, 1, generator=g) / k
        b = torch.randn(C, generator=g) * 0.1
        act = rnd.choice([None, "relu", "silu", "gelu"])
        assert lib.vip_dwconv2d_s1_supported_h2(B, H, W, C, k, Ho, Wo) == 1
        got = ops.dwconv2d(A(x, "strict"), ops.make_dw_weight(w), dev(b), k, 1, (pt, pb, pl, pr), act=act)
        ops.h2_check("dwconv fuzz")
        ref = R.act(R.dwconv2d(x, w, b, 1, (pt, pb, pl, pr)), act)
        err = (ops.unpack_h2(got).cpu() - ref).abs().max().item() / (ref.abs().max().item() + 1e-6)
        worst = max(worst, err)
        assert err <= TOL_OP, (it, B, H, W, C, k, (pt, pb, pl, pr), act, err)
    report(f"[strict-ops] dwconv(lds) fuzz: worst rel err {worst:.3e} over 60 random shapes")


def test_mlp_and_gated_conv_h2_fuzz(report):
    """random token counts / widths through the fused MLP and random shapes through the gated GEMM, against the fp32 oracle"""
    import random
    ops = _ops()
    rnd = random.Random(99)
    worst = 0.0
    for it in range(8):
        C = rnd.choice([64, 96, 128])
        hid = 32 * rnd.randint(2, 16)
        M = 8192 + rnd.randint(0, 700)
        g = torch.Generator().manual_seed(it)
        x = torch.randn(M, C, generator=g)
        k1, b1 = torch.randn(C, hid, generator=g) / math.sqrt(C), torch.randn(hid, generator=g) * 0.1
        k2, b2 = torch.randn(hid, C, generator=g) / math.sqrt(hid), torch.randn(C, generator=g) * 0.1
        with ops.precision("strict"):
            fc1, fc2 = ops.make_dense_weight(k1, b1), ops.make_dense_weight(k2, b2)
        xa = A(x, "strict")
        got = ops.mlp(xa, fc1, fc2, act="gelu", residual=xa)
        ops.h2_check("mlp fuzz")
        ref = x + R.dense(R.act(R.dense(x, k1, b1), "gelu"), k2, b2)
        err = (ops.unpack_h2(got).cpu() - ref).abs().max().item() / ref.abs().max().item()
        worst = max(worst, err)
        assert err <= TOL_OP, ("mlp", it, M, C, hid, err)
    for it in range(16):
        B, HW = rnd.choice([(1, 1), (3, 7), (2, 14), (9, 5), (1, 56), (33, 3)])
        Cin, Cout = 8 * rnd.randint(1, 60), 8 * rnd.randint(1, 40)
        g = torch.Generator().manual_seed(100 + it)
        x = torch.randn(B, HW, HW, Cin, generator=g)
        gate = torch.rand(B, Cin, generator=g) * 1.5
        w, b = torch.randn(1, 1, Cin, Cout, generator=g) / math.sqrt(Cin), torch.randn(Cout, generator=g) * 0.1
        res = rnd.random() < 0.5
        r = torch.randn(B, HW, HW, Cout, generator=g) if res else None
        act = None if res else rnd.choice([None, "silu", "relu"])
        with ops.precision("strict"):
            cw = ops.make_conv_weight(w, b)
        got = ops.conv2d(A(x, "strict"), cw, act=act, gate=A(gate, "strict"), residual=A(r, "strict") if res else None)
        ops.h2_check("gated fuzz")
        ref = R.act(R.conv2d(x * gate[:, None, None, :], w, b), act) + (r if res else 0)
        err = (ops.unpack_h2(got).cpu() - ref).abs().max().item() / (ref.abs().max().item() + 1e-6)
        worst = max(worst, err)
        assert err <= TOL_OP, ("gated", it, B, HW, Cin, Cout, act, res, err)
    report(f"[strict-ops] fused MLP / gated conv fuzz: worst rel err {worst:.3e}")


def test_dwconv_lds_h2_identity_is_exact():
    """a centre-tap-only filter returns the input VALUES exactly (the sign of a zero lo term may differ) - small magnitudes included, whose
    lo terms are fp16 subnormals (the kernel joins hi + lo with v_fma_mix_f32; a flushed subnormal would show here and nowhere in the
    tolerance tests)"""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 14, 14, 32, generator=g) * torch.logspace(-6, 1, 32)
    xp = ops.pack_h2(dev(x))
    for k in (3, 5, 7):
        w = torch.zeros(k, k, 32, 1)
        w[k // 2, k // 2] = 1.0
        got = ops.dwconv2d(xp, ops.make_dw_weight(w), None, k, 1, (k // 2,) * 4, act=None)
        assert torch.equal(ops.unpack_h2(got).cpu(), ops.unpack_h2(xp).cpu()), k


@pytest.mark.parametrize("mode", MODES)
def test_norm_pool_heads_strict(mode, report):
    ops = _ops()
    act = lambda t: A(t, mode)  # noqa: E731
    g = torch.Generator().manual_seed(8)
    for C in (64, 96, 768, 1536):
        x = torch.randn(37, C, generator=g) * 2 + 0.3
        gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        check(report, f"layernorm C={C}", ops.layernorm(act(x), dev(gam), dev(bet), 1e-6), R.layernorm(x, gam, bet, 1e-6))
    x = torch.randn(2, 13, 11, 24, generator=g)
    check(report, "avgpool same", ops.pool2d(act(x), 2, 2, (0, 1, 0, 1), ops.POOL_AVG_VALID), R.avgpool_same(x, 2, 2))
    check(report, "avgpool full", ops.pool2d(act(x), 3, 2, (1, 1, 1, 1), ops.POOL_AVG_FULL), R.avgpool_valid(x, 3, 2, (1, 1, 1, 1)))
    check(report, "maxpool zero-pad", ops.pool2d(act(x), 3, 2, (1, 1, 1, 1), ops.POOL_MAX_ZEROPAD), R.maxpool_valid(x, 3, 2, (1, 1, 1, 1)))
    check(report, "zero-pad copy", ops.pool2d(act(x), 1, 1, (0, 1, 1, 2), ops.POOL_MAX_ZEROPAD), R.zero_pad(x, (0, 1, 1, 2)))
    check(report, "crop", ops.pool2d(act(x), 1, 1, (0, 0, 0, 0), ops.POOL_MAX_ZEROPAD, out_hw=(9, 7)), x[:, :9, :7].contiguous())
    check(report, "global_avgpool", ops.global_avgpool(act(x), split=True), x.mean((1, 2)))
    wn, bn = torch.randn(3, 24, generator=g), torch.randn(3, generator=g)
    check(report, "gap_dense", ops.gap_dense_f32(act(x), dev(wn), dev(bn)), x.mean((1, 2)) @ wn.t() + bn)
    gam, bet = 1 + 0.1 * torch.randn(24, generator=g), 0.1 * torch.randn(24, generator=g)
    check(report, "gap_ln_dense", ops.gap_ln_dense_f32(act(x), dev(gam), dev(bet), 1e-6, dev(wn), dev(bn)),
          R.layernorm(x.mean((1, 2)), gam, bet, 1e-6) @ wn.t() + bn)
    t = torch.randn(3, 17, 24, generator=g)
    check(report, "cls_dense", ops.cls_dense_f32(act(t), dev(wn), dev(bn)), t[:, 0] @ wn.t() + bn)
    cls, pos = torch.randn(24, generator=g), torch.randn(18, 24, generator=g)
    check(report, "vit_tokens", ops.vit_tokens(act(t), act(cls), act(pos)),
          torch.cat([cls.expand(3, 1, 24), t], 1) + pos[None])
    xr, sr = torch.randn(2, 5, 6, 32, generator=g), torch.rand(2, 32, generator=g)
    check(report, "radix_combine", ops.radix_combine(act(xr), act(sr), 2),
          xr[..., :16] * sr[:, None, None, :16] + xr[..., 16:] * sr[:, None, None, 16:])
    a, b = torch.randn(2, 5, 48, generator=g), torch.randn(2, 5, 32, generator=g)
    check(report, "mul", ops.mul(act(a), act(b), 16, 32, 8), a[..., 32:48] * b[..., 8:24])


# ws 7 / 14: the matrix-core kernel (attn_h2.hip) in the packed mode; ws 5: the fp32 VALU kernel in both storages
@pytest.mark.parametrize("ws,heads,nwin,glob", [(7, 2, (2, 3), False), (7, 4, (1, 2), True), (14, 8, (1, 1), False), (14, 8, (1, 1), True),
                                                (14, 8, (2, 1), False), (5, 2, (2, 2), False), (5, 2, (1, 2), True)])
@pytest.mark.parametrize("mode", MODES)
def test_window_attention_strict(ws, heads, nwin, glob, mode, report):
    ops = _ops()
    g = torch.Generator().manual_seed(ws * 100 + heads + glob)
    B, C, N = 2, heads * 32, ws * ws
    Hp, Wp = nwin[0] * ws, nwin[1] * ws
    nq = 2 if glob else 3
    qkv = torch.randn(B, Hp, Wp, nq * C, generator=g)
    qg = torch.randn(B, N, C, generator=g) if glob else None
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g) * 0.5
    scale = 32 ** -0.5
    got = ops.window_attention(A(qkv, mode), None if qg is None else A(qg, mode), dev(table), heads, ws, scale)
    win = R.window_partition(qkv, ws).reshape(-1, N, nq, heads, 32).permute(2, 0, 3, 1, 4)      # [nq, B_, heads, N, hd]
    if glob:
        k, v = win[0], win[1]
        q = torch.repeat_interleave(qg, win.shape[1] // B, dim=0).reshape(-1, N, heads, 32).permute(0, 2, 1, 3)
    else:
        q, k, v = win[0], win[1], win[2]
    o = gcvit_ref.window_attention_core(q, k, v, table, ws, scale).permute(0, 2, 1, 3).reshape(-1, ws, ws, C)
    ref = R.window_reverse(o, ws, Hp, Wp, C)
    check(report, f"window_attention ws{ws} heads{heads} global={glob}", got, ref)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", [197, 50, 224])
def test_mhsa_strict(N, mode, report):
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    B, heads = 3, 3
    D = heads * 64
    qkv = torch.randn(B, N, 3 * D, generator=g)
    got = ops.mhsa(A(qkv, mode), heads, 64 ** -0.5)
    t = qkv.reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    attn = torch.softmax((64 ** -0.5) * (t[0] @ t[1].transpose(-1, -2)), dim=-1)
    ref = (attn @ t[2]).permute(0, 2, 1, 3).reshape(B, N, D)
    check(report, "mhsa", got, ref)


def test_resize_strict_matches_oracle_bitwise(report):
    """the strict input: the fp32 values of cast -> bicubic -> /255 (dataset.py:31-38), not rounded to fp16"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    raws = [synth_jpeg(100), synth_jpeg(101)]          # 256x192 and 200x200
    batch = pipeline.decode_jpegs(raws)
    pix = P.decode_pixels(raws)
    for hw in (200, 224):
        got = batch.resized(hw, hw, dtype=torch.float32).cpu()
        ref = torch.stack([R.decode_resize_normalize(p, hw, hw) for p in pix])
        d = (got[..., :3] - ref).abs().max().item()
        report(f"[strict-ops] resize {hw}: max|d| {d:.3e}")
        assert d <= 1e-6 and float(got[..., 3:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# whole members: the CALIBRATED logit (amplifying synthetic heads, tests/gen_synth_heads.py) within the north-star 1e-3
# ---------------------------------------------------------------------------------------------------------------------------------
STRICT_MEMBERS = ["convnext_tiny_in22k", "resnest50", "gcvit_tiny", "efficientnet_v2t", "efficientnet_v1b4", "eca_nfnet_l0",
                  "resnet_rs50", "vit_small_patch16_224", "vit_tiny_patch16_224"]
_Z = {}


def _strict_logits(key, raws, tag, mode="strict"):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops, pipeline
    if (key, tag, mode) not in _Z:
        spec, model = P.gpu_member(key, mode)
        assert model.precision == mode
        x = pipeline.decode_jpegs(raws).resized(spec.input_hw, spec.input_hw, dtype=ops.act_dtype(mode))
        _Z[(key, tag, mode)] = model.logits(x)[:, 0].float().cpu().numpy()
        if mode == "strict":
            ops.h2_check(f"{key} ({tag})")                  # no activation left the fp16 range of the packed storage
    return _Z[(key, tag, mode)]


# every member in the packed mode; the fp32-storage reference arithmetic on three (one per attention / conv / MBConv family)
@pytest.mark.parametrize("key,mode", [(k, "strict") for k in STRICT_MEMBERS] +
                         [(k, "f32") for k in ("gcvit_tiny", "efficientnet_v1b4", "vit_tiny_patch16_224")])
def test_member_logit_within_north_star(key, mode, report):
    n = N_IMG
    raws = [synth_jpeg(i) for i in P.e2e_image_ids(n)]
    z = P.oracle_logits(key, "e2e", raws)               # the CLI test's image set: one oracle pass per member and session
    zg = _strict_logits(key, raws, "e2e", mode)
    dz = np.abs(zg - z)
    report(f"[{mode}] {key:22s} {n} images: max|dz|={dz.max():.3e} mean|dz|={dz.mean():.3e} logit std {z.std():.2f}")
    assert np.isfinite(zg).all()
    assert dz.max() <= P.TOL_NORTH_STAR


@pytest.mark.parametrize("key", ["efficientnet_v1b4", "efficientnet_v2t", "resnest50"])
def test_member_logit_two_term_gemm(key, report, monkeypatch):
    """VIP_STRICT_GEMM=bf16x2 (opt-in: twice the matrix rate, +32 % images/s for the strict step): the three members with the largest
    errors still sit inside the north-star 1e-3 (measured 2.4e-4 ... 3.4e-4 here, 4.5e-4 on the photographs), with a margin of 2-4x
    instead of the default arithmetic's 20x"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops, pipeline
    monkeypatch.setattr(ops, "STRICT_GEMM", "bf16x2")
    n = N_IMG
    raws = [synth_jpeg(i) for i in P.e2e_image_ids(n)]
    z = P.oracle_logits(key, "e2e", raws)
    spec, model = P.gpu_member(key, "f32")
    x = pipeline.decode_jpegs(raws).resized(spec.input_hw, spec.input_hw, dtype=torch.float32)
    zg = model.logits(x)[:, 0].float().cpu().numpy()
    dz = np.abs(zg - z)
    report(f"[f32/bf16x2] {key:22s} {n} images: max|dz|={dz.max():.3e} mean|dz|={dz.mean():.3e}")
    assert np.isfinite(zg).all() and dz.max() <= P.TOL_NORTH_STAR


def test_ensemble_logit_within_north_star(report):
    """logit(ensemble mean) - the north-star axis - for the 7 manifest members, config 5's 8 and config 4's 4, on the synthetic set
    and on the photo tiles (off the synthetic distribution: nothing is calibrated in strict mode, so there is no distribution to be off)"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import zoo
    n = N_IMG
    sets = {"e2e": [synth_jpeg(i) for i in P.e2e_image_ids(n)], "photo": P.real_photo_tiles()}
    for tag, raws in sets.items():
        for name, members in (("ensemble7", zoo.ENSEMBLE), ("ensemble8", zoo.ENSEMBLE8), ("ensemble4", zoo.ENSEMBLE4)):
            po = np.mean([P.sigmoid(P.oracle_logits(k, "e2e" if tag == "e2e" else "photo_tiles", raws)) for k in members], 0)
            pg = np.mean([P.sigmoid(_strict_logits(k, raws, tag)) for k in members], 0)
            dl = np.abs(P.logit(pg) - P.logit(po)).max()
            flips = int(((pg > 0.487) != (po > 0.487)).sum())
            report(f"[strict] {name} on {tag}: max|d logit(mean)|={dl:.3e} max|dp|={np.abs(pg - po).max():.3e} decision flips {flips}")
            assert dl <= P.TOL_NORTH_STAR and flips == 0
        if tag == "photo":
            for k in zoo.ENSEMBLE8:
                z = P.oracle_logits(k, "photo_tiles", raws)
                dz = np.abs(_strict_logits(k, raws, tag) - z)
                report(f"[strict] photo {k:22s} max|dz|={dz.max():.3e} (absolute) z range [{z.min():+.2f},{z.max():+.2f}]")
                assert dz.max() <= P.TOL_NORTH_STAR


def test_member_inside_batch_256_strict(report):
    """B = 256 (what bench.py's strict leg times): the batch-EDGE images P.B256_EDGE_IMAGES (first, middle, last - where a wrong last M
    tile, a wrong tile at a persistent workgroup's wrap-around or a wrong second LDS channel chunk lands) against the oracle, EVERY
    member of config 5"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import zoo
    idx = P.B256_EDGE_IMAGES
    for key in zoo.ENSEMBLE8:
        raws = [synth_jpeg(1000 + i) for i in range(256)]
        z = P.oracle_logits(key, "b256_edges", [raws[i] for i in idx])
        zg = _strict_logits(key, raws, "b256")
        d = np.abs(zg[idx] - z).max()
        report(f"[strict] {key:22s} images {idx} of a 256-batch: max|dz| {d:.3e}")
        assert np.isfinite(zg).all() and d <= P.TOL_NORTH_STAR


def test_precision_mismatch_is_an_error():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    spec, model = P.gpu_member("vit_tiny_patch16_224", "strict")
    x16 = pipeline.decode_jpegs([synth_jpeg(3)]).resized(224, 224)
    with pytest.raises(_abi.VipError):
        model.predict(x16)
    x32 = pipeline.decode_jpegs([synth_jpeg(3)]).resized(224, 224, dtype=torch.float32)
    with pytest.raises(_abi.VipError):
        model.predict(x32)


def test_packed_storage_round_trip_and_range_guard(report):
    """pack -> unpack keeps 2^-22 relative (2^-25 absolute below 2^-3); a value beyond the fp16 range raises the status word"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, ops
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(4, 33, 40, generator=g) * torch.logspace(-6, 4, 40)).cuda().contiguous()
    back = ops.unpack_h2(ops.pack_h2(x))
    ops.h2_check("round trip")
    err = (back - x).abs()
    bound = torch.maximum(x.abs() * 2.0 ** -22, torch.full_like(x, 2.0 ** -25))
    report(f"[strict-ops] pack/unpack: max rel err {float((err / x.abs().clamp_min(1e-30)).max()):.3e}, worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    big = torch.zeros(8, 16).cuda()
    big[3, 5] = 7.0e4
    ops.pack_h2(big)
    with pytest.raises(_abi.VipError):
        ops.h2_check("overflow probe")
    ops.h2_check("cleared")                                  # the failed check reset the word
