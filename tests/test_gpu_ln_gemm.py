"""LayerNorm folded into the GEMM that consumes it (vip_ln_gemm_bias_act_f16 / ops.ln_dense, pwx_ln_kernel in csrc/conv_igemm.hip):

* against the fp32 oracle  R.dense(R.layernorm(x), w, b) (+ act / residual)  at the tolerance test_mlp_fused[use_ln=True] uses for the
  same rounding structure (the normalised operand is rounded to fp16 inside the dot product): 4e-3 of the output scale;
* against the two launches it replaces (ops.layernorm + ops.dense inside ops.unfused()): the operand is rounded at the same point, the
  statistics are summed in another order (in-lane over 8-channel groups, then two lane exchanges, instead of layernorm_kernel's
  allreduce), so a normalised value that sits on an fp16 rounding boundary may fall to the other side;
* two launches on the same operands agree bit for bit;
* every test asserts through vip_ln_gemm_supported / ops.ln_gemm_fused that the fused kernel really ran.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ops_ref as R  # noqa: E402

EPS = 1e-6
ACT_CODE = {None: 0, "relu": 1, "silu": 2, "gelu": 3, "sigmoid": 4}

# (M, K, N): every (K, N) of the LayerNorm -> Dense sites - ViT-S norm1 -> qkv (384, 1152) and norm2 -> fc1 (384, 1536, also ConvNeXt-T
# stage 2), GCViT-T level 2 norm1 -> qkv and norm2 -> fc1 (256, 768; qkv with a global query 256, 512), level 1 norm2 -> fc1 (128, 384) -
# at a ragged M and at the sites' own M, a K tail (200), a half-empty last channel tile (N = 320), and the 2- / 3- / 6-chunk
# instantiations.  The operator tests run with VIP_LN_GEMM_ALL=1 (read per call): the kernel is tested on every shape it can run,
# whatever vip_ln_gemm_supported's measured policy sends to it by default (POLICY below).
SHAPES = [(16384 + 37, 384, 1152), (50432, 384, 1152), (16384 + 37, 384, 1536), (50432, 384, 1536), (16384 + 37, 256, 768),
          (50176, 256, 768), (50176, 256, 512), (16384 + 37, 256, 512), (17000, 200, 1024), (20000, 192, 320), (16500, 128, 256),
          (16384 + 37, 128, 384), (16390, 320, 384)]
# (M, K, N, act, fused by default): the ensemble's sites
POLICY = [(147456, 384, 1536, "gelu", True), (200704, 128, 384, "gelu", True), (50176, 256, 512, None, True),
          (50432, 384, 1152, None, False), (50432, 384, 1536, "gelu", False), (50176, 256, 768, None, False), (50176, 256, 768, "gelu", False)]
MODES = ["none", "gelu", "res", "res_relu"]


def _ops():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    return ops


def h(t):
    return t.to(torch.float16).to(torch.float32)


def dev(t):
    return t.to(torch.float16).cuda().contiguous()


def check(report, name, got, ref, tol):
    got = got.float().cpu()
    scale = ref.abs().max().item() + 1e-6
    err = (got - ref).abs().max().item()
    rms = ((got - ref) ** 2).mean().sqrt().item()
    report(f"[ln_gemm] {name}: max_abs_err={err:.3e} rms={rms:.3e} ref_absmax={scale:.3e} rel={err / scale:.3e}")
    assert torch.isfinite(got).all(), name
    assert err <= tol * scale, f"{name}: err {err} > {tol}*{scale}"


def _case(M, K, N, mode):
    ops = _ops()
    g = torch.Generator().manual_seed(M + K + N)
    x = h(torch.randn(M, K, generator=g) * 1.5 + 0.3)               # the inputs of test_mlp_fused
    w = h(torch.randn(K, N, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g) * 0.1
    lg, lb = torch.randn(K, generator=g) * 0.2 + 1, torch.randn(K, generator=g) * 0.1
    res = h(torch.randn(M, N, generator=g)) if mode in ("res", "res_relu") else None
    act = "gelu" if mode == "gelu" else None
    post = "relu" if mode == "res_relu" else None
    cw = ops.make_dense_weight(w, b)
    ln = (lg.cuda(), lb.cuda(), EPS)
    xd, rd = dev(x), None if res is None else dev(res)
    run = lambda: ops.ln_dense(xd, ln, cw, act=act, act_post=post, residual=rd)  # noqa: E731
    return ops, (x, w, b, lg, lb, res, act, post), (xd, ln, cw, rd), run


def _assert_fused(ops, M, K, N, xd, cw, rd, act, post):
    from vipcup_amd import _abi
    assert _abi.lib().vip_ln_gemm_supported(M, K, N, ACT_CODE[act]), "the shape must be one the fused kernel takes"
    assert ops.ln_gemm_fused(xd, cw, act, post, rd), "ops.ln_dense would fall back to layernorm + dense"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_ln_dense_vs_oracle(M, K, N, mode, report, monkeypatch):
    monkeypatch.setenv("VIP_LN_GEMM_ALL", "1")
    ops, (x, w, b, lg, lb, res, act, post), (xd, ln, cw, rd), run = _case(M, K, N, mode)
    _assert_fused(ops, M, K, N, xd, cw, rd, act, post)
    ref = R.act(R.dense(R.layernorm(x, lg, lb, EPS), w, b), act)
    if res is not None:
        ref = R.act(ref + res, post)
    got = run()
    torch.cuda.synchronize()
    check(report, f"ln_dense {mode} {M}x{K}x{N}", got, ref, tol=4e-3)
    assert torch.equal(got, run()), "two launches on the same operands must agree bit for bit"


# Largest |fused - (layernorm + dense)| measured on MI355X over SHAPES x MODES: see MEASURED_MAX_DIFF below (the per-case figures are
# reported by the test).  Asserted at that value plus one fp16 ulp of the output magnitude of the case.
MEASURED_MAX_DIFF = 2.0 ** -8       # 3.9062e-03: one fp16 ulp of an output in [4, 8); about 0.1 % of the outputs differ at all


def _ulp16(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(max(v, 2.0 ** -14))) - 10)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_ln_dense_vs_the_launches_it_replaces(M, K, N, mode, report, monkeypatch):
    monkeypatch.setenv("VIP_LN_GEMM_ALL", "1")
    ops, (_, _, _, _, _, _, act, post), (xd, ln, cw, rd), run = _case(M, K, N, mode)
    _assert_fused(ops, M, K, N, xd, cw, rd, act, post)
    with ops.unfused():
        assert not ops.ln_gemm_fused(xd, cw, act, post, rd)
        two = ops.dense(ops.layernorm(xd, ln[0], ln[1], EPS), cw, act=act, act_post=post, residual=rd)
    got = run()
    torch.cuda.synchronize()
    diff = (got.float() - two.float()).abs()
    mag = two.float().abs().max().item()
    n_diff = int((diff > 0).sum())
    report(f"[ln_gemm] fused vs layernorm + dense {mode} {M}x{K}x{N}: max |d| = {diff.max().item():.4e}, {n_diff} of {diff.numel()} "
           f"outputs differ, |out| max {mag:.3f}, ulp16 {_ulp16(mag):.3e}")
    assert diff.max().item() <= MEASURED_MAX_DIFF + _ulp16(mag)


def test_unsupported_shapes_fall_back_to_two_launches(report):
    """K beyond the resident fragments, few rows, narrow N, non-contiguous rows and the unfused contexts keep layernorm + dense - and the
    C entry point refuses them instead of computing something else"""
    ops = _ops()
    from vipcup_amd import _abi
    lib = _abi.lib()
    for M, K, N in [(50432, 512, 1536), (12544, 384, 1152), (50432, 384, 128), (50432, 64, 256), (50432, 388, 1152)]:
        assert not lib.vip_ln_gemm_supported(M, K, N, 0), (M, K, N)
    for M, K, N, act, fused in POLICY:      # the measured policy: which of the ensemble's sites take the fused kernel by default
        assert bool(lib.vip_ln_gemm_supported(M, K, N, ACT_CODE[act])) == fused, (M, K, N, act)
    g = torch.Generator().manual_seed(5)
    M, K, N = 16384, 512, 512
    x = h(torch.randn(M, K, generator=g) * 1.5 + 0.3)
    w = h(torch.randn(K, N, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g) * 0.1
    lg, lb = torch.randn(K, generator=g) * 0.2 + 1, torch.randn(K, generator=g) * 0.1
    cw = ops.make_dense_weight(w, b)
    xd, ln = dev(x), (lg.cuda(), lb.cuda(), EPS)
    assert not ops.ln_gemm_fused(xd, cw)
    got = ops.ln_dense(xd, ln, cw)
    assert torch.equal(got, ops.dense(ops.layernorm(xd, ln[0], ln[1], EPS), cw))
    check(report, f"ln_dense fallback {M}x{K}x{N}", got, R.dense(R.layernorm(x, lg, lb, EPS), w, b), tol=4e-3)
    out = torch.empty(M, N, dtype=torch.float16, device="cuda")
    st = lib.vip_ln_gemm_bias_act_f16(xd.data_ptr(), ln[0].data_ptr(), ln[1].data_ptr(), EPS, cw.w.data_ptr(), cw.bias.data_ptr(), None,
                                      out.data_ptr(), M, N, K, K, cw.ldw, N, 0, 0, 0, None)
    assert st == -3, "VIP_ERR_UNSUPPORTED: the entry point has no silent fall-back"
    # a strided view of a wider tensor: not contiguous -> two launches
    wide = dev(torch.randn(20000, 512, generator=g))
    cw2 = ops.make_dense_weight(h(torch.randn(256, 512, generator=g) / 16), None)
    assert not ops.ln_gemm_fused(wide[:, :256], cw2)


def test_mlp_takes_the_ln_gemm_branch(report):
    """ops.mlp at a width vip_mlp_fused_supported rejects (ConvNeXt-T stage 2: C = 384) and a row count the default policy takes: LN
    folded into fc1, then fc2 + residual"""
    ops = _ops()
    from vipcup_amd import _abi
    M, C_, hid = 65536 + 37, 384, 1536
    assert not _abi.lib().vip_mlp_fused_supported(M, C_, hid, 3)
    g = torch.Generator().manual_seed(M + C_ + hid)
    x = h(torch.randn(M, C_, generator=g) * 1.5 + 0.3)
    w1 = h(torch.randn(C_, hid, generator=g) / math.sqrt(C_))
    b1 = torch.randn(hid, generator=g) * 0.1
    w2 = h(torch.randn(hid, C_, generator=g) / math.sqrt(hid))
    b2 = torch.randn(C_, generator=g) * 0.1
    res = h(torch.randn(M, C_, generator=g))
    lg, lb = torch.randn(C_, generator=g) * 0.2 + 1, torch.randn(C_, generator=g) * 0.1
    f1, f2 = ops.make_dense_weight(w1, b1), ops.make_dense_weight(w2, b2)
    xd, ln = dev(x), (lg.cuda(), lb.cuda(), EPS)
    assert ops.ln_gemm_fused(xd, f1, "gelu")
    ref = R.dense(R.act(R.dense(R.layernorm(x, lg, lb, EPS), w1, b1), "gelu"), w2, b2) + res
    run = lambda: ops.mlp(xd, f1, f2, act="gelu", residual=dev(res), ln=ln)  # noqa: E731
    got = run()
    torch.cuda.synchronize()
    check(report, f"mlp via ln_dense M{M} C{C_} hid{hid}", got, ref, tol=4e-3)
    assert torch.equal(got, run())
