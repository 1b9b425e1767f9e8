"""GPU: the output-gated epilogue of the block-final 1x1 layers (vip_conv2d_out_gated_nhwc_f16, modes 7 / 8 of pw_gemm_kernel and
pwk_direct_kernel) - out = post((x . W + b) * g[image, channel] + residual) - one row per instantiation the mode is built for
(tests/_out_gate_cases.py), each proven by the dry run before it is launched:

1. exact operands: small integers and power-of-two gates, every partial sum exact in fp32 -> ``torch.equal`` with the fp64 reference
   (tests/test_se_tail_cpu.py shows that the reference itself is exact for them);
2. gate == 1.0: bit-identical to the residual (mode 5) and residual + ReLU (mode 6) launches of ``ops.conv2d``;
3. random operands against the fp64 reference at 2e-3 of the output scale - the bound tests/test_gpu_ops.py holds the residual epilogue
   of the same kernels to (``check``: the fp16 rounding of the output; the only new arithmetic is one fp32 multiply);
4. the same launch twice, bit for bit."""
import pytest
import torch

from tests import _out_gate_cases as T

pytestmark = pytest.mark.gpu


def _ops():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    return ops


def _dev(t):
    return t.to(torch.float16).cuda().contiguous()


_cache = {}


def _row(B, K, N, hilo, kind):
    """operands of a row with both references (no ReLU / ReLU), built once per row and left unchanged (the row's cases are consecutive)"""
    key = (B, K, N, hilo, kind)
    if key not in _cache:
        _cache.clear()
        x, w, b, planes, r = T.exact_operands(B, K, N, hilo) if kind == "exact" else T.random_operands(B, K, N, hilo)
        _cache[key] = (x, w, b, planes, r, {relu: T.reference(x, w, b, planes, r, relu) for relu in (False, True)})
    return _cache[key]


def _launch(ops, B, K, N, hilo, inst, x, w, b, planes, r, relu):
    """the dry run proves the selection, then the one-launch form runs (a fallback to two launches would fail the assert, not hide)"""
    cw = ops.make_conv_weight(w, b, hilo=hilo)
    assert (cw.w_lo is not None) == hilo
    d = T.desc(B, K, N, relu, cw.ldw)
    variant = ops.out_gate_variant(d, hilo)
    assert variant is not None and variant.endswith(" ogate") and T.instantiation(variant[:-6]) == inst, (variant, inst)
    assert variant[:-6] == ops.conv_kernel_variant(d, True, False, hilo), "the gated call must select what the residual call selects"
    xd, gd, rd = _dev(x), _dev(planes), _dev(r)
    act = "relu" if relu else None
    assert ops._out_gate_desc(xd, cw, gd, rd, act) is not None
    return cw, xd, gd, rd, ops.conv2d_out_gated(xd, cw, gd, rd, act)


@pytest.mark.parametrize("relu", [False, True], ids=["res", "res-relu"])
@pytest.mark.parametrize("B,K,N,hilo,inst,what", T.ROWS, ids=T.IDS)
def test_out_gate_exact_operands(B, K, N, hilo, inst, what, relu, report):
    ops = _ops()
    x, w, b, planes, r, refs = _row(B, K, N, hilo, "exact")
    cw, xd, gd, rd, got = _launch(ops, B, K, N, hilo, inst, x, w, b, planes, r, relu)
    torch.cuda.synchronize()
    ref16 = refs[relu].to(torch.float16)
    bad = (got.cpu() != ref16)
    if bad.any():
        idx = bad.reshape(-1, N).nonzero()[0].tolist()
        report(f"[out_gate] {inst} exact: first mismatch at row {idx[0]} (image {idx[0] // 49}), channel {idx[1]}; {int(bad.sum())} differ")
    assert torch.equal(got.cpu(), ref16), what


@pytest.mark.parametrize("relu", [False, True], ids=["res", "res-relu"])
@pytest.mark.parametrize("B,K,N,hilo,inst,what", T.ROWS, ids=T.IDS)
def test_out_gate_random_operands(B, K, N, hilo, inst, what, relu, report):
    ops = _ops()
    x, w, b, planes, r, refs = _row(B, K, N, hilo, "random")
    cw, xd, gd, rd, got = _launch(ops, B, K, N, hilo, inst, x, w, b, planes, r, relu)
    again = ops.conv2d_out_gated(xd, cw, gd, rd, "relu" if relu else None)
    ones = torch.zeros_like(gd)
    ones[:, 0] = 1.0
    unit = ops.conv2d_out_gated(xd, cw, ones, rd, "relu" if relu else None)
    plain = ops.conv2d(xd, cw, residual=rd, act_post="relu" if relu else None)
    torch.cuda.synchronize()
    ref = refs[relu]
    scale = ref.abs().max().item() + 1e-6
    err = (got.cpu().double() - ref).abs().max().item()
    report(f"[out_gate] {inst} {B}x7x7x{K}->{N}{' relu' if relu else ''}: max_abs_err={err:.3e} ref_absmax={scale:.3e} rel={err / scale:.3e}")
    assert torch.isfinite(got).all()
    assert err <= 2e-3 * scale, what
    assert torch.equal(got, again), "two launches on the same operands must agree bit for bit"
    assert torch.equal(unit, plain), "a gate of 1.0 must reproduce the residual epilogue bit for bit"


def test_out_gate_fallback_is_two_launches(report):
    """a shape the gated kernels decline (K = 184 on the streaming kernel) takes conv2d + scale_add_act: same values as the two calls"""
    ops = _ops()
    B, K, N = 11, 184, 64
    x, w, b, planes, r = T.random_operands(B, K, N)
    cw = ops.make_conv_weight(w, b, hilo=True)
    xd, gd, rd = _dev(x), _dev(planes), _dev(r)
    assert ops._out_gate_desc(xd, cw, gd, rd, "relu") is None
    got = ops.conv2d_out_gated(xd, cw, gd, rd, "relu")
    two = ops.scale_add_act(ops.conv2d(xd, cw), gd, rd, "relu")
    torch.cuda.synchronize()
    assert torch.equal(got, two)
