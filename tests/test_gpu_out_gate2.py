"""GPU: the two-output form of the output-gated epilogue (vip_conv2d_out_gated2_nhwc_f16: pw_gemm_kernel<.., OG, Y2> and
pwk_direct_kernel<.., OG2>) - y = post((x . W + b) * g[image, channel] + residual) and y2 = silu(y) from the rounded y - one row per
instantiation that is built with the second output: the rows of tests/_out_gate_cases.py (7 x 7 maps: tiles straddle image boundaries,
ragged last tiles, K tails), each proven by the dry run before it is launched.

1. exact operands (every partial sum exact in fp32): ``y`` is ``torch.equal`` to the fp64 reference rounded once, and ``y2`` is
   ``torch.equal`` to ``ops.scale_add_act(y, None, None, "silu")`` on the returned ``y`` - the elementwise kernel the epilogue replaces;
2. random operands: ``y`` within 2e-3 of the output scale (the bound tests/test_gpu_out_gate.py holds the one-output epilogue to),
   ``torch.equal`` to the one-output call, two launches bit for bit, a gate of 1.0 reproduces the residual epilogue; ``y2`` as in 1;
3. where the call declines, ``conv2d_out_gated(..., act2=)`` is the two launches, bit for bit."""
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
    variant = ops.out_gate2_variant(d, hilo, "silu")
    assert variant is not None and variant.endswith(" ogate y2") and T.instantiation(variant[:-9]) == inst, (variant, inst)
    assert variant[:-9] == ops.conv_kernel_variant(d, True, False, hilo), "the two-output call must select what the residual call selects"
    xd, gd, rd = _dev(x), _dev(planes), _dev(r)
    act = "relu" if relu else None
    assert ops._out_gate_desc(xd, cw, gd, rd, act) is not None
    y, y2 = ops.conv2d_out_gated(xd, cw, gd, rd, act, act2="silu")
    return cw, xd, gd, rd, y, y2


def _second_output_is_the_elementwise_kernels(ops, y, y2, inst, report):
    want = ops.scale_add_act(y, None, None, "silu")          # the parent's kernel on the returned y
    torch.cuda.synchronize()
    bad = y2 != want
    if bad.any():
        report(f"[out_gate2] {inst}: y2 differs from scale_add_act(y) at {int(bad.sum())} of {bad.numel()} elements")
    assert y2.shape == y.shape and y2.dtype == torch.float16 and torch.equal(y2, want)


@pytest.mark.parametrize("relu", [False, True], ids=["res", "res-relu"])
@pytest.mark.parametrize("B,K,N,hilo,inst,what", T.ROWS, ids=T.IDS)
def test_out_gate2_exact_operands(B, K, N, hilo, inst, what, relu, report):
    ops = _ops()
    x, w, b, planes, r, refs = _row(B, K, N, hilo, "exact")
    cw, xd, gd, rd, y, y2 = _launch(ops, B, K, N, hilo, inst, x, w, b, planes, r, relu)
    torch.cuda.synchronize()
    ref16 = refs[relu].to(torch.float16)
    bad = (y.cpu() != ref16)
    if bad.any():
        idx = bad.reshape(-1, N).nonzero()[0].tolist()
        report(f"[out_gate2] {inst} exact: first mismatch at row {idx[0]} (image {idx[0] // 49}), channel {idx[1]}; {int(bad.sum())} differ")
    assert torch.equal(y.cpu(), ref16), what
    _second_output_is_the_elementwise_kernels(ops, y, y2, inst, report)


@pytest.mark.parametrize("relu", [False, True], ids=["res", "res-relu"])
@pytest.mark.parametrize("B,K,N,hilo,inst,what", T.ROWS, ids=T.IDS)
def test_out_gate2_random_operands(B, K, N, hilo, inst, what, relu, report):
    ops = _ops()
    act = "relu" if relu else None
    x, w, b, planes, r, refs = _row(B, K, N, hilo, "random")
    cw, xd, gd, rd, y, y2 = _launch(ops, B, K, N, hilo, inst, x, w, b, planes, r, relu)
    y_again, y2_again = ops.conv2d_out_gated(xd, cw, gd, rd, act, act2="silu")
    one = ops.conv2d_out_gated(xd, cw, gd, rd, act)
    ones = torch.zeros_like(gd)
    ones[:, 0] = 1.0
    unit, _ = ops.conv2d_out_gated(xd, cw, ones, rd, act, act2="silu")
    plain = ops.conv2d(xd, cw, residual=rd, act_post=act)
    torch.cuda.synchronize()
    ref = refs[relu]
    scale = ref.abs().max().item() + 1e-6
    err = (y.cpu().double() - ref).abs().max().item()
    report(f"[out_gate2] {inst} {B}x7x7x{K}->{N}{' relu' if relu else ''}: max_abs_err={err:.3e} ref_absmax={scale:.3e} rel={err / scale:.3e}")
    assert torch.isfinite(y).all() and torch.isfinite(y2).all()
    assert err <= 2e-3 * scale, what
    assert torch.equal(y, one), "the first output must be the one-output call's, bit for bit"
    assert torch.equal(y, y_again) and torch.equal(y2, y2_again), "two launches on the same operands must agree bit for bit"
    assert torch.equal(unit, plain), "a gate of 1.0 must reproduce the residual epilogue bit for bit"
    _second_output_is_the_elementwise_kernels(ops, y, y2, inst, report)


def test_out_gate2_fallback_is_two_launches():
    """a shape the gated kernels decline (K = 184 on the streaming kernel) and a second activation that is not built take conv2d +
    scale_add_act with its second output: the same values as the two calls"""
    ops = _ops()
    B, K, N = 11, 184, 64
    x, w, b, planes, r = T.random_operands(B, K, N)
    cw = ops.make_conv_weight(w, b, hilo=True)
    xd, gd, rd = _dev(x), _dev(planes), _dev(r)
    assert ops._out_gate_desc(xd, cw, gd, rd, None) is None
    y, y2 = ops.conv2d_out_gated(xd, cw, gd, rd, None, act2="silu")
    t, t2 = ops.scale_add_act(ops.conv2d(xd, cw), gd, rd, None, act2="silu")
    torch.cuda.synchronize()
    assert torch.equal(y, t) and torch.equal(y2, t2)
    B, K, N = 11, 56, 136
    x, w, b, planes, r = T.random_operands(B, K, N, True)
    cw = ops.make_conv_weight(w, b, hilo=True)
    xd, gd, rd = _dev(x), _dev(planes), _dev(r)
    assert ops._out_gate_desc(xd, cw, gd, rd, None) is not None        # the shape is taken, the second activation is not
    y, y2 = ops.conv2d_out_gated(xd, cw, gd, rd, None, act2="relu")
    t, t2 = ops.scale_add_act(ops.conv2d(xd, cw), gd, rd, None, act2="relu")
    torch.cuda.synchronize()
    assert torch.equal(y, t) and torch.equal(y2, t2)
