"""CPU: the folded squeeze-excite tail of ResNet-RS (gate from conv_3's input, tail in conv_3's epilogue) - the host side.

* ops.se_fold: the folded reduce layer is Wr W3 and Wr b3 + br (fp64), to the rounding of its two fp16 terms / its fp32 bias; it is kept, built
  again after a bias changed (bias calibration replaces the tensor; an in-place write counts too), and bypassed inside
  ops.calibration() / unfused() / exact_weights();
* through tests/emul_ops.py the folded wiring gives the logits of the three-call graph;
* the dry run (vip_conv2d_out_gated_variant, host code alone) selects for every row of tests/_out_gate_cases.py the instantiation the
  row names - the one the residual call selects - and declines everything else;
* the fp64 reference of tests/test_gpu_out_gate.py's exact-operand check is itself exact for those operands."""
import ctypes as C

import pytest
import torch

from tests import _out_gate_cases as T
from tests import emul_ops


def _ops():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    return ops


def _block(f=16, hilo=True, seed=0):
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    w3 = torch.randn(1, 1, f, 4 * f, generator=g) / f ** 0.5
    b3 = torch.randn(4 * f, generator=g) * 0.1
    wr = torch.randn(1, 1, 4 * f, f, generator=g) / (4 * f) ** 0.5
    br = torch.randn(f, generator=g) * 0.1
    we = torch.randn(1, 1, f, 4 * f, generator=g) / f ** 0.5
    be = torch.randn(4 * f, generator=g) * 0.1
    return (ops.make_conv_weight(w3, b3, device="cpu", hilo=hilo), ops.make_conv_weight(wr, br, device="cpu"),
            ops.make_conv_weight(we, be, device="cpu"))


@pytest.mark.parametrize("hilo", [True, False], ids=["two-term", "one-term"])
def test_fold_is_the_product_of_the_layers(hilo):
    ops = _ops()
    c3, se_r, se_e = _block(16, hilo)
    assert (c3.w_lo is not None) == hilo
    fold = ops.se_fold(c3, se_r)
    assert (fold.cin, fold.cout, fold.kh, fold.kw, fold.groups) == (16, 16, 1, 1, 1) and fold.w.dtype == torch.float16
    w3 = c3.w.double() + (c3.w_lo.double() if hilo else 0)          # what conv_3 multiplies by
    W = se_r.w.double() @ w3
    bvec = se_r.w.double() @ c3.bias.double() + se_r.bias.double()
    # two terms: hi = rn16(W) leaves at most half an fp16 ulp (2^-11 relative), lo = rn16(W - hi) half an ulp of THAT (2^-22 relative to
    # W; 2^-25 absolute where lo is subnormal); 2^-24 relative: W itself passed through fp32
    assert fold.w_lo is not None and fold.w_lo.dtype == torch.float16 and fold.w_lo.shape == fold.w.shape
    assert torch.equal(fold.w, W.float().to(torch.float16))
    assert (((fold.w.double() + fold.w_lo.double()) - W).abs() <= (2.0 ** -22 + 2.0 ** -24) * W.abs() + 2.0 ** -25).all()
    assert ((fold.bias.double() - bvec).abs() <= 2.0 ** -23 * bvec.abs() + 1e-30).all()          # fp32 storage
    if hilo:    # the second weight term is in the fold: dropping it moves the product by more than the rounding does
        assert (se_r.w.double() @ c3.w.double() - W).abs().max() > 0


def test_fold_is_kept_and_rebuilt_after_a_bias_change():
    ops = _ops()
    c3, se_r, se_e = _block(16, True, seed=1)
    f0 = ops.se_fold(c3, se_r)
    assert ops.se_fold(c3, se_r) is f0
    c3.bias = (c3.bias + 0.5).contiguous()                          # what ops._bias_correct does: a NEW tensor
    f1 = ops.se_fold(c3, se_r)
    assert f1 is not f0 and ops.se_fold(c3, se_r) is f1
    want = se_r.w.double() @ c3.bias.double() + se_r.bias.double()
    assert ((f1.bias.double() - want).abs() <= 2.0 ** -23 * want.abs() + 1e-30).all()
    assert (f1.bias - f0.bias).abs().max() > 1e-3
    se_r.bias.add_(0.25)                                            # an in-place write
    f2 = ops.se_fold(c3, se_r)
    assert f2 is not f1 and torch.allclose(f2.bias, f1.bias + 0.25, atol=1e-6)
    assert torch.equal(f2.w, f1.w) and torch.equal(f2.w_lo, f1.w_lo)  # the matrix does not depend on the biases
    other = _block(16, True, seed=2)[1]
    assert ops.se_fold(c3, other) is not f2                         # another reduce layer


def test_folded_tail_is_bypassed_while_calibrating():
    ops = _ops()
    c3, se_r, se_e = _block(16, True)
    assert ops.se_tail_folded(c3, se_r, se_e)
    for ctx in (ops.calibration, ops.unfused, ops.exact_weights):
        with ctx():
            assert not ops.se_tail_folded(c3, se_r, se_e), ctx.__name__
    assert ops.se_tail_folded(c3, se_r, se_e)
    old = ops._SE_TAIL
    try:
        ops._SE_TAIL = False
        assert not ops.se_tail_folded(c3, se_r, se_e)
    finally:
        ops._SE_TAIL = old
    with ops.precision("f32"):
        s3 = ops.make_conv_weight(torch.randn(1, 1, 16, 64), None, device="cpu")
    assert not ops.se_tail_folded(s3, se_r, se_e)                    # the strict storages keep the three calls


def _resnet(p, ba):
    from vipcup_amd import resnet_rs
    return resnet_rs.ResNetRS(p, depth=50, block_args=ba, device="cpu")


def test_folded_wiring_gives_the_three_call_logits_in_emulation(monkeypatch):
    """The product's host graph on the CPU (tests/emul_ops.py), folded against three-call.  In exact arithmetic the two are the same
    function; what differs is the rounding of the folded matrix to two fp16 terms (2^-22 relative per element) and fp32 summation
    order: 1e-5 of the logit scale leaves both two orders of magnitude.  With every operator output rounded to fp16 (round_act) the
    three-call graph also rounds conv_3's un-gated output, which the folded one never forms: there the bound is that rounding, 2^-11
    relative per block on the residual branch, 5 blocks -> 2.5e-3."""
    ops = _ops()
    from vipcup_amd import resnet_rs
    ba = [(64, 2), (128, 1), (256, 1), (512, 1)]
    p = resnet_rs.synth_params(50, seed=3, block_args=ba)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 64, 64, 3, generator=g).to(torch.float16).to(torch.float32)
    seen = []
    for round_act, tol in ((False, 1e-5), (True, 2.5e-3)):
        z = {}
        for folded in (True, False):
            monkeypatch.setattr(ops, "_SE_TAIL", folded)
            with torch.no_grad(), emul_ops.patched(round_act=round_act):
                gate_in = []
                inner = ops.se_gate
                monkeypatch.setattr(ops, "se_gate", lambda x_, *a, **k: (gate_in.append(x_.shape[-1]), inner(x_, *a, **k))[1])
                m = _resnet(p, ba)
                z[folded] = m.logits(emul_ops.to_device_nhwc8(x)).float()
                monkeypatch.setattr(ops, "se_gate", inner)
            # the gate's input: conv_3's input (f channels) when folded, its output (4 f) otherwise
            assert gate_in == [f * (1 if folded else 4) for f, reps in ba for _ in range(reps)], (folded, gate_in)
        err = (z[True] - z[False]).abs().max().item()
        seen.append(err)
        assert err <= tol * max(1.0, z[False].abs().max().item()), (round_act, err, z)
    assert max(seen) > 0, "the two graphs round differently: identical logits mean the folded path did not run"
    # inside calibration() the model runs the three calls whatever the switch says
    monkeypatch.setattr(ops, "_SE_TAIL", True)
    with torch.no_grad(), emul_ops.patched(round_act=False), ops.calibration():
        gate_in = []
        inner = ops.se_gate
        monkeypatch.setattr(ops, "se_gate", lambda x_, *a, **k: (gate_in.append(x_.shape[-1]), inner(x_, *a, **k))[1])
        _resnet(p, ba).logits(emul_ops.to_device_nhwc8(x))
        monkeypatch.setattr(ops, "se_gate", inner)
    assert gate_in == [4 * f for f, reps in ba for _ in range(reps)]


@pytest.mark.parametrize("B,K,N,hilo,inst,what", T.ROWS, ids=T.IDS)
def test_dry_run_selects_the_rows_instantiation(B, K, N, hilo, inst, what):
    ops = _ops()
    for relu in (False, True):
        d = T.desc(B, K, N, relu, (K + 7) // 8 * 8)
        v = ops.out_gate_variant(d, hilo)
        assert v is not None and v.endswith(" ogate") and T.instantiation(v[:-6]) == inst, (v, what)
        assert v[:-6] == ops.conv_kernel_variant(d, True, False, hilo)
    d.act_post = ops._act("silu")                       # only none / ReLU after the residual
    assert ops.out_gate_variant(d, hilo) is None
    d = T.desc(B, K, N, True, (K + 7) // 8 * 8)
    d.ldy, d.cout_off = N + 8, 8                        # the gate indexes the layer's own channels from 0
    assert ops.out_gate_variant(d, hilo) is None


def test_dry_run_declines_every_other_kernel():
    ops = _ops()
    from vipcup_amd import _abi
    for B, H, W, K, N, k, hilo, why in T.DECLINED:
        d = T.desc(B, K, N, True, (k * k * K + 7) // 8 * 8, k, H, W)
        assert ops.conv_kernel_variant(d, True, False, hilo) is not None, why      # the residual call itself is served
        assert ops.out_gate_variant(d, hilo) is None, why
    lib = _abi.lib()
    p = C.c_void_p(64)
    d = T.desc(11, 184, 64, True, 184)
    assert lib.vip_conv2d_out_gated_nhwc_f16(p, p, p, None, p, p, p, C.byref(d), None) == -3 and b"output gate" in lib.vip_last_error()
    assert lib.vip_conv2d_out_gated_nhwc_f16(p, p, None, None, None, p, p, C.byref(d), None) == -1
    assert lib.vip_conv2d_out_gated_nhwc_f16(p, p, None, None, p, None, p, C.byref(d), None) == -1


def test_existing_descriptors_select_what_they_selected():
    """the un-gated queries do not see the new mode: same names with and without the new argument's default"""
    ops = _ops()
    for B, K, N, hilo, inst, what in T.ROWS:
        d = T.desc(B, K, N, True, (K + 7) // 8 * 8)
        assert T.instantiation(ops.conv_kernel_variant(d, True, has_w_lo=hilo)) == inst
        assert "ogate" not in ops.conv_kernel_variant(d, True, has_w_lo=hilo)


@pytest.mark.parametrize("B,K,N,hilo,inst,what", T.ROWS, ids=T.IDS)
def test_exact_operands_reference_is_exact(B, K, N, hilo, inst, what):
    """Every stage of the fp64 reference is representable in fp32 - so any fp32 summation order gives the same value and the stored
    fp16 is one rounding of it - and equals integer arithmetic on the operands scaled by their powers of two."""
    x, w, b, planes, r = T.exact_operands(B, K, N, hilo)
    f16 = lambda t: t.to(torch.float16).to(torch.float32)           # noqa: E731
    assert torch.equal(f16(x), x) and torch.equal(f16(r), r) and torch.equal(f16(planes), planes)
    hi = f16(w)
    assert torch.equal(hi + f16(w - hi), w) and (hilo or torch.equal(hi, w))      # the weight planes carry W exactly
    x2, w2 = x.double().reshape(-1, K), w.double()[0, 0]
    # the largest partial sum in any order: sum |x w| + |b| stays below 2^11, on a grid of 2^-12 (two-term) or 1 -> at most 23 bits
    assert (x2.abs() @ w2.abs() + b.double().abs()).max().item() < 2.0 ** 11
    y = (x2 @ w2 + b.double()).reshape(B, 49, N)
    gsum = (planes[:, 0].double() + planes[:, 1].double())[:, None, :]
    for t in (y, y * gsum, y * gsum + r.double().reshape(B, 49, N)):
        assert torch.equal(t.float().double(), t)
    # integers: x, r, b as they are, W * 2^12, gate * 2^14 (the matrix product in fp64 on integers below 2^23 is integer arithmetic)
    yi = (x2 @ (w2 * 4096) + b.double() * 4096).long()
    gi = (gsum * 16384).long()
    for relu in (False, True):
        ref = T.reference(x, w, b, planes, r, relu)
        assert torch.equal(ref.float().double(), ref)
        want = yi.reshape(B, 49, N) * gi + r.long().reshape(B, 49, N) * (4096 * 16384)
        if relu:
            want = want.clamp_min(0)
        assert torch.equal((ref.reshape(B, 49, N) * (4096.0 * 16384.0)).long(), want)
    # neighbouring images and neighbouring channels never share a gate
    assert (gsum[1:] != gsum[:-1]).all() and (gsum[:, :, 1:] != gsum[:, :, :-1]).all()
