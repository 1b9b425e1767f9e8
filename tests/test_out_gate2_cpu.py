"""CPU: the two-output form of the output-gated epilogue (vip_conv2d_out_gated2_nhwc_f16) and the folded ECA tail of ECA-NFNet - the
host side.

* the dry run (vip_conv2d_out_gated2_variant, host code alone) selects for every row of tests/_out_gate_cases.py the instantiation the
  one-output call selects, and declines what that call declines and every second activation but SiLU;
* ops.se_fold(d4, eca): the ECA matrix folded with deep_4 is (band / 2 alpha) . W4' with the bias (band / 2 alpha) . b4' (fp64), to the
  rounding of its two fp16 terms; it is rebuilt after a bias change and bypassed inside ops.calibration() / unfused() / exact_weights()
  and with the switch off;
* through tests/emul_ops.py the folded wiring of a small NormFreeNet gives the logits of the three-call graph;
* the two-output instantiations carry no scratch and at most 256 VGPRs (the code objects' metadata, read with llvm-readelf)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

from tests import _out_gate_cases as T
from tests import emul_ops

LLVM = "/opt/rocm/lib/llvm/bin"


def _ops():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    return ops


@pytest.mark.parametrize("B,K,N,hilo,inst,what", T.ROWS, ids=T.IDS)
def test_dry_run_selects_what_the_one_output_call_selects(B, K, N, hilo, inst, what):
    ops = _ops()
    for relu in (False, True):
        d = T.desc(B, K, N, relu, (K + 7) // 8 * 8)
        one, two = ops.out_gate_variant(d, hilo), ops.out_gate2_variant(d, hilo, "silu")
        assert one is not None and two == one + " y2", (one, two, what)
        assert T.instantiation(two[:-9]) == inst and two[:-9] == ops.conv_kernel_variant(d, True, False, hilo)
        for act2 in (None, "relu", "gelu", "sigmoid"):          # the second output is built for SiLU
            assert ops.out_gate2_variant(d, hilo, act2) is None, act2
    d.ldy, d.cout_off = N + 8, 8
    assert ops.out_gate2_variant(d, hilo) is None


def test_dry_run_declines_what_the_one_output_call_declines():
    ops = _ops()
    from vipcup_amd import _abi
    for B, H, W, K, N, k, hilo, why in T.DECLINED:
        d = T.desc(B, K, N, False, (k * k * K + 7) // 8 * 8, k, H, W)
        assert ops.conv_kernel_variant(d, True, False, hilo) is not None, why
        assert ops.out_gate2_variant(d, hilo) is None, why
    lib = _abi.lib()
    p = C.c_void_p(64)
    d = T.desc(11, 184, 64, False, 184)
    silu = ops._act("silu")
    assert lib.vip_conv2d_out_gated2_nhwc_f16(p, p, p, None, p, p, p, p, silu, C.byref(d), None) == -3 and b"output gate" in lib.vip_last_error()
    d = T.desc(11, 56, 64, False, 56)
    assert lib.vip_conv2d_out_gated2_nhwc_f16(p, p, None, None, p, p, p, None, silu, C.byref(d), None) == -1          # no second output
    assert lib.vip_conv2d_out_gated2_nhwc_f16(p, p, None, None, None, p, p, p, silu, C.byref(d), None) == -1          # no gate
    assert lib.vip_conv2d_out_gated2_nhwc_f16(p, p, None, None, p, p, p, p, ops._act("relu"), C.byref(d), None) == -3


ALPHA = 0.2


def _eca_block(hid=16, seed=0, k=5):
    """deep_4 (attn_gain * alpha folded in, as NormFreeNet builds it) and the banded ECA matrix / (2 alpha)"""
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    oc = 4 * hid
    w4 = torch.randn(1, 1, hid, oc, generator=g) / hid ** 0.5 * (2.0 * ALPHA)
    b4 = torch.randn(oc, generator=g) * 0.1 * (2.0 * ALPHA)
    wk = torch.randn(k, generator=g) * 0.5
    band = torch.zeros(oc, oc)
    for j in range(k):
        off = j - k // 2
        idx = torch.arange(max(0, -off), min(oc, oc - off))
        band[idx + off, idx] = wk[j]
    return ops.make_conv_weight(w4, b4, device="cpu"), ops.make_dense_weight(band / (2.0 * ALPHA), None, "cpu")


def test_eca_fold_is_the_band_times_deep_4():
    ops = _ops()
    d4, eca = _eca_block()
    assert ops.eca_tail_folded(d4, eca) and eca.bias is None
    fold = ops.se_fold(d4, eca)
    assert (fold.cin, fold.cout, fold.kh, fold.kw, fold.groups) == (16, 64, 1, 1, 1)
    W = eca.w.double() @ d4.w.double()                   # eca.w = fp16(band / 2 alpha) [oc, oc], d4.w = W4' [oc, hid]
    bvec = eca.w.double() @ d4.bias.double()
    # two terms: hi = rn16(W), lo = rn16(W - hi) leaves 2^-22 relative (2^-25 absolute where lo is subnormal); 2^-24: W went through fp32
    assert fold.w_lo is not None and torch.equal(fold.w, W.float().to(torch.float16))
    assert (((fold.w.double() + fold.w_lo.double()) - W).abs() <= (2.0 ** -22 + 2.0 ** -24) * W.abs() + 2.0 ** -25).all()
    assert ((fold.bias.double() - bvec).abs() <= 2.0 ** -23 * bvec.abs() + 1e-30).all()
    # and it gates what the three calls gate: sigmoid(band' . mean(W4' z + b4')) = sigmoid(fold . mean(z) + fold bias), in fp64
    z = torch.randn(3, 7, 7, 16, generator=torch.Generator().manual_seed(1)).double()
    three = torch.sigmoid((z.reshape(3, 49, 16) @ d4.w.double().t() + d4.bias.double()).mean(1) @ eca.w.double().t())
    folded = torch.sigmoid(z.reshape(3, 49, 16).mean(1) @ (fold.w.double() + fold.w_lo.double()).t() + fold.bias.double())
    assert (three - folded).abs().max() < 1e-6


def test_eca_fold_is_rebuilt_after_a_bias_change():
    ops = _ops()
    d4, eca = _eca_block(seed=1)
    f0 = ops.se_fold(d4, eca)
    assert ops.se_fold(d4, eca) is f0
    d4.bias = (d4.bias + 0.5).contiguous()               # what ops._bias_correct does: a NEW tensor
    f1 = ops.se_fold(d4, eca)
    assert f1 is not f0 and ops.se_fold(d4, eca) is f1
    want = eca.w.double() @ d4.bias.double()
    assert ((f1.bias.double() - want).abs() <= 2.0 ** -23 * want.abs() + 1e-30).all()
    assert torch.equal(f1.w, f0.w) and torch.equal(f1.w_lo, f0.w_lo)
    eca.bias = torch.full((eca.cout,), 0.25)             # bias calibration gives the ECA layer a bias
    f2 = ops.se_fold(d4, eca)
    assert f2 is not f1 and torch.allclose(f2.bias, f1.bias + 0.25, atol=1e-6)


def test_folded_eca_tail_is_bypassed_while_calibrating():
    ops = _ops()
    d4, eca = _eca_block()
    assert ops.eca_tail_folded(d4, eca)
    for ctx in (ops.calibration, ops.unfused, ops.exact_weights):
        with ctx():
            assert not ops.eca_tail_folded(d4, eca), ctx.__name__
    assert ops.eca_tail_folded(d4, eca)
    old = ops._SE_TAIL
    try:
        ops._SE_TAIL = False
        assert not ops.eca_tail_folded(d4, eca)
    finally:
        ops._SE_TAIL = old
    with ops.precision("f32"):
        s4 = ops.make_conv_weight(torch.randn(1, 1, 16, 64), None, device="cpu")
    assert not ops.eca_tail_folded(s4, eca)               # the strict storages keep the three calls


def test_folded_wiring_gives_the_three_call_logits_in_emulation(monkeypatch):
    """The host graph of a small NormFreeNet on the CPU (tests/emul_ops.py; off the GPU conv2d_out_gated is its two launches), folded
    against three-call.  In exact arithmetic the two are one function; what differs without rounding is the fold's two fp16 terms
    (2^-22 per element) and fp32 summation order: 1e-5 of the logit scale.  With every operator output rounded to fp16 the three-call
    graph also rounds the pooled map's source (deep_4's output, before the pool) and the stem's un-activated output, which the folded
    graph never forms: 2^-11 relative per block on the residual branch, 6 blocks and the stem -> 3.5e-3."""
    ops = _ops()
    from vipcup_amd import kecam_models as km
    cfg = dict(km.NFNET_L0, num_blocks=(1, 2, 2, 1), out_channels=(64, 128, 256, 256), stem_width=32, group_size=16)
    p = km.nfnet_synth_params(7, cfg=cfg)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 64, 64, 3, generator=g).to(torch.float16).to(torch.float32)
    seen = []
    for round_act, tol in ((False, 1e-5), (True, 3.5e-3)):
        z = {}
        for folded in (True, False):
            monkeypatch.setattr(ops, "_SE_TAIL", folded)
            with torch.no_grad(), emul_ops.patched(round_act=round_act):
                pooled, saa = [], []
                inner_gap, inner_saa = ops.global_avgpool, ops.scale_add_act
                monkeypatch.setattr(ops, "global_avgpool", lambda x_, *a, **k: (pooled.append(x_.shape[-1]), inner_gap(x_, *a, **k))[1])
                monkeypatch.setattr(ops, "scale_add_act", lambda x_, s_=None, *a, **k: (saa.append(s_ is None), inner_saa(x_, s_, *a, **k))[1])
                m = km.NormFreeNet(p, cfg=cfg, device="cpu")
                z[folded] = m.logits(emul_ops.to_device_nhwc8(x)).float()
                monkeypatch.setattr(ops, "global_avgpool", inner_gap)
                monkeypatch.setattr(ops, "scale_add_act", inner_saa)
            # the gate pools deep_4's input (oc / 4 channels) when folded, its output otherwise (the last pool is the head's)
            want = [oc // (4 if folded else 1) for oc, nb in zip(cfg["out_channels"], cfg["num_blocks"]) for _ in range(nb)]
            assert pooled[:len(want)] == want, (folded, pooled)
            # the un-gated pass over the stem's output (scale is None) runs only in the three-call graph
            assert saa.count(True) == (0 if folded else 1), (folded, saa)
        err = (z[True] - z[False]).abs().max().item()
        seen.append(err)
        assert err <= tol * max(1.0, z[False].abs().max().item()), (round_act, err, z)
    assert max(seen) > 0, "the two graphs round differently: identical logits mean the folded path did not run"


def _kernel_resources(pattern):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import build
    lib = build.build_lib()
    tmp = tempfile.mkdtemp(prefix="out_gate2_res_")
    seen = {}
    try:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", so], capture_output=True, text=True, check=True)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", os.path.join(tmp, f)], capture_output=True, text=True, check=True).stdout
            for blk in re.split(r"\n\s*- \.agpr_count:", notes):       # one block per kernel of amdhsa.kernels
                name = re.search(r"\.name:\s+(\S+)", blk)
                if not name or not re.search(pattern, name.group(1)):
                    continue
                seen[name.group(1)] = tuple(int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                                            for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return seen


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-objdump") or not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm tools in this image")
def test_two_output_kernels_have_no_scratch():
    # pw_gemm_kernel<KS, 4, PRE, HILO, OG = true, Y2 = true> and pwk_direct_kernel<NG, GATED = false, PT, OG2 = true> (Itanium names)
    seen = _kernel_resources(r"pw_gemm_kernelILi\d+ELi4ELb[01]ELb[01]ELb1ELb1EEE|pwk_direct_kernelILi\d+ELb0ELi\d+ELb1EEE")
    pw = sorted((int(m.group(1)), int(m.group(2))) for m in (re.search(r"pw_gemm_kernelILi(\d+)ELi4ELb[01]ELb([01])E", k) for k in seen) if m)
    pwk = sorted((int(m.group(1)), int(m.group(2))) for m in (re.search(r"pwk_direct_kernelILi(\d+)ELb0ELi(\d+)ELb1E", k) for k in seen) if m)
    assert pw == [(ks, hilo) for ks in (1, 2, 3, 4) for hilo in (0, 1)], seen         # the metadata really listed every instantiation
    assert pwk == [(1, 1), (1, 4), (2, 1), (2, 4)], seen
    assert all(v[0] == 0 and v[1] == 0 and v[2] <= 256 for v in seen.values()), seen
