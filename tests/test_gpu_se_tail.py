"""GPU: the squeeze-excite gate computed from conv_3's INPUT through the folded reduce layer (ops.se_fold + ops.se_gate on z) against an
fp64 gate from the fp32 master weights - pool(z W3 + b3) -> reduce -> ReLU -> expand -> sigmoid - at the tolerance tests/test_gpu_ops.py
(test_se_gate) holds ops.se_gate to: 2e-5 of the gate scale for the one-launch kernel, 4e-5 for the pool + two split GEMMs of the wide
gates.  As there, the master weights are fp16-representable, so that what is measured is the gate arithmetic and - new here - the
rounding of the FOLDED matrix Wr W3, which is not representable: as ONE fp16 term it alone put the gate at 3.8e-5 / 5.5e-5, so the fold
carries two (measured 2.0e-7 / 2.9e-7).  The three-call path (conv_3 stored as fp16, its pooled output through the unfolded reduce layer)
goes through the same comparison and is printed, not asserted: 2.7e-5 / 4.8e-5, the fp16 rounding of the pooled map.

One block shape per stage class: the two-term-weight stages (1, 2: one-launch gate kernel) on a 13 x 13 map, and the deep stages (3, 4:
f = 256 is the smallest width whose folded gate still exceeds the one-launch kernel's weight budget) on a 7 x 7 map."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, H, W, f, two-term conv_3 weights, gate path, tolerance of test_se_gate for that path)
BLOCKS = [(3, 13, 13, 64, True, "fused", 2e-5), (2, 7, 7, 256, False, "wide", 4e-5)]


def _h(t):
    return t.to(torch.float16).to(torch.float32)


@pytest.mark.parametrize("B,H,W,f,hilo,path,tol", BLOCKS, ids=[f"f{b[3]}-{b[1]}x{b[2]}-{b[5]}" for b in BLOCKS])
def test_gate_from_pooled_input(B, H, W, f, hilo, path, tol, report):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    C4, r = 4 * f, f
    g = torch.Generator().manual_seed(f * 31 + H)
    z = _h(torch.relu(torch.randn(B, H, W, f, generator=g) + 0.3))                  # conv_2's output: post-ReLU
    w3 = _h(torch.randn(1, 1, f, C4, generator=g) / math.sqrt(f) * 0.5)
    b3 = torch.randn(C4, generator=g) * 0.1
    wr = _h(torch.randn(1, 1, C4, r, generator=g) / math.sqrt(C4) * 3)
    br = torch.randn(r, generator=g) * 0.1
    we = _h(torch.randn(1, 1, r, C4, generator=g) / math.sqrt(r) * 2)
    be = torch.randn(C4, generator=g) * 0.1
    # fp64 from the master weights
    y = z.double().reshape(B, H * W, f) @ w3.double()[0, 0] + b3.double()
    hid = torch.relu(y.mean(1) @ wr.double()[0, 0] + br.double())
    ref = torch.sigmoid(hid @ we.double()[0, 0] + be.double())
    c3 = ops.make_conv_weight(w3, b3, hilo=hilo)
    se_r, se_e = ops.make_conv_weight(wr, br), ops.make_conv_weight(we, be)
    assert (c3.w_lo is not None) == hilo and ops.se_tail_folded(c3, se_r, se_e)
    fold = ops.se_fold(c3, se_r)
    assert (fold.cin, fold.cout) == (f, r)
    assert ops._se_chain_ok(fold, se_e, f) == (path == "fused") and ops._se_chain_ok(se_r, se_e, C4) == (path == "fused"), \
        "the folded gate must take the path the unfolded one takes on this stage"
    zd = z.to(torch.float16).cuda()
    new = ops.se_gate(zd, fold, se_e, "relu", "sigmoid")
    old = ops.se_gate(ops.conv2d(zd, c3), se_r, se_e, "relu", "sigmoid")
    torch.cuda.synchronize()
    assert new.shape == (B, 2, C4)
    scale = ref.abs().max().item() + 1e-6
    e_new = ((new[:, 0].double() + new[:, 1].double()).cpu() - ref).abs().max().item()
    e_old = ((old[:, 0].double() + old[:, 1].double()).cpu() - ref).abs().max().item()
    report(f"[se_tail] gate f={f} {H}x{W} {path}: from pooled z (folded) max_abs_err={e_new:.3e}, from pooled fp16 y (parent) {e_old:.3e}, "
           f"bound {tol * scale:.3e}")
    assert e_new <= tol * scale, (e_new, e_old, tol * scale)
    assert torch.equal(new, ops.se_gate(zd, fold, se_e, "relu", "sigmoid"))
