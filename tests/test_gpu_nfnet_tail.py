"""GPU: the folded block tail of ECA-NFNet.

1. The ECA gate computed from deep_4's INPUT - pool(z) through ops.se_fold(d4, eca) - against an fp64 gate from the master weights,
   sigmoid(band' . mean_hw(z W4 + b4)), in the construction of tests/test_gpu_se_tail.py: the master weights are fp16-representable, so
   what is measured is the gate arithmetic and the rounding of the folded matrix (two fp16 terms).  The bound is the 4e-5 of the gate
   scale that tests/test_gpu_ops.py (test_se_gate) holds the pool + split-GEMM gate chain to.  The three-call path (deep_4's output
   stored as fp16, pooled, through the unfolded ECA matrix) goes through the same comparison and is printed, not asserted.
   One block of the streaming-kernel stages (hid = 64, 13 x 13) and one of the deep stages (hid = 384, 7 x 7); oc = 4 hid.
2. The member: the reduced-depth NormFreeNet of tests/test_gpu_kecam.py against the fp32 oracle, folded and with the switch off; the
   folded logits stay inside that file's 6e-3, both errors and their difference are printed."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ALPHA = 0.2
BLOCKS = [(3, 13, 13, 64), (2, 7, 7, 384)]


def _h(t):
    return t.to(torch.float16).to(torch.float32)


@pytest.mark.parametrize("B,H,W,hid", BLOCKS, ids=[f"hid{b[3]}-{b[1]}x{b[2]}" for b in BLOCKS])
def test_eca_gate_from_pooled_input(B, H, W, hid, report):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import kecam_models as km, ops
    oc = 4 * hid
    g = torch.Generator().manual_seed(hid * 31 + H)
    z = torch.randn(B, H, W, hid, generator=g) + 0.3
    z = _h(z * torch.sigmoid(z))                                                     # deep_3's output: post-SiLU
    w4 = _h(torch.randn(1, 1, hid, oc, generator=g) / math.sqrt(hid) * (2.0 * ALPHA))  # attn_gain * alpha folded in, as the model has it
    b4 = torch.randn(oc, generator=g) * 0.1 * (2.0 * ALPHA)
    k = km.eca_kernel_size(oc)
    wk = torch.randn(k, generator=g) * 0.5
    band = torch.zeros(oc, oc)
    for j in range(k):
        off = j - k // 2
        idx = torch.arange(max(0, -off), min(oc, oc - off))
        band[idx + off, idx] = wk[j]
    band = _h(band / (2.0 * ALPHA))                                                  # [in, out], undoing the folded gain
    # fp64 from the master weights
    y = z.double().reshape(B, H * W, hid) @ w4.double()[0, 0] + b4.double()
    ref = torch.sigmoid(y.mean(1) @ band.double())
    d4, eca = ops.make_conv_weight(w4, b4), ops.make_dense_weight(band, None)
    assert d4.w_lo is None and ops.eca_tail_folded(d4, eca)
    fold = ops.se_fold(d4, eca)
    assert (fold.cin, fold.cout) == (hid, oc) and fold.w_lo is not None
    zd = z.to(torch.float16).cuda()
    new = ops.dense_split(ops.global_avgpool(zd, split=True), fold, act="sigmoid")
    old = ops.dense_split(ops.global_avgpool(ops.conv2d(zd, d4), split=True), eca, act="sigmoid")
    torch.cuda.synchronize()
    assert new.shape == (B, 2, oc)
    scale = ref.abs().max().item() + 1e-6
    e_new = ((new[:, 0].double() + new[:, 1].double()).cpu() - ref).abs().max().item()
    e_old = ((old[:, 0].double() + old[:, 1].double()).cpu() - ref).abs().max().item()
    report(f"[nfnet_tail] gate hid={hid} {H}x{W}: from pooled z (folded) max_abs_err={e_new:.3e}, from pooled fp16 d (parent) {e_old:.3e}, "
           f"bound {4e-5 * scale:.3e}")
    assert e_new <= 4e-5 * scale, (e_new, e_old, 4e-5 * scale)
    assert torch.equal(new, ops.dense_split(ops.global_avgpool(zd, split=True), fold, act="sigmoid"))


def test_member_logits_folded_and_three_call(report, monkeypatch):
    import vipcup_amd  # noqa: F401
    from oracle import kecam_ref as ref
    from tests.test_gpu_resnet_rs import _images
    from vipcup_amd import kecam_models as km, ops
    x = _images(2, 200).to(torch.float16).to(torch.float32)
    xd = ops.to_device_nhwc8(x)
    cfg = dict(km.NFNET_L2, num_blocks=(1, 2, 2, 1))
    p = km.nfnet_synth_params(1025, cfg=cfg)
    with torch.no_grad():
        f = ref.nfnet_features(p, x, num_blocks=cfg["num_blocks"], num_features_factor=cfg["num_features_factor"])
        z_ref = ref.R.dense(ref.R.global_avgpool(f), p["predictions/kernel"], p["predictions/bias"])
    m = km.NormFreeNet(p, cfg=cfg)
    launches = []
    inner = ops.conv2d_out_gated
    monkeypatch.setattr(ops, "conv2d_out_gated", lambda *a, **k: (launches.append(1), inner(*a, **k))[1])
    assert ops._SE_TAIL, "the default is the folded tail"
    z_new = m.logits(xd).cpu()
    assert len(launches) == sum(cfg["num_blocks"]), "every block takes the folded tail"
    monkeypatch.setattr(ops, "_SE_TAIL", False)
    z_old = m.logits(xd).cpu()
    assert len(launches) == sum(cfg["num_blocks"])
    torch.cuda.synchronize()
    e_new, e_old = (z_new - z_ref).abs().max().item(), (z_old - z_ref).abs().max().item()
    report(f"[nfnet_tail] ECA_NFNetL2 d1221 logit max_abs_err vs fp32 oracle: folded {e_new:.3e}, VIP_SE_TAIL=0 {e_old:.3e}, "
           f"difference {e_new - e_old:+.3e} (logit absmax {z_ref.abs().max().item():.3f})")
    assert e_new < 6e-3 * max(1.0, z_ref.abs().max().item())
