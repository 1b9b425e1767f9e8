"""usage: python tools/bench_nfnet_tail.py  (from the repository root, one GPU) - per stage of eca_nfnet_l0 at batch 256 / 200 px: the block
tail as three launches (deep_4, the ECA gate on its output d, scale_add_act with the second output) against the folded tail (the gate on
deep_4's input z through se_fold, deep_4 with the gate, the shortcut and the second output in its epilogue); median of 30 timed repeats
each, microseconds"""
import math, sys, os
sys.path.insert(0, os.getcwd())
import torch
import vipcup_amd  # noqa
from vipcup_amd import ops, kecam_models as km

def med(fn, n=30):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ts)[n // 2]

B, ALPHA = 256, 0.2
for stage, (oc, hw) in enumerate([(256, 50), (512, 25), (1536, 13), (1536, 7)], 1):
    hid = oc // 4
    g = torch.Generator().manual_seed(stage)
    d4 = ops.make_conv_weight(torch.randn(1, 1, hid, oc, generator=g) / math.sqrt(hid) * 2 * ALPHA, torch.randn(oc, generator=g) * 0.1)
    k = km.eca_kernel_size(oc)
    band = torch.zeros(oc, oc)
    for j in range(k):
        off = j - k // 2
        idx = torch.arange(max(0, -off), min(oc, oc - off))
        band[idx + off, idx] = float(torch.randn(1, generator=g)) * 0.5
    eca = ops.make_dense_weight(band / (2 * ALPHA), None)
    z = torch.randn(B, hw, hw, hid, generator=g)
    z = (z * torch.sigmoid(z)).to(torch.float16).cuda()
    sc = torch.randn(B, hw, hw, oc, generator=g).to(torch.float16).cuda()
    fold = ops.se_fold(d4, eca)
    d = ops.conv2d(z, d4)
    gate_old = lambda: ops.dense_split(ops.global_avgpool(d, split=True), eca, act="sigmoid")
    gate_new = lambda: ops.dense_split(ops.global_avgpool(z, split=True), fold, act="sigmoid")
    a = gate_new()
    desc = ops._out_gate_desc(z, d4, a, sc, None)
    t_gold, t_gnew = med(gate_old), med(gate_new)
    t_conv = med(lambda: ops.conv2d(z, d4))
    t_saa = med(lambda: ops.scale_add_act(d, a, sc, None, act2="silu"))
    t_fused = med(lambda: ops.conv2d_out_gated(z, d4, a, sc, None, act2="silu"))
    old = med(lambda: (ops.conv2d(z, d4), gate_old(), ops.scale_add_act(d, a, sc, None, act2="silu")))
    new = med(lambda: (gate_new(), ops.conv2d_out_gated(z, d4, a, sc, None, act2="silu")))
    print(f"stage {stage} oc={oc} {hw}x{hw}: gate on d {t_gold:7.1f} us -> folded gate on z {t_gnew:7.1f} us | deep_4 {t_conv:7.1f} + scale_add_act {t_saa:7.1f}"
          f" = {t_conv + t_saa:7.1f} us -> gated deep_4 {t_fused:7.1f} us | tail (back to back) {old:7.1f} -> {new:7.1f} us"
          f" | {(desc is not None and ops.out_gate2_variant(desc, False)) or 'two launches'}", flush=True)
