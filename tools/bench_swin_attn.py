"""usage: python tools/bench_swin_attn.py [--out profiles/swin_attn_bench.log] [--no-members] [--one H]   (repository root, one GPU)

ops.swin_window_attention at batch 256 on the four stacks of the 200 pixel SwinTransformerV2Tiny_window8 member - maps 50 / 25 / 13 / 7
with 3 / 6 / 12 / 24 heads, windows 8 / 8 / 8 / 7 - unshifted and shifted, in the three storages, next to
  (a) the same layer written in torch on the device in fp16: pad, two cats, partition, normalise, matmul, bias, mask, softmax, matmul,
      reverse, two cats, crop - after checking that the two agree within the fp16 tolerance;
  (b) window_attn_kernel (GCViT's core, ops.window_attention) at ws 7 on a 7-divisible map of about as many tokens and the same heads,
      as the in-house yardstick PER TOKEN;
  (c) a plain copy_ of the qkv bytes.
Then images per second of the two registered members at batch 256 in fast and strict mode (no bias calibration, random inputs).
Timing: BURSTS of back-to-back launches between two HIP events, per-launch time = burst / launches; the median of the bursts is
reported with the minimum - maximum spread.  --one H: only the fp16 launches of the stack whose map is H (for counter runs)."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import vipcup_amd  # noqa: E402,F401
from vipcup_amd import ops, zoo  # noqa: E402

B = 256
STACKS = [(50, 3, 8), (25, 6, 8), (13, 12, 8), (7, 24, 7)]       # (map, heads, clamped window)


def bursts(fn, launches=10, n=9):
    """(median, min, max) microseconds per launch over n bursts"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / launches)
    ts.sort()
    return ts[n // 2], ts[0], ts[-1]


def fmt(t):
    return f"{t[0]:8.1f} us ({t[1]:.1f} - {t[2]:.1f})"


def torch_layer(qkv, v_bias, tau, bias, mask, heads, ws, shift):
    """the layer as the reference writes it, on the device in the dtype of qkv: bias [heads, N, N], mask [windows, N, N] or None"""
    Bn, H, W, C3 = qkv.shape
    C = C3 // 3
    ph, pw = -(-H // ws), -(-W // ws)
    x = qkv
    if ph * ws != H or pw * ws != W:
        x = F.pad(x, (0, 0, 0, pw * ws - W, 0, ph * ws - H))
        x[:, H:, :, 2 * C:] = v_bias
        x[:, :, W:, 2 * C:] = v_bias
    if shift:
        x = torch.cat([x[:, shift:], x[:, :shift]], 1)
        x = torch.cat([x[:, :, shift:], x[:, :, :shift]], 2)
    N = ws * ws
    nn = x.reshape(Bn, ph, ws, pw, ws, 3, heads, 32).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, Bn, ph * pw, heads, N, 32)
    q, k, v = nn[0], nn[1], nn[2]
    qn = q * torch.rsqrt(torch.clamp((q.float() ** 2).sum(-1, keepdim=True), min=1e-6)).to(q.dtype)
    kn = k * torch.rsqrt(torch.clamp((k.float() ** 2).sum(-1, keepdim=True), min=1e-6)).to(k.dtype)
    attn = (qn @ kn.transpose(-1, -2)) * tau.reshape(1, 1, heads, 1, 1).to(q.dtype) + bias[None, None]
    if mask is not None:
        attn = attn + mask[None, :, None]
    o = torch.softmax(attn, -1) @ v
    o = o.reshape(Bn, ph, pw, heads, ws, ws, 32).permute(0, 1, 4, 2, 5, 3, 6).reshape(Bn, ph * ws, pw * ws, C)
    if shift:
        o = torch.cat([o[:, -shift:], o[:, :-shift]], 1)
        o = torch.cat([o[:, :, -shift:], o[:, :, :-shift]], 2)
    return o[:, :H, :W].contiguous()


def bias_and_mask(table, H, ws, shift, dtype):
    N = ws * ws
    t = torch.arange(N)
    idx = (t[:, None] // ws - t[None, :] // ws + ws - 1) * (2 * ws - 1) + (t[:, None] % ws - t[None, :] % ws + ws - 1)
    bias = table[idx.cuda()].permute(2, 0, 1).to(dtype).contiguous()
    if not shift:
        return bias, None
    Hp = -(-H // ws) * ws
    r = lambda v: (v >= Hp - ws).long() + (v >= Hp - shift).long()      # noqa: E731
    reg = 3 * r(torch.arange(Hp))[:, None] + r(torch.arange(Hp))[None, :]
    reg = reg.reshape(Hp // ws, ws, Hp // ws, ws).permute(0, 2, 1, 3).reshape(-1, N)
    mask = torch.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0).to(dtype).cuda()
    return bias, mask


def store(x32, kind):
    return {"f16": lambda t: t.half(), "h2": ops.pack_h2, "s32": lambda t: t}[kind](x32.contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-members", action="store_true")
    ap.add_argument("--one", type=int, default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"swin_window_attention at B = {B}; medians of 9 bursts of 10 launches between two HIP events (min - max)")
    g = torch.Generator().manual_seed(0)
    for H, heads, ws in STACKS:
        if a.one is not None and H != a.one:
            continue
        C = heads * 32
        x = torch.randn(B, H, H, 3 * C, generator=g).cuda()
        v_bias = (0.3 * torch.randn(C, generator=g)).cuda()
        tau = torch.exp(math.log(10.0) + 0.3 * torch.randn(heads, generator=g)).float().cuda()
        table = (16.0 * torch.sigmoid(torch.randn((2 * ws - 1) ** 2, heads, generator=g))).cuda()
        for shift in ((0, ws // 2) if ws < H else (0,)):
            Hp, _, items = ops.swin_attn_plan(B, H, H, heads, ws, shift)
            xs = store(x, "f16")
            if a.one is not None:
                for _ in range(5):
                    ops.swin_window_attention(xs, v_bias, tau, table, heads, ws, shift)
                torch.cuda.synchronize()
                continue
            bias, mask = bias_and_mask(table, H, ws, shift, torch.float16)
            ref = torch_layer(xs, v_bias.half(), tau, bias, mask, heads, ws, shift)
            got = ops.swin_window_attention(xs, v_bias, tau, table, heads, ws, shift)
            rel = ((got.float() - ref.float()).abs().max() / ref.float().abs().max()).item()
            assert rel <= 2e-2, rel        # torch's fp16 form rounds q, k, logits and P to fp16: a sanity check, the tests hold the kernel
            t_k = bursts(lambda: ops.swin_window_attention(xs, v_bias, tau, table, heads, ws, shift))
            t_th = bursts(lambda: torch_layer(xs, v_bias.half(), tau, bias, mask, heads, ws, shift), launches=3)
            dst = torch.empty_like(xs)
            t_cp = bursts(lambda: dst.copy_(xs))
            H7 = max(7, round(H / 7) * 7)
            x7 = torch.randn(B, H7, H7, 3 * C, generator=g).cuda().half()
            t7 = (torch.randn(169, heads, generator=g) * 0.5).cuda()
            t_w7 = bursts(lambda: ops.window_attention(x7, None, t7, heads, 7, 32 ** -0.5))
            mb = xs.numel() * 2 / 1e6
            say(f"\n[{B},{H},{H},3x{C}] {heads} heads ws {ws} shift {shift}: padded map {Hp}, {items} work items, qkv {mb:.1f} MB")
            say(f"  f16: swin_attn_kernel {fmt(t_k)} = {t_k[0] * 1e3 / (B * H * H):.2f} ns/token | (a) torch fp16 layer {fmt(t_th)} = "
                f"{t_th[0] / t_k[0]:.1f}x | (b) window_attn_kernel ws7 on {H7}x{H7} {fmt(t_w7)} = {t_w7[0] * 1e3 / (B * H7 * H7):.2f} ns/token | "
                f"(c) copy_ of qkv {fmt(t_cp)} | vs torch fp16 rel err {rel:.1e}")
            for kind in ("h2", "s32"):
                xk = store(x, kind)
                t = bursts(lambda: ops.swin_window_attention(xk, v_bias, tau, table, heads, ws, shift), launches=3, n=5)
                say(f"  {kind}: swin_attn_strict_kernel {fmt(t)}")
                if kind == "h2":
                    ops.h2_check("bench")
    if not a.no_members and a.one is None:
        say(f"\nmembers at batch {B} (no bias calibration, random inputs; median of 5 bursts of 2 predict() calls):")
        for name in ("swin_v2_tiny_window8", "swin_v2_base_window8"):
            for mode in ("fast", "strict"):
                spec, model = zoo.build_member(name, bias_calibration=False, precision=mode)
                xd = ops.to_device_nhwc8(torch.rand(B, spec.input_hw, spec.input_hw, 3, generator=g), dtype=ops.act_dtype(mode))
                t = bursts(lambda: model.predict(xd), launches=2, n=5)
                say(f"  {name:22s} {spec.input_hw}px {mode:6s} {t[0] / 1e3:8.2f} ms ({t[1] / 1e3:.2f} - {t[2] / 1e3:.2f})  {B / t[0] * 1e6:9.0f} img/s")
                del model
                torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
