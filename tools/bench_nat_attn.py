"""usage: python tools/bench_nat_attn.py [--out profiles/nat_attn_bench.log] [--no-members]   (repository root, one GPU)

ops.nat_attention at batch 256 on the stacks of the two registered members - NAT_Mini at 200 pixels (maps 50 / 25 / 13 / 7 with
2 / 4 / 8 / 16 heads) and NAT_Base at 224 (56 / 28 / 14 / 7 with 4 / 8 / 16 / 32 heads) - in the three storages, next to
  (a) the same layer written in torch on the device in fp16 on the same bits of input: unfold, replicate-pad (as a gather of patch rows
      and columns), the gathered bias, softmax, matmul - after checking that the two agree within the fp16 tolerance;
  (b) swin_attn_kernel (ops.swin_window_attention, ws 8, unshifted) on the same map and heads, as the in-house yardstick PER TOKEN;
  (c) a plain copy_ of the qkv bytes.
The fp32 storage's launch is the VALU form of the layer (one thread per query, K / V of the halo in LDS as fp32), the fp16 launch the
dense-and-masked matrix-core form on 8 x 8 query tiles: the two forms that were built, side by side.
Then images per second of the two registered members at batch 256 in fast and strict mode (no bias calibration, random inputs).
Timing: BURSTS of back-to-back launches between two HIP events, per-launch time = burst / launches; the median of the bursts is
reported with the minimum - maximum spread."""
import argparse
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
import vipcup_amd  # noqa: E402,F401
from vipcup_amd import ops, zoo  # noqa: E402

B = 256
K = 7
STACKS = [(50, 2), (25, 4), (13, 8), (7, 16), (56, 4), (28, 8), (14, 16), (7, 32)]       # (map, heads)


def bursts(fn, launches=10, n=9):
    """(median, min, max) microseconds per launch over n bursts"""
    for _ in range(2):
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


def gather_plan(H, W, table, dtype):
    """(iy, ix, bias): the patch row / column every position reads (what the replicate padding amounts to) and the bias
    [heads, HW, K^2] gathered by the key-minus-query offset"""
    r = K // 2
    y, x = torch.arange(H), torch.arange(W)
    iy, ix = (y - r).clamp(0, H - K), (x - r).clamp(0, W - K)
    j = torch.arange(K)
    dy = iy[:, None] + j[None, :] - y[:, None] + K - 1                       # [H, K]
    dx = ix[:, None] + j[None, :] - x[:, None] + K - 1                       # [W, K]
    idx = (dy[:, None, :, None] * (2 * K - 1) + dx[None, :, None, :]).reshape(H * W, K * K)
    return iy.cuda(), ix.cuda(), table[:, idx.cuda()].to(dtype).contiguous()


def torch_layer(qkv, plan, heads):
    """the layer as the reference writes it, on the device in the dtype of qkv"""
    iy, ix, bias = plan
    Bn, H, W, C3 = qkv.shape
    C = C3 // 3
    q = qkv[..., :C].reshape(Bn, H * W, heads, 1, 32)
    pt = qkv[..., C:].unfold(1, K, 1).unfold(2, K, 1)                        # [B, H-K+1, W-K+1, 2C, K, K]
    pt = pt[:, iy][:, :, ix].permute(0, 1, 2, 4, 5, 3).reshape(Bn, H * W, K * K, 2, heads, 32)
    k = pt[:, :, :, 0].permute(0, 1, 3, 4, 2)                                # [B, HW, heads, 32, KK]
    v = pt[:, :, :, 1].permute(0, 1, 3, 2, 4)                                # [B, HW, heads, KK, 32]
    s = (q @ k) * (32 ** -0.5) + bias.permute(1, 0, 2)[None, :, :, None, :]
    return (torch.softmax(s, -1) @ v).reshape(Bn, H, W, C)


def store(x32, kind):
    return {"f16": lambda t: t.half(), "h2": ops.pack_h2, "s32": lambda t: t}[kind](x32.contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-members", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"nat_attention (kernel_size {K}) at B = {B}; medians of 9 bursts of 10 launches between two HIP events (min - max)")
    g = torch.Generator().manual_seed(0)
    slower = []
    for H, heads in STACKS:
        C = heads * 32
        x = torch.randn(B, H, H, 3 * C, generator=g).cuda()
        table = (0.5 * torch.randn(heads, (2 * K - 1) ** 2, generator=g)).cuda()
        xs = store(x, "f16")
        _, _, items = ops.nat_attn_plan(B, H, H, heads, K)
        plan = gather_plan(H, H, table, torch.float16)
        ref = torch_layer(xs, plan, heads)
        got = ops.nat_attention(xs, None, table, heads, K)
        rel = ((got.float() - ref.float()).abs().max() / ref.float().abs().max()).item()
        assert rel <= 2e-2, rel            # torch's fp16 form rounds logits and P to fp16: a sanity check, the tests hold the kernel
        del ref, got
        t_k = bursts(lambda: ops.nat_attention(xs, None, table, heads, K))
        t_th = bursts(lambda: torch_layer(xs, plan, heads), launches=2, n=5)
        dst = torch.empty_like(xs)
        t_cp = bursts(lambda: dst.copy_(xs))
        tau = torch.full((heads,), 10.0).cuda()
        ws = min(8, H)
        t_sw = (16.0 * torch.sigmoid(torch.randn((2 * ws - 1) ** 2, heads, generator=g))).cuda()
        vb = torch.zeros(C).cuda()
        t_s = bursts(lambda: ops.swin_window_attention(xs, vb, tau, t_sw, heads, ws, 0))
        tok = B * H * H
        say(f"\n[{B},{H},{H},3x{C}] {heads} heads: {items} work items, qkv {xs.numel() * 2 / 1e6:.1f} MB")
        say(f"  f16: nat_attn_kernel {fmt(t_k)} = {t_k[0] * 1e3 / tok:.2f} ns/token | (a) torch fp16 layer {fmt(t_th)} = "
            f"{t_th[0] / t_k[0]:.1f}x | (b) swin_attn_kernel ws{ws} on the same map {fmt(t_s)} = {t_s[0] * 1e3 / tok:.2f} ns/token | "
            f"(c) copy_ of qkv {fmt(t_cp)} | vs torch fp16 rel err {rel:.1e}")
        if t_k[0] >= t_th[0]:
            slower.append((H, heads))
        for kind in ("h2", "s32"):
            xk = store(x, kind)
            t = bursts(lambda: ops.nat_attention(xk, None, table, heads, K), launches=3, n=5)
            say(f"  {kind}: nat_attn_strict_kernel (fp32 VALU form) {fmt(t)}")
            if kind == "h2":
                ops.h2_check("bench")
        del x, xs, plan, dst
        torch.cuda.empty_cache()
    say("\nthe fp16 launch is faster than the torch formulation at every member shape" if not slower else
        f"\nthe fp16 launch is NOT faster than the torch formulation at {slower}")
    if not a.no_members:
        say(f"\nmembers at batch {B} (no bias calibration, random inputs; median of 5 bursts of 2 predict() calls):")
        for name in ("nat_mini", "nat_base"):
            for mode in ("fast", "strict"):
                spec, model = zoo.build_member(name, bias_calibration=False, precision=mode)
                xd = ops.to_device_nhwc8(torch.rand(B, spec.input_hw, spec.input_hw, 3, generator=g), dtype=ops.act_dtype(mode))
                t = bursts(lambda: model.predict(xd), launches=2, n=5)
                say(f"  {name:10s} {spec.input_hw}px {mode:6s} {t[0] / 1e3:8.2f} ms ({t[1] / 1e3:.2f} - {t[2] / 1e3:.2f})  {B / t[0] * 1e6:9.0f} img/s")
                del model
                torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
