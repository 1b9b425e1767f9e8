"""usage: python tools/bench_global_filter.py [--out profiles/global_filter_bench.log] [--no-members]   (repository root, one GPU)

ops.global_local_filter at batch 256 on the maps of hornet_base_gf - (14,14,960), (12,12,960), (7,7,1984), (6,6,1984) - in the three
storages, next to
  * the launch it stands in for in the plain model: ops.dwconv2d 7x7 on the same [256,H,W,S] map;
  * the same operator in torch on the device (torch.fft.rfft2, a multiply, irfft2, a 3x3 conv2d, the interleave), after checking that
    the two agree within the tolerance of the storage (fp32 torch arithmetic on the values the storage holds);
  * a plain copy_ of the same bytes;
and the achieved FMA rate of the global sum (B H W S/2 x H W multiply-adds) against the fp32 vector peak of the MI355X (157.3 TFLOPS).
Then images per second of hornet_base_gf against hornet_base at batch 256 (fast mode, no bias calibration, random inputs).
Timing: BURSTS of back-to-back launches between two HIP events, per-launch time = burst / launches; the median of the bursts is
reported with the minimum - maximum spread."""
import argparse
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
import vipcup_amd  # noqa: E402,F401
from vipcup_amd import ops, zoo  # noqa: E402

PEAK_FP32_VECTOR = 157.3e12      # FLOP/s, MI355X spec
B = 256
SHAPES = [(14, 14, 960), (12, 12, 960), (7, 7, 1984), (6, 6, 1984)]
TOL = {"f16": 2e-3, "h2": 2e-5, "s32": 2e-5}


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


def torch_operator(x32, w3, wc):
    """the operator in torch on the device: x32 [B,H,W,S] fp32, w3 [3,3,half], wc complex [H,W//2+1,half]"""
    Bn, H, W, S = x32.shape
    half = S // 2
    loc = torch.nn.functional.conv2d(x32[..., :half].permute(0, 3, 1, 2), w3.permute(2, 0, 1)[:, None], padding=1, groups=half)
    glob = torch.fft.irfft2(torch.fft.rfft2(x32[..., half:], dim=(1, 2)) * wc, s=(H, W), dim=(1, 2))
    return torch.stack([loc.permute(0, 2, 3, 1), glob], -1).reshape(Bn, H, W, S)


def store(x32, kind):
    return {"f16": lambda t: t.half(), "h2": ops.pack_h2, "s32": lambda t: t}[kind](x32.contiguous())


def load(t):
    return ops.unpack_h2(t) if t.dtype == ops.PACKED else t.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-members", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"global_local_filter at B = {B}; medians of 9 bursts of 10 launches between two HIP events (min - max); "
        f"fp32 vector peak {PEAK_FP32_VECTOR / 1e12:.1f} TFLOPS")
    g = torch.Generator().manual_seed(0)
    for H, W, S in SHAPES:
        half = S // 2
        x = torch.randn(B, H, W, S, generator=g).cuda()
        w3 = (torch.randn(3, 3, half, generator=g) / 3).cuda()
        cw = torch.randn(2, H, W // 2 + 1, half, generator=g) * 0.5 ** 0.5
        gd = ops.make_global_filter_weight(cw, H, W)
        wc = torch.complex(cw[0], cw[1]).cuda()
        w7 = (torch.randn(7, 7, S, generator=g) / 7).cuda()
        b7 = torch.zeros(S, device="cuda")
        blocks, bc, lds = ops.global_filter_plan(H, W, S)
        fma = B * H * W * half * H * W
        say(f"\n[{B},{H},{W},{S}]: {blocks} workgroups per image x {bc} channels, {lds} B of LDS each; global sum {fma / 1e9:.2f} G FMA, "
            f"floor {2 * fma / PEAK_FP32_VECTOR * 1e6:.1f} us")
        for kind in ("f16", "h2", "s32"):
            xs = store(x, kind)
            ref = torch_operator(load(xs), w3, wc)
            got = load(ops.global_local_filter(xs, w3, gd))
            if kind == "h2":
                ops.h2_check("bench")
            rel = ((got - ref).abs().max() / ref.abs().max()).item()
            assert rel <= TOL[kind], (kind, rel)
            t_gf = bursts(lambda: ops.global_local_filter(xs, w3, gd))
            t_dw = bursts(lambda: ops.dwconv2d(xs, w7, b7, 7, 1, (3, 3, 3, 3)))
            dst = torch.empty_like(xs)
            t_cp = bursts(lambda: dst.copy_(xs))
            x32 = load(xs)
            t_th = bursts(lambda: torch_operator(x32, w3, wc), launches=5)
            rate = 2 * fma / (t_gf[0] * 1e-6)
            say(f"  {kind}: global_local_filter {fmt(t_gf)} | dwconv2d 7x7 {fmt(t_dw)} | torch fft+conv (fp32) {fmt(t_th)} | copy_ {fmt(t_cp)}"
                f" | vs torch rel err {rel:.1e} | global sum at {rate / 1e12:.1f} TFLOPS = {100 * rate / PEAK_FP32_VECTOR:.0f}% of the vector peak "
                f"(the launch's whole time charged to it)")
    if not a.no_members:
        say(f"\nmembers at batch {B} (fast mode, no bias calibration, random inputs; median of 5 bursts of 2 predict() calls):")
        for name in ("hornet_base", "hornet_base_gf"):
            spec, model = zoo.build_member(name, bias_calibration=False, precision="fast")
            xd = ops.to_device_nhwc8(torch.rand(B, spec.input_hw, spec.input_hw, 3, generator=g))
            t = bursts(lambda: model.predict(xd), launches=2, n=5)
            say(f"  {name:16s} {spec.input_hw}px {t[0] / 1e3:8.2f} ms ({t[1] / 1e3:.2f} - {t[2] / 1e3:.2f})  {B / t[0] * 1e6:9.0f} img/s")
            del model
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
