"""Colour stress tests, timed: 256 synthetic 200x200 images (tools/make_synth), decoded once.
  gray, hue30, con150, gam080    vip_colour_rgb_u8, one launch (con150: vip_image_mean_u8 + the launch, as pipeline.contrast runs it;
                                 gam080: the table already on the device) - HIP events, us
  copy                           dst.copy_(src) of the same bytes: the traffic floor of a 3-bytes-in, 3-bytes-out kernel
  torch yardstick                a straightforward torch formulation of the same variant on the same uint8 pixels: to float, matmul
                                 with the real-valued matrix (+ the per-image mean term / the power law), round, clamp, to uint8
The launches are timed alternately in the same loop, after 5 warm-up rounds.  GB/s counts the image bytes moved: every pixel read once
and written once.
usage: python tools/bench_colour.py [--n 256] [--reps 50]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)


def _stats(t):
    return {"us": round(float(np.median(t)), 1), "us_min_max": [round(min(t), 1), round(max(t), 1)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_colour: no GPU visible - nothing to measure")
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    from tools.make_synth import synth_jpeg
    raws = [synth_jpeg(i) for i in range(a.n + a.n // 49 + 1) if i % 50 != 49][:a.n]          # the 200x200 ones
    batch = pipeline.decode_images(raws)
    n, H, W, _ = batch.rgb.shape
    assert all(s == (H, W) for s in batch.sizes_host)
    dst = torch.zeros_like(batch.rgb)
    w = torch.tensor(pipeline.GRAY_Q16, dtype=torch.float64) / 65536

    def case(name, variant, real, gamma=None):
        """variant = (M, K, O, lut) of pipeline; real = (M, K, O) as real numbers for the yardstick -> (name, ours, yardstick)"""
        coef, lut = pipeline._colour_coef(*variant)
        Mf = torch.as_tensor(real[0], dtype=torch.float32, device="cuda")
        Kf = None if real[1] is None else torch.as_tensor(real[1], dtype=torch.float32, device="cuda")

        def ours():
            pipeline._colour_into(batch, coef, lut, None, dst)

        def yard():
            x = batch.rgb.float()
            y = x @ Mf.T
            if Kf is not None:
                y = y + Kf * x.mean(dim=(1, 2), keepdim=True)
            if gamma is not None:
                y = 255.0 * (y / 255.0) ** gamma
            return y.round().clamp(0, 255).to(torch.uint8)

        return name, ours, yard

    eye = np.eye(3)
    t = np.deg2rad(30.0)
    T = np.array(pipeline.YIQ)
    rot = np.linalg.inv(T) @ np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]]) @ T
    cases = [case("gray", pipeline.colour_gray(), (w.repeat(3, 1).numpy(), None, None)),
             case("hue30", pipeline.colour_hue(30), (rot, None, None)),
             case("con150", pipeline.colour_contrast(150), (1.5 * eye, np.full(3, -0.5), None)),
             case("gam080", pipeline.colour_gamma(0.8), (eye, None, None), gamma=0.8)]

    def copy():
        dst.copy_(batch.rgb)

    for name, ours, yard in cases:                       # the two sides compute the same thing
        ours()
        worst = int((dst.int() - yard().int()).abs().max())
        assert worst <= 1, f"{name}: the kernel and the torch yardstick differ by {worst} levels"
    t_ours, t_yard, t_copy = {c[0]: [] for c in cases}, {c[0]: [] for c in cases}, {c[0]: [] for c in cases}
    for rep in range(a.reps + 5):                        # 5 warm-up rounds; the launches alternate
        for name, ours, yard in cases:
            o_, c_, y_ = _timed(ours), _timed(copy), _timed(yard)
            if rep >= 5:
                t_ours[name].append(o_), t_copy[name].append(c_), t_yard[name].append(y_)
    by = 2 * batch.rgb.numel()                           # every pixel read once and written once
    out = {"images": n, "size": f"{W}x{H}", "reps": a.reps, "image_bytes_moved": by, "launches": {}}
    for name, _, _ in cases:
        o, c, y = _stats(t_ours[name]), _stats(t_copy[name]), _stats(t_yard[name])
        out["launches"][name] = {**o, "GB_per_s": round(by / o["us"] / 1e3, 1), "copy_us": c["us"], "copy_us_min_max": c["us_min_max"],
                                 "kernel_over_copy": round(o["us"] / c["us"], 2), "torch_us": y["us"], "torch_us_min_max": y["us_min_max"],
                                 "torch_over_kernel": round(y["us"] / o["us"], 2)}
    print(json.dumps(out))
    for name, v in out["launches"].items():              # the same figures, one line per launch
        verdict = "faster than" if v["torch_over_kernel"] > 1 else "SLOWER than"
        print(f"{name}: {v['us']} us (min {v['us_min_max'][0]}, max {v['us_min_max'][1]}), {v['GB_per_s']} GB/s of image bytes; plain copy "
              f"{v['copy_us']} us -> {v['kernel_over_copy']}x the copy; torch yardstick {v['torch_us']} us -> {v['torch_over_kernel']}x: "
              f"the kernel is {verdict} the yardstick")


if __name__ == "__main__":
    main()
