"""Noise stress tests, timed: 256 synthetic 200x200 images (tools/make_synth), decoded once.
  n030, nm030, spk20, imp010     vip_noise_rgb_u8, one launch (table and keys already on the device) - HIP events, us
  placements                     modes 0..2 through vip_noise_rgb_u8_placed with the table gathered from global memory (one tile per
                                 workgroup) and copied into LDS (8 tiles per workgroup): the measurement behind the default
  copy                           dst.copy_(src) of the same bytes: the traffic floor of a 3-bytes-in, 3-bytes-out kernel
  gray                           vip_colour_rgb_u8's gray launch: the same traffic and the same LDS staging without a generator, so the
                                 difference is what Philox and the table cost
  torch yardstick                the same perturbation in torch on the same uint8 pixels: randn (rand for the impulses), multiply-add,
                                 round, clamp, to uint8 - another generator, so only the noise's statistics are comparable
The launches are timed alternately in the same loop, after 5 warm-up rounds.  GB/s counts the image bytes moved: every pixel read once
and written once.
usage: python tools/bench_noise.py [--n 256] [--reps 50]"""
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
        raise SystemExit("bench_noise: no GPU visible - nothing to measure")
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    from tools.make_synth import synth_jpeg
    raws = [synth_jpeg(i) for i in range(a.n + a.n // 49 + 1) if i % 50 != 49][:a.n]          # the 200x200 ones
    batch = pipeline.decode_images(raws)
    n, H, W, _ = batch.rgb.shape
    assert all(s == (H, W) for s in batch.sizes_host)
    dst = torch.zeros_like(batch.rgb)
    keys_d = pipeline.noise_keys_device(batch, pipeline.noise_keys([f"img_{i:05d}.jpg" for i in range(n)]))
    gray_coef, _ = pipeline._colour_coef(*pipeline.colour_gray())

    def ours(kind, value, placement=None):
        mode, amount = pipeline.NOISE_KINDS[kind], pipeline.noise_amount(kind, value)
        return lambda: pipeline._noise_into(batch, mode, amount, 0, keys_d, dst, placement)

    def yard(kind, value):
        def additive(mono):
            x = batch.rgb.float()
            z = torch.randn((n, H, W, 1 if mono else 3), device=x.device)
            return (x + float(value) * z).round().clamp(0, 255).to(torch.uint8)

        def speckle():
            x = batch.rgb.float()
            return (x + x * (value / 100.0) * torch.randn_like(x)).round().clamp(0, 255).to(torch.uint8)

        def impulse():
            u = torch.rand((n, H, W, 1), device=batch.rgb.device)
            salt = torch.where(u < value / 200.0, 255, 0).to(torch.uint8)
            return torch.where(u < value / 100.0, salt.expand(-1, -1, -1, 3), batch.rgb)
        return {"gaussian": lambda: additive(False), "mono": lambda: additive(True), "speckle": speckle, "impulse": impulse}[kind]

    cases = [("n030", "gaussian", 3), ("nm030", "mono", 3), ("spk20", "speckle", 20), ("imp010", "impulse", 1)]

    def copy():
        dst.copy_(batch.rgb)

    def gray():
        pipeline._colour_into(batch, gray_coef, None, None, dst)

    for name, kind, value in cases:                      # the two sides apply noise of the same strength, the two placements the same bytes
        ours(kind, value)()
        got = dst.clone()
        d_ours = (got.float() - batch.rgb.float())
        d_yard = (yard(kind, value)().float() - batch.rgb.float())
        assert abs(float(d_ours.std()) - float(d_yard.std())) <= 0.05 * float(d_yard.std()) + 0.05, (name, float(d_ours.std()), float(d_yard.std()))
        if kind != "impulse":
            for placement in (0, 1):
                ours(kind, value, placement)()
                assert torch.equal(dst, got), (name, placement)
    timers = {}
    for name, kind, value in cases:
        timers[name] = {"kernel": ours(kind, value), "copy": copy, "gray": gray, "torch": yard(kind, value)}
        if kind != "impulse":
            timers[name]["global"], timers[name]["lds"] = ours(kind, value, 0), ours(kind, value, 1)
    times = {name: {k: [] for k in fns} for name, fns in timers.items()}
    for rep in range(a.reps + 5):                        # 5 warm-up rounds; the launches alternate
        for name, fns in timers.items():
            for k, fn in fns.items():
                t = _timed(fn)
                if rep >= 5:
                    times[name][k].append(t)
    by = 2 * batch.rgb.numel()                           # every pixel read once and written once
    out = {"images": n, "size": f"{W}x{H}", "reps": a.reps, "image_bytes_moved": by, "launches": {}}
    for name, _, _ in cases:
        st = {k: _stats(t) for k, t in times[name].items()}
        o = st["kernel"]
        row = {**o, "GB_per_s": round(by / o["us"] / 1e3, 1)}
        for k in ("copy", "gray", "torch", "global", "lds"):
            if k in st:
                row[f"{k}_us"], row[f"{k}_us_min_max"] = st[k]["us"], st[k]["us_min_max"]
        row["kernel_over_copy"], row["kernel_over_gray"] = round(o["us"] / st["copy"]["us"], 2), round(o["us"] / st["gray"]["us"], 2)
        row["torch_over_kernel"] = round(st["torch"]["us"] / o["us"], 2)
        out["launches"][name] = row
    print(json.dumps(out))
    for name, v in out["launches"].items():              # the same figures, one line per launch
        verdict = "faster than" if v["torch_over_kernel"] > 1 else "SLOWER than"
        placed = f"; table gathered from global memory {v['global_us']} us, copied into LDS {v['lds_us']} us" if "lds_us" in v else "; no table"
        print(f"{name}: {v['us']} us (min {v['us_min_max'][0]}, max {v['us_min_max'][1]}), {v['GB_per_s']} GB/s of image bytes{placed}; plain "
              f"copy {v['copy_us']} us -> {v['kernel_over_copy']}x the copy; gray launch {v['gray_us']} us -> {v['kernel_over_gray']}x gray; torch "
              f"yardstick {v['torch_us']} us -> {v['torch_over_kernel']}x: the kernel is {verdict} the yardstick")


if __name__ == "__main__":
    main()
