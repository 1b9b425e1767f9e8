"""Sharpening stress test, timed: 256 synthetic 200x200 images (tools/make_synth), decoded once; per sigma (1.0 -> R 3, 2.5 -> R 8)
  sharpen               vip_sharpen_rgb_u8, ONE launch: blur and unsharp-mask epilogue, the blurred image stays in LDS      - HIP events, us
  blur                  vip_blur_gauss_rgb_u8 at the same sigma, one launch: the part of the work the two kernels share
  blur + torch combine  what the fused launch replaces: pipeline's blur into a buffer, then the combine written in torch on the two uint8
                        batches (int32 arithmetic, the same integers: the result is compared bit for bit before anything is timed)
  copy                  a plain copy_ of the same bytes: the floor of anything that reads and writes every pixel once
Every figure is the median over --reps of ``--burst`` back-to-back launches between two HIP events, divided by the burst (a single launch
of this size is short against the events' own resolution); min and max of the per-launch figure show the spread.  The four sides are
timed alternately in the same loop, after 5 warm-up rounds, at P = 150 %, T = 0 (neither changes the work).  GB/s counts the image bytes
moved: every pixel read once and written once.
usage: python tools/bench_sharpen.py [--n 256] [--reps 30] [--burst 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMAS = [1.0, 2.5]
PERCENT, THRESHOLD = 150, 0


def _timed(fn, burst):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(burst):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / burst


def _stats(t):
    return {"us": round(float(np.median(t)), 1), "us_min_max": [round(min(t), 1), round(max(t), 1)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sharpen: no GPU visible - nothing to measure")
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    from tools.make_synth import synth_jpeg
    raws = [synth_jpeg(i) for i in range(a.n + a.n // 49 + 1) if i % 50 != 49][:a.n]          # the 200x200 ones
    batch = pipeline.decode_images(raws)
    n, maxH, maxW, _ = batch.rgb.shape
    assert all(s == (maxH, maxW) for s in batch.sizes_host)
    dst, blurred, two_step = torch.zeros_like(batch.rgb), torch.zeros_like(batch.rgb), torch.zeros_like(batch.rgb)
    amount = pipeline.sharpen_amount(PERCENT)

    def combine():
        x, d = batch.rgb.to(torch.int32), batch.rgb.to(torch.int32) - blurred.to(torch.int32)
        out = torch.clamp(x + ((amount * d + 128) >> 8), 0, 255)                              # >> on int32 is arithmetic
        two_step.copy_(torch.where(d.abs() <= THRESHOLD, x, out).to(torch.uint8))

    cases = {}                                                                                # name -> launch
    for sigma in SIGMAS:
        key = pipeline._blur_args(sigma, None)
        tag = f"s{sigma:g}_R{key[1]}"

        def blur(key=key):
            pipeline._filter_into(batch, blurred, "gauss", key)

        def blur_combine(blur=blur):
            blur()
            combine()

        cases[f"sharpen_{tag}"] = lambda key=key: pipeline._filter_into(batch, dst, "sharpen", key + (amount, THRESHOLD))
        cases[f"blur_{tag}"] = blur
        cases[f"blur_torch_combine_{tag}"] = blur_combine
        cases[f"sharpen_{tag}"]()                        # the two ways compute the same pixels
        blur_combine()
        torch.cuda.synchronize()
        assert torch.equal(dst, two_step), f"{tag}: the fused launch and blur + the torch combine differ"
        assert not torch.equal(dst, batch.rgb)
    cases["copy"] = lambda: dst.copy_(batch.rgb)

    times = {name: [] for name in cases}
    for rep in range(a.reps + 5):                        # 5 warm-up rounds; the sides alternate
        for name, fn in cases.items():
            t = _timed(fn, a.burst)
            if rep >= 5:
                times[name].append(t)
    by = 2 * n * maxH * maxW * 3                         # pixels read once + pixels written once
    out = {"images": n, "size": f"{maxW}x{maxH}", "reps": a.reps, "burst": a.burst, "percent": PERCENT, "threshold": THRESHOLD,
           "image_bytes_moved": by, "launches": {}}
    for name in cases:
        st = _stats(times[name])
        out["launches"][name] = {**st, "GB_per_s": round(by / st["us"] / 1e3, 1)}
    print(json.dumps(out))
    for sigma in SIGMAS:                                 # the same figures, one line per sigma
        tag = f"s{sigma:g}_R{pipeline._blur_args(sigma, None)[1]}"
        s, b, c = (out["launches"][f"{k}_{tag}"] for k in ("sharpen", "blur", "blur_torch_combine"))
        verdict = "faster than" if c["us"] > s["us"] else "NOT faster than"
        print(f"sharpen {tag}: {s['us']} us (min {s['us_min_max'][0]}, max {s['us_min_max'][1]}), {s['GB_per_s']} GB/s of image bytes; "
              f"blur alone {b['us']} us ({s['us'] - b['us']:+.1f} us for the epilogue); blur + torch combine {c['us']} us -> "
              f"{c['us'] / s['us']:.2f}x: the fused launch is {verdict} the two steps")
    c = out["launches"]["copy"]
    print(f"copy_ of the same bytes: {c['us']} us (min {c['us_min_max'][0]}, max {c['us_min_max'][1]}), {c['GB_per_s']} GB/s")


if __name__ == "__main__":
    main()
