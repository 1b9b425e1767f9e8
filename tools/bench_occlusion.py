"""Occlusion gather, timed: one chunk of 128 variants (8 x 8 grid, 2 x 2 windows, the image's mean colour) of synthetic 200 x 200 images
(tools/make_synth fields) as the network inputs of a 200 x 200 member (identity branch) and of a 224 x 224 member (bicubic branch), fp16,
8 channels.
  gather         DecodedBatch.occluded: vip_occlude_resize_bicubic_norm_f16, one launch                                   - HIP events, us
  two-step       torch: the images gathered into a uint8 batch [V, 200, 200, 3] and the window overwritten with the fill
                 (torch.where on a rectangle mask), then DecodedBatch.resized on it                                          - HIP events, us
The two are timed alternately in the same loop, after 5 warm-up rounds; medians.  Their outputs are compared first (they must be equal).
usage: python tools/bench_occlusion.py [--variants 128] [--reps 50]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_occlusion: no GPU visible - nothing to measure")
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    from tools.make_synth import synth_pixels
    side = 200
    n = -(-a.variants // 49)
    imgs = [synth_pixels(i) for i in range(n)]
    batch = pipeline.DecodedBatch(torch.from_numpy(np.stack(imgs)).cuda(), torch.tensor([[side, side]] * n, dtype=torch.int32, device="cuda"),
                                  [(side, side)] * n)
    plan = pipeline.occlusion_plan(batch.sizes_host)
    V = min(a.variants, plan.tab.shape[0])
    tab_d = torch.from_numpy(plan.tab).cuda()
    fill_d = batch.mean_colour()
    idx = torch.from_numpy(plan.tab[:V].astype(np.int64)).cuda()
    ar = torch.arange(side, device="cuda")
    sizes = torch.tensor([[side, side]] * V, dtype=torch.int32, device="cuda")

    def two_step(out):
        ys, xs = ar[None, :, None], ar[None, None, :]
        mask = (ys >= idx[:, 1, None, None]) & (ys < idx[:, 3, None, None]) & (xs >= idx[:, 2, None, None]) & (xs < idx[:, 4, None, None])
        copies = torch.where(mask[..., None], fill_d[idx[:, 0]][:, None, None, :3], batch.rgb[idx[:, 0]])
        return pipeline.DecodedBatch(copies, sizes, [(side, side)] * V).resized(out, out)

    result = {"variants": V, "side": side, "reps": a.reps}
    for out in (200, 224):
        assert torch.equal(batch.occluded(tab_d, 0, V, fill_d, out, out), two_step(out)), out
        t_gather, t_two = [], []
        for r in range(a.reps + 5):
            g = _timed(lambda: batch.occluded(tab_d, 0, V, fill_d, out, out))
            s = _timed(lambda: two_step(out))
            if r >= 5:
                t_gather.append(g)
                t_two.append(s)
        g, s = float(np.median(t_gather)), float(np.median(t_two))
        out_bytes = V * out * out * 8 * 2
        print(f"{V} variants {side} -> {out}: gather {g:8.1f} us ({out_bytes / g / 1e3:6.1f} GB/s written)   two-step {s:8.1f} us   "
              f"ratio {s / g:.2f}x")
        result[f"{side}to{out}"] = {"gather_us": g, "two_step_us": s, "out_bytes": out_bytes}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
