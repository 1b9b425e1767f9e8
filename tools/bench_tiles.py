"""Tile gather, timed: 256 tiles of 200 x 200 cut from synthetic 1000 x 1000 images (a 5 x 5 grid each, tools/make_synth fields), as the
network inputs of a 200 x 200 member (identity branch) and of a 224 x 224 member (bicubic branch), fp16, 8 channels.
  gather         DecodedBatch.tiles: vip_tile_resize_bicubic_norm_f16, one launch                                  - HIP events, us
  two-step       torch slicing of the tiles into a uint8 batch [T, 200, 200, 3], then DecodedBatch.resized on it  - HIP events, us
The two are timed alternately in the same loop, after 5 warm-up rounds; medians.  Their outputs are compared first (they must be equal).
usage: python tools/bench_tiles.py [--tiles 256] [--reps 50]"""
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
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tiles: no GPU visible - nothing to measure")
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    from tools.make_synth import synth_pixels
    tile, side = 200, 1000
    n = -(-a.tiles // 25)
    imgs = [np.tile(synth_pixels(i), (side // 200, side // 200, 1)) for i in range(n)]
    batch = pipeline.DecodedBatch(torch.from_numpy(np.stack(imgs)).cuda(), torch.tensor([[side, side]] * n, dtype=torch.int32, device="cuda"),
                                  [(side, side)] * n)
    plan = pipeline.tile_plan(batch.sizes_host, tile)
    T = min(a.tiles, plan.tab.shape[0])
    tab_d = torch.from_numpy(plan.tab).cuda()
    idx = torch.from_numpy(plan.tab[:T].astype(np.int64)).cuda()
    ar = torch.arange(tile, device="cuda")
    sizes = torch.tensor([[tile, tile]] * T, dtype=torch.int32, device="cuda")

    def two_step(out):
        rows = (idx[:, 1, None] + ar)[:, :, None]                                      # [T, tile, 1]
        cols = (idx[:, 2, None] + ar)[:, None, :]                                      # [T, 1, tile]
        crops = batch.rgb[idx[:, 0, None, None], rows, cols]                           # one gather into a uint8 batch
        return pipeline.DecodedBatch(crops, sizes, [(tile, tile)] * T).resized(out, out)

    result = {"tiles": T, "tile": tile, "reps": a.reps}
    for out in (200, 224):
        assert torch.equal(batch.tiles(tab_d, 0, T, tile, out), two_step(out)), out
        t_gather, t_two = [], []
        for r in range(a.reps + 5):
            g = _timed(lambda: batch.tiles(tab_d, 0, T, tile, out))
            s = _timed(lambda: two_step(out))
            if r >= 5:
                t_gather.append(g)
                t_two.append(s)
        g, s = float(np.median(t_gather)), float(np.median(t_two))
        out_bytes = T * out * out * 8 * 2
        print(f"{T} tiles {tile} -> {out}: gather {g:8.1f} us ({out_bytes / g / 1e3:6.1f} GB/s written)   two-step {s:8.1f} us   "
              f"ratio {s / g:.2f}x")
        result[f"{tile}to{out}"] = {"gather_us": g, "two_step_us": s, "out_bytes": out_bytes}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
