"""PNG input path, timed: 256 PNGs of 200x200 (RGB, 8-bit, every filter type, zlib level 6) through
  host stage   pipeline.host_decode (chunk walk + CRCs + inflate on C++ threads)              - wall ms
  device stage vip_png_unfilter_rgb_u8 on the staged batch (H2D copy not included)          - HIP events, us
  end to end   pipeline.decode_images + resized(200, 200)                                    - images/s
  comparison   Pillow decode + convert("RGB") on a 16-thread pool                            - images/s
usage: python tools/bench_png.py [--n 256] [--threads 16] [--reps 20]"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    from vipcup_amd.ops import _p, _stream
    from tests import _png
    from tools.make_synth import synth_jpeg
    pngs = [_png.write_png(np.asarray(Image.open(io.BytesIO(synth_jpeg(i))).convert("RGB")), 2, 8, filter_seed=i)
            for i in range(a.n)]
    # host stage
    pipeline.host_decode(pngs, a.threads, pinned=True)
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        staged = pipeline.host_decode(pngs, a.threads, pinned=True)
        t.append(time.perf_counter() - t0)
    host_ms = 1e3 * float(np.median(t))
    # device stage: the kernel alone, on a fresh device copy of the filtered stream each time (it unfilters in place)
    staged = staged.png                                # an all-PNG batch: the MixedStage's PNG part is the whole batch
    dev = torch.device("cuda")
    desc_d = torch.from_numpy(np.frombuffer(bytes(staged.desc), dtype=np.uint8).copy()).to(dev)
    src = staged.stream.to(dev)
    maxH = max(d.height for d in staged.desc)
    maxW = max(d.width for d in staged.desc)
    rgb = torch.zeros((a.n, maxH, maxW, 3), dtype=torch.uint8, device=dev)
    lib = _abi.lib()
    us = []
    for r in range(a.reps + 3):
        s = src.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _abi.check(lib.vip_png_unfilter_rgb_u8(_p(s), _p(desc_d), a.n, _p(rgb), maxH, maxW, _stream()), "vip_png_unfilter_rgb_u8")
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            us.append(1e3 * e0.elapsed_time(e1))
    dev_us = float(np.median(us))
    # end to end
    pipeline.decode_images(pngs).resized(200, 200)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        pipeline.decode_images(pngs, threads=a.threads).resized(200, 200)
    torch.cuda.synchronize()
    e2e = a.n * a.reps / (time.perf_counter() - t0)
    with ThreadPoolExecutor(a.threads) as ex:
        t0 = time.perf_counter()
        for _ in range(max(1, a.reps // 4)):
            list(ex.map(lambda b: np.asarray(Image.open(io.BytesIO(b)).convert("RGB")), pngs))
        pil = a.n * max(1, a.reps // 4) / (time.perf_counter() - t0)
    print(json.dumps({"images": a.n, "size": "200x200 RGB8", "threads": a.threads, "host_stage_ms": round(host_ms, 3),
                      "device_stage_us": round(dev_us, 1), "decode_images_resize_img_per_s": round(e2e, 1),
                      "pillow_img_per_s": round(pil, 1)}))


if __name__ == "__main__":
    main()
