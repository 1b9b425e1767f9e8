"""Lossless WebP input path, timed: 256 WebPs of 200x200 (the synthetic JPEGs' decoded pixels, Pillow's encoder at
method 4, quality 75) through
  host stage   pipeline.host_decode (container walk + VP8L entropy decode on C++ threads)     - wall ms
  device stage vip_webp_inverse_rgb_u8 on the staged batch (H2D copy not included)           - HIP events, us
  end to end   pipeline.decode_images + resized(200, 200)                                    - images/s
  comparison   the PNG path on the same pixels (host ms, device us, images/s), and Pillow decode + convert("RGB") on a
               thread pool (images/s)
The device launches work in place, so every launch of a burst gets its own device copy of the staged words; a burst is
timed between two HIP events and the median over the bursts is reported.  Appends one JSON line to profiles/webp_bench.log.
usage: python tools/bench_webp.py [--n 256] [--threads 16] [--reps 20] [--burst 8]"""
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
    ap.add_argument("--burst", type=int, default=8)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "webp_bench.log"))
    a = ap.parse_args()
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    from vipcup_amd.ops import _p, _stream
    from tests import _png, _webp
    from tools.make_synth import synth_jpeg
    if not torch.cuda.is_available():
        raise SystemExit("bench_webp.py needs a GPU: there is no CPU fallback")
    pix = [np.asarray(Image.open(io.BytesIO(synth_jpeg(i))).convert("RGB")) for i in range(a.n)]
    with ThreadPoolExecutor(a.threads) as ex:
        webps = list(ex.map(_webp.pillow_webp, pix))
    pngs = [_png.write_png(p, 2, 8, filter_seed=i) for i, p in enumerate(pix)]
    dev = torch.device("cuda")
    lib = _abi.lib()

    def host_ms(raws):
        pipeline.host_decode(raws, a.threads, pinned=True)
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            staged = pipeline.host_decode(raws, a.threads, pinned=True)
            t.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(t)), staged

    def device_us(staged, entry):
        desc_d = torch.from_numpy(np.frombuffer(bytes(staged.desc), dtype=np.uint8).copy()).to(dev)
        src = staged.stream.to(dev)
        maxH, maxW = max(d.height for d in staged.desc), max(d.width for d in staged.desc)
        rgb = torch.zeros((a.n, maxH, maxW, 3), dtype=torch.uint8, device=dev)
        fn = getattr(lib, entry)
        us = []
        for r in range(a.reps + 3):
            copies = [src.clone() for _ in range(a.burst)]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for s in copies:
                _abi.check(fn(_p(s), _p(desc_d), a.n, _p(rgb), maxH, maxW, _stream()), entry)
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:
                us.append(1e3 * e0.elapsed_time(e1) / a.burst)
        return float(np.median(us)), rgb

    def end_to_end(raws):
        pipeline.decode_images(raws).resized(200, 200)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            pipeline.decode_images(raws, threads=a.threads).resized(200, 200)
        torch.cuda.synchronize()
        return a.n * a.reps / (time.perf_counter() - t0)

    w_ms, w_staged = host_ms(webps)
    p_ms, p_staged = host_ms(pngs)
    w_us, w_rgb = device_us(w_staged, "vip_webp_inverse_rgb_u8")
    p_us, p_rgb = device_us(p_staged.png, "vip_png_unfilter_rgb_u8")
    assert torch.equal(w_rgb, p_rgb), "the two paths disagree on the same pixels"
    w_e2e, p_e2e = end_to_end(webps), end_to_end(pngs)
    with ThreadPoolExecutor(a.threads) as ex:
        t0 = time.perf_counter()
        for _ in range(max(1, a.reps // 4)):
            list(ex.map(lambda b: np.asarray(Image.open(io.BytesIO(b)).convert("RGB")), webps))
        pil = a.n * max(1, a.reps // 4) / (time.perf_counter() - t0)
    line = json.dumps({"images": a.n, "size": "200x200 RGB8", "threads": a.threads, "burst": a.burst,
                       "webp_file_bytes_mean": int(np.mean([len(b) for b in webps])),
                       "webp_host_stage_ms": round(w_ms, 3), "webp_device_stage_us": round(w_us, 1),
                       "webp_decode_images_resize_img_per_s": round(w_e2e, 1),
                       "png_host_stage_ms": round(p_ms, 3), "png_device_stage_us": round(p_us, 1),
                       "png_decode_images_resize_img_per_s": round(p_e2e, 1), "pillow_webp_img_per_s": round(pil, 1)})
    print(line)
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
