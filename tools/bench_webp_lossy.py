"""Lossy WebP input path, timed: 256 lossy WebPs of 200x200 (the synthetic JPEGs' decoded pixels, Pillow's encoder at
quality 75, method 4) through
  host stage    pipeline.host_decode(lossy_webp=True) (container walk + VP8 token decode on C++ threads)        - wall ms
  device stages vip_vp8_reconstruct_stages_rgb_u8 on the staged batch (H2D copy not included): reconstruction alone,
                reconstruction + filter and all three, each with the planes in device scratch and in LDS, and the
                output kernel alone                                                                            - HIP events, us
  end to end    pipeline.decode_images(lossy_webp=True) + resized(200, 200)                                     - images/s
  baseline      Pillow / libwebp decode + convert("RGB") of the same files on a thread pool                     - images/s
  context       the lossless WebP and the JPEG path on the same pixels (host ms, images/s)
A burst of launches is timed between two HIP events and the median over the bursts is reported.  Appends one JSON line to
profiles/webp_lossy_bench.log.
usage: python tools/bench_webp_lossy.py [--n 256] [--threads 16] [--reps 20] [--burst 8]"""
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
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "webp_lossy_bench.log"))
    a = ap.parse_args()
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    from vipcup_amd.ops import _p, _stream
    from tests import _vp8, _webp
    from tools.make_synth import synth_jpeg
    if not torch.cuda.is_available():
        raise SystemExit("bench_webp_lossy.py needs a GPU: there is no CPU fallback")
    jpegs = [synth_jpeg(i) for i in range(a.n)]
    pix = [np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs]
    with ThreadPoolExecutor(a.threads) as ex:
        lossy = list(ex.map(_vp8.pillow_lossy, pix))
        lossless = list(ex.map(_webp.pillow_webp, pix))
    dev = torch.device("cuda")
    lib = _abi.lib()

    def host_ms(raws, **kw):
        pipeline.host_decode(raws, a.threads, pinned=True, **kw)
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            staged = pipeline.host_decode(raws, a.threads, pinned=True, **kw)
            t.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(t)), staged

    def end_to_end(raws, **kw):
        pipeline.decode_images(raws, **kw).resized(200, 200)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            pipeline.decode_images(raws, threads=a.threads, **kw).resized(200, 200)
        torch.cuda.synchronize()
        return a.n * a.reps / (time.perf_counter() - t0)

    v_ms, staged = host_ms(lossy, lossy_webp=True)
    desc_d = torch.from_numpy(np.frombuffer(bytes(staged.desc), dtype=np.uint8).copy()).to(dev)
    src = staged.stream.to(dev)
    scratch = torch.empty((staged.scratch_bytes,), dtype=torch.uint8, device=dev)
    maxH, maxW = max(d.height for d in staged.desc), max(d.width for d in staged.desc)
    rgb = torch.zeros((a.n, maxH, maxW, 3), dtype=torch.uint8, device=dev)

    def device_us(stages):
        us = []
        for r in range(a.reps + 3):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.burst):
                _abi.check(lib.vip_vp8_reconstruct_stages_rgb_u8(_p(src), src.numel(), _p(desc_d), a.n, _p(scratch), scratch.numel(), _p(rgb),
                                                                 maxH, maxW, stages, _stream()), "vip_vp8_reconstruct_stages_rgb_u8")
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:
                us.append(1e3 * e0.elapsed_time(e1) / a.burst)
        return float(np.median(us))

    LDS = 8                                                  # VIP_VP8_STAGE_LDS_PLANES: the planes of an image in LDS, not in scratch
    wants = [_vp8.pillow_rgb(r) for r in lossy]
    timed = {}
    for tag, extra in (("scratch", 0), ("lds", LDS)):
        rgb.zero_()
        timed[tag, "all"] = device_us(7 | extra)             # first: the planes are whole for the output kernel's run below
        got = rgb.cpu().numpy()
        for i, want in enumerate(wants):
            assert np.array_equal(got[i, :want.shape[0], :want.shape[1]], want), f"image {i} ({tag}): the device stages and Pillow disagree"
        timed[tag, "recon"], timed[tag, "recon_filter"] = device_us(1 | extra), device_us(3 | extra)
    out_us = device_us(4)
    v_e2e = end_to_end(lossy, lossy_webp=True)
    l_ms, _ = host_ms(lossless)
    l_e2e = end_to_end(lossless)
    j_ms, _ = host_ms(jpegs)
    j_e2e = end_to_end(jpegs)
    with ThreadPoolExecutor(a.threads) as ex:
        t0 = time.perf_counter()
        for _ in range(max(1, a.reps // 4)):
            list(ex.map(lambda b: np.asarray(Image.open(io.BytesIO(b)).convert("RGB")), lossy))
        pil = a.n * max(1, a.reps // 4) / (time.perf_counter() - t0)
    line = json.dumps({"images": a.n, "size": f"{maxH}x{maxW} RGB8", "threads": a.threads, "burst": a.burst,
                       "shipped_planes": "lds" if lib.vip_vp8_default_stages() & LDS else "scratch",
                       "vp8_file_bytes_mean": int(np.mean([len(b) for b in lossy])), "vp8_stream_bytes": int(staged.stream.numel()),
                       "vp8_host_stage_ms": round(v_ms, 3),
                       **{f"vp8_device_{k}_{tag}_planes_us": round(v, 1) for (tag, k), v in timed.items()},
                       "vp8_device_output_us": round(out_us, 1),
                       "vp8_decode_images_resize_img_per_s": round(v_e2e, 1), "pillow_vp8_img_per_s": round(pil, 1),
                       "vp8l_host_stage_ms": round(l_ms, 3), "vp8l_decode_images_resize_img_per_s": round(l_e2e, 1),
                       "jpeg_host_stage_ms": round(j_ms, 3), "jpeg_decode_images_resize_img_per_s": round(j_e2e, 1)})
    print(line)
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
