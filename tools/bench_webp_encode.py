"""The lossy WebP re-save, timed: 256 synthetic 200x200 images (tools/make_synth), decoded once, at quality 75
  encode                the encode launch (vip_vp8_encode_rgb_u8) on buffers allocated beforehand              - HIP events, us
  filter_output         the decoder's loop filter and RGB output on what it wrote (vip_vp8_reconstruct_stages_rgb_u8, FILTER | OUTPUT)
  webp_recompress       the whole pipeline.webp_recompress call: the layout on the host, the descriptors' copy, five torch.empty / zeros
                        and the two launches
  jpeg_recompress       pipeline.recompress at quality 75 (4:2:0) on the same batch: the JPEG re-save
  copy                  a plain copy_ of the same bytes: the floor of anything that reads and writes every pixel once
  pillow                Pillow (libwebp, method 4) encoding and decoding the same images on 16 threads               - wall clock, ms
Every device figure is the median over --reps of ``--burst`` back-to-back calls between two HIP events, divided by the burst; min and
max of the per-call figure show the spread.  The sides are timed alternately in the same loop, after 5 warm-up rounds.
Before anything is timed, three images of the batch are checked against Pillow's decode of the file their levels make.
usage: python tools/bench_webp_encode.py [--n 256] [--reps 20] [--burst 5] [--quality 75]"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--quality", type=int, default=75)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_webp_encode: no GPU visible - nothing to measure")
    import vipcup_amd  # noqa: F401
    from PIL import Image
    from vipcup_amd import pipeline
    from vipcup_amd.ops import _launch, _p
    from tests import _vp8, _vp8_enc
    from tools.make_synth import synth_jpeg
    raws = [synth_jpeg(i) for i in range(a.n + a.n // 49 + 1) if i % 50 != 49][:a.n]          # the 200x200 ones
    batch = pipeline.decode_images(raws)
    n, H, W, _ = batch.rgb.shape
    assert all(s == (H, W) for s in batch.sizes_host)
    q = a.quality

    enc = pipeline.webp_encode(batch, q)
    out = pipeline.webp_recompress(batch, q)
    torch.cuda.synchronize()
    stream, levels, rgb = enc.stream.cpu().numpy(), enc.levels.cpu().numpy(), out.rgb.cpu().numpy()
    i4 = []
    for i, d in enumerate(enc.desc):
        nmb = d.mb_w * d.mb_h
        mbs = np.frombuffer(stream[d.stream_off:d.stream_off + nmb * 40].tobytes(), dtype=_vp8_enc.MB_DTYPE)
        i4.append(float((mbs["ymode"] == 4).mean()))
        if i < 3:                                        # the pixels are those of the file these levels make
            first = d.plane_off // 384
            e = _vp8_enc.Encoded(W, H, q, enc.params.base_q, enc.params.filter_level, mbs, levels[first:first + nmb], None, None, rgb[i])
            assert np.array_equal(_vp8.pillow_rgb(_vp8_enc.keyframe(e)), rgb[i]), f"image {i}: libwebp decodes the file to other pixels"
    src = batch.rgb.cpu().numpy()
    psnr = float(np.mean([10 * np.log10(255.0 ** 2 / np.mean((rgb[i].astype(np.float64) - src[i]) ** 2)) for i in range(n)]))

    dst = torch.zeros_like(batch.rgb)

    def f_encode():
        _launch("vip_vp8_encode_rgb_u8", _p(batch.rgb), _p(enc.desc_d), n, H, W, q, _p(enc.stream), enc.stream.numel(), _p(enc.levels),
                enc.levels.numel(), _p(enc.scratch), enc.scratch.numel())

    keep = enc.scratch.clone()                           # the filter works in place: every call starts from the unfiltered planes

    def f_filter_output():
        enc.scratch.copy_(keep)
        _launch("vip_vp8_reconstruct_stages_rgb_u8", _p(enc.stream), enc.stream.numel(), _p(enc.desc_d), n, _p(enc.scratch), enc.scratch.numel(),
                _p(dst), H, W, 2 | 4)

    cases = {"encode": f_encode, "filter_output": f_filter_output, "planes_copy": lambda: enc.scratch.copy_(keep),
             "webp_recompress": lambda: pipeline.webp_recompress(batch, q), "jpeg_recompress": lambda: pipeline.recompress(batch, q),
             "copy": lambda: dst.copy_(batch.rgb)}
    times = {name: [] for name in cases}
    for rep in range(a.reps + 5):                        # 5 warm-up rounds; the sides alternate
        for name, fn in cases.items():
            t = _timed(fn, a.burst)
            if rep >= 5:
                times[name].append(t)
    f_encode()
    torch.cuda.synchronize()

    def pillow_one(img):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "WEBP", quality=q, method=4)
        return np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))

    walls = []
    with ThreadPoolExecutor(max_workers=16) as ex:
        for rep in range(4):
            t0 = time.perf_counter()
            done = list(ex.map(pillow_one, [src[i] for i in range(n)]))
            walls.append(1e3 * (time.perf_counter() - t0))
    psnr_pillow = float(np.mean([10 * np.log10(255.0 ** 2 / np.mean((done[i].astype(np.float64) - src[i]) ** 2)) for i in range(n)]))

    L = {name: _stats(times[name]) for name in cases}
    res = {"images": n, "size": f"{W}x{H}", "quality": q, "reps": a.reps, "burst": a.burst, "i4_share": round(float(np.mean(i4)), 4),
           "psnr_db": round(psnr, 2), "psnr_pillow_db": round(psnr_pillow, 2), "launches": L,
           "pillow_16_threads_ms": {"median": round(float(np.median(walls[1:])), 1), "all": [round(w, 1) for w in walls]}}
    print(json.dumps(res))
    fo = L["filter_output"]["us"] - L["planes_copy"]["us"]
    print(f"encode launch {L['encode']['us']} us (min {L['encode']['us_min_max'][0]}, max {L['encode']['us_min_max'][1]}) = "
          f"{L['encode']['us'] / n:.1f} us per image; filter + output {fo:.1f} us (timed with a copy of the planes in front, "
          f"{L['planes_copy']['us']} us, taken off); pipeline.webp_recompress {L['webp_recompress']['us']} us; pipeline.recompress (JPEG q{q}) "
          f"{L['jpeg_recompress']['us']} us -> the WebP re-save costs {L['webp_recompress']['us'] / L['jpeg_recompress']['us']:.1f}x the JPEG one; "
          f"copy_ {L['copy']['us']} us; Pillow on 16 threads {res['pillow_16_threads_ms']['median']} ms -> "
          f"{1e3 * res['pillow_16_threads_ms']['median'] / L['webp_recompress']['us']:.1f}x the GPU call")
    print(f"sub-block macroblocks {100 * res['i4_share']:.1f} %; PSNR against the source {psnr:.2f} dB (Pillow's own file at quality {q}: "
          f"{psnr_pillow:.2f} dB)")


if __name__ == "__main__":
    main()
