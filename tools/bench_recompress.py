"""Recompression stress test, timed: 256 synthetic 200x200 images (tools/make_synth), decoded once.
  forward stage  vip_jpeg_fdct_quant_u8 (colour + downsample, then FDCT + quantise)           - HIP events, us
  decode stage   vip_jpeg_idct_rgb_u8 on the coefficients the forward stage wrote (yardstick)  - HIP events, us
  recompress     pipeline.recompress (layout on the host, descriptor H2D, both stages)         - HIP events, us
  ensemble       one stress_batch with three qualities against one plain _score_batch          - HIP events, ms  (--members 0 skips it)
The two stages are timed alternately in the same loop.  Algorithmic bytes of the forward stage per image = pixels read + planes
written and read + coefficients written; its rate is given against the 6.1 TB/s the project's copy probe measured.
usage: python tools/bench_recompress.py [--n 256] [--reps 50] [--quality 75] [--members 1]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_PEAK = 6.1e12      # bytes/s, bench.py's copy probe on the MI355X


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--members", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_recompress: no GPU visible - nothing to measure")
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, ensemble, pipeline, zoo
    from vipcup_amd.ops import _p, _stream
    from tools.make_synth import synth_jpeg
    raws = [synth_jpeg(i) for i in range(a.n + a.n // 49 + 1) if i % 50 != 49][:a.n]          # the 200x200 ones
    batch = pipeline.decode_images(raws)
    n, maxH, maxW, _ = batch.rgb.shape
    lib = _abi.lib()
    out = {"images": n, "size": f"{maxW}x{maxH}", "quality": a.quality, "reps": a.reps}
    for sampling in ("4:2:0", "4:4:4"):
        desc, total, max_blocks = pipeline.encode_layout(batch.sizes_host, a.quality, sampling)
        desc_d = torch.from_numpy(np.frombuffer(bytes(desc), dtype=np.uint8).copy()).cuda()
        coef = torch.empty((total,), dtype=torch.int16, device="cuda")
        planes = torch.empty((total,), dtype=torch.uint8, device="cuda")
        rgb = torch.zeros_like(batch.rgb)

        def fwd():
            _abi.check(lib.vip_jpeg_fdct_quant_u8(_p(batch.rgb), _p(desc_d), n, max_blocks, _p(planes), _p(coef), maxH, maxW, _stream()),
                       "vip_jpeg_fdct_quant_u8")

        def dec():
            _abi.check(lib.vip_jpeg_idct_rgb_u8(_p(coef), _p(desc_d), n, max_blocks, _p(planes), _p(rgb), maxH, maxW, _stream()),
                       "vip_jpeg_idct_rgb_u8")

        t_f, t_d, t_r = [], [], []
        for r in range(a.reps + 5):                     # 5 warm-up rounds; the stages alternate
            f_, d_ = _timed(fwd), _timed(dec)
            r_ = _timed(lambda: pipeline.recompress(batch, a.quality, sampling))
            if r >= 5:
                t_f.append(f_), t_d.append(d_), t_r.append(r_)
        by = n * maxH * maxW * 3 + 2 * total + 2 * total    # pixels in, planes out and in again, int16 coefficients out
        fwd_us = float(np.median(t_f))
        out[sampling] = {"forward_us": round(fwd_us, 1), "forward_us_min_max": [round(min(t_f), 1), round(max(t_f), 1)],
                         "decode_us": round(float(np.median(t_d)), 1), "decode_us_min_max": [round(min(t_d), 1), round(max(t_d), 1)],
                         "recompress_us": round(float(np.median(t_r)), 1),
                         "forward_bytes_per_image": by // n, "forward_TB_per_s": round(by / fwd_us / 1e6, 3),
                         "forward_share_of_copy_peak": round(by / (fwd_us * 1e-6) / COPY_PEAK, 3)}
    if a.members:
        members = []
        for name, dim, idx in json.load(open(os.path.join(ROOT, "vip-cup-2022_amd", "ckpts", "ckpts.json"))):
            key = zoo.by_ckpt_name(name)
            members.append((zoo.MEMBERS[key], zoo.FoldMean([zoo.build_member(key)[1]])))
        qs = [90, 70, 50]
        for _ in range(2):                              # stream calibration + warm-up of every shape
            ensemble.stress_batch(batch, members, qs)
        torch.cuda.synchronize()
        t_p, t_s = [], []
        for _ in range(max(3, a.reps // 10)):
            t_p.append(_timed(lambda: ensemble._score_batch(batch, members)) / 1e3)
            t_s.append(_timed(lambda: ensemble.stress_batch(batch, members, qs)) / 1e3)
        out["ensemble"] = {"members": len(members), "qualities": qs, "score_batch_ms": round(float(np.median(t_p)), 2),
                           "stress_batch_ms": round(float(np.median(t_s)), 2),
                           "ratio": round(float(np.median(t_s)) / float(np.median(t_p)), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
