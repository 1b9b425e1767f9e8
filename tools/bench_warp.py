"""Geometric stress tests, timed: 256 synthetic 200x200 images (tools/make_synth), decoded once.
  flip_h, crop80, rot7.5_crop / _mirror / _black    vip_warp_affine_rgb_u8, one launch (transforms and sizes already on the device) - HIP events, us
  torch yardstick       the same transform on the same pixels, already converted to fp32 NCHW (the conversion is NOT timed):
                        F.affine_grid + F.grid_sample(bilinear, align_corners=False; zeros padding, reflection for the mirror fill)
  step                  one plain _score_batch of the ensemble on the batch: what a stress variant costs  - HIP events, ms  (--members 0 skips it)
The launches are timed alternately in the same loop, after 5 warm-up rounds.  GB/s counts the image bytes moved: every output pixel
written once and as many source pixels read once.
usage: python tools/bench_warp.py [--n 256] [--reps 50] [--members 1]"""
import argparse
import json
import math
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
    ap.add_argument("--members", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp: no GPU visible - nothing to measure")
    import torch.nn.functional as F
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, pipeline, zoo
    from tools.make_synth import synth_jpeg
    raws = [synth_jpeg(i) for i in range(a.n + a.n // 49 + 1) if i % 50 != 49][:a.n]          # the 200x200 ones
    batch = pipeline.decode_images(raws)
    n, H, W, _ = batch.rgb.shape
    assert all(s == (H, W) for s in batch.sizes_host)
    x32 = batch.rgb.permute(0, 3, 1, 2).float().contiguous()                                  # the yardstick's input, fp32 NCHW

    def case(name, m, out_hw, fill):
        """m = (a, b, tx, c, d, ty), the inverse map in pixel-edge coordinates -> (name, ours, yardstick, dst, inside mask)"""
        ho, wo = out_hw
        xf = np.array([pipeline.warp_matrix(*m)] * n, np.int64)
        xf_d, sizes_d = torch.from_numpy(xf).cuda(), torch.tensor([out_hw] * n, dtype=torch.int32, device="cuda")
        dst = torch.zeros((n, ho, wo, 3), dtype=torch.uint8, device="cuda")
        code = pipeline.WARP_FILLS[fill]

        def ours():
            pipeline._launch("vip_warp_affine_rgb_u8", pipeline._p(batch.rgb), pipeline._p(batch.sizes), H, W, pipeline._p(dst),
                             pipeline._p(sizes_d), ho, wo, pipeline._p(xf_d), code, n)

        # the same map in grid_sample's normalised coordinates (align_corners=False: -1 .. 1 are the image's edges)
        ca, cb, tx, cc, cd, ty = m
        theta = torch.tensor([[ca * wo / W, cb * ho / W, (ca * wo + cb * ho + 2 * tx) / W - 1],
                              [cc * wo / H, cd * ho / H, (cc * wo + cd * ho + 2 * ty) / H - 1]], dtype=torch.float32, device="cuda")
        theta = theta[None].expand(n, 2, 3).contiguous()
        pad = "zeros" if fill == "black" else "reflection"

        def yard():
            return F.grid_sample(x32, F.affine_grid(theta, (n, 3, ho, wo), align_corners=False), mode="bilinear", padding_mode=pad,
                                 align_corners=False)

        g = F.affine_grid(theta[:1], (1, 3, ho, wo), align_corners=False)[0]                  # taps inside: where the fills cannot matter
        inside = (g[..., 0].abs() <= 1 - 3.0 / W) & (g[..., 1].abs() <= 1 - 3.0 / H)
        return name, ours, yard, dst, inside

    t = math.radians(7.5)
    rot = (math.cos(t), -math.sin(t), math.sin(t), math.cos(t))

    def rotation(out_hw):
        ho, wo = out_hw
        return (rot[0], rot[1], W / 2 - rot[0] * wo / 2 - rot[1] * ho / 2, rot[2], rot[3], H / 2 - rot[2] * wo / 2 - rot[3] * ho / 2)

    ch, cw = pipeline.scaled_size(H, W, 80)
    rect = pipeline.rotated_rect(H, W, 7.5)
    cases = [case("flip_h", (-1, 0, W, 0, 1, 0), (H, W), "black"),
             case("crop80", (1, 0, (W - cw) // 2, 0, 1, (H - ch) // 2), (ch, cw), "black"),
             case("rot7.5_crop", rotation(rect), rect, "mirror"),
             case("rot7.5_mirror", rotation((H, W)), (H, W), "mirror"),
             case("rot7.5_black", rotation((H, W)), (H, W), "black")]

    for name, ours, yard, dst, inside in cases:          # the two sides compute the same thing
        ours()
        want = yard().round().clamp(0, 255).permute(0, 2, 3, 1)
        worst = float((dst.float() - want).abs()[:, inside].max())
        assert worst <= 1, f"{name}: the kernel and the torch yardstick differ by {worst} levels where every tap is inside"
    t_ours, t_yard = {c[0]: [] for c in cases}, {c[0]: [] for c in cases}
    for rep in range(a.reps + 5):                        # 5 warm-up rounds; the launches alternate
        for name, ours, yard, _, _ in cases:
            o_, y_ = _timed(ours), _timed(yard)
            if rep >= 5:
                t_ours[name].append(o_), t_yard[name].append(y_)
    out = {"images": n, "size": f"{W}x{H}", "reps": a.reps, "launches": {}}
    for name, _, _, dst, _ in cases:
        o, y = _stats(t_ours[name]), _stats(t_yard[name])
        by = 2 * dst.numel()                             # output pixels written once + as many source pixels read once
        out["launches"][name] = {**o, "out_size": f"{dst.shape[2]}x{dst.shape[1]}", "image_bytes_moved": by,
                                 "GB_per_s": round(by / o["us"] / 1e3, 1), "torch_fp32_us": y["us"], "torch_fp32_us_min_max": y["us_min_max"],
                                 "torch_over_kernel": round(y["us"] / o["us"], 2)}
    step_ms = None
    if a.members:
        members = []
        for mname, dim, idx in json.load(open(os.path.join(ROOT, "vip-cup-2022_amd", "ckpts", "ckpts.json"))):
            key = zoo.by_ckpt_name(mname)
            members.append((zoo.MEMBERS[key], zoo.FoldMean([zoo.build_member(key)[1]])))
        for _ in range(2):                               # stream calibration + warm-up of every shape
            ensemble._score_batch(batch, members)
        torch.cuda.synchronize()
        t_s = [_timed(lambda: ensemble._score_batch(batch, members)) / 1e3 for _ in range(max(20, a.reps // 2))]
        step_ms = float(np.median(t_s))
        out["ensemble"] = {"members": len(members), "score_batch_ms": round(step_ms, 2),
                           "score_batch_ms_min_max": [round(min(t_s), 2), round(max(t_s), 2)]}
        for name, *_ in cases:
            out["launches"][name]["share_of_step"] = round(out["launches"][name]["us"] / 1e3 / step_ms, 5)
    print(json.dumps(out))
    for name, v in out["launches"].items():              # the same figures, one line per launch
        share = f", {100 * v['share_of_step']:.3f} % of a plain step ({step_ms:.1f} ms)" if step_ms else ""
        verdict = "faster than" if v["torch_over_kernel"] > 1 else "SLOWER than"
        print(f"{name}: {v['us']} us (min {v['us_min_max'][0]}, max {v['us_min_max'][1]}), {v['GB_per_s']} GB/s of image bytes{share}; "
              f"torch fp32 yardstick {v['torch_fp32_us']} us -> {v['torch_over_kernel']}x: the kernel is {verdict} the yardstick")


if __name__ == "__main__":
    main()
