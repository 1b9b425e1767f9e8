"""Tone stress tests, timed: 256 synthetic 200x200 images (tools/make_synth), decoded once; for ac02, acl02, eq and clahe20 (grid 8)
  hist, lut, apply      the three launches of a variant one by one (vip_tone_hist_u8, vip_tone_lut_u8, vip_tone_apply_rgb_u8), buffers
                        allocated beforehand                                                                             - HIP events, us
  tone                  the variant as pipeline runs it: the three launches and their two torch.empty
  torch                 the same variant written in torch on the same uint8 pixels (bincount, cumsum, gather; float64 for the
                        auto-contrast table); its pixels are compared with the kernels' bit for bit before anything is timed
  gray                  the gray launch of vip_colour_rgb_u8: the same bytes through the same staging
  copy                  a plain copy_ of the same bytes: the floor of anything that reads and writes every pixel once
and, for clahe20's apply launch, the tile tables in their two placements (0: gathered from global memory through L1, 1: copied into LDS),
and, for the whole-image modes, the histogram and table launches with the image spread over 1, 4 or 16 workgroups (grid 1, 2, 4).
Every figure is the median over --reps of ``--burst`` back-to-back launches between two HIP events, divided by the burst; min and max of
the per-launch figure show the spread.  The sides are timed alternately in the same loop, after 5 warm-up rounds.  GB/s counts the image
bytes moved by a whole variant: every pixel read twice (histogram, apply) and written once.
usage: python tools/bench_tone.py [--n 256] [--reps 20] [--burst 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = [("ac02", "autocontrast", 2), ("acl02", "autocontrast_luma", 2), ("eq", "equalize", None), ("clahe20", "clahe", 2.0)]
GRID = 8


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


# ---- the variants in torch ----------------------------------------------------------------------------------------------------------
def _luma(rgb):
    x = rgb.to(torch.int32)
    return (19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 32768) >> 16


def _hist(values, groups, n_groups):
    """``values`` (0..255) counted per group -> int64 [n_groups, 256]"""
    return torch.bincount((groups * 256 + values).reshape(-1), minlength=n_groups * 256).view(n_groups, 256)


def _autocontrast_tables(h, cutoff):
    total = h.sum(-1, keepdim=True)
    cut = (total * cutoff) // 100
    lo = (h.cumsum(-1) > cut).to(torch.int32).argmax(-1)
    hi = 255 - (h.flip(-1).cumsum(-1) > cut).to(torch.int32).argmax(-1)
    i = torch.arange(256, device=h.device, dtype=torch.float64)
    d = (hi - lo).clamp(min=1).to(torch.float64)
    scale = torch.full_like(d, 255.0) / d                  # a true division: "255.0 / d" is reciprocal(d) * 255 in torch, rounded twice
    offset = (-lo).to(torch.float64) * scale
    lut = (i * scale[..., None] + offset[..., None]).trunc().clamp(0, 255)
    return torch.where((hi > lo)[..., None], lut, i.expand_as(lut)).to(torch.uint8)


def _equalize_tables(h):
    total = h.sum(-1)
    last = h.gather(-1, (255 - (h.flip(-1) > 0).to(torch.int32).argmax(-1))[..., None])[..., 0]
    step = (total - last) // 255
    ok = ((h > 0).sum(-1) >= 2) & (step > 0)
    s = step.clamp(min=1)[..., None]
    lut = ((s // 2 + h.cumsum(-1) - h) // s).clamp(max=255)
    return torch.where(ok[..., None], lut, torch.arange(256, device=h.device).expand_as(lut)).to(torch.uint8)


def _torch_global(rgb, mode, arg):
    n = rgb.shape[0]
    img = torch.arange(n, device=rgb.device).view(n, 1, 1)
    if mode == "autocontrast_luma":
        lut = _autocontrast_tables(_hist(_luma(rgb).long(), img, n), arg)
        return lut.gather(1, rgb.reshape(n, -1).long()).view(rgb.shape)
    chan = torch.arange(3, device=rgb.device)
    h = _hist(rgb.long(), img[..., None] * 3 + chan, n * 3)
    lut = (_autocontrast_tables(h, arg) if mode == "autocontrast" else _equalize_tables(h)).view(n, 3, 256)
    return lut.gather(2, rgb.permute(0, 3, 1, 2).reshape(n, 3, -1).long()).view(n, 3, rgb.shape[1], rgb.shape[2]).permute(0, 2, 3, 1)


def _torch_clahe(rgb, tt, axes):
    """every image H x W with H, W multiples of GRID: tiles of equal size; ``axes`` = the neighbours and weights per row and column"""
    n, H, W, _ = rgb.shape
    th, tw = H // GRID, W // GRID
    Y = _luma(rgb).long()
    tile = (torch.arange(H, device=rgb.device) // th)[:, None] * GRID + (torch.arange(W, device=rgb.device) // tw)[None, :]
    h = _hist(Y, torch.arange(n, device=rgb.device).view(n, 1, 1) * GRID * GRID + tile, n * GRID * GRID)
    A = th * tw
    hc = h.clamp(max=max(1, tt * A // 2560))
    E = A - hc.sum(-1, keepdim=True)
    i = torch.arange(256, device=rgb.device)
    rem = E % 256
    h2 = hc + E // 256 + ((i * rem) // 256 != ((i + 1) * rem) // 256)
    T = ((h2.cumsum(-1) * 255 + A // 2) // A).view(n, GRID, GRID, 256)
    (ky0, ky1, wy), (kx0, kx1, wx) = axes
    flat = T.view(n, -1)

    def at(ky, kx):
        return flat.gather(1, (((ky[:, None] * GRID + kx[None, :]) * 256)[None] + Y).view(n, -1)).view(n, H, W)

    wy, wx = wy[:, None], wx[None, :]
    V = ((256 - wy) * ((256 - wx) * at(ky0, kx0) + wx * at(ky0, kx1)) + wy * ((256 - wx) * at(ky1, kx0) + wx * at(ky1, kx1)) + 32768) >> 16
    return (rgb.long() + (V - Y)[..., None]).clamp(0, 255).to(torch.uint8)


def _axis(side, g, device):
    """the neighbouring tiles and the weight per pixel of an axis (include/vipcup_hip.h), on the host once"""
    b = [(k * side) // g for k in range(g + 1)]
    c2 = [b[k] + b[k + 1] for k in range(g)]
    k0, k1, wq = [], [], []
    for x in range(side):
        X2 = 2 * x + 1
        if X2 < c2[0]:
            k0.append(0), k1.append(0), wq.append(0)
        elif X2 >= c2[-1]:
            k0.append(g - 1), k1.append(g - 1), wq.append(0)
        else:
            k = max(j for j in range(g - 1) if c2[j] <= X2)
            k0.append(k), k1.append(k + 1), wq.append(((X2 - c2[k]) << 8) // (c2[k + 1] - c2[k]))
    return tuple(torch.tensor(v, device=device) for v in (k0, k1, wq))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tone: no GPU visible - nothing to measure")
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    from vipcup_amd.ops import _launch, _p
    from tools.make_synth import synth_jpeg
    raws = [synth_jpeg(i) for i in range(a.n + a.n // 49 + 1) if i % 50 != 49][:a.n]          # the 200x200 ones
    batch = pipeline.decode_images(raws)
    n, H, W, _ = batch.rgb.shape
    assert all(s == (H, W) for s in batch.sizes_host) and H % GRID == 0 and W % GRID == 0 and pipeline.tone_grid(H, W, GRID) == (GRID, GRID)
    dst = torch.zeros_like(batch.rgb)
    axes = (_axis(H, GRID, batch.rgb.device), _axis(W, GRID, batch.rgb.device))
    cases, bursts = {}, {}                                                                    # name -> launch, name -> burst

    def launches(mode, arg, grid):
        """the three launches of a variant on buffers of their own -> (hist, lut, apply(placement))"""
        m, param, _ = pipeline._tone_args(mode, arg, grid)
        c = 3 if m in (0, 2) else 1
        gy, gx = pipeline.tone_grid(H, W, grid)
        hist = torch.empty((n, gy * gx, c, 256), dtype=torch.int32, device="cuda")
        lut = torch.empty((n, gy * gx if m == 3 else c, 256), dtype=torch.uint8, device="cuda")

        def f_hist():
            _launch("vip_tone_hist_u8", _p(batch.rgb), _p(batch.sizes), n, H, W, grid, c, _p(hist), gy * gx)

        def f_lut():
            _launch("vip_tone_lut_u8", _p(hist), n, gy * gx, m, param, _p(lut))

        def f_apply(placement=0):
            _launch("vip_tone_apply_rgb_u8_placed", _p(batch.rgb), _p(batch.sizes), H, W, _p(dst), H, W, _p(lut), m, grid, gy * gx, placement, n)

        return f_hist, f_lut, f_apply

    for name, mode, arg in VARIANTS:
        grid = GRID if mode == "clahe" else pipeline._TONE_GLOBAL_GRID
        f_hist, f_lut, f_apply = launches(mode, arg, grid)
        if mode == "clahe":
            yard = lambda arg=arg: _torch_clahe(batch.rgb, int(round(arg * 10)), axes)        # noqa: E731
        else:
            yard = lambda mode=mode, arg=arg: _torch_global(batch.rgb, mode, arg)             # noqa: E731
        whole = lambda mode=mode, arg=arg: pipeline._tone_into(batch, mode, arg, GRID, dst)   # noqa: E731
        whole()                                          # the kernels and the torch formulation compute the same pixels
        want = yard()
        torch.cuda.synchronize()
        assert torch.equal(dst, want), f"{name}: the kernels and the torch formulation differ in {int((dst != want).sum())} samples"
        assert not torch.equal(dst, batch.rgb)
        f_hist(), f_lut()
        for placement in ((0, 1) if mode == "clahe" else (0,)):
            dst.zero_()
            f_apply(placement)
            torch.cuda.synchronize()
            assert torch.equal(dst, want), (name, placement)
        cases[f"{name}_hist"], cases[f"{name}_lut"], cases[f"{name}_tone"], cases[f"{name}_torch"] = f_hist, f_lut, whole, yard
        bursts[f"{name}_torch"] = max(1, a.burst // 10)
        if mode == "clahe":
            cases[f"{name}_apply_global"], cases[f"{name}_apply_lds"] = (lambda f=f_apply: f(0)), (lambda f=f_apply: f(1))
        else:
            cases[f"{name}_apply"] = f_apply
    for grid in (1, 2, 4):                               # the whole-image histogram over 1, 4 or 16 workgroups per image
        f_hist, f_lut, _ = launches("autocontrast", 2, grid)
        cases[f"ac02_hist_grid{grid}"], cases[f"ac02_lut_grid{grid}"] = f_hist, f_lut
    gray_coef, _ = pipeline._colour_coef(*pipeline.colour_gray())
    cases["gray"] = lambda: pipeline._colour_into(batch, gray_coef, None, None, dst)
    cases["copy"] = lambda: dst.copy_(batch.rgb)

    times = {name: [] for name in cases}
    for rep in range(a.reps + 5):                        # 5 warm-up rounds; the sides alternate
        for name, fn in cases.items():
            t = _timed(fn, bursts.get(name, a.burst))
            if rep >= 5:
                times[name].append(t)
    by = 3 * n * H * W * 3                               # pixels read twice + pixels written once
    out = {"images": n, "size": f"{W}x{H}", "reps": a.reps, "burst": a.burst, "grid": GRID, "global_grid": pipeline._TONE_GLOBAL_GRID,
           "image_bytes_moved_by_a_variant": by, "launches": {name: _stats(times[name]) for name in cases}}
    print(json.dumps(out))
    L = out["launches"]
    for name, mode, _ in VARIANTS:                       # the same figures, one line per variant
        ap_ = L[f"{name}_apply_global"] if mode == "clahe" else L[f"{name}_apply"]
        parts = L[f"{name}_hist"]["us"] + L[f"{name}_lut"]["us"] + ap_["us"]
        t, y = L[f"{name}_tone"], L[f"{name}_torch"]
        verdict = "faster than" if y["us"] > t["us"] else "NOT faster than"
        print(f"{name}: hist {L[f'{name}_hist']['us']} + lut {L[f'{name}_lut']['us']} + apply {ap_['us']} = {parts:.1f} us; as pipeline.tone "
              f"{t['us']} us (min {t['us_min_max'][0]}, max {t['us_min_max'][1]}), {by / t['us'] / 1e3:.1f} GB/s of image bytes; "
              f"{t['us'] / L['gray']['us']:.2f}x the gray launch, {t['us'] / L['copy']['us']:.2f}x the copy; torch {y['us']} us -> "
              f"{y['us'] / t['us']:.1f}x: the kernels are {verdict} the torch formulation")
    g, l = L["clahe20_apply_global"], L["clahe20_apply_lds"]
    print(f"clahe20 apply, tile tables gathered from global memory: {g['us']} us (min {g['us_min_max'][0]}, max {g['us_min_max'][1]}); copied "
          f"into LDS: {l['us']} us (min {l['us_min_max'][0]}, max {l['us_min_max'][1]})")
    for grid in (1, 2, 4):
        hh, ll = L[f"ac02_hist_grid{grid}"], L[f"ac02_lut_grid{grid}"]
        print(f"ac02 histogram over grid {grid}: hist {hh['us']} us + lut {ll['us']} us = {hh['us'] + ll['us']:.1f} us")
    print(f"gray launch {L['gray']['us']} us; copy_ of the same bytes {L['copy']['us']} us")


if __name__ == "__main__":
    main()
