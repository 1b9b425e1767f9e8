"""CPU: the two constants of the lossy WebP re-save that are fitted to libwebp's encoder ("Lossy WebP re-save").

    python tools/fit_vp8_encoder.py [--synth 8]

Set: the first ``--synth`` synthetic JPEGs (tools/make_synth.py) and tests/golden/ref_*.jpg, decoded by Pillow.  libwebp's side: the
pixels saved by Pillow as lossy WebP (method 4) and read back by the host decoder (``vip_vp8_entropy_h``), whose macroblock records
hold what libwebp's encoder chose.
 (1) mode bias: the share of macroblocks with sub-block modes at quality 50, 75, 90, against the share the project's encoder
     (tests/fuzz/vp8_enc_check.cpp, ``--k K``) gives for K = 0..64; the K whose share, averaged over the set, is closest.
 (2) filter level: the mean ``flevel`` of libwebp's records at quality 30, 50, 75, 90, and the least-squares integers a, b of
     level = clamp((a * base_q + b) >> 4, 0, 63) over those readings."""
import argparse
import ctypes as C
import glob
import io
import os
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def libwebp_records(img, quality):
    from tests import _vp8
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    raw = _vp8.pillow_lossy(img, quality, 4)
    lib = _abi.lib()
    buf = np.frombuffer(raw, dtype=np.uint8)
    ptrs = (C.c_void_p * 1)(buf.ctypes.data)
    lens = (C.c_size_t * 1)(len(raw))
    desc = (_abi.Vp8Desc * 1)()
    need, used = C.c_size_t(0), C.c_size_t(0)
    _abi.check(lib.vip_vp8_probe_h(ptrs[0], lens[0], C.byref(desc[0]), C.byref(need)), "vip_vp8_probe_h")
    stream = np.zeros((need.value + 8,), np.uint8)
    _abi.check(lib.vip_vp8_entropy_h(ptrs, lens, 1, desc, stream.ctypes.data_as(C.c_void_p), stream.size, C.byref(used), 1), "vip_vp8_entropy_h")
    from tests import _vp8_enc
    nmb = desc[0].mb_w * desc[0].mb_h
    return np.frombuffer(stream[desc[0].stream_off + desc[0].mb_off:][:nmb * 40].tobytes(), dtype=_vp8_enc.MB_DTYPE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synth", type=int, default=8)
    a = ap.parse_args()
    from tests import _vp8_enc
    from tools.make_synth import synth_jpeg
    images = [(f"synth_{i}", np.array(Image.open(io.BytesIO(synth_jpeg(i))).convert("RGB"))) for i in range(a.synth)]
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_*.jpg"))):
        images.append((os.path.basename(path), np.array(Image.open(path).convert("RGB"))))
    print("set:", ", ".join(f"{n} {im.shape[1]}x{im.shape[0]}" for n, im in images))
    with tempfile.TemporaryDirectory() as tmp:
        exe = _vp8_enc.build_check(tmp)
        # (1)
        qs = (50, 75, 90)
        theirs = {q: [float((libwebp_records(im, q)["ymode"] == 4).mean()) for _, im in images] for q in qs}
        target = float(np.mean([theirs[q] for q in qs]))
        for q in qs:
            print(f"libwebp i4 share at quality {q}: {np.mean(theirs[q]):.4f}")
        print(f"libwebp i4 share, mean: {target:.4f}")
        items = [(f"{n}_{q}", q, im) for q in qs for n, im in images]
        best = None
        for k in range(0, 65):
            encs = _vp8_enc.run_check(exe, items, tmp, k=k)
            share = float(np.mean([(e.mbs["ymode"] == 4).mean() for e in encs]))
            per_q = [float(np.mean([(e.mbs["ymode"] == 4).mean() for e in encs[i * len(images):(i + 1) * len(images)]])) for i in range(len(qs))]
            print(f"k = {k:2d}: own i4 share {share:.4f}  (per quality {', '.join(f'{v:.4f}' for v in per_q)})")
            if best is None or abs(share - target) < abs(best[1] - target):
                best = (k, share)
        print(f"chosen k = {best[0]}: own share {best[1]:.4f} against libwebp's {target:.4f}")
        # (2)
        readings = []
        for q in (30, 50, 75, 90):
            level = float(np.mean([libwebp_records(im, q)["flevel"].mean() for _, im in images]))
            readings.append((_vp8_enc.BASE_Q[q - 1], level))
            print(f"libwebp at quality {q}: base_q {_vp8_enc.BASE_Q[q - 1]}, mean flevel {level:.3f}")
        x = np.array([r[0] for r in readings], float)
        y = np.array([r[1] for r in readings], float)
        best = None
        for fa in range(0, 64):
            for fb in range(-256, 257):
                err = float(((np.clip((fa * x.astype(int) + fb) // 16, 0, 63) - y) ** 2).sum())
                if best is None or err < best[0]:
                    best = (err, fa, fb)
        print(f"fit: level = clamp(({best[1]} * base_q + {best[2]}) >> 4, 0, 63), squared error {best[0]:.3f}: "
              + ", ".join(f"base_q {int(bq)} -> {int(np.clip((best[1] * int(bq) + best[2]) // 16, 0, 63))} (libwebp {lv:.2f})" for bq, lv in readings))


if __name__ == "__main__":
    main()
