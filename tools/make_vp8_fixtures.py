"""Make tests/golden/vp8/*.webp and MANIFEST.json: small lossy WebP files with the encoder settings Pillow cannot be asked
for - filter_type 0 / 1, partitions 0..3, segments 1..4, filter_sharpness 0 / 3 / 7, filter_strength 0 / 20 / 100.

    python tools/make_vp8_fixtures.py --include DIR --libdir DIR [--decoder LIBWEBP.so ...]

Compiles tools/make_vp8_fixtures.c against the libwebp under --include / --libdir, encodes every setting, and writes a
file only after every decoder at hand - Pillow's bundled libwebp and each --decoder library (WebPDecodeRGB through ctypes)
- has given the same pixels for it.  Run once; the files are committed."""
import argparse
import ctypes as C
import io
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "vp8")

# name, width, height, quality, method, filter_type, partitions, segments, sharpness, strength
# (libwebp's encoder writes more than one partition only at methods 0..2)
SETTINGS = [
    ("simple_p0_s1_sh0_f20", 48, 40, 60, 4, 0, 0, 1, 0, 20),
    ("simple_p1_s2_sh3_f100", 33, 17, 40, 2, 0, 1, 2, 3, 100),
    ("simple_p2_s4_sh7_f20", 64, 64, 30, 2, 0, 2, 4, 7, 20),
    ("normal_p3_s4_sh0_f100", 64, 64, 50, 1, 1, 3, 4, 0, 100),
    ("normal_p1_s3_sh3_f20", 17, 16, 75, 0, 1, 1, 3, 3, 20),
    ("normal_p2_s1_sh7_f100", 40, 64, 20, 2, 1, 2, 1, 7, 100),
    ("normal_p0_s2_sh0_f0", 48, 40, 60, 4, 1, 0, 2, 0, 0),
    ("simple_p3_s3_sh3_f0", 64, 48, 80, 0, 0, 3, 3, 3, 0),
    ("normal_p3_s4_sh7_f63", 64, 64, 5, 4, 1, 3, 4, 7, 63),
]


def decode_with(lib, raw):
    lib.WebPDecodeRGB.restype = C.POINTER(C.c_uint8)
    lib.WebPDecodeRGB.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    w, h = C.c_int(0), C.c_int(0)
    p = lib.WebPDecodeRGB(raw, len(raw), C.byref(w), C.byref(h))
    assert p, "WebPDecodeRGB failed"
    out = np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    lib.WebPFree.argtypes = [C.c_void_p]
    lib.WebPFree(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--include", required=True)
    ap.add_argument("--libdir", required=True)
    ap.add_argument("--decoder", action="append", default=[], help="a libwebp shared library to decode with, besides Pillow's")
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    decoders = [C.CDLL(p) for p in a.decoder]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "make_vp8_fixtures")
        subprocess.run(["gcc", "-O1", f"-I{a.include}", os.path.join(HERE, "make_vp8_fixtures.c"), "-o", exe, f"-L{a.libdir}",
                        f"-Wl,-rpath,{a.libdir}", "-lwebp", "-lm"], check=True)
        files = []
        for k, (name, w, h, q, m, ft, parts, segs, sharp, strength) in enumerate(SETTINGS):
            path = os.path.join(tmp, name + ".webp")
            subprocess.run([exe, path, str(w), str(h), str(k + 1), str(q), str(m), str(ft), str(parts), str(segs), str(sharp),
                            str(strength)], check=True)
            raw = open(path, "rb").read()
            assert len(raw) <= 8192 and w <= 64 and h <= 64, (name, len(raw))
            want = np.array(Image.open(io.BytesIO(raw)).convert("RGB"))
            for d, p in zip(decoders, a.decoder):
                assert np.array_equal(decode_with(d, raw), want), f"{name}: {p} and Pillow decode different pixels"
            with open(os.path.join(OUT, name + ".webp"), "wb") as f:
                f.write(raw)
            files.append({"name": name + ".webp", "width": w, "height": h, "quality": q, "method": m, "filter_type": ft, "partitions": parts,
                          "segments": segs, "filter_sharpness": sharp, "filter_strength": strength, "bytes": len(raw)})
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as f:
        json.dump({"made_by": "tools/make_vp8_fixtures.py", "decoders_agreeing": 1 + len(decoders), "files": files}, f, indent=1)
        f.write("\n")
    print(f"{len(files)} fixtures, {sum(x['bytes'] for x in files)} bytes, {1 + len(decoders)} decoders agree")
    return 0


if __name__ == "__main__":
    sys.exit(main())
