"""Test helpers for the lossy WebP re-save (csrc/vp8_enc.hpp, vp8_enc_host.cpp, vp8_encode.hip): the corpus, the CPU check
program (tests/fuzz/vp8_enc_check.cpp: the same arithmetic compiled as plain C++ and run serially) and the way from an
encoder's modes and levels to a file libwebp decodes (``_vp8.write_keyframe``).  No torch here."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from tests import _vp8

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ZIGZAG = _vp8.ZIGZAG

# libwebp's quality -> quantiser index curve, quality 1..100 (include/vipcup_hip.h states it); literals, so that it cannot drift
BASE_Q = (103, 96, 92, 89, 86, 83, 81, 79, 77, 75, 73, 72, 70, 69, 68, 66, 65, 64, 63, 62, 61, 60, 59, 58, 57, 56, 55, 54, 53, 52,
          51, 51, 50, 49, 48, 48, 47, 46, 45, 45, 44, 43, 43, 42, 41, 41, 40, 40, 39, 38, 38, 37, 37, 36, 36, 35, 35, 34, 33, 33,
          32, 32, 31, 31, 30, 30, 29, 29, 28, 28, 28, 27, 27, 26, 26, 24, 23, 22, 21, 19, 18, 17, 16, 15, 14, 13, 12, 11, 10, 9,
          8, 7, 6, 5, 4, 3, 2, 1, 0, 0)


class Mb(C.Structure):
    """mirror of vip_vp8_mb (include/vipcup_hip.h); the package's _abi.Vp8Mb needs torch to import"""
    _fields_ = [("ymode", C.c_uint8), ("uvmode", C.c_uint8), ("flevel", C.c_uint8), ("ilevel", C.c_uint8), ("hev", C.c_uint8),
                ("inner", C.c_uint8), ("segment", C.c_uint8), ("skip", C.c_uint8), ("bmodes", C.c_uint8 * 16), ("nz", C.c_uint32),
                ("dc_only", C.c_uint32), ("coef_idx", C.c_uint32), ("reserved", C.c_uint32)]


MB_DTYPE = np.dtype([("ymode", "u1"), ("uvmode", "u1"), ("flevel", "u1"), ("ilevel", "u1"), ("hev", "u1"), ("inner", "u1"), ("segment", "u1"),
                     ("skip", "u1"), ("bmodes", "u1", (16,)), ("nz", "<u4"), ("dc_only", "<u4"), ("coef_idx", "<u4"), ("reserved", "<u4")])
assert MB_DTYPE.itemsize == C.sizeof(Mb) == 40


# ---- images ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def photograph():
    """the first committed photograph of tests/golden (ref_*.jpg), decoded by Pillow: uint8 [h, w, 3]"""
    from PIL import Image
    golden = os.path.join(HERE, "golden")
    name = sorted(f for f in os.listdir(golden) if f.startswith("ref_") and f.endswith(".jpg"))[0]
    return np.array(Image.open(os.path.join(golden, name)).convert("RGB"))


def image(kind, h, w):
    """uint8 [h, w, 3] of one content kind"""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "flat":
        return np.full((h, w, 3), 130, np.uint8)              # Y = U = V = 128, what the frame's border predicts: nothing to code
    if kind == "photo":
        p = photograph()
        reps = (-(-h // p.shape[0]), -(-w // p.shape[1]), 1)
        return np.ascontiguousarray(np.tile(p, reps)[:h, :w])
    if kind == "noise":
        return np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "hramp":
        v = (xx * 255 // max(1, w - 1)).astype(np.uint8)
    elif kind == "vramp":
        v = (yy * 255 // max(1, h - 1)).astype(np.uint8)
    elif kind == "dramp":
        v = ((xx + yy) * 255 // max(1, h + w - 2)).astype(np.uint8)
    elif kind == "adramp":                                   # the other diagonal, in steps: edges at 45 degrees
        v = (((xx - yy) // 3 * 40) % 256).astype(np.uint8)
    elif kind == "checker":
        v = ((((xx >> 2) + (yy >> 2)) & 1) * 200 + 20).astype(np.uint8)
    else:
        raise ValueError(kind)
    return np.stack([v, (v.astype(np.int32) * 3 // 4 + 30).astype(np.uint8), 255 - v], axis=-1)


SHAPES = ((16, 16), (33, 17), (40, 48), (200, 200), (16, 224))      # (h, w): 16 x 16, 17 x 33, 48 x 40, 200 x 200, 224 x 16 as w x h
KINDS = ("flat", "photo", "noise", "hramp", "vramp", "dramp", "adramp", "checker")
QUALITIES = (1, 30, 75, 100)


def cases():
    """(name, quality, image): every shape with every content, the qualities going round so that every content meets every
    quality on some shape; uniform noise always at 100 (large levels) and once more at 1; 200 x 200 only for three contents"""
    out = []
    for si, (h, w) in enumerate(SHAPES):
        for ki, kind in enumerate(KINDS):
            if (h, w) == (200, 200) and kind not in ("photo", "checker", "flat"):
                continue
            q = 100 if kind == "noise" else QUALITIES[(si + ki) % 4]
            out.append((f"{kind}_{w}x{h}_q{q}", q, image(kind, h, w)))
    out.append(("noise_48x40_q1", 1, image("noise", 40, 48)))
    return out


# ---- the check program -----------------------------------------------------------------------------------------

def build_check(tmp):
    exe = os.path.join(str(tmp), "vp8_enc_check")
    cmd = ["g++", "-O2", "-std=c++17", f"-I{ROOT}/include", f"-I{ROOT}/vip-cup-2022_amd/csrc", os.path.join(HERE, "fuzz", "vp8_enc_check.cpp"),
           os.path.join(ROOT, "vip-cup-2022_amd", "csrc", "vp8_enc_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


class Encoded:
    """what an encoder gave for one image: ``mbs`` (structured array, MB_DTYPE), ``levels`` int16 [nmb, 25, 16] raster, ``coefs`` int16
    [nmb, 25, 16] (coded blocks back to back per macroblock, the rest zero), ``planes`` uint8 (unfiltered), ``rgb`` uint8 [h, w, 3]"""

    def __init__(self, w, h, quality, base_q, filter_level, mbs, levels, coefs, planes, rgb):
        self.w, self.h, self.quality, self.base_q, self.filter_level = w, h, quality, base_q, filter_level
        self.mbs, self.levels, self.coefs, self.planes, self.rgb = mbs, levels, coefs, planes, rgb


def run_check(exe, items, tmp, k=None):
    """items: [(name, quality, image)] -> [Encoded], one process for all"""
    args = [exe] + (["--k", str(k)] if k is not None else [])
    paths = []
    for name, q, img in items:
        path = os.path.join(str(tmp), name + ".rgb")
        np.ascontiguousarray(img).tofile(path)
        h, w, _ = img.shape
        args += [str(q), str(w), str(h), path]
        paths.append(path)
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(items)
    out = []
    for (name, q, img), path, line in zip(items, paths, lines):
        w, h, base_q, level, n_i4, nmb = (int(v) for v in line.split())
        tag = f"{path}.q{q}"
        out.append(Encoded(w, h, q, base_q, level, np.fromfile(tag + ".mb", dtype=MB_DTYPE), np.fromfile(tag + ".lv", dtype=np.int16).reshape(nmb, 25, 16),
                           np.fromfile(tag + ".cf", dtype=np.int16).reshape(nmb, 25, 16), np.fromfile(tag + ".pl", dtype=np.uint8),
                           np.fromfile(tag + ".out", dtype=np.uint8).reshape(h, w, 3)))
    return out


# ---- modes and levels -> a file --------------------------------------------------------------------------------

def keyframe(enc):
    """the lossy WebP file of an encoder's decisions: modes from the records, levels raster -> zigzag, the frame's quantiser index and
    filter level, the normal filter at sharpness 0, ``skip`` exactly on the macroblocks without a non-zero level"""
    mbs = []
    for m, lv in zip(enc.mbs, enc.levels):
        i4 = int(m["ymode"]) == _vp8.B_PRED
        coefs = {}
        for b in range(25):
            if b == 24 and i4:
                continue
            if lv[b].any():
                coefs[b] = [int(lv[b][ZIGZAG[n]]) for n in range(16)]
        M = dict(ymode=int(m["ymode"]), uvmode=int(m["uvmode"]), skip=not lv.any(), coefs=coefs)
        if i4:
            M["bmodes"] = [int(v) for v in m["bmodes"]]
        mbs.append(M)
    return _vp8.write_keyframe(enc.w, enc.h, mbs, base_q=enc.base_q, level=enc.filter_level, simple=0, sharpness=0)


def coverage(encs):
    """what occurred over a list of Encoded: sets of 16 x 16, chroma and sub-block modes, skipped / coded, the largest |level|"""
    y16, uv, sub, skipped, coded, top = set(), set(), set(), False, False, 0
    for e in encs:
        for m, lv in zip(e.mbs, e.levels):
            uv.add(int(m["uvmode"]))
            if int(m["ymode"]) == _vp8.B_PRED:
                sub.update(int(v) for v in m["bmodes"])
            else:
                y16.add(int(m["ymode"]))
            skipped |= not lv.any()
            coded |= bool(lv.any())
            top = max(top, int(np.abs(lv).max()))
    return y16, uv, sub, skipped, coded, top
