"""NumPy restatement of the inverse affine warp of the geometric stress tests, the suite's oracle for csrc/warp.hip.  Written from the
specification (include/vipcup_hip.h), not from the kernel or from pipeline.py; tests/test_warp_cpu.py checks it against a float64
bilinear and against Pillow's ``Image.rotate``.

    quantise(a, b, tx, c, d, ty)       -> int64 [6]: coefficients floor(v 2^24 + 0.5), offsets floor(v 2^25 + 0.5)
    source_coords(xf, out_h, out_w)    -> (SX, SY) int64 [out_h, out_w]: the source sample-centre coordinates in Q25
    warp(px, xf, out_h, out_w, fill)   -> uint8 [out_h, out_w, C], integer bilinear; fill "black" or "mirror"
    taps_inside(xf, out_h, out_w, h, w, margin) -> bool [out_h, out_w]: all four taps at least ``margin`` pixels inside the source
    flip_xf / crop_xf / rotate_xf      -> the float matrices (a, b, tx, c, d, ty) of the three perturbations, pixel-edge coordinates
    crop_box(h, w, percent, origin)    -> (y0, x0, h', w')
    rotated_rect(h, w, degrees)        -> (h', w'): the largest axis-aligned rectangle inside the rotated image, floored, at least 1
    exact_bilinear(px, a, ..., ty, out_h, out_w) -> float64, unrounded, taps clamped to the edge (compare on taps_inside pixels only)
``px`` is uint8 [h, w, C].  Pixel x covers [x, x + 1); an output pixel's centre (x + 0.5, y + 0.5) is mapped to the source point
(a X + b Y + tx, c X + d Y + ty), whose sample-centre coordinate is that minus 0.5.
"""
import math

import numpy as np


def quantise(a, b, tx, c, d, ty) -> np.ndarray:
    q = [math.floor(v * 2.0 ** 24 + 0.5) for v in (a, b)] + [math.floor(tx * 2.0 ** 25 + 0.5)] + \
        [math.floor(v * 2.0 ** 24 + 0.5) for v in (c, d)] + [math.floor(ty * 2.0 ** 25 + 0.5)]
    return np.array(q, dtype=np.int64)


def source_coords(xf, out_h: int, out_w: int):
    A, B, TX, C, D, TY = (int(v) for v in xf)
    u = (2 * np.arange(out_w, dtype=np.int64) + 1)[None, :]
    v = (2 * np.arange(out_h, dtype=np.int64) + 1)[:, None]
    return A * u + B * v + TX - (1 << 24), C * u + D * v + TY - (1 << 24)


def _mirror(i: np.ndarray, n: int) -> np.ndarray:
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def warp(px: np.ndarray, xf, out_h: int, out_w: int, fill: str = "black") -> np.ndarray:
    px = np.asarray(px)
    assert px.dtype == np.uint8 and px.ndim == 3 and fill in ("black", "mirror")
    h, w = px.shape[:2]
    SX, SY = source_coords(xf, out_h, out_w)
    ix, iy = SX >> 25, SY >> 25
    wx, wy = ((SX >> 15) & 1023)[..., None], ((SY >> 15) & 1023)[..., None]
    src = px.astype(np.int64)

    def tap(yy, xx):
        if fill == "mirror":
            return src[_mirror(yy, h), _mirror(xx, w)]
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] * ok[..., None]

    top = tap(iy, ix) * (1024 - wx) + tap(iy, ix + 1) * wx
    bot = tap(iy + 1, ix) * (1024 - wx) + tap(iy + 1, ix + 1) * wx
    out = (top * (1024 - wy) + bot * wy + (1 << 19)) >> 20
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def taps_inside(xf, out_h: int, out_w: int, h: int, w: int, margin: int = 0) -> np.ndarray:
    SX, SY = source_coords(xf, out_h, out_w)
    ix, iy = SX >> 25, SY >> 25
    return (ix >= margin) & (ix + 1 <= w - 1 - margin) & (iy >= margin) & (iy + 1 <= h - 1 - margin)


def flip_xf(h: int, w: int, axis: str):
    return (-1.0, 0.0, float(w), 0.0, 1.0, 0.0) if axis == "h" else (1.0, 0.0, 0.0, 0.0, -1.0, float(h))


def crop_box(h: int, w: int, percent: int, origin: str = "centre"):
    hh, ww = max(1, int(h * percent / 100 + 0.5)), max(1, int(w * percent / 100 + 0.5))
    return ((h - hh) // 2, (w - ww) // 2, hh, ww) if origin == "centre" else (0, 0, hh, ww)


def crop_xf(y0: int, x0: int):
    return (1.0, 0.0, float(x0), 0.0, 1.0, float(y0))


def rotate_xf(h: int, w: int, degrees: float, out_h: int = None, out_w: int = None):
    """counter-clockwise by ``degrees`` about the centre (Pillow's direction); the centre of the output maps to the centre of the source"""
    out_h, out_w = h if out_h is None else out_h, w if out_w is None else out_w
    t = math.radians(degrees)
    a, b, c, d = math.cos(t), -math.sin(t), math.sin(t), math.cos(t)
    return (a, b, w / 2 - a * out_w / 2 - b * out_h / 2, c, d, h / 2 - c * out_w / 2 - d * out_h / 2)


def rotated_rect(h: int, w: int, degrees: float):
    t = math.radians(degrees)
    s, c = abs(math.sin(t)), abs(math.cos(t))
    wide = w >= h
    long_, short = (w, h) if wide else (h, w)
    if short <= 2.0 * s * c * long_ or s == c:
        x = 0.5 * short
        wr, hr = (x / s, x / c) if wide else (x / c, x / s)
    else:
        cos2 = c * c - s * s
        wr, hr = (w * c - h * s) / cos2, (h * c - w * s) / cos2
    return max(1, int(math.floor(hr))), max(1, int(math.floor(wr)))


def exact_bilinear(px: np.ndarray, a, b, tx, c, d, ty, out_h: int, out_w: int) -> np.ndarray:
    h, w = px.shape[:2]
    X = (np.arange(out_w, dtype=np.float64) + 0.5)[None, :]
    Y = (np.arange(out_h, dtype=np.float64) + 0.5)[:, None]
    sx, sy = a * X + b * Y + tx - 0.5, c * X + d * Y + ty - 0.5
    ix, iy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = (sx - ix)[..., None], (sy - iy)[..., None]
    src = px.astype(np.float64)

    def tap(yy, xx):
        return src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]

    top = tap(iy, ix) * (1 - fx) + tap(iy, ix + 1) * fx
    bot = tap(iy + 1, ix) * (1 - fx) + tap(iy + 1, ix + 1) * fx
    return top * (1 - fy) + bot * fy
