"""NumPy restatement of an antialiased 8-bit resize, the test suite's oracle for csrc/resample_host.cpp and csrc/resample.hip.  Written
from the published behaviour of Pillow's ``Image.resize`` on 8-bit images (coefficient tables in double precision, rounded to 22
fractional bits; a horizontal pass to uint8, then a vertical pass over the rounded rows; a pass whose size does not change is skipped);
tests/test_resample_cpu.py checks it pixel by pixel against Pillow itself.  The passes are integer arithmetic.

    coeffs(in_size, out_size, filter)   -> (bounds int32 [out, 2] = (xmin, count), k int32 [out, ksize], ksize)
    resize(px, out_h, out_w, filter)    -> uint8 [out_h, out_w, C]
    scaled_size(h, w, percent)          -> the size ``pipeline.rescale`` gives an image
and ``pil_resize`` (the arbiter) and ``two_level`` (0 / 255 content, for overshoot and the clamp).
"""
import math

import numpy as np

PRECISION_BITS = 22
FILTERS = ("bilinear", "bicubic", "lanczos")
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
FILTER_ID = {"bilinear": 0, "bicubic": 1, "lanczos": 2}        # VIP_RESAMPLE_* of include/vipcup_hip.h


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


_FILTER = {"bilinear": _bilinear, "bicubic": _bicubic, "lanczos": _lanczos}


def coeffs(in_size: int, out_size: int, filter: str):
    f = _FILTER[filter]
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = SUPPORT[filter] * fscale
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fscale                      # the argument is scaled by the reciprocal, as Pillow does
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ksize), np.int32)
    for x in range(out_size):
        center = (x + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), in_size) - xmin
        w = [f((j + xmin - center + 0.5) * ss) for j in range(count)]
        total = 0.0
        for v in w:                        # left to right
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        bounds[x] = (xmin, count)
        for j, v in enumerate(w):
            k[x, j] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
    return bounds, k, ksize


def _pass_axis0(px: np.ndarray, out_size: int, filter: str) -> np.ndarray:
    """resample axis 0 of uint8 ``px`` [in, ...] to ``out_size`` samples"""
    bounds, k, _ = coeffs(px.shape[0], out_size, filter)
    src = px.astype(np.int64)
    out = np.empty((out_size,) + px.shape[1:], np.uint8)
    for x in range(out_size):
        xmin, count = int(bounds[x, 0]), int(bounds[x, 1])
        kk = k[x, :count].astype(np.int64).reshape((count,) + (1,) * (px.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (src[xmin:xmin + count] * kk).sum(axis=0)
        assert np.abs(acc).max() < 2 ** 31          # the kernel's accumulator is 32 bits wide
        out[x] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(px: np.ndarray, out_h: int, out_w: int, filter: str = "bicubic") -> np.ndarray:
    px = np.asarray(px)
    assert px.dtype == np.uint8 and px.ndim == 3
    if px.shape[1] != out_w:               # horizontal first, to uint8
        px = _pass_axis0(px.transpose(1, 0, 2), out_w, filter).transpose(1, 0, 2)
    if px.shape[0] != out_h:
        px = _pass_axis0(px, out_h, filter)
    return np.ascontiguousarray(px)


def scaled_size(h: int, w: int, percent: int):
    return max(1, int(h * percent / 100 + 0.5)), max(1, int(w * percent / 100 + 0.5))


def pil_resize(px: np.ndarray, out_h: int, out_w: int, filter: str = "bicubic") -> np.ndarray:
    from PIL import Image
    method = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC, "lanczos": Image.Resampling.LANCZOS}[filter]
    return np.asarray(Image.fromarray(px).resize((out_w, out_h), method))


def two_level(seed: int, h: int, w: int) -> np.ndarray:
    return (np.random.default_rng(seed).integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)


def noise(seed: int, h: int, w: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
