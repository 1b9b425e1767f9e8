"""NumPy restatement of the two smoothing filters of the stress tests, the suite's oracle for csrc/blur_host.cpp and csrc/blur.hip.  Written
from the specification (include/vipcup_hip.h), not from the kernel; tests/test_blur_cpu.py checks it against scipy.ndimage.

    mirror(i, n)               -> sample index under REFLECT without repeating the edge sample (scipy's mode='mirror')
    radius(sigma)              -> max(1, ceil(3 sigma))
    weights(sigma, radius)     -> int64 [2 radius + 1]: a sampled Gaussian, 16 fractional bits, non-negative, sum 65536
    gauss(px, sigma, radius)   -> uint8, the separable integer blur: 8.8 intermediate, unsigned 32-bit vertical sum
    median(px, k)              -> uint8, the element of rank k * k // 2 of the mirrored k x k window
``px`` is uint8 [h, w] or [h, w, C]; each channel is filtered on its own.
"""
import math

import numpy as np


def mirror(i, n: int):
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)                       # non-negative
    return np.where(i >= n, p - i, i)


def radius(sigma: float) -> int:
    return max(1, int(math.ceil(3 * sigma)))


def weights(sigma: float, r: int = None) -> np.ndarray:
    r = radius(sigma) if r is None else r
    g = [math.exp(-float(j * j) / (2.0 * sigma * sigma)) for j in range(-r, r + 1)]
    total = 0.0
    for v in g:                            # left to right
        total += v
    w = np.array([math.floor(v / total * 65536 + 0.5) for v in g], dtype=np.int64)
    w[r] += 65536 - int(w.sum())
    return w


def _window(px: np.ndarray, axis: int, r: int) -> np.ndarray:
    """[2 r + 1, ...]: ``px`` shifted by -r .. r along ``axis`` with mirrored edges"""
    idx = np.arange(px.shape[axis])
    return np.stack([np.take(px, mirror(idx + j, px.shape[axis]), axis=axis) for j in range(-r, r + 1)])


def gauss(px: np.ndarray, sigma: float, r: int = None) -> np.ndarray:
    px = np.asarray(px)
    assert px.dtype == np.uint8 and px.ndim in (2, 3)
    r = radius(sigma) if r is None else r
    w = weights(sigma, r).reshape((2 * r + 1,) + (1,) * px.ndim)
    t = ((_window(px.astype(np.int64), 1, r) * w).sum(axis=0) + 128) >> 8
    assert t.max() <= 65280                                   # fits the u16 intermediate
    acc = (_window(t, 0, r) * w).sum(axis=0) + (1 << 23)
    assert acc.max() < 2 ** 32                                # the kernel's accumulator is unsigned 32 bits wide
    return np.minimum(acc >> 24, 255).astype(np.uint8)


def median(px: np.ndarray, k: int) -> np.ndarray:
    px = np.asarray(px)
    assert px.dtype == np.uint8 and px.ndim in (2, 3) and k in (3, 5)
    r = k // 2
    rows = _window(px, 0, r)                                  # [k, h, w, ...]
    win = np.concatenate([np.take(rows, mirror(np.arange(px.shape[1]) + j, px.shape[1]), axis=2) for j in range(-r, r + 1)])
    return np.ascontiguousarray(np.sort(win, axis=0)[k * k // 2])


def exact_gauss(px: np.ndarray, sigma: float, r: int = None) -> np.ndarray:
    """the float64 convolution with the normalised sampled Gaussian through scipy.ndimage.correlate1d(mode='mirror'), unrounded"""
    from scipy import ndimage
    r = radius(sigma) if r is None else r
    g = np.exp(-np.arange(-r, r + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    g /= g.sum()
    out = ndimage.correlate1d(px.astype(np.float64), g, axis=1, mode="mirror")
    return ndimage.correlate1d(out, g, axis=0, mode="mirror")


def two_level(seed: int, h: int, w: int) -> np.ndarray:
    return (np.random.default_rng(seed).integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
