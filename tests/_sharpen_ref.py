"""NumPy restatement of the unsharp mask of the stress tests, the suite's oracle for ``vip_sharpen_rgb_u8`` (csrc/blur.hip).  Written from
the specification (include/vipcup_hip.h) on top of tests/_blur_ref.gauss, not from the kernel.

    amount(percent)                                 -> a = round(256 percent / 100), in integers
    sharpen(px, percent, sigma, r, threshold)       -> uint8: with B = gauss(px, sigma, r) (uint8) and d = X - B,
                                                       X where |d| <= threshold, clamp(X + ((a d + 128) >> 8), 0, 255) elsewhere
    exact_sharpen(px, percent, sigma, r, threshold) -> uint8: round(X + percent / 100 * d) clamped, in float64 on the same uint8 B
``px`` is uint8 [h, w] or [h, w, C]; each channel is filtered on its own.
"""
import numpy as np

from tests import _blur_ref as B


def amount(percent: int) -> int:
    assert isinstance(percent, (int, np.integer)) and 1 <= percent <= 500
    return (256 * int(percent) + 50) // 100


def sharpen(px: np.ndarray, percent: int, sigma: float = 1.0, r: int = None, threshold: int = 0) -> np.ndarray:
    px = np.asarray(px)
    assert px.dtype == np.uint8 and 0 <= threshold <= 255
    x = px.astype(np.int64)
    d = x - B.gauss(px, sigma, r).astype(np.int64)
    out = np.clip(x + ((amount(percent) * d + 128) >> 8), 0, 255)          # numpy's >> on negative int64 is arithmetic: floor
    return np.where(np.abs(d) <= threshold, x, out).astype(np.uint8)


def exact_sharpen(px: np.ndarray, percent: int, sigma: float = 1.0, r: int = None, threshold: int = 0) -> np.ndarray:
    px = np.asarray(px)
    x = px.astype(np.float64)
    d = x - B.gauss(px, sigma, r).astype(np.float64)
    out = np.clip(np.floor(x + percent / 100.0 * d + 0.5), 0, 255)
    return np.where(np.abs(d) <= threshold, x, out).astype(np.uint8)
