"""The arithmetic of csrc/noise.hip (``vip_noise_rgb_u8``, include/vipcup_hip.h) restated in numpy - independent of vipcup_amd.pipeline:
its own Philox, its own inverse normal (a bisection on ``math.erfc``), its own amounts.

Random words: Philox4x32-10, counter (x, y, 0, 0) - the pixel in its image's own coordinates - and key (seed, key of the image); the four
output words are w0..w3.  Standard normal in Q12 from a word w, with the table T of 4097 integers:
    z(w) = T[w >> 20] + (((T[(w >> 20) + 1] - T[w >> 20]) * ((w >> 5) & 0x7FFF) + 16384) >> 15)
Modes (X the input sample, int64 here; the kernel's 32 bits suffice, ``headroom`` checks it):
    gaussian  out_c = clip(X_c + ((a z(w_c) + 2^19) >> 20), 0, 255)            a = round(256 sigma)
    mono      the same with z(w0) on all three channels
    speckle   out_c = clip(X_c + ((X_c a z(w_c) + 2^19) >> 20), 0, 255)        a = round(256 P / 100)
    impulse   w3 < thr: all three channels (w2 & 1) ? 255 : 0, else the pixel  thr = round(P / 100 * 2^32)
"""
import functools
import math
from fractions import Fraction

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
KINDS = ("gaussian", "mono", "speckle", "impulse")
MASK = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of 32-bit words -> (w0, w1, w2, w3) as uint64 arrays holding 32-bit values"""
    c = [np.asarray(v, np.uint64) & MASK for v in (c0, c1, c2, c3)]
    shape = np.broadcast(*c).shape
    c = [np.broadcast_to(v, shape).copy() for v in c]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                    # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c)


def _phi(x: float) -> float:
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def _inv_phi(p: float) -> float:
    """the x <= 0 with Phi(x) = p, 0 < p <= 1/2, by bisection"""
    lo, hi = -8.0, 0.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if _phi(mid) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def table() -> np.ndarray:
    """T[i] = round(4096 Phi^-1(i / 4096)) for 0 < i < 4096, T[0] = -16384, T[4096] = 16384; int64 [4097], read-only"""
    t = np.zeros(4097, np.int64)
    for i in range(1, 2049):
        t[i] = math.floor(4096.0 * _inv_phi(i / 4096.0) + 0.5)
        t[4096 - i] = -t[i]
    t[0], t[4096] = -16384, 16384
    t.setflags(write=False)
    return t


def z(w) -> np.ndarray:
    """the Q12 standard normal of 32-bit words, int64"""
    w = np.asarray(w, np.uint64).astype(np.int64)
    t = table()
    i = w >> 20
    return t[i] + (((t[i + 1] - t[i]) * ((w >> 5) & 0x7FFF) + 16384) >> 15)


def words(h: int, w: int, seed: int, key: int):
    """(w0, w1, w2, w3), each [h, w] uint64: the field of an h x w image"""
    y, x = np.mgrid[0:h, 0:w]
    return philox(x, y, 0, 0, seed, key)


def amount(kind: str, value) -> int:
    """the entry point's integer: a for gaussian / mono (sigma) and speckle (percent), thr for impulse (percent); exact rationals"""
    v = Fraction(str(value))
    if kind in ("gaussian", "mono"):
        assert Fraction(1, 2) <= v <= 50 and (v * 10).denominator == 1, value
        return math.floor(256 * v + Fraction(1, 2))
    if kind == "speckle":
        assert 1 <= v <= 50 and v.denominator == 1, value
        return math.floor(256 * v / 100 + Fraction(1, 2))
    assert kind == "impulse" and Fraction(1, 10) <= v <= 50 and (v * 10).denominator == 1, (kind, value)
    return math.floor(v / 100 * 2 ** 32 + Fraction(1, 2))


def apply_int(px: np.ndarray, kind: str, a: int, seed: int = 0, key: int = 0, check=None) -> np.ndarray:
    """``px`` [h, w, 3] uint8 under mode ``kind`` with the entry point's integer amount ``a``.  ``check``: a list that receives the
    largest magnitude of any intermediate sum (``headroom``)."""
    h, w = px.shape[:2]
    w0, w1, w2, w3 = words(h, w, seed, key)
    X = px.astype(np.int64)
    if kind == "impulse":
        hit = w3 < np.uint64(a)
        value = np.where((w2 & np.uint64(1)) != 0, 255, 0)
        return np.where(hit[..., None], value[..., None], X).astype(np.uint8)
    zs = np.stack([z(w0)] * 3 if kind == "mono" else [z(w0), z(w1), z(w2)], axis=2)
    prod = (X * a * zs if kind == "speckle" else a * zs) + (1 << 19)
    if check is not None:
        check.append(int(np.abs(prod).max()))
    assert kind in ("gaussian", "mono", "speckle"), kind
    return np.clip(X + (prod >> 20), 0, 255).astype(np.uint8)


def apply(px: np.ndarray, kind: str, value, seed: int = 0, key: int = 0) -> np.ndarray:
    """``px`` under ``kind`` at ``value`` in the user's units (sigma in levels; percent)"""
    return apply_int(px, kind, amount(kind, value), seed, key)


def headroom(px: np.ndarray, kind: str, a: int, seed: int = 0, key: int = 0) -> int:
    """the largest |sum| before the shift that ``apply_int`` meets on ``px``"""
    got = []
    apply_int(px, kind, a, seed, key, got)
    return got[0]
