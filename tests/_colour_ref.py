"""The arithmetic of csrc/colour.hip (``vip_colour_rgb_u8``, include/vipcup_hip.h) restated in numpy, and the named colour variants of
the stress tests built from their definitions - independent of vipcup_amd.pipeline: its own constants, its own constructors.

Per pixel (R, G, B) and output channel c, in exact integers (int64 here; the kernel's 32 bits suffice for the admitted coefficients):
    s_c = M[c][0] R + M[c][1] G + M[c][2] B + K[c] mean[c] + O[c] + 32768
    v_c = clip(s_c >> 16, 0, 255)                (``>>`` on a numpy int64 is an arithmetic shift: floor)
    out_c = lut[v_c] if a table is given
"""
import math

import numpy as np

LUMA = (19595, 38470, 7471)                                   # Pillow's ImagingConvert rgb2l: (R 19595 + G 38470 + B 7471 + 0x8000) >> 16
NTSC_YIQ = [[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]]
HUES = [-180, -90, -30, -1, 1, 30, 90, 180]
SATURATIONS = [0, 50, 150, 200]
CONTRASTS = [0, 50, 150, 200]
BRIGHTNESSES = [-50, -10, 10, 50]
GAMMAS = [0.5, 0.8, 1.25, 2.0]


def q(x):
    """floor(x * 65536 + 0.5) of a float64, element by element, as Python integers in an object-free int64 array"""
    x = np.asarray(x, np.float64)
    return np.array([math.floor(float(v) * 65536.0 + 0.5) for v in x.ravel()], np.int64).reshape(x.shape)


def int_mean(px: np.ndarray) -> np.ndarray:
    """(sum + hw // 2) // hw per channel: the rounded mean colour of an [h, w, 3] image, as ``vip_image_mean_u8`` defines it"""
    hw = px.shape[0] * px.shape[1]
    return (px.reshape(-1, 3).astype(np.int64).sum(axis=0) + hw // 2) // hw


def apply(px: np.ndarray, M, K=None, O=None, lut=None, mean=None) -> np.ndarray:
    """``px`` [h, w, 3] uint8 under the formula above; ``mean`` (3 integers) defaults to ``int_mean(px)`` and matters only when K != 0"""
    M = np.asarray(M, np.int64).reshape(3, 3)
    K = np.zeros(3, np.int64) if K is None else np.asarray(K, np.int64).reshape(3)
    O = np.zeros(3, np.int64) if O is None else np.asarray(O, np.int64).reshape(3)
    mean = int_mean(px) if mean is None else np.asarray(mean, np.int64).reshape(3)
    s = px.astype(np.int64) @ M.T + K * mean + O + 32768
    v = np.clip(s >> 16, 0, 255)
    if lut is not None:
        v = np.asarray(lut, np.int64)[v]
    return v.astype(np.uint8)


def exact(px: np.ndarray, M, K=None, O=None) -> np.ndarray:
    """the float64 formula the integers approximate: ``clip(floor(M x + K mean + O + 0.5), 0, 255)`` with real coefficients (not Q16)
    and the image's exact, unrounded mean"""
    x = px.astype(np.float64)
    y = x @ np.asarray(M, np.float64).T
    if K is not None:
        y = y + np.asarray(K, np.float64) * x.reshape(-1, 3).mean(axis=0)
    if O is not None:
        y = y + np.asarray(O, np.float64)
    return np.clip(np.floor(y + 0.5), 0, 255).astype(np.uint8)


# ---- the named variants: (M, K, O) as real numbers, and as the kernel's integers -----------------------------------------------------------
def gray_real():
    return np.tile(np.array(LUMA, np.float64) / 65536.0, (3, 1)), None, None


def hue_real(degrees):
    t = math.radians(degrees)
    rot = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(t), -math.sin(t)], [0.0, math.sin(t), math.cos(t)]])
    T = np.array(NTSC_YIQ, np.float64)
    return np.linalg.inv(T) @ rot @ T, None, None


def saturation_real(percent):
    f = percent / 100
    return f * np.eye(3) + (1 - f) * gray_real()[0], None, None


def contrast_real(percent):
    f = percent / 100
    return f * np.eye(3), np.full(3, 1 - f), None


def brightness_real(percent):
    return np.eye(3), None, np.full(3, percent / 100 * 255)


def quantise(M, K, O):
    return q(M), None if K is None else q(K), None if O is None else q(O)


def gray():
    return np.array([LUMA] * 3, np.int64), None, None, None


def bgr():
    return np.array([[0, 0, 65536], [0, 65536, 0], [65536, 0, 0]], np.int64), None, None, None


def hue(degrees):
    return quantise(*hue_real(degrees)) + (None,)


def saturation(percent):
    return quantise(*saturation_real(percent)) + (None,)


def contrast(percent):
    return quantise(*contrast_real(percent)) + (None,)


def brightness(percent):
    return quantise(*brightness_real(percent)) + (None,)


def gamma(g):
    lut = np.array([math.floor(255.0 * (v / 255.0) ** g + 0.5) for v in range(256)], np.int64)
    return np.array([[65536, 0, 0], [0, 65536, 0], [0, 0, 65536]], np.int64), None, None, lut


VARIANTS = {"gray": gray, "bgr": bgr, "hue": hue, "saturation": saturation, "contrast": contrast, "brightness": brightness, "gamma": gamma}


def variant(kind, arg=None):
    """(M, K, O, lut) of a named variant"""
    return VARIANTS[kind]() if arg is None else VARIANTS[kind](arg)
