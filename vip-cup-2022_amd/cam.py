"""Grad-CAM evidence maps - the counterpart of the reference's two Grad-CAM helpers (models/gcvit/utils/gradcam.py:14-65 and
keras_cv_attention_models/visualizing/visualizing.py:186-245, ``use_v2=False``).

Every map-capable member's head is ``GAP -> [LayerNorm] -> Dense -> activation``, so the gradient Grad-CAM pools has a closed form
(``ops.cam``, csrc/cam.hip) and the map comes out of the forward pass that produces the score: no backward pass through the body.
A member family describes its head with ``head_spec()``; ``CamMixin`` adds ``cam`` / ``predict_with_cam`` on top of it.

Deliberate differences from the reference: the gradient mean is taken per image (gradcam.py:51 averages over the batch axis too, which
it only ever calls with one image), an all-negative map gives zeros instead of 0 / 0 = NaN (gradcam.py:55), and ViT members - whose
head reads the class token only, so the gradient on every patch token is zero - are reported as unsupported instead of an empty map.
"""
import os
import struct
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _abi, ops


@dataclass
class HeadSpec:
    """the classifier head of a member: fp32 ``w`` ``[N, C]`` and ``b`` ``[N]``, ``ln`` = (gamma, beta, eps) of the LayerNorm between
    the pool and the Dense or None, ``act`` = the head activation as ``ops.head_prob`` takes it"""
    w: torch.Tensor
    b: Optional[torch.Tensor]
    ln: Optional[Tuple[torch.Tensor, torch.Tensor, float]] = None
    act: str = "default"


class CamMixin:
    """``cam`` / ``predict_with_cam`` for a model with ``features(x)`` -> the map its head pools and ``head_spec()``."""
    cam_supported = True

    def _head_logits(self, f):
        """the member's own head launch on an existing feature map (what ``logits`` runs after ``features``)"""
        hs = self.head_spec()
        if hs.ln is not None:
            return ops.gap_ln_dense_f32(f, hs.ln[0], hs.ln[1], hs.ln[2], hs.w, hs.b)
        return ops.gap_dense_f32(f, hs.w, hs.b)

    def cam(self, x, target="score"):
        """``(cam [B,H,W], peak [B], z [B,N])`` of ``ops.cam`` on ``features(x)``: the un-normalised Grad-CAM map of ``target``
        (``"score"``: the number the ensemble averages; an int: that class's probability)."""
        hs = self.head_spec()
        return ops.cam(self.features(x), hs.w, hs.b, ln=hs.ln, act=hs.act, target=target)

    def predict_with_cam(self, x, target="score"):
        """``(predict(x), cam, peak)`` from ONE pass through the body: the probabilities come from the member's own head launch on the
        feature map (bit-identical to ``predict``), the map from ``ops.cam`` on the same tensor."""
        hs = self.head_spec()
        f = self.features(x)
        p = ops.head_prob(self._head_logits(f), hs.act)
        m, peak, _ = ops.cam(f, hs.w, hs.b, ln=hs.ln, act=hs.act, target=target)
        return p, m, peak


VIT_REASON = ("the head reads the class token only, so the Grad-CAM gradient on every patch token is zero: a ViT member has no spatial "
              "evidence map under this definition (attention roll-out is not implemented)")


def unsupported_reason(model) -> Optional[str]:
    """None when ``model`` can produce a map, otherwise why not"""
    if getattr(model, "cam_supported", False):
        return None
    return getattr(model, "cam_unsupported_reason", "the member defines no head_spec()")


# ---- colour table ------------------------------------------------------------------------------------------------------------------
# "jet" as published (matplotlib _cm.py `_jet_data`): piecewise-linear (x, y) breakpoints per channel
_JET = {
    "red": ((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
    "green": ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
    "blue": ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0)),
}


def jet_table() -> np.ndarray:
    """uint8 ``[256, 3]``: jet sampled at i / 255 (``cmap(np.arange(256))[:, :3]``, gradcam.py:59-60), rounded to 0 .. 255"""
    xs = np.arange(256, dtype=np.float64) / 255.0
    cols = [np.interp(xs, [p[0] for p in _JET[ch]], [p[1] for p in _JET[ch]]) for ch in ("red", "green", "blue")]
    return np.round(np.stack(cols, 1) * 255.0).astype(np.uint8)


_TABLE_DEV = {}


def jet_table_device(device) -> torch.Tensor:
    key = str(torch.device(device))
    if key not in _TABLE_DEV:
        _TABLE_DEV[key] = torch.from_numpy(jet_table()).to(device).contiguous()
    return _TABLE_DEV[key]


# ---- PNG writer --------------------------------------------------------------------------------------------------------------------
def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_bytes(img: np.ndarray, level: int = 6) -> bytes:
    """uint8 ``[H, W, 3]`` (RGB) or ``[H, W]`` (gray) -> a PNG byte string: 8-bit, not interlaced, every row with filter type 0"""
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise _abi.VipError(f"png_bytes: expected uint8 [H,W,3] or [H,W] with H, W >= 1, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + w * (3 if a.ndim == 3 else 1)), dtype=np.uint8)       # column 0: the filter byte
    rows[:, 1:] = a.reshape(h, -1)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b"")


def write_png(path: str, img: np.ndarray) -> None:
    with open(path, "wb") as f:
        f.write(png_bytes(img))


def heatmap_stem(filename: str) -> str:
    """file name (relative, as the input CSV lists it) -> the stem its heat-map files carry: path separators flattened, so that the
    outputs of ``a/1.jpg`` and ``b/1.jpg`` do not collide"""
    stem = os.path.splitext(filename)[0]
    return stem.replace("\\", "/").strip("/").replace("/", "__") or "image"
