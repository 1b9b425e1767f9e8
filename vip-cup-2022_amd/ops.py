"""Operator layer: torch tensors in, torch tensors out, all arithmetic in libvipcup_hip.so.

PyTorch is used for device memory and streams only.  Activations are fp16, contiguous, NHWC
(``[B,H,W,C]``) or row-major ``[rows, C]``.  Every function launches on torch's current stream.
"""
import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _abi


# ---- knobs: every VIP_* variable this module reads -------------------------------------------------------------------------------
def _env_flag(name: str, default: bool) -> bool:
    """a default-on switch is off only at "0", a default-off switch is on only at "1" """
    v = os.environ.get(name)
    return default if v is None else (v != "0" if default else v == "1")


def _env_int(name: str, default: int) -> int:
    return int(os.environ.get(name, default))


# read once, at import (tests and tools set the module attribute instead)
PRECISION = os.environ.get("VIP_PRECISION", "fast")            # "fast" | "strict" | "f32": see "precision mode" below
# STRICT GEMM arithmetic: "bf16x3" (default) = three-term bf16 splits, six bf16 MFMAs per block (vip_conv2d_nhwc_s32x); "f32" = the
# f32-input MFMA (vip_conv2d_nhwc_s32), 2.7x lower matrix rate.  Same results to f32 round-off (tests/test_gpu_strict.py runs both).
# "bf16x2" = two-term splits, three MFMAs per block (vip_conv2d_nhwc_s32x2): 2^-17 of each product dropped - NOT f32 quality, 64x finer
# than fp16 storage; the member logits stay inside the 1e-3 tolerance with less margin.
STRICT_GEMM = os.environ.get("VIP_STRICT_GEMM", "bf16x3")
_LN_GEMM = _env_flag("VIP_LN_GEMM", True)                      # ln_dense as one launch (vip_ln_gemm_bias_act_f16)
_MLP_H2_FUSED = _env_flag("VIP_MLP_H2_FUSED", True)            # packed strict: mlp as one launch (vip_mlp_fused_h2)
_SE_H2_FUSED = _env_flag("VIP_SE_H2_FUSED", True)              # packed strict: se_gate as one launch (vip_se_gate_h2)
_H2_GATED = _env_flag("VIP_H2_GATED", True)                    # packed strict: the gate folded into the GEMM's activation operand
_DW_H2_LDS = _env_int("VIP_DW_H2_LDS", 3)                      # smallest k the LDS-staged strict depthwise kernel takes (0: never)
_SE_TAIL = _env_flag("VIP_SE_TAIL", True)                      # squeeze-excite / ECA block tails (ResNet-RS, ECA-NFNet): gate from the final 1x1 layer's input, tail in its epilogue
_DW_SE_FUSED = _env_flag("VIP_DW_SE_POOL", True)               # dwconv2d_se: the depthwise kernel leaves the pool's partial sums
_GCVIT_BLOCK_FUSED = _env_flag("VIP_GCVIT_BLOCK_FUSED", True)  # gcvit_attn_block as one launch
# the 14 x 14-window form of the fused block (C = 256, 8 heads: csrc/gcvit_block14.hip) is correct and NOT faster than the four launches
# (116 us either way at B = 256: one 8-wave workgroup per CU, three barriers and a synchronous 51 KB weight stage per head) - opt-in
_GCVIT_BLOCK14 = _env_flag("VIP_GCVIT_BLOCK14", False)


# read at every call (tests and tools flip the variable between calls)
def hilo_enabled() -> bool:
    """two-term (w + w_lo) weights where ``hilo_eligible`` (VIP_HILO=0 switches them off)"""
    return _env_flag("VIP_HILO", True)


def mbconv_fused() -> bool:
    """``mbconv_expand_dw`` as one launch where the C ABI takes the shape (VIP_MBCONV_FUSED=1; measured slower, see there)"""
    return _env_flag("VIP_MBCONV_FUSED", False)


def offset_calibration() -> bool:
    """``zoo.calibrate``'s whole-model second pass (VIP_OFFSET_CALIBRATION=1): the K-doubled twins are built and kept for it"""
    return _env_flag("VIP_OFFSET_CALIBRATION", False)


ACT = {None: 0, "none": 0, "linear": 0, "relu": 1, "silu": 2, "swish": 2, "gelu": 3, "sigmoid": 4}


_PROF = None


def set_profiler(p):
    """Install (or clear with None) a per-launch profiler: an object with start(kernel, flops, bytes, tag=None) / stop(tok);
    ``tag`` describes the launch's shape (GEMM-like operators only)."""
    global _PROF
    _PROF = p


def _act(a):
    if isinstance(a, int):
        return a
    return ACT[a]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _chk16(t: torch.Tensor, name: str):
    if t.dtype != torch.float16 or not t.is_cuda or not t.is_contiguous():
        raise _abi.VipError(f"{name}: expected a contiguous CUDA float16 tensor, got {t.dtype} {t.device} "
                            f"contiguous={t.is_contiguous()}")


def _chk32(t: torch.Tensor, name: str):
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise _abi.VipError(f"{name}: expected a contiguous CUDA float32 tensor (strict path), got {t.dtype} {t.device} "
                            f"contiguous={t.is_contiguous()}")


def _is32(t: torch.Tensor, name: str) -> bool:
    """True: ``t`` is an fp32 activation (the ``_s32`` entry points); False: fp16 (fast path).  Raises otherwise."""
    if t.dtype == torch.float32:
        _chk32(t, name)
        return True
    _chk16(t, name)
    return False


# The packed STRICT storage (csrc/common.hpp, include/vipcup_hip.h "_h2"): 4 bytes per element - an fp16 (hi, lo) pair, 8 channels =
# [hi x 8][lo x 8].  Its carrier on the torch side is an int32 tensor of the LOGICAL shape ([B, H, W, C], C % 8 == 0): torch only
# allocates, reshapes and slices it (on whole 8-channel groups); no torch arithmetic ever touches the bits.
PACKED = torch.int32


def _chkp(t: torch.Tensor, name: str):
    if t.dtype != PACKED or not t.is_cuda or not t.is_contiguous() or t.shape[-1] % 8:
        raise _abi.VipError(f"{name}: expected a contiguous CUDA packed-strict (int32 carrier) tensor with C % 8 == 0, got {t.dtype} "
                            f"{t.device} {tuple(t.shape)} contiguous={t.is_contiguous()}")


def _kind(t: torch.Tensor, name: str) -> str:
    """storage of an activation tensor: "f16" (fast path), "s32" (fp32 storage) or "h2" (packed strict); raises otherwise"""
    if t.dtype == PACKED:
        _chkp(t, name)
        return "h2"
    return "s32" if _is32(t, name) else "f16"


def _chk_kind(t: torch.Tensor, kind: str, name: str):
    {"f16": _chk16, "s32": _chk32, "h2": _chkp}[kind](t, name)


_H2_STATUS: dict = {}


def h2_status(device=None) -> torch.Tensor:
    """the device word packed-strict producers raise when a value does not fit the fp16 range (VIP_H2_OVERFLOW); one per device"""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _H2_STATUS:
        _H2_STATUS[key] = torch.zeros((1,), dtype=torch.int32, device=dev)
    return _H2_STATUS[key]


def h2_check(what: str = "strict forward pass", device=None):
    """Synchronising check of the status word; raises (and clears the word) when a packed-strict producer met a value beyond the fp16
    range - the caller then reruns in ``precision("f32")`` (fp32 storage)."""
    st = h2_status(device)
    if int(st.item()) != 0:
        st.zero_()
        raise _abi.VipError(f"{what}: an activation left the fp16 range of the packed strict storage (|v| > 65504 or NaN); "
                            "use --precision f32 (fp32 storage) for this model")


def _launch(name: str, *args, status: bool = False, prof=None):
    """The one way onto the device: ``name(*args[, the h2 status word], current stream)``, its status checked under that name.
    ``prof``: a callable -> ``(kernel, flops, bytes[, tag])``, evaluated (and the launch bracketed) only while a profiler is installed."""
    fn = getattr(_abi.lib(), name)
    if status:
        args += (_p(h2_status()),)
    tok = _PROF.start(*prof()) if (_PROF is not None and prof is not None) else None
    st = fn(*args, _stream())
    if tok is not None:
        _PROF.stop(tok)
    _abi.check(st, name)


# Operators with ONE signature across storages: base name -> ({storage kind: entry-point suffix}, whether the packed entry point
# takes the status word).  Where the fp16 signature differs (scale_add_act3, radix_combine2, gap_*_f32) only the strict two are listed.
_ALL_KINDS = {"f16": "f16", "s32": "s32", "h2": "h2"}
_STRICT_KINDS = {"s32": "s32", "h2": "h2"}
_KIND_OPS = {
    "layernorm": (_ALL_KINDS, True),
    "pool2d_nhwc": (_ALL_KINDS, True),
    "global_avgpool": (_ALL_KINDS, True),
    "mul": (_ALL_KINDS, True),
    "vit_tokens": (_ALL_KINDS, True),
    "mhsa_fwd": (_ALL_KINDS, True),
    "dwconv2d_nhwc": (_ALL_KINDS, True),
    "window_attn_fwd": (_ALL_KINDS, True),
    "global_local_filter_nhwc": (_ALL_KINDS, True),
    "swin_attn_fwd": (_ALL_KINDS, True),
    "nat_attn_fwd": (_ALL_KINDS, True),
    "cam": ({"f16": "f32", "s32": "s32", "h2": "h2"}, False),
    "scale_add_act": (_STRICT_KINDS, True),
    "radix_combine": (_STRICT_KINDS, True),
    "gap_ln_dense": (_STRICT_KINDS, False),
}


def _launch_kind(base: str, kind: str, *args, prof=None):
    """``vip_<base>_<suffix of kind>`` through ``_launch``"""
    suffix, status = _KIND_OPS[base]
    _launch(f"vip_{base}_{suffix[kind]}", *args, status=status and kind == "h2", prof=prof)


def pack_h2(x: torch.Tensor) -> torch.Tensor:
    """fp32 ``[..., C]`` (C % 8 == 0) -> packed strict tensor of the same logical shape"""
    _chk32(x, "pack_h2.x")
    assert x.shape[-1] % 8 == 0, x.shape
    out = torch.empty(x.shape, dtype=PACKED, device=x.device)
    _launch("vip_pack_h2", _p(x), _p(out), x.numel(), status=True)
    return out


def unpack_h2(x: torch.Tensor) -> torch.Tensor:
    """packed strict tensor -> fp32 of the same logical shape (hi + lo)"""
    _chkp(x, "unpack_h2.x")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _launch("vip_unpack_h2", _p(x), _p(out), x.numel())
    return out


# ---- precision mode ------------------------------------------------------------------------------------------------------------
# "fast":   fp16 storage of activations and weights, fp32 accumulate (the throughput path; member logits at the fp16 storage floor).
# "strict": the mode in which BASELINE.json's |dz| <= 1e-3 holds for every member (the reference computes in fp32: main.py:107-109).
#           Since round 4: PACKED storage - every activation / weight value is an fp16 (hi, lo) pair (22 significant bits, 4 bytes),
#           contractions are three v_mfma_f32_16x16x32_f16 per fragment pair with fp32 accumulation (the fast path's own GEMM kernels
#           instantiated for this storage: csrc/conv_h2.hip), everything else fp32 arithmetic on the joined value.
# "f32":    fp32 storage, fp32 matrix arithmetic (v_mfma_f32_32x32x2_f32 or three-term bf16 splits) - round 3's strict mode, kept as
#           the reference arithmetic and as the fallback when an activation leaves the fp16 range (h2_check).
# The mode is a property of the WEIGHTS a model was constructed with (``precision(mode)`` around the constructor) and of the
# activation dtype it is fed: every operator below dispatches on ``x.dtype``.
PRECISIONS = ("fast", "strict", "f32")


class precision:
    """Context: models constructed inside carry weights for the given precision mode (see PRECISION)."""

    def __init__(self, mode: str):
        if mode not in PRECISIONS:
            raise ValueError(f"precision {mode!r}: expected one of {PRECISIONS}")
        self.mode = mode

    def __enter__(self):
        global PRECISION
        self._old, PRECISION = PRECISION, self.mode
        return self

    def __exit__(self, *exc):
        global PRECISION
        PRECISION = self._old
        return False


def to_act(t: torch.Tensor, device="cuda", dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """a host fp32 tensor -> the activation storage ``dtype`` (default: the current precision mode's) on ``device``: a cast for fp16 /
    fp32, the (hi, lo) split for the packed strict storage (last axis % 8 == 0).  For parameters that enter the graph as activations
    (ViT class token / position embeddings)."""
    dtype = dtype or act_dtype()
    if dtype == PACKED:
        return pack_h2(t.detach().to(device=device, dtype=torch.float32).contiguous())
    return t.detach().to(device=device, dtype=dtype).contiguous()


def act_dtype(mode: Optional[str] = None) -> torch.dtype:
    """storage type of activations in a precision mode"""
    return {"fast": torch.float16, "strict": PACKED, "f32": torch.float32}[mode or PRECISION]


@dataclass
class ConvWeight:
    """Device-resident conv / dense weight in the kernel's layout: ``w[Cout][kh*kw*Cin_g (padded to ldw)]``
    fp16 (filter taps outermost, channels innermost) and an fp32 bias."""
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    kh: int
    kw: int
    cin_g: int
    cout: int
    groups: int = 1
    alg_cin_g: int = 0   # un-padded input channels per group (algorithmic FLOP count)
    err: Optional[torch.Tensor] = None   # fp32 [cout, ldw]: (fp32 weight - stored fp16 weight), kept only until calibrate()
    w_lo: Optional[torch.Tensor] = None  # fp16 [cout, ldw]: fp16(W32 - w) for the two-term-weight kernel (see make_conv_weight)
    exact: Optional["ConvWeight"] = None  # calibration only (exact_weights()): [w | fp16(W32 - w)] along K, the uncorrected bias
    w_bf3: Optional[torch.Tensor] = None  # f32 mode: the fp32 weights as three bf16 planes [3, cout, ldwp] (w = p0 + p1 + p2 exactly)
    h2_scale: float = 0.0                 # packed strict mode (> 0): ``w`` holds fp16 (hi, lo) pairs of W * h2_scale, ``bias`` = b * h2_scale
    fold: Optional[tuple] = None          # se_fold(): (what it was made from, the squeeze-excite reduce layer folded with this layer)

    @property
    def cin(self):
        return self.cin_g * self.groups

    @property
    def strict(self):
        """fp32 weights (constructed under ``precision("f32")``)"""
        return self.w.dtype == torch.float32

    @property
    def kind(self):
        """the activation storage this weight was built for: "f16" | "s32" | "h2" """
        return "h2" if self.h2_scale > 0 else ("s32" if self.strict else "f16")

    @property
    def ldw(self):
        return self.w.shape[1]


KEEP_ROUNDING_ERROR = False   # set while a model is constructed for bias calibration: ConvWeight.err is populated
_CALIB = False                # inside calibration(): conv/dense fold  (W32 - W16) . E[x]  into their bias, once
_UNFUSED = False              # inside calibration() / unfused() / exact_weights(): every Dense / conv is its own launch
_EXACT = False                # inside exact_weights(): layers run with ConvWeight.exact (two-term weights, K doubled)
_EXACT_REG: list = []         # the ConvWeights that currently hold an .exact twin (dropped by drop_exact_weights())


class calibration:
    """Context for ONE forward pass over a small representative batch that removes the image-independent part of the
    fp16 weight-rounding error.  A layer computes W16 x instead of W32 x; the difference (W32 - W16) x has a data
    mean (W32 - W16) E[x] that no rounding scheme can cancel when E[x_k] varies along K (LayerNorm beta/gamma, GELU /
    swish outputs) - on GCViT-Tiny it is a constant +0.027 on the logit, 10x the image-dependent part.  Inside this
    context every conv / dense measures its input's per-channel mean on the GPU, adds (W32 - W16) . mean to its fp32
    bias and drops the error matrix; fused paths (MLP, SE gate) run unfused so that their inner layers are seen.
    Standard post-training-quantisation bias correction; it needs inputs, not labels."""

    def __enter__(self):
        global _CALIB, _UNFUSED
        self._old = (_CALIB, _UNFUSED)
        _CALIB = _UNFUSED = True
        return self

    def __exit__(self, *exc):
        global _CALIB, _UNFUSED
        _CALIB, _UNFUSED = self._old
        if not offset_calibration():
            drop_exact_weights()           # nothing will read the twins: do not let a caller without zoo.calibrate() leak them
        return False


class unfused:
    """Context: the launch structure of calibration() (MLP and squeeze-excite chains as separate Dense launches, gates multiplied
    in before the convolution) without touching any bias - the fp16-weight leg of the whole-model offset (zoo.calibrate)."""

    def __enter__(self):
        global _UNFUSED
        self._old = _UNFUSED
        _UNFUSED = True
        return self

    def __exit__(self, *exc):
        global _UNFUSED
        _UNFUSED = self._old
        return False


class exact_weights:
    """Context: the same launches as unfused(), every layer that went through calibration() with ~22-bit weights: its ``exact`` twin
    holds ``[w | fp16(W32 - w)]`` per filter tap and group along K, the input channels are fed twice, and the SAME kernels accumulate
    both terms in fp32 and round the output where the fp16-weight layer rounds it.  Twice the K, so calibration only: the difference
    of the two legs' mean logits is what the layer-wise bias correction leaves of the weight rounding (second-order through the
    nonlinearities, border taps), an offset shared by all images, and goes into the head bias."""

    def __enter__(self):
        global _UNFUSED, _EXACT
        self._old = (_UNFUSED, _EXACT)
        _UNFUSED = _EXACT = True
        return self

    def __exit__(self, *exc):
        global _UNFUSED, _EXACT
        _UNFUSED, _EXACT = self._old
        return False


def drop_exact_weights():
    """free the calibration-only twins"""
    for cw in _EXACT_REG:
        cw.exact = None
    _EXACT_REG.clear()


def _exact_operands(x: torch.Tensor, cw: "ConvWeight", cin_off: int = 0):
    """(x with every group's channels repeated, the K-doubled twin, cin_off = 0)"""
    xs = x[..., cin_off:cin_off + cw.cin]
    lead = xs.shape[:-1]
    xg = xs.reshape(*lead, cw.groups, cw.cin_g)
    return torch.cat([xg, xg], -1).reshape(*lead, 2 * cw.cin).contiguous(), cw.exact, 0


def _bias_correct(cw: "ConvWeight", x_eff: torch.Tensor):
    """x_eff [..., cin] (already sliced / gated): fold (W32 - W16) . E[x] into cw.bias; E over all leading axes."""
    mu = x_eff.reshape(-1, x_eff.shape[-1]).float().mean(0)                       # [cin]
    k = cw.kh * cw.kw * cw.cin_g
    cog = cw.cout // cw.groups
    taps = cw.kh * cw.kw
    if offset_calibration():       # the K-doubled twin is only read by zoo.calibrate's opt-in second pass
        w2 = torch.cat([cw.w[:, :k].reshape(cw.cout, taps, cw.cin_g), cw.err[:, :k].to(torch.float16).reshape(cw.cout, taps, cw.cin_g)], 2)
        w2 = w2.reshape(cw.cout, 2 * k)
        if (2 * k) % 8:
            w2 = torch.cat([w2, w2.new_zeros(cw.cout, 8 - (2 * k) % 8)], 1)
        cw.exact = ConvWeight(w=w2.contiguous(), bias=cw.bias, kh=cw.kh, kw=cw.kw, cin_g=2 * cw.cin_g, cout=cw.cout, groups=cw.groups,
                              alg_cin_g=cw.alg_cin_g)
        _EXACT_REG.append(cw)
    e = cw.err[:, :k].reshape(cw.groups, cog, cw.kh * cw.kw, cw.cin_g)
    corr = (e * mu.reshape(cw.groups, 1, 1, cw.cin_g)).sum((2, 3)).reshape(cw.cout)
    cw.bias = corr if cw.bias is None else (cw.bias + corr)
    cw.bias = cw.bias.contiguous()
    cw.err = None


def diffuse_round_f16(w_rows: torch.Tensor) -> torch.Tensor:
    """fp32 ``[rows, K]`` -> fp16 with ERROR-DIFFUSION rounding along K: q_k = rn16(w_k + e), e = (w_k + e) - q_k.
    Every stored value is one of the two fp16 neighbours of the fp32 weight, and the running sum of the rounding
    errors along a row stays below half an ulp — so the error of a dot product with a non-zero-mean input
    (post-ReLU / swish activations) no longer grows like sqrt(K) half-ulps.  With round-to-nearest that term is a
    fixed, image-independent offset of the logit (measured: 1.2e-2 on ResNet-RS-50, 4.6e-2 on EfficientNetV1-B4);
    with diffusion it drops by ~10x at zero run-time cost."""
    wt = w_rows.detach().to(torch.float32).t().contiguous()            # [K, rows]: row access per step
    q = torch.empty_like(wt, dtype=torch.float16)
    e = torch.zeros(wt.shape[1], dtype=torch.float32)
    for k in range(wt.shape[0]):
        t = wt[k] + e
        qk = t.to(torch.float16)
        q[k] = qk
        e = t - qk.to(torch.float32)
    return q.t().contiguous()


def split_bf16x3(w_rows: torch.Tensor) -> torch.Tensor:
    """fp32 ``[rows, K]`` -> bf16 ``[3, rows, ldwp]`` (ldwp = K rounded up to 8, zero padded) with ``p0 + p1 + p2 == w`` exactly:
    each plane takes the next 8 significant bits (round-to-nearest of the remainder; both subtractions are exact in fp32).  The weight
    operand of vip_conv2d_nhwc_s32x."""
    w = w_rows.detach().to(torch.float32)
    p0 = w.to(torch.bfloat16)
    r1 = w - p0.to(torch.float32)
    p1 = r1.to(torch.bfloat16)
    r2 = r1 - p1.to(torch.float32)
    p2 = r2.to(torch.bfloat16)
    planes = torch.stack([p0, p1, p2], 0)
    pad = (-w.shape[1]) % 8
    if pad:
        planes = torch.cat([planes, planes.new_zeros(3, w.shape[0], pad)], 2)
    return planes.contiguous()


def split_h2_weights(w_rows: torch.Tensor):
    """fp32 ``[rows, K]`` (K % 8 == 0) -> (fp16 ``[rows, 2 K]``, scale): per 8 consecutive k the 16 halfs ``[hi x 8][lo x 8]`` of
    ``W * scale``, hi = rn16(W scale), lo = rn16(W scale - hi) - the weight operand of vip_conv2d_nhwc_h2.  ``scale`` is the power of
    two that puts the layer's largest |W| in [4096, 8192): every lo term of a weight within 2^-15 of that maximum is then an fp16
    NORMAL (22 significant bits for hi + lo), nothing overflows, and the kernel undoes it exactly on the fp32 accumulators."""
    w = w_rows.detach().to(torch.float32)
    rows, K = w.shape
    assert K % 8 == 0, K
    mx = float(w.abs().max()) if w.numel() else 0.0
    scale = 1.0
    if mx > 0.0 and mx == mx and mx != float("inf"):
        scale = 2.0 ** math.floor(math.log2(8191.0 / mx))
    ws = w * scale
    hi = ws.to(torch.float16)
    lo = (ws - hi.to(torch.float32)).to(torch.float16)
    packed = torch.stack([hi.reshape(rows, K // 8, 8), lo.reshape(rows, K // 8, 8)], 2).reshape(rows, 2 * K)
    return packed.contiguous(), float(scale)


HILO_MAX_K = 256     # vip_conv2d_hilo_nhwc_f16: the streaming kernel's K limit


def hilo_eligible(kh: int, kw: int, cin: int, groups: int = 1) -> bool:
    """Can a layer carry two-term weights (w + w_lo)?  1x1, ungrouped, K <= 256 (VIP_HILO=0 switches them off)."""
    return kh == 1 and kw == 1 and groups == 1 and cin <= HILO_MAX_K and hilo_enabled()


def make_conv_weight(kernel_hwio: torch.Tensor, bias: Optional[torch.Tensor], groups: int = 1,
                     device="cuda", pad_cin_to: Optional[int] = None,
                     pad_cout_to: Optional[int] = None, hilo: bool = False) -> ConvWeight:
    """Keras HWIO kernel ``[kh,kw,Cin_g,Cout]`` (fp32, BN already folded) -> ConvWeight.
    (OIHW->HWIO is the reference's own convention, tfimm/utils/timm.py:164-170.)
    Optionally zero-pads Cin (e.g. RGB 3 -> 8) and Cout (e.g. a 1-class head -> 8).
    ``hilo``: also keep ``w_lo = fp16(W32 - fp16(W32))``; ``conv2d`` then runs the layer with both terms (~22-bit
    weights) - for the HBM-bound short-K 1x1 layers whose weight rounding dominates a member's logit error
    (EfficientNet expand convolutions); only where ``hilo_eligible`` holds, and the layer must not be gated."""
    kh, kw, cin_g, cout = kernel_hwio.shape
    alg_cin_g = cin_g
    k = kernel_hwio.detach().to(torch.float32)
    if pad_cin_to is not None and pad_cin_to > cin_g:
        assert groups == 1
        k = torch.cat([k, k.new_zeros(kh, kw, pad_cin_to - cin_g, cout)], dim=2)
        cin_g = pad_cin_to
    b = None if bias is None else bias.detach().to(torch.float32)
    if pad_cout_to is not None and pad_cout_to > cout:
        assert groups == 1
        k = torch.cat([k, k.new_zeros(kh, kw, cin_g, pad_cout_to - cout)], dim=3)
        if b is not None:
            b = torch.cat([b, b.new_zeros(pad_cout_to - cout)])
        cout = pad_cout_to
    if PRECISION == "strict":          # packed (hi, lo) fp16 pairs of W * 2^s: nothing to calibrate
        if cin_g % 8 or (cout // groups) % 8:
            raise _abi.VipError(f"make_conv_weight(strict): Cin_g={cin_g} / Cout_g={cout // groups} must be multiples of 8 "
                                "(pad_cin_to / pad_cout_to)")
        w32 = k.permute(3, 0, 1, 2).reshape(cout, kh * kw * cin_g).contiguous()
        wp, scale = split_h2_weights(w32)
        return ConvWeight(w=wp.to(device), bias=None if b is None else (b * scale).to(device).contiguous(), kh=kh, kw=kw, cin_g=cin_g,
                          cout=cout, groups=groups, alg_cin_g=alg_cin_g, h2_scale=scale)
    if PRECISION == "f32":             # fp32 weights as they are: nothing to round, nothing to calibrate
        if cin_g % 4 or (cout // groups) % 4:
            raise _abi.VipError(f"make_conv_weight(f32): Cin_g={cin_g} / Cout_g={cout // groups} must be multiples of 4 "
                                "(pad_cin_to / pad_cout_to)")
        w32 = k.permute(3, 0, 1, 2).reshape(cout, kh * kw * cin_g).contiguous()
        return ConvWeight(w=w32.to(device), bias=None if b is None else b.to(device).contiguous(), kh=kh, kw=kw, cin_g=cin_g,
                          cout=cout, groups=groups, alg_cin_g=alg_cin_g, w_bf3=split_bf16x3(w32).to(device))
    # round along (channel, tap): the taps of one input channel see the same mean activation, so their rounding
    # errors are diffused into each other first; the carry then runs on across channels
    hilo = hilo and hilo_eligible(kh, kw, cin_g * groups, groups)
    if hilo:    # plain round-to-nearest high part; the low part carries what it misses
        w = k.permute(3, 0, 1, 2).reshape(cout, kh * kw * cin_g).to(torch.float16)
    else:
        w = diffuse_round_f16(k.permute(3, 2, 0, 1).reshape(cout, cin_g * kh * kw))
        w = w.reshape(cout, cin_g, kh, kw).permute(0, 2, 3, 1).reshape(cout, kh * kw * cin_g)
    ktot = w.shape[1]
    ldw = (ktot + 7) // 8 * 8
    if ldw != ktot:
        w = torch.cat([w, w.new_zeros(cout, ldw - ktot)], dim=1)
    err, w_lo = None, None
    if KEEP_ROUNDING_ERROR or hilo:
        w32 = k.permute(3, 0, 1, 2).reshape(cout, kh * kw * cin_g)
        if ldw != ktot:
            w32 = torch.cat([w32, w32.new_zeros(cout, ldw - ktot)], dim=1)
        resid = w32 - w.to(torch.float32)
        if hilo:                                   # nothing left for the bias calibration to correct
            w_lo = resid.to(torch.float16).to(device).contiguous()
        else:
            err = resid.to(device).contiguous()
    return ConvWeight(w=w.to(device=device, dtype=torch.float16).contiguous(),
                      bias=None if b is None else b.to(device).contiguous(),
                      kh=kh, kw=kw, cin_g=cin_g, cout=cout, groups=groups, alg_cin_g=alg_cin_g, err=err, w_lo=w_lo)


def make_dense_weight(kernel_io: torch.Tensor, bias: Optional[torch.Tensor], device="cuda",
                      pad_cout_to: Optional[int] = None) -> ConvWeight:
    """Keras Dense kernel ``[in, out]`` -> ConvWeight (1x1)."""
    return make_conv_weight(kernel_io.reshape(1, 1, *kernel_io.shape), bias, 1, device, None, pad_cout_to)


def _conv_dry_run(query, d: "_abi.ConvDesc", *flags) -> Optional[str]:
    buf = C.create_string_buffer(64)
    return buf.value.decode() if query(C.byref(d), *map(int, flags), buf, 64) == 0 else None


def conv_kernel_name(d: "_abi.ConvDesc", has_residual: bool, has_gate: bool = False, has_w_lo: bool = False) -> Optional[str]:
    """The kernel vip_conv2d_nhwc_f16 (/ _gated_ / _hilo_) launches for this descriptor - asked of the C dispatcher
    itself (a dry run of the selection, vip_conv2d_kernel_name); None when the combination is not supported."""
    return _conv_dry_run(_abi.lib().vip_conv2d_kernel_name, d, has_residual, has_gate, has_w_lo)


def conv_kernel_name_h2(d: "_abi.ConvDesc", has_residual: bool) -> Optional[str]:
    """the kernel vip_conv2d_nhwc_h2 launches for this descriptor (a dry run of the C dispatcher)"""
    return _conv_dry_run(_abi.lib().vip_conv2d_kernel_name_h2, d, has_residual)


def conv_kernel_variant(d: "_abi.ConvDesc", has_residual: bool, has_gate: bool = False, has_w_lo: bool = False) -> Optional[str]:
    """The same dry run down to the instantiation and its tile grid ("pwk_gemm<2,2> 65 x 4", "pwk_direct<2,gated> PT=4", "im2col<2>":
    vip_conv2d_kernel_variant); None when the combination is not supported."""
    return _conv_dry_run(_abi.lib().vip_conv2d_kernel_variant, d, has_residual, has_gate, has_w_lo)


def conv_kernel_variant_h2(d: "_abi.ConvDesc", has_residual: bool) -> Optional[str]:
    """the instantiation vip_conv2d_nhwc_h2 launches for this descriptor (vip_conv2d_kernel_variant_h2)"""
    return _conv_dry_run(_abi.lib().vip_conv2d_kernel_variant_h2, d, has_residual)


# Dry runs of the persistent launches (nothing is launched; each launcher calls the function its query calls).  A plan is
# ``(units, workgroups, ...)``: a workgroup walks ceil(units / workgroups) units at the most - its "passes".  None: shape not taken.
def mlp_plan(M: int, C_: int, hidden: int, packed: bool = False, act="gelu"):
    """``(tiles, workgroups, tokens per tile)`` of the fused MLP launch ``mlp`` makes for [M, C_] rows (``packed``: the strict storage).
    Asks the current device for its CU count."""
    wg, rows = C.c_int(0), C.c_int(0)
    fn = _abi.lib().vip_mlp_fused_plan_h2 if packed else _abi.lib().vip_mlp_fused_plan
    n = fn(M, C_, hidden, _act(act), C.byref(wg), C.byref(rows))
    return (n, wg.value, rows.value) if n > 0 else None


def dwconv_tile_plan(B: int, H: int, W: int, Cc: int, k: int, pad=None, pooled: bool = False, packed: bool = False):
    """``(tile groups, workgroups per channel block, {cb, tiles_per_block, channel_blocks, cap})`` of the fp16 stride-1 depthwise
    launch (``pooled``: the pooling form ``dwconv2d_se`` uses; ``packed``: the tile kernel of the strict storage, ``cb`` in 4-channel
    chunks - what ``dwconv2d`` launches where the LDS-staged kernel does not take the call).  Host arithmetic only: works without a GPU."""
    pad = (k // 2,) * 4 if pad is None else pad
    Ho, Wo = _out_hw(H, W, k, k, 1, 1, pad)
    wg, geom = C.c_int(0), (C.c_int * 4)()
    if packed:
        n = 0 if pooled else _abi.lib().vip_dwconv2d_tile_plan_h2(B, H, W, Cc, k, 1, pad[0], pad[2], Ho, Wo, C.byref(wg), geom)
    else:
        n = _abi.lib().vip_dwconv2d_tile_plan(B, H, W, Cc, k, 1, Ho, Wo, int(pooled), C.byref(wg), geom)
    return (n, wg.value, dict(zip(("cb", "tiles_per_block", "channel_blocks", "cap"), geom))) if n > 0 else None


def dwconv_lds_plan(B: int, H: int, W: int, Cc: int, k: int, pad=None):
    """``(items, workgroups, {img, lty, ltx, rgy, rgx, channel_blocks})`` of the LDS-staged packed depthwise launch (plain and pooling
    form share it).  Asks the current device for its CU count."""
    pad = (k // 2,) * 4 if pad is None else pad
    Ho, Wo = _out_hw(H, W, k, k, 1, 1, pad)
    wg, geom = C.c_int(0), (C.c_int * 6)()
    n = _abi.lib().vip_dwconv2d_s1_plan_h2(B, H, W, Cc, k, Ho, Wo, C.byref(wg), geom)
    return (n, wg.value, dict(zip(("img", "lty", "ltx", "rgy", "rgx", "channel_blocks"), geom))) if n > 0 else None


# ---- named terms of the fusion decisions below -------------------------------------------------------------------------------------
SE_FUSED_MAX_WEIGHTS = 256 * 1024      # the one-launch gate kernels re-read both matrices per image: beyond this the batched GEMMs win


def _pointwise(cw: ConvWeight) -> bool:
    """1x1 and ungrouped: a plain GEMM over the channel axis"""
    return cw.kh == cw.kw == 1 and cw.groups == 1


def _se_chain_ok(fc1: ConvWeight, fc2: ConvWeight, C_: int) -> bool:
    """fc1 -> fc2 is a squeeze-excite chain on ``C_`` channels that the one-launch gate kernels take"""
    return (_pointwise(fc1) and _pointwise(fc2) and fc1.cin == C_ and fc2.cin == fc1.cout
            and C_ * fc1.cout + fc1.cout * fc2.cout <= SE_FUSED_MAX_WEIGHTS)


def _epilogue_ok(act, act_post, residual) -> bool:
    """what the fused-prologue GEMMs (LayerNorm / gate in the activation load) carry: (activation) or (residual [+ ReLU])"""
    if residual is None:
        return act_post is None
    return act is None and act_post in (None, "relu")


def _dw_filter_ok(w_khwc: torch.Tensor, k: int, C_: int) -> bool:
    return w_khwc.dtype == torch.float32 and w_khwc.is_contiguous() and w_khwc.shape == (k, k, C_)


def _ln_args(ln):
    """``ln = (gamma, beta, eps)`` or None -> the three arguments of a C entry point with an optional LayerNorm prologue"""
    return (ln[0], ln[1], float(ln[2])) if ln is not None else (None, None, 0.0)


def _out_hw(H: int, W: int, kh: int, kw: int, sh: int, sw: int, pad):
    pt, pb, pl, pr = pad
    return (H + pt + pb - kh) // sh + 1, (W + pl + pr - kw) // sw + 1


# ---- convolution / dense ------------------------------------------------------------------------------------------------------------
def _conv_front(kind: str, x, cw: ConvWeight, stride, pad, act, act_post, residual, out, cin_off, cout_off):
    """What the three storages share: operand checks, output size, ``out`` allocated in the storage of ``x`` -> ``(out, ConvDesc)``"""
    B, H, W, ldx = x.shape
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    Ho, Wo = _out_hw(H, W, cw.kh, cw.kw, sh, sw, pad)
    if out is None:
        out = torch.empty((B, Ho, Wo, cw.cout), dtype=x.dtype, device=x.device)
    else:
        _chk_kind(out, kind, "conv2d.out")
        assert out.shape[:3] == (B, Ho, Wo), (out.shape, (B, Ho, Wo))
    if residual is not None:
        _chk_kind(residual, kind, "conv2d.residual")
        assert residual.shape[:3] == (B, Ho, Wo) and residual.shape[3] >= cw.cout
    return out, _abi.ConvDesc(B=B, H=H, W=W, Cin=cw.cin, Cout=cw.cout, kh=cw.kh, kw=cw.kw, sh=sh, sw=sw, pt=pad[0], pl=pad[2], Ho=Ho, Wo=Wo,
                              groups=cw.groups, ldx=ldx, cin_off=cin_off, ldy=out.shape[3], cout_off=cout_off,
                              ldr=0 if residual is None else residual.shape[3], res_off=0, ldw=cw.ldw, act_pre=_act(act),
                              act_post=_act(act_post))


def _conv_prof(kernel: str, d, cw: ConvWeight, residual, act_bytes: float, w_bytes: float, tag: str = ""):
    """profiler entry of a convolution launch: algorithmic FLOPs, bytes at ``act_bytes`` per activation / ``w_bytes`` per weight element"""
    M = d.B * d.Ho * d.Wo
    return (kernel, 2.0 * M * cw.cout * (cw.kh * cw.kw * cw.alg_cin_g),
            act_bytes * (d.B * d.H * d.W * cw.cin + M * cw.cout * (2 if residual is not None else 1)) + w_bytes * cw.w.numel(),
            f"M={M} N={cw.cout} K={cw.kh * cw.kw * cw.cin_g} k{cw.kh} s{d.sh} g{cw.groups}{tag}")


def conv2d(x: torch.Tensor, cw: ConvWeight, stride=1, pad=(0, 0, 0, 0), act=None, act_post=None,
           residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
           cin_off: int = 0, cout_off: int = 0, gate: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = act_post(act(conv(x * gate) + bias) + residual).  ``pad`` = (top, bottom, left, right) zero padding.
    ``gate`` [B, 2, Cin] fp16 (a split squeeze-excite scale from ``se_gate``) is folded into the activation load of
    pointwise convolutions; where the C ABI does not take it, x * gate is materialised first - the same fp16 values
    either way.
    ``x`` may carry more channels than the weight consumes (``cin_off`` selects the slice); ``out`` may
    be a wider tensor written at ``cout_off`` (concat-free channel splits / joins)."""
    kind = _kind(x, "conv2d.x")
    if kind != cw.kind:
        raise _abi.VipError(f"conv2d: {kind} activations with {cw.kind} weights - build the model and its input in the same precision")
    if kind != "f16":
        return _CONV_STRICT[kind](x, cw, stride, pad, act, act_post, residual, out, cin_off, cout_off, gate)
    if gate is not None and _UNFUSED:
        assert gate.shape == (x.shape[0], 2, cw.cin) and x.shape[3] == cw.cin and cin_off == 0
        x, gate = scale_add_act(x, gate, None, None), None
    if _CALIB and cw.err is not None:
        _bias_correct(cw, x[..., cin_off:cin_off + cw.cin])
    if _EXACT and cw.exact is not None:
        x, cw, cin_off = _exact_operands(x, cw, cin_off)
    out, d = _conv_front("f16", x, cw, stride, pad, act, act_post, residual, out, cin_off, cout_off)
    if gate is not None:
        _chk16(gate, "conv2d.gate")
        assert gate.shape == (d.B, 2, cw.cin) and d.ldx == cw.cin and cin_off == 0
        if conv_kernel_name(d, residual is not None, has_gate=True) is None:
            x, gate = scale_add_act(x, gate, None, None), None
    has_gate, has_lo = gate is not None, cw.w_lo is not None

    def prof():
        return _conv_prof(conv_kernel_name(d, residual is not None, has_gate, has_lo) or "unsupported", d, cw, residual, 2.0, 2.0,
                          f"{' gate' if has_gate else ''}{' res' if residual is not None else ''} act={act}")
    tail = (_p(cw.bias), _p(residual), _p(out), C.byref(d))
    if has_lo:
        if has_gate:
            raise _abi.VipError("conv2d: a two-term-weight layer cannot take a gate")
        _launch("vip_conv2d_hilo_nhwc_f16", _p(x), _p(cw.w), _p(cw.w_lo), *tail, prof=prof)
    elif has_gate:
        _launch("vip_conv2d_gated_nhwc_f16", _p(x), _p(gate), _p(cw.w), *tail, prof=prof)
    else:
        _launch("vip_conv2d_nhwc_f16", _p(x), _p(cw.w), *tail, prof=prof)
    return out


def se_tail_folded(c3: ConvWeight, se_r: ConvWeight, se_e: ConvWeight) -> bool:
    """Whether a squeeze-excite block tail ``scale_add_act(y, se_gate(y), shortcut)``, ``y = conv2d(z, c3)``, runs in its folded form:
    gate from ``z`` with ``se_fold(c3, se_r)``, then ``conv2d_out_gated``.  The fp16 storage only, and never inside ``calibration()`` /
    ``unfused()`` / ``exact_weights()``: there every layer is its own launch and sees its own input."""
    return bool(_SE_TAIL and not (_UNFUSED or _CALIB or _EXACT) and c3.kind == se_r.kind == se_e.kind == "f16" and _pointwise(c3)
                and _pointwise(se_r) and _pointwise(se_e) and se_r.cin == c3.cout and se_e.cin == se_r.cout and se_e.cout == c3.cout)


def eca_tail_folded(d4: ConvWeight, eca: ConvWeight) -> bool:
    """Whether an ECA-NFNet block tail ``scale_add_act(d, gate(d), shortcut, act2=)``, ``d = conv2d(z, d4)``, runs in its folded form: the
    one-layer gate from the pooled ``z`` through ``se_fold(d4, eca)``, then ``conv2d_out_gated(..., act2=)``.  The exclusions of
    ``se_tail_folded``: the fp16 storage only, never inside ``calibration()`` / ``unfused()`` / ``exact_weights()``."""
    return bool(_SE_TAIL and not (_UNFUSED or _CALIB or _EXACT) and d4.kind == eca.kind == "f16" and _pointwise(d4) and _pointwise(eca)
                and eca.cin == d4.cout and eca.cout == d4.cout)


def _fold_tag(c3: ConvWeight, se_r: ConvWeight) -> list:
    """what a fold was made from: the reduce layer and the two bias tensors with their write counters (the weights never change)"""
    return [se_r] + [v for b in (c3.bias, se_r.bias) for v in (b, None if b is None else b._version)]


def se_fold(c3: ConvWeight, se_r: ConvWeight) -> ConvWeight:
    """The reduce layer of a squeeze-excite block folded with the linear 1x1 layer ``c3`` in front of the pool:
    ``Wr . mean_hw(W3 z + b3) + br = (Wr W3) . mean_hw(z) + (Wr b3 + br)`` -> the ConvWeight ``[r, f]`` that ``se_gate`` applies to the
    pooled INPUT of ``c3`` (a quarter of the channels of its output, and a matrix four times smaller).  Folded in fp64 from the tensors
    the layers multiply by - ``c3.w`` plus its second term ``w_lo`` where it has one, the fp32 biases as they are NOW.  The product's
    elements are not fp16 values and one rounding of them would be the gate's largest error (4e-5 where ``se_gate`` itself is held to
    2e-5), so the fold carries TWO terms, ``w = fp16(W)`` and ``w_lo = fp16(W - w)``, which ``se_gate`` joins in fp32.  Built on first
    use and kept on ``c3``; built again when a bias tensor was replaced or written to (bias calibration does the former)."""
    tag = _fold_tag(c3, se_r)
    f = c3.fold
    if f is not None and all(a is b or (type(a) is int and type(b) is int and a == b) for a, b in zip(f[0], tag)):
        return f[1]
    k, c = c3.cin, c3.cout
    w3 = c3.w[:, :k].detach().cpu().double()
    if c3.w_lo is not None:
        w3 = w3 + c3.w_lo[:, :k].detach().cpu().double()
    wr = se_r.w[:, :c].detach().cpu().double()
    wf = (wr @ w3).float()                                                    # [r, f]
    bf = torch.zeros(se_r.cout, dtype=torch.float64)
    if c3.bias is not None:
        bf = bf + wr @ c3.bias.detach().cpu().double()
    if se_r.bias is not None:
        bf = bf + se_r.bias.detach().cpu().double()
    dev = c3.w.device
    hi = wf.to(torch.float16)
    folded = ConvWeight(w=hi.to(dev).contiguous(), bias=bf.float().to(dev).contiguous(), kh=1, kw=1, cin_g=k, cout=se_r.cout, groups=1,
                        alg_cin_g=k, w_lo=(wf - hi.float()).to(torch.float16).to(dev).contiguous())
    c3.fold = (tag, folded)
    return folded


def out_gate_variant(d: "_abi.ConvDesc", has_w_lo: bool = False) -> Optional[str]:
    """The instantiation vip_conv2d_out_gated_nhwc_f16 launches for this descriptor ("pw_gemm<KS=2,hilo> 1 x 256 ogate": a dry run of
    the C dispatcher, vip_conv2d_out_gated_variant) - the one the same call with a residual selects; None where it is not taken."""
    return _conv_dry_run(_abi.lib().vip_conv2d_out_gated_variant, d, has_w_lo)


def out_gate2_variant(d: "_abi.ConvDesc", has_w_lo: bool = False, act2="silu") -> Optional[str]:
    """The instantiation of the two-output form (vip_conv2d_out_gated2_nhwc_f16, "pwk_direct<2> PT=4 ogate y2": the dry run
    vip_conv2d_out_gated2_variant) - the one-output call's selection; None where it is not taken (any ``act2`` but SiLU included)."""
    return _conv_dry_run(_abi.lib().vip_conv2d_out_gated2_variant, d, has_w_lo, _act(act2))


def _out_gate_desc(x, cw: ConvWeight, gate, residual, act_post):
    """the descriptor of the one-launch form of ``conv2d_out_gated``, or None where the call takes the two launches"""
    if not (_SE_TAIL and not (_UNFUSED or _CALIB or _EXACT) and x.dtype == torch.float16 and x.is_cuda and x.dim() == 4 and x.is_contiguous()
            and cw.kind == "f16" and _pointwise(cw) and x.shape[3] == cw.cin and residual is not None and residual.dtype == torch.float16
            and residual.is_contiguous() and residual.shape == (*x.shape[:3], cw.cout) and gate.dtype == torch.float16
            and gate.is_contiguous() and gate.shape == (x.shape[0], 2, cw.cout) and act_post in (None, "none", "linear", "relu")):
        return None
    B, H, W, ldx = x.shape
    d = _abi.ConvDesc(B=B, H=H, W=W, Cin=cw.cin, Cout=cw.cout, kh=1, kw=1, sh=1, sw=1, pt=0, pl=0, Ho=H, Wo=W, groups=1, ldx=ldx, cin_off=0,
                      ldy=cw.cout, cout_off=0, ldr=cw.cout, res_off=0, ldw=cw.ldw, act_pre=0, act_post=_act(act_post))
    return d if out_gate_variant(d, cw.w_lo is not None) is not None else None


def conv2d_out_gated(x: torch.Tensor, cw: ConvWeight, gate: torch.Tensor, residual: torch.Tensor, act_post=None, act2=None):
    """``act_post(conv2d(x, cw) * gate + residual)`` for a 1x1 layer without activation and a split gate ``[B, 2, cw.cout]`` that does
    not depend on the layer's output (``se_fold``): ONE launch where the C ABI takes the shape (``out_gate_variant``: the gate multiply,
    the residual add and the ReLU run on the fp32 accumulators, the un-gated map is never stored), otherwise ``conv2d`` then
    ``scale_add_act`` - there the un-gated map is rounded to fp16 in between.
    With ``act2`` returns ``(y, act2(y))`` as ``scale_add_act`` does - the second output from the rounded ``y``, from the same launch
    where ``act2`` is SiLU (``out_gate2_variant``)."""
    d = _out_gate_desc(x, cw, gate, residual, act_post)
    if d is not None and act2 is not None and out_gate2_variant(d, cw.w_lo is not None, act2) is None:
        d = None
    if d is None:
        return scale_add_act(conv2d(x, cw), gate, residual, act_post, act2=act2)
    out = torch.empty((*x.shape[:3], cw.cout), dtype=torch.float16, device=x.device)
    has_lo = cw.w_lo is not None
    if act2 is not None:
        out2 = torch.empty_like(out)
        _launch("vip_conv2d_out_gated2_nhwc_f16", _p(x), _p(cw.w), _p(cw.w_lo), _p(cw.bias), _p(gate), _p(residual), _p(out), _p(out2),
                _act(act2), C.byref(d),
                prof=lambda: _conv_prof(conv_kernel_name(d, True, False, has_lo) or "unsupported", d, cw, residual, 2.0, 2.0,
                                        f" ogate res act_post={act_post} act2={act2}"))
        return out, out2
    _launch("vip_conv2d_out_gated_nhwc_f16", _p(x), _p(cw.w), _p(cw.w_lo), _p(cw.bias), _p(gate), _p(residual), _p(out), C.byref(d),
            prof=lambda: _conv_prof(conv_kernel_name(d, True, False, has_lo) or "unsupported", d, cw, residual, 2.0, 2.0,
                                    f" ogate res act_post={act_post}"))
    return out


_H2_SPAN_MAX = 0xFFFFFFE0       # the C kernels address every tensor through 32-bit buffer offsets


def _conv2d_h2(x, cw: ConvWeight, stride, pad, act, act_post, residual, out, cin_off, cout_off, gate):
    """packed-STRICT conv2d: packed x / residual / out, vip_conv2d_nhwc_h2; a packed gate [B, Cin] is multiplied in first.  Tensors
    beyond the 4 GiB the kernels can address are processed in batch slices (images are independent)."""
    if gate is not None:
        assert gate.shape == (x.shape[0], cw.cin) and x.shape[3] == cw.cin and cin_off == 0, (gate.shape, x.shape, cw.cin)
        _chkp(gate, "conv2d.gate")
        sh, sw = (stride, stride) if isinstance(stride, int) else stride
        # in the GEMM's activation operand (vip_conv2d_gated_nhwc_h2) where the C ABI carries it: 1x1 stride-1 ungrouped, no padding,
        # (activation) or (residual [+ReLU]) epilogue; otherwise a separate multiply pass first
        fold = (_H2_GATED and not _UNFUSED and _pointwise(cw) and (sh, sw) == (1, 1) and pad == (0, 0, 0, 0)
                and 4 * x.numel() < 0xFFFF0000 - 4 * cw.cin and _epilogue_ok(act, act_post, residual))
        if not fold:
            x, gate = scale_add_act(x, gate, None, None), None
    out, d = _conv_front("h2", x, cw, stride, pad, act, act_post, residual, out, cin_off, cout_off)
    B = d.B
    per_img = 4 * max(d.H * d.W * d.ldx, d.Ho * d.Wo * d.ldy, d.Ho * d.Wo * d.ldr)
    bmax = max(1, (_H2_SPAN_MAX - 1) // per_img)

    def prof():
        return _conv_prof("h2:" + ("pwk_direct_kernel" if gate is not None else conv_kernel_name_h2(d, residual is not None) or "unsupported"),
                          d, cw, residual, 4.0, 2.0)
    for b0 in range(0, B, bmax):
        b1 = min(B, b0 + bmax)
        d.B = b1 - b0
        rs = None if residual is None else residual[b0:b1]
        tail = (_p(cw.w), _p(cw.bias), _p(rs), _p(out[b0:b1]), C.byref(d), 1.0 / cw.h2_scale)
        if gate is not None:
            _launch("vip_conv2d_gated_nhwc_h2", _p(x[b0:b1]), _p(gate[b0:b1]), *tail, status=True, prof=prof)
        else:
            _launch("vip_conv2d_nhwc_h2", _p(x[b0:b1]), *tail, status=True, prof=prof)
    return out


def _conv2d_s32(x, cw: ConvWeight, stride, pad, act, act_post, residual, out, cin_off, cout_off, gate):
    """fp32-storage conv2d: fp32 x / weights / residual / out, vip_conv2d_nhwc_s32; a gate [B, Cin] fp32 is multiplied in first."""
    if gate is not None:
        assert gate.shape == (x.shape[0], cw.cin) and x.shape[3] == cw.cin and cin_off == 0, (gate.shape, x.shape, cw.cin)
        x = scale_add_act(x, gate, None, None)
    out, d = _conv_front("s32", x, cw, stride, pad, act, act_post, residual, out, cin_off, cout_off)
    split = STRICT_GEMM in ("bf16x3", "bf16x2") and cw.w_bf3 is not None     # bf16 planes of the weights; otherwise the f32-input MFMA

    def prof():
        return _conv_prof("sconv6_kernel" if split else "sconv_kernel", d, cw, residual, 4.0, 4.0)
    tail = (_p(cw.bias), _p(residual), _p(out), C.byref(d))
    if split:
        _launch("vip_conv2d_nhwc_s32x2" if STRICT_GEMM == "bf16x2" else "vip_conv2d_nhwc_s32x", _p(x), _p(cw.w_bf3), cw.w_bf3.shape[2], *tail,
                prof=prof)
    else:
        _launch("vip_conv2d_nhwc_s32", _p(x), _p(cw.w), *tail, prof=prof)
    return out


_CONV_STRICT = {"s32": _conv2d_s32, "h2": _conv2d_h2}


def _rows_out(x, cw: ConvWeight, residual, name: str):
    """``x [..., K]`` as M rows -> ``(M, K, out [..., cout] fp16, ldr)`` with the fp16 ``residual`` checked against ``out``"""
    K = x.shape[-1]
    out = torch.empty((*x.shape[:-1], cw.cout), dtype=torch.float16, device=x.device)
    if residual is not None:
        _chk16(residual, name)
        assert residual.shape == out.shape
    return x.numel() // K, K, out, 0 if residual is None else cw.cout


def dense(x: torch.Tensor, cw: ConvWeight, act=None, act_post=None, residual: Optional[torch.Tensor] = None):
    """Dense over the last axis of ``x`` (any leading shape)."""
    kind = _kind(x, "dense.x")
    if kind != "f16":
        if kind != cw.kind:
            raise _abi.VipError(f"dense: {kind} activations with {cw.kind} weights - build the model and its input in the same precision")
        lead, K = x.shape[:-1], x.shape[-1]
        r4 = None if residual is None else residual.reshape(-1, 1, 1, cw.cout)
        return _CONV_STRICT[kind](x.reshape(-1, 1, 1, K), cw, 1, (0, 0, 0, 0), act, act_post, r4, None, 0, 0, None).reshape(*lead, cw.cout)
    if _CALIB and cw.err is not None:
        _bias_correct(cw, x)
    if _EXACT and cw.exact is not None:
        x, cw, _ = _exact_operands(x, cw)
    M, K, out, ldr = _rows_out(x, cw, residual, "dense.residual")

    def prof():
        d = _abi.ConvDesc(B=M, H=1, W=1, Cin=K, Cout=cw.cout, kh=1, kw=1, sh=1, sw=1, pt=0, pl=0, Ho=1, Wo=1, groups=1, ldx=K,
                          cin_off=0, ldy=cw.cout, cout_off=0, ldr=ldr, res_off=0, ldw=cw.ldw, act_pre=_act(act),
                          act_post=_act(act_post))
        return (conv_kernel_name(d, residual is not None) or "unsupported", 2.0 * M * cw.cout * K,
                2.0 * (M * K + M * cw.cout * (2 if residual is not None else 1) + cw.w.numel()),
                f"M={M} N={cw.cout} K={K} dense{' res' if residual is not None else ''} act={act}")
    _launch("vip_gemm_bias_act_f16", _p(x), _p(cw.w), _p(cw.bias), _p(residual), _p(out), M, cw.cout, K, K, cw.ldw, cw.cout, ldr,
            _act(act), _act(act_post), prof=prof)
    return out


def ln_gemm_fused(x: torch.Tensor, cw: ConvWeight, act=None, act_post=None, residual: Optional[torch.Tensor] = None) -> bool:
    """whether ``ln_dense`` runs as ONE launch (``vip_ln_gemm_bias_act_f16``) for these operands"""
    K = x.shape[-1]
    return bool(_LN_GEMM and not (_UNFUSED or _CALIB or _EXACT) and x.dtype == torch.float16 and x.is_contiguous() and cw.kind == "f16"
                and _pointwise(cw) and cw.cin == K and 2 * x.numel() < 0xFFFF0000 - 2 * K and _epilogue_ok(act, act_post, residual)
                and _abi.lib().vip_ln_gemm_supported(x.numel() // K, K, cw.cout, _act(act)))


def ln_dense(x: torch.Tensor, ln, cw: ConvWeight, act=None, act_post=None, residual: Optional[torch.Tensor] = None):
    """``dense(layernorm(x), cw, ...)`` with ``ln = (gamma, beta, eps)``: on the fp16 storage ONE launch where the C ABI takes the shape
    (``vip_ln_gemm_supported``: the row is normalised in the registers of the GEMM, LN(x) never goes to memory), otherwise - and always
    on the strict storages and inside ``unfused()`` / ``calibration()`` / ``exact_weights()`` - LayerNorm then Dense, two launches.
    Same arithmetic either way: the normalised operand is rounded to fp16 where the separate launch stored it."""
    g, b, eps = _ln_args(ln)
    if not ln_gemm_fused(x, cw, act, act_post, residual):
        return dense(layernorm(x, g, b, eps), cw, act=act, act_post=act_post, residual=residual)
    M, K, out, ldr = _rows_out(x, cw, residual, "ln_dense.residual")
    # bytes: x in, y out (+ residual), the weights - no LN(x) round trip
    _launch("vip_ln_gemm_bias_act_f16", _p(x), _p(g), _p(b), eps, _p(cw.w), _p(cw.bias), _p(residual), _p(out), M, cw.cout, K, K, cw.ldw,
            cw.cout, ldr, _act(act), _act(act_post),
            prof=lambda: ("pwx_ln_kernel", 2.0 * M * cw.cout * K,
                          2.0 * (M * K + M * cw.cout * (2 if residual is not None else 1) + cw.w.numel()) + 8.0 * K,
                          f"M={M} N={cw.cout} K={K} ln+dense{' res' if residual is not None else ''} act={act}"))
    return out


def mlp(x: torch.Tensor, fc1: ConvWeight, fc2: ConvWeight, act="gelu", residual: Optional[torch.Tensor] = None, ln=None):
    """``fc2(act(fc1(LN(x)))) (+ residual)`` over the last axis; ``ln = (gamma, beta, eps)`` or None.  One fused launch
    (LayerNorm in the prologue, hidden tensor in registers) when the C ABI supports the shape, otherwise LayerNorm +
    two Dense launches - same arithmetic either way."""
    kind = _kind(x, "mlp.x")
    C_ = x.shape[-1]
    M = x.numel() // C_
    hid = fc1.cout
    g, b, eps = _ln_args(ln)
    ldr = C_ if residual is not None else 0
    if kind == "f16":
        fused = (not _UNFUSED and fc2.cout == C_ and fc1.groups == 1 and fc2.groups == 1 and x.is_contiguous()
                 and _abi.lib().vip_mlp_fused_supported(M, C_, hid, _act(act)))
    else:
        fused = (kind == "h2" and _MLP_H2_FUSED and not _UNFUSED and fc1.kind == fc2.kind == "h2" and fc2.cout == C_ and fc1.cin == C_
                 and fc2.cin == hid and _pointwise(fc1) and _pointwise(fc2) and x.is_contiguous() and 4 * x.numel() < _H2_SPAN_MAX
                 and _abi.lib().vip_mlp_fused_supported_h2(M, C_, hid, _act(act)))
    if not fused:
        if ln is not None and kind == "f16":      # LayerNorm folded into fc1 where the shape allows (ln_dense): two launches, else three
            return dense(ln_dense(x, ln, fc1, act=act), fc2, residual=residual)
        if ln is not None:
            x = layernorm(x, g, b, eps)
        return dense(dense(x, fc1, act=act), fc2, residual=residual)
    # one launch: LayerNorm in the prologue, the hidden tensor in registers
    out = torch.empty_like(x)
    if residual is not None:
        _chk_kind(residual, kind, "mlp.residual")
        assert residual.shape == out.shape
    if kind == "h2":
        _launch("vip_mlp_fused_h2", _p(x), _p(g), _p(b), eps, _p(fc1.w), _p(fc1.bias), 1.0 / fc1.h2_scale, _p(fc2.w), _p(fc2.bias),
                1.0 / fc2.h2_scale, _p(residual), _p(out), M, C_, hid, C_, fc1.ldw, fc2.ldw, C_, ldr, _act(act), status=True,
                prof=lambda: ("h2:mlp_h2_kernel", 4.0 * M * C_ * hid,
                              4.0 * M * C_ * (3 if residual is not None else 2) + 2.0 * (fc1.w.numel() + fc2.w.numel()),
                              f"M={M} C={C_} hidden={hid}"))
    else:
        _launch("vip_mlp_fused_f16", _p(x), _p(g), _p(b), eps, _p(fc1.w), _p(fc1.bias), _p(fc2.w), _p(fc2.bias), _p(residual), _p(out),
                M, C_, hid, C_, fc1.ldw, fc2.ldw, C_, ldr, _act(act),
                prof=lambda: ("mlp_fused_kernel" if C_ <= 96 else "mlp_stream_kernel", 4.0 * M * C_ * hid,
                              2.0 * (M * C_ * (3 if residual is not None else 2) + fc1.w.numel() + fc2.w.numel())))
    return out


def se_gate(x: torch.Tensor, fc1: ConvWeight, fc2: ConvWeight, act1, act2="sigmoid", split: bool = True) -> torch.Tensor:
    """``g = act2(fc2(act1(fc1(global_avgpool(x)))))`` -> the SPLIT gate [B, 2, fc2.cout] fp16 (``fp16(g)`` and
    ``fp16(g - fp16(g))``: a gate scales a whole channel map, so its rounding error would not average out over pixels),
    or with ``split=False`` the plain [B, fc2.cout] fp16 gate.

    One launch (vip_se_gate_f16: a workgroup per image, matrix-vector products out of L2) when the two weight matrices
    are small - every image re-reads them, so for wide gates (ResNet-RS / ResNeSt: Cr = C/4) the pool + two batched
    GEMMs are cheaper and are used instead (the last one with the split epilogue)."""
    kind = _kind(x, "se_gate.x")
    if kind != "f16":    # STRICT: the gate is a plain [B, C] in the activation storage
        B, Cc = x.shape[0], x.shape[-1]
        if kind == "h2" and _SE_H2_FUSED and fc1.kind == fc2.kind == "h2" and _se_chain_ok(fc1, fc2, Cc) and x.dim() == 4:
            # one launch (vip_se_gate_h2: the fp16 path's one-workgroup-per-image kernel on the packed storage)
            out = torch.empty((B, fc2.cout), dtype=PACKED, device=x.device)
            _launch("vip_se_gate_h2", _p(x), _p(fc1.w), _p(fc1.bias), 1.0 / fc1.h2_scale, _p(fc2.w), _p(fc2.bias), 1.0 / fc2.h2_scale,
                    _p(out), B, x.shape[1] * x.shape[2], Cc, Cc, fc1.cout, fc1.ldw, fc2.cout, fc2.ldw, _act(act1), _act(act2), status=True)
            return out
        return dense(dense(global_avgpool(x), fc1, act=act1), fc2, act=act2)    # pool -> Dense -> Dense
    B, H, W, Cc = x.shape
    assert _pointwise(fc1) and _pointwise(fc2)
    assert fc1.cin == Cc and fc2.cin == fc1.cout, (fc1.cin, Cc, fc2.cin, fc1.cout)
    if _UNFUSED or not _se_chain_ok(fc1, fc2, Cc):
        # pooled and hidden vectors as hi/lo planes too (the one-launch kernel keeps them in fp32)
        g = dense_split(dense_split(global_avgpool(x, split=True), fc1, act=act1), fc2, act=act2)
        return g if split else g[:, 0].contiguous()
    out = torch.empty((B, 2, fc2.cout) if split else (B, fc2.cout), dtype=torch.float16, device=x.device)
    tail = (_p(fc1.bias), _p(fc2.w), _p(fc2.bias), _p(out), B, H * W, Cc, Cc, fc1.cout, fc1.ldw, fc2.cout, fc2.ldw, _act(act1), _act(act2),
            int(split))
    if fc1.w_lo is not None:        # a two-term first layer (se_fold)
        _launch("vip_se_gate_hilo_f16", _p(x), _p(fc1.w), _p(fc1.w_lo), *tail)
    else:
        _launch("vip_se_gate_f16", _p(x), _p(fc1.w), *tail)
    return out


def dense_split(x: torch.Tensor, cw: ConvWeight, act=None) -> torch.Tensor:
    """Dense on a few rows with the output as two fp16 planes ``[M, 2, N]`` (``fp16(v)``, ``fp16(v - fp16(v))``).  ``x`` is ``[M, K]``
    or itself split, ``[M, 2, K]`` (a pooled vector from ``global_avgpool(split=True)`` or the previous layer of the chain)."""
    if _kind(x, "dense_split.x") != "f16":    # STRICT: the vectors need no extra hi / lo planes
        return dense(x, cw, act=act)
    split_in = x.dim() == 3
    assert x.dim() == 2 or (split_in and x.shape[1] == 2), x.shape
    if _CALIB and cw.err is not None:
        _bias_correct(cw, x.float().sum(1) if split_in else x)
    if _EXACT and cw.exact is not None:
        x, cw, _ = _exact_operands(x, cw)
    M, K = x.shape[0], x.shape[-1]
    if cw.w_lo is not None and not split_in:
        raise _abi.VipError("dense_split: two-term weights take split rows [M, 2, K] only (vip_gemm_split2_hilo_f16)")
    out = torch.empty((M, 2, cw.cout), dtype=torch.float16, device=x.device)
    for m0 in range(0, M, 256):       # the C entry points take at most 256 rows (a batch of pooled vectors)
        m1 = min(M, m0 + 256)
        head = (_p(x[m0:m1]), _p(cw.w), _p(cw.bias), _p(out[m0:m1]), m1 - m0, cw.cout, K)
        if cw.w_lo is not None:
            _launch("vip_gemm_split2_hilo_f16", _p(x[m0:m1]), _p(cw.w), _p(cw.w_lo), *head[2:], cw.ldw, _act(act))
        elif split_in:
            _launch("vip_gemm_split2_f16", *head, cw.ldw, _act(act))
        else:
            _launch("vip_gemm_split_f16", *head, K, cw.ldw, _act(act))
    return out


# ---- depthwise convolution ----------------------------------------------------------------------------------------------------------
_DW_QUAD = {}      # filter storage -> (filter, its quad-major copy); the filter is kept alive so that the address cannot be reused


def _dw_quad_major(w_khwc: torch.Tensor, k: int) -> torch.Tensor:
    """``[k,k,C]`` fp32 -> ``[C/4, k*k, 4]`` (vip_dw_filter_quad_major), built once per filter tensor"""
    key = (w_khwc.data_ptr(), w_khwc._version, tuple(w_khwc.shape))
    hit = _DW_QUAD.get(key)
    if hit is None:
        wq = torch.empty_like(w_khwc)
        _launch("vip_dw_filter_quad_major", _p(w_khwc), _p(wq), k, w_khwc.shape[-1])
        hit = _DW_QUAD[key] = (w_khwc, wq)
    return hit[1]


def dwconv2d(x, w_khwc: torch.Tensor, bias: Optional[torch.Tensor], k: int, stride=1, pad=(0, 0, 0, 0), act=None):
    """Depthwise conv; ``w_khwc`` fp32 ``[k,k,C]``, bias fp32 ``[C]``."""
    kind = _kind(x, "dwconv2d.x")
    B, H, W, Cc = x.shape
    if not _dw_filter_ok(w_khwc, k, Cc):
        raise ValueError("dwconv2d: the filter must be a contiguous fp32 [k,k,C] tensor")
    pt, _, pl, _ = pad
    Ho, Wo = _out_hw(H, W, k, k, stride, stride, pad)
    out = torch.empty((B, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    if (kind == "h2" and _DW_H2_LDS and stride == 1 and k >= _DW_H2_LDS
            and _abi.lib().vip_dwconv2d_s1_supported_h2(B, H, W, Cc, k, Ho, Wo)):
        # the LDS-staged kernel (dwconv_lds_h2.hip) on the quad-major copy of the filter
        _launch("vip_dwconv2d_s1_h2", _p(x), _p(_dw_quad_major(w_khwc, k)), _p(bias), _p(out), B, H, W, Cc, k, pt, pl, Ho, Wo, _act(act),
                status=True)
    else:
        _launch_kind("dwconv2d_nhwc", kind, _p(x), _p(w_khwc), _p(bias), _p(out), B, H, W, Cc, k, stride, pt, pl, Ho, Wo, _act(act))
    return out


def dwconv2d_se(x, w_khwc: torch.Tensor, bias: Optional[torch.Tensor], k: int, stride, pad, act, fc1: ConvWeight, fc2: ConvWeight,
                act1, act2="sigmoid", split: bool = True):
    """``h = act(dwconv(x))`` and the squeeze-excite gate of ``h`` (``se_gate(h, fc1, fc2, act1, act2, split)``) - the
    DepthwiseConv2D -> activation -> se_module run of an MBConv block (kecam efficientnet_v2.py:85-97) and of GCViT's FeatExtract /
    ReduceSize (gcvit/layers/feature.py:46-70,93-96).  Returns ``(h, gate)``.  Where the C ABI takes the shape (stride 1, the tile
    kernel; gate matrices small enough for the one-launch gate) the depthwise kernel leaves per-workgroup partial sums of its fp32
    outputs and the gate kernel finishes the mean from those instead of reading ``h`` again (``vip_dwconv2d_pool_nhwc_f16`` +
    ``vip_se_gate_pooled_f16``; ``VIP_DW_SE_POOL=0``: always the two plain calls)."""
    B, H, W, Cc = x.shape
    pt, _, pl, _ = pad
    Ho, Wo = _out_hw(H, W, k, k, stride, stride, pad)
    # both storages: the depthwise kernel leaves the pool's partial sums and the one-launch gate kernel finishes from them
    pooled = _DW_SE_FUSED and not _UNFUSED and stride == 1 and _se_chain_ok(fc1, fc2, Cc) and _dw_filter_ok(w_khwc, k, Cc)
    parts = 0
    if pooled and x.dtype == PACKED and _SE_H2_FUSED and _DW_H2_LDS and k >= _DW_H2_LDS and fc1.kind == fc2.kind == "h2":
        parts = _abi.lib().vip_dwconv2d_s1_pool_parts_h2(B, H, W, Cc, k, Ho, Wo)      # the LDS-staged depthwise kernel
    elif pooled and x.dtype == torch.float16 and not _CALIB and not _EXACT:
        parts = _abi.lib().vip_dwconv2d_pool_parts(B, H, W, Cc, k, stride, Ho, Wo)
    if parts <= 0:
        h = dwconv2d(x, w_khwc, bias, k, stride, pad, act=act)
        return h, se_gate(h, fc1, fc2, act1, act2, split=split)
    kind = _kind(x, "dwconv2d_se.x")
    h = torch.empty((B, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    partials = torch.empty((B, parts, Cc), dtype=torch.float32, device=x.device)
    if kind == "h2":
        _launch("vip_dwconv2d_s1_pool_h2", _p(x), _p(_dw_quad_major(w_khwc, k)), _p(bias), _p(h), _p(partials), parts, B, H, W, Cc, k,
                pt, pl, Ho, Wo, _act(act), status=True)
        gate = torch.empty((B, fc2.cout), dtype=PACKED, device=x.device)
        _launch("vip_se_gate_pooled_h2", _p(partials), parts, _p(fc1.w), _p(fc1.bias), 1.0 / fc1.h2_scale, _p(fc2.w), _p(fc2.bias),
                1.0 / fc2.h2_scale, _p(gate), B, Ho * Wo, Cc, fc1.cout, fc1.ldw, fc2.cout, fc2.ldw, _act(act1), _act(act2), status=True)
    else:
        _launch("vip_dwconv2d_pool_nhwc_f16", _p(x), _p(w_khwc), _p(bias), _p(h), _p(partials), parts, B, H, W, Cc, k, stride, pt, pl,
                Ho, Wo, _act(act))
        gate = torch.empty((B, 2, fc2.cout) if split else (B, fc2.cout), dtype=torch.float16, device=x.device)
        _launch("vip_se_gate_pooled_f16", _p(partials), parts, _p(fc1.w), _p(fc1.bias), _p(fc2.w), _p(fc2.bias), _p(gate), B, Ho * Wo,
                Cc, fc1.cout, fc1.ldw, fc2.cout, fc2.ldw, _act(act1), _act(act2), int(split))
    return h, gate


def mbconv_expand_dw(x, cw: ConvWeight, w_khwc: torch.Tensor, dw_bias: Optional[torch.Tensor], k: int, stride: int, pad, act=None):
    """``act(dwconv(act(conv1x1(x, cw)), w_khwc) + dw_bias)`` - the expand convolution and the depthwise convolution of an MBConv
    block - as ``conv2d`` then ``dwconv2d``, or with ``VIP_MBCONV_FUSED=1`` in ONE launch where the C ABI takes the shape (the
    expanded tensor stays in LDS): the same fp16 values either way up to fp32 summation order.  The fused kernel is opt-in because
    it measured 0.4-0.8x the speed of the two launches (``tools/bench_mbconv.py``, ``profiles/r02_mbconv_fused_vs_two_launches.log``):
    the two HBM-bound kernels hide their swish evaluations (exp + rcp each) behind memory, the fused one is VALU-bound on them plus
    the halo recompute.  Calibration / exact-weight passes always run the two launches."""
    B, H, W, ldx = x.shape
    ok = (not _UNFUSED and x.dtype == torch.float16 and mbconv_fused() and _pointwise(cw) and ldx == cw.cin
          and w_khwc.shape == (k, k, cw.cout) and _abi.lib().vip_mbconv_expand_dw_supported(cw.cin, cw.cout, k, stride))
    if not ok:
        return dwconv2d(conv2d(x, cw, act=act), w_khwc, dw_bias, k, stride, pad, act=act)
    _chk16(x, "mbconv_expand_dw.x")
    Ho, Wo = _out_hw(H, W, k, k, stride, stride, pad)
    out = torch.empty((B, Ho, Wo, cw.cout), dtype=torch.float16, device=x.device)
    _launch("vip_mbconv_expand_dw_f16", _p(x), _p(cw.w), _p(cw.w_lo), _p(cw.bias), _p(w_khwc), _p(dw_bias), _p(out), B, H, W,
            cw.cin, cw.cout, cw.ldw, k, stride, pad[0], pad[2], Ho, Wo, _act(act), _act(act),
            prof=lambda: ("mbconv_expand_dw_kernel", 2.0 * B * (H * W * cw.cin + Ho * Wo * k * k) * cw.cout,
                          2.0 * (x.numel() + out.numel() + cw.w.numel()), f"{H}x{W} Cin={cw.cin} Ce={cw.cout} k{k} s{stride}"))
    return out


# ---- elementwise, pooling, heads ----------------------------------------------------------------------------------------------------
def layernorm(x, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    kind = _kind(x, "layernorm.x")
    Cc = x.shape[-1]
    out = torch.empty_like(x)
    _launch_kind("layernorm", kind, _p(x), _p(gamma), _p(beta), _p(out), x.numel() // Cc, Cc, float(eps))
    return out


POOL_MAX_ZEROPAD, POOL_AVG_VALID, POOL_AVG_FULL = 0, 1, 2


def pool2d(x, k: int, stride: int, pad=(0, 0, 0, 0), mode=POOL_MAX_ZEROPAD, out_hw=None):
    """``out_hw`` = (Ho, Wo) asks for fewer output rows / columns than the padding implies (a top-left crop); with k = 1,
    stride 1 and zero-pad max pooling the op is a zero-padded copy (GCViT FitWindow) or a crop (level.py:61)."""
    kind = _kind(x, "pool2d.x")
    B, H, W, Cc = x.shape
    Ho, Wo = _out_hw(H, W, k, k, stride, stride, pad)
    if out_hw is not None:
        assert out_hw[0] <= Ho and out_hw[1] <= Wo
        Ho, Wo = out_hw
    out = torch.empty((B, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    _launch_kind("pool2d_nhwc", kind, _p(x), _p(out), B, H, W, Cc, Cc, Cc, k, stride, pad[0], pad[2], Ho, Wo, mode)
    return out


def global_avgpool(x, split: bool = False):
    """[B,H,W,C] (or [B,N,C]) -> [B,C]; ``split``: [B,2,C], the mean as a hi and a lo fp16 plane (for ``dense_split``)."""
    B, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * Cc)
    kind = _kind(x, "global_avgpool.x")
    if split and kind == "f16":     # the STRICT storages: [B, C] whatever ``split`` says
        out = torch.empty((B, 2, Cc), dtype=torch.float16, device=x.device)
        _launch("vip_global_avgpool_split_f16", _p(x), _p(out), B, HW, Cc, Cc)
    else:
        out = torch.empty((B, Cc), dtype=x.dtype, device=x.device)
        _launch_kind("global_avgpool", kind, _p(x), _p(out), B, HW, Cc, Cc)
    return out


def gap_dense_f32(x, w_nc: torch.Tensor, bias: Optional[torch.Tensor]):
    """Classifier head: mean over the middle axes of ``x`` ([B,...,C]) then Dense -> fp32 ``[B,N]``.
    ``w_nc`` fp32 ``[N,C]``."""
    kind = _kind(x, "gap_dense_f32.x")
    B, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * Cc)
    N = w_nc.shape[0]
    assert w_nc.dtype == torch.float32 and w_nc.shape == (N, Cc) and w_nc.is_contiguous()
    out = torch.empty((B, N), dtype=torch.float32, device=x.device)
    if kind != "f16":
        _launch_kind("gap_ln_dense", kind, _p(x), None, None, 0.0, _p(w_nc), _p(bias), _p(out), B, HW, Cc, Cc, HW * Cc, N)
    else:
        _launch("vip_gap_dense_f32", _p(x), _p(w_nc), _p(bias), _p(out), B, HW, Cc, Cc, N)
    return out


def gap_ln_dense_f32(x, gamma: torch.Tensor, beta: torch.Tensor, eps: float, w_nc: torch.Tensor, bias: Optional[torch.Tensor]):
    """Classifier head with a LayerNorm on the pooled vector: mean over the middle axes of ``x`` ([B,...,C]) -> LayerNorm over C
    -> Dense, fp32 throughout -> fp32 ``[B,N]``.  ``gamma``/``beta`` fp32 ``[C]``, ``w_nc`` fp32 ``[N,C]``."""
    kind = _kind(x, "gap_ln_dense_f32.x")
    B, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * Cc)
    N = w_nc.shape[0]
    assert w_nc.dtype == torch.float32 and w_nc.shape == (N, Cc) and w_nc.is_contiguous()
    assert gamma.dtype == beta.dtype == torch.float32 and gamma.shape == beta.shape == (Cc,)
    out = torch.empty((B, N), dtype=torch.float32, device=x.device)
    head = (_p(x), _p(gamma), _p(beta), float(eps), _p(w_nc), _p(bias), _p(out), B, HW, Cc, Cc)
    if kind != "f16":
        _launch_kind("gap_ln_dense", kind, *head, HW * Cc, N)
    else:
        _launch("vip_gap_ln_dense_f32", *head, N)
    return out


HEAD_ACTS = {"linear": 0, None: 0, "none": 0, "sigmoid": 1, "softmax": 2}


def head_prob(z: torch.Tensor, act="default") -> torch.Tensor:
    """fp32 logits ``[B, N]`` -> what ``model.predict`` returns (fp32 ``[B, N]``).  ``act="default"``: sigmoid for one class, softmax
    otherwise - the pairing of every constructor default; otherwise the classifier activation the checkpoint's model_config names
    (``"sigmoid"`` / ``"softmax"`` / ``"linear"``: resnet_rs_model.py:474-476 ``classifier_activation``, gcvit models/gcvit.py:113 ``head_act``)."""
    assert z.dtype == torch.float32 and z.is_cuda and z.dim() == 2 and z.is_contiguous()
    out = torch.empty_like(z)
    n = z.shape[1]
    if act == "default" or (act == "sigmoid" and n == 1) or (act == "softmax" and n > 1):
        _launch("vip_head_prob_f32", _p(z), _p(out), None, z.shape[0], n)
        return out
    if act not in HEAD_ACTS:
        raise ValueError(f"head activation {act!r}: expected one of {sorted(k for k in HEAD_ACTS if isinstance(k, str))}")
    _launch("vip_head_act_f32", _p(z), _p(out), z.shape[0], n, HEAD_ACTS[act])
    return out


def binary_score(p: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """probabilities ``[n, C]`` (a model's ``predict``) -> the per-image score of main.py:113-114 (``p`` for one class, ``1 - p[:, 0]``
    otherwise), fp32 ``[n]``; ``out``: a row of the members x images score matrix."""
    n, Cc = p.shape
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=p.device)
    assert out.dtype == torch.float32 and out.shape == (n,) and out.is_contiguous()
    pf = p if (p.dtype == torch.float32 and p.is_contiguous()) else p.float().contiguous()
    _launch("vip_prob_to_score_f32", _p(pf), _p(out), n, Cc)
    return out


def ensemble_mean(scores: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 ``[M, n]`` member scores -> ``[n]`` ensemble mean (main.py:142-143); ``out``: a contiguous fp32 ``[n]`` row to write it to."""
    assert scores.dtype == torch.float32 and scores.is_cuda and scores.dim() == 2 and scores.stride(1) == 1
    if out is None:
        out = torch.empty((scores.shape[1],), dtype=torch.float32, device=scores.device)
    assert out.dtype == torch.float32 and out.shape == (scores.shape[1],) and out.is_contiguous() and out.device == scores.device
    _launch("vip_ensemble_mean_f32", _p(scores), _p(out), scores.shape[0], scores.shape[1], scores.stride(0))
    return out


def tile_aggregate(scores: torch.Tensor, seg: torch.Tensor, thr: float) -> torch.Tensor:
    """fp32 ``[R, T]`` tile scores and ``seg`` int32 ``[n + 1]`` (image i owns columns ``seg[i]:seg[i + 1]``) -> fp32 ``[3, R, n]``: per row
    and image the mean of its tile scores (a sequential fp32 sum in tile order), their max and the fraction ``> thr``; NaN for an
    image without tiles (``vip_tile_aggregate_f32``)."""
    assert scores.dtype == torch.float32 and scores.is_cuda and scores.dim() == 2 and scores.is_contiguous()
    assert seg.dtype == torch.int32 and seg.dim() == 1 and seg.is_contiguous() and seg.device == scores.device and seg.numel() >= 2
    R, T = scores.shape
    n = seg.numel() - 1
    if T == 0:                                           # no image of the batch is tiled: nothing to read
        return torch.full((3, R, n), float("nan"), dtype=torch.float32, device=scores.device)
    out = torch.empty((3, R, n), dtype=torch.float32, device=scores.device)
    _launch("vip_tile_aggregate_f32", _p(scores), _p(seg), n, R, T, C.c_float(float(thr)), _p(out))
    return out


def occlusion_cells(scores: torch.Tensor, plain: torch.Tensor, seg, grid: int, window: int, thr: float):
    """fp32 ``[R, V]`` variant scores, ``[R, n]`` plain scores and ``seg`` int32 ``[n + 1]`` - the HOST array of ``pipeline.occlusion_plan``
    (image i owns columns ``seg[i]:seg[i + 1]``: none, or its ``(grid - window + 1)^2`` windows row-major; anything else raises
    ``ValueError``) -> ``(cells [R, n, grid, grid], stats [R, n, 4])``: per cell the mean of ``plain - score`` over the windows covering it
    (a sequential fp32 sum in variant order), and per image (max delta, min delta, index of the variant with the max, variants whose
    side of ``thr`` differs from the plain score's); NaN for an image without variants (``vip_occlusion_cells_f32``)."""
    seg = np.ascontiguousarray(np.asarray(seg))
    if seg.dtype != np.int32 or seg.ndim != 1 or seg.size < 2:
        raise ValueError(f"occlusion_cells: seg must be a host int32 [n + 1] array, got {seg.dtype} {seg.shape}")
    G, K = int(grid), int(window)
    if not (2 <= G <= 32 and 1 <= K <= G):
        raise ValueError(f"occlusion_cells: grid {grid!r} / window {window!r}: expected 2 <= grid <= 32 and 1 <= window <= grid")
    n, per = seg.size - 1, (G - K + 1) ** 2
    counts = np.diff(seg.astype(np.int64))
    if seg[0] != 0 or not np.isin(counts, (0, per)).all():
        raise ValueError(f"occlusion_cells: every image has 0 or {per} variants at grid {G}, window {K}; seg gives {counts.tolist()} "
                         f"from {int(seg[0])}")
    if scores.dim() != 2 or int(seg[-1]) != scores.shape[1]:
        raise ValueError(f"occlusion_cells: seg ends at {int(seg[-1])}, the scores are {tuple(scores.shape)}")
    assert scores.dtype == torch.float32 and scores.is_cuda and scores.is_contiguous()
    R, V = scores.shape
    assert plain.dtype == torch.float32 and plain.shape == (R, n) and plain.is_contiguous() and plain.device == scores.device
    if V == 0:                                           # no image of the batch has variants: nothing to read
        nan = float("nan")
        return (torch.full((R, n, G, G), nan, dtype=torch.float32, device=scores.device),
                torch.full((R, n, 4), nan, dtype=torch.float32, device=scores.device))
    cells = torch.empty((R, n, G, G), dtype=torch.float32, device=scores.device)
    stats = torch.empty((R, n, 4), dtype=torch.float32, device=scores.device)
    seg_d = torch.from_numpy(seg).to(scores.device)
    _launch("vip_occlusion_cells_f32", _p(scores), _p(plain), _p(seg_d), n, R, V, G, K, C.c_float(float(thr)), _p(cells), _p(stats))
    return cells, stats


def occlusion_map(cells_row: torch.Tensor, sizes: torch.Tensor, max_hw, out: str = "f32") -> torch.Tensor:
    """One row of ``occlusion_cells``' cells, fp32 ``[n, G, G]``, as full-size maps ``[n, maxH, maxW]``: every pixel of an image takes its
    cell's value (cell g of an axis of length L = pixels ``(g L) // G .. ((g + 1) L) // G - 1``, the occluder's own edges), 0 outside the
    image.  ``sizes`` int32 ``[n, 2]`` (h, w) and ``max_hw`` = the slot size, as ``DecodedBatch.sizes`` / ``.rgb.shape[1:3]``.  ``out``:
    ``"f32"`` the values as they are; ``"u8"`` uint8 ``round(255 * (0.5 + 0.5 * v / peak))`` with ``peak`` = the image's largest ``|cell|``,
    128 (no effect) everywhere when that is 0 or the cells are NaN - what ``cam_overlay`` blends (``vip_occlusion_map``)."""
    if out not in ("f32", "u8"):
        raise ValueError(f"occlusion_map out={out!r}: expected 'f32' or 'u8'")
    _chk32(cells_row, "occlusion_map.cells_row")
    assert cells_row.dim() == 3 and cells_row.shape[1] == cells_row.shape[2], cells_row.shape
    n, G = int(cells_row.shape[0]), int(cells_row.shape[1])
    maxH, maxW = int(max_hw[0]), int(max_hw[1])
    assert sizes.dtype == torch.int32 and sizes.shape == (n, 2) and sizes.is_cuda and sizes.is_contiguous()
    res = torch.empty((n, maxH, maxW), dtype=torch.uint8 if out == "u8" else torch.float32, device=cells_row.device)
    _launch("vip_occlusion_map", _p(cells_row), _p(sizes), n, maxH, maxW, G, _p(res), int(out == "u8"))
    return res


def cam(features, w_nc: torch.Tensor, bias: Optional[torch.Tensor], ln=None, act="default", target="score"):
    """Grad-CAM of a ``GAP -> [LayerNorm] -> Dense -> activation`` head from the feature map alone (csrc/cam.hip: the gradient has a
    closed form, no backward pass).  ``features`` ``[B,H,W,C]`` in any activation storage; ``w_nc`` fp32 ``[N,C]``; ``ln`` =
    ``(gamma, beta, eps)`` or None; ``act`` as ``head_prob``; ``target``: ``"score"`` (what ``binary_score`` makes of the probabilities)
    or a class index.  Returns ``(cam [B,H,W]`` fp32, after the max with 0 and NOT normalised, ``peak [B]``, ``z [B,N])``.  The
    normalised map is ``cam / peak``, all zero where ``peak == 0``; a NaN ``peak`` marks a non-finite map (``cam_check``)."""
    if features.dim() != 4:
        raise _abi.VipError(f"cam: expected a [B,H,W,C] feature map, got {tuple(features.shape)}")
    B, H, W, Cc = features.shape
    # images may sit at a pitch of their own (a batch slice of a wider buffer); inside an image the map is dense
    pitch = features.stride(0) if B > 1 else H * W * Cc
    if features.stride()[1:] != (W * Cc, Cc, 1) or pitch < H * W * Cc:
        raise _abi.VipError(f"cam.features: expected dense [H,W,C] images at a pitch >= H*W*C, got strides {features.stride()}")
    kind = _kind(features[:1], "cam.features")
    N = w_nc.shape[0]
    assert w_nc.dtype == torch.float32 and w_nc.shape == (N, Cc) and w_nc.is_contiguous()
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() == N)
    if act == "default":
        act = "sigmoid" if N == 1 else "softmax"
    if act not in HEAD_ACTS:
        raise ValueError(f"head activation {act!r}: expected one of {sorted(k for k in HEAD_ACTS if isinstance(k, str))}")
    if target == "score":
        tgt = -1
    elif isinstance(target, int) and not isinstance(target, bool) and 0 <= target < N:
        tgt = target
    else:
        raise ValueError(f"cam target {target!r}: expected 'score' or a class index below {N}")
    g, b, eps = _ln_args(ln)
    if ln is not None:
        assert g.dtype == b.dtype == torch.float32 and g.shape == b.shape == (Cc,)
    out = torch.empty((B, H, W), dtype=torch.float32, device=features.device)
    peak = torch.empty((B,), dtype=torch.float32, device=features.device)
    z = torch.empty((B, N), dtype=torch.float32, device=features.device)
    _launch_kind("cam", kind, _p(features), _p(g), _p(b), eps, _p(w_nc), _p(bias), _p(out), _p(peak), _p(z), B, H * W, Cc, Cc, pitch, N,
                 HEAD_ACTS[act], tgt)
    return out, peak, z


def cam_check(peak: torch.Tensor, what: str = "cam") -> torch.Tensor:
    """Synchronising check of ``ops.cam``'s peaks: a non-finite peak is an error, not a map.  Returns the peaks on the host."""
    host = peak.detach().float().cpu()
    if not bool(torch.isfinite(host).all()):
        raise _abi.VipError(f"{what}: the evidence map of image(s) {torch.nonzero(~torch.isfinite(host)).tolist()} is not finite")
    return host


CAM_MAX_MEMBERS = 16


def cam_compose(maps, peaks, sizes: torch.Tensor, max_hw, weights=None, out: str = "f32") -> torch.Tensor:
    """Members' low-resolution maps -> one full-size map per image: each ``maps[m]`` ``[n,gh,gw]`` fp32 (``ops.cam``) is normalised by
    ``peaks[m]`` ``[n]``, resampled to the image's own size (bilinear, half-pixel centres, edge clamp) and the results are averaged
    (``weights``: default 1 / members) - one pass, the full-size map is written once.  ``sizes`` int32 ``[n,2]`` (h, w) and ``max_hw`` =
    the slot size, as ``DecodedBatch.sizes`` / ``.rgb.shape[1:3]``.  ``out``: ``"f32"`` -> fp32 ``[n,maxH,maxW]`` in [0, 1], ``"u8"`` ->
    uint8 ``round(255 * map)``; zero outside an image."""
    M = len(maps)
    if not 1 <= M <= CAM_MAX_MEMBERS or len(peaks) != M:
        raise _abi.VipError(f"cam_compose: {M} maps / {len(peaks)} peaks (1 .. {CAM_MAX_MEMBERS} members)")
    if out not in ("f32", "u8"):
        raise ValueError(f"cam_compose out={out!r}: expected 'f32' or 'u8'")
    n = maps[0].shape[0]
    maxH, maxW = int(max_hw[0]), int(max_hw[1])
    assert sizes.dtype == torch.int32 and sizes.shape == (n, 2) and sizes.is_cuda and sizes.is_contiguous()
    for m_, p_ in zip(maps, peaks):
        _chk32(m_, "cam_compose.map")
        _chk32(p_, "cam_compose.peak")
        assert m_.dim() == 3 and m_.shape[0] == n and p_.shape == (n,), (m_.shape, p_.shape)
    w = [1.0 / M] * M if weights is None else [float(v) for v in weights]
    assert len(w) == M
    res = torch.empty((n, maxH, maxW), dtype=torch.uint8 if out == "u8" else torch.float32, device=maps[0].device)
    _launch("vip_cam_compose_f32", (C.c_void_p * M)(*[m_.data_ptr() for m_ in maps]), (C.c_int * M)(*[m_.shape[1] for m_ in maps]),
            (C.c_int * M)(*[m_.shape[2] for m_ in maps]), (C.c_void_p * M)(*[p_.data_ptr() for p_ in peaks]),
            (C.c_float * M)(*w), M, _p(sizes), n, maxH, maxW, _p(res), int(out == "u8"))
    return res


def cam_overlay(rgb: torch.Tensor, map_u8: torch.Tensor, table: torch.Tensor, alpha: float = 0.4) -> torch.Tensor:
    """``clip(round(rgb + alpha * table[map]))``: the colour table (uint8 ``[256,3]``) applied to a uint8 map ``[n,maxH,maxW]``
    (``cam_compose(..., out="u8")``) and blended over the decoded pixels ``rgb`` uint8 ``[n,maxH,maxW,3]`` (``DecodedBatch.rgb``)."""
    for t, name in ((rgb, "rgb"), (map_u8, "map"), (table, "table")):
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
            raise _abi.VipError(f"cam_overlay.{name}: expected a contiguous CUDA uint8 tensor, got {t.dtype} {t.device}")
    n, maxH, maxW, ch = rgb.shape
    assert ch == 3 and map_u8.shape == (n, maxH, maxW) and table.shape == (256, 3), (rgb.shape, map_u8.shape, table.shape)
    out = torch.empty_like(rgb)
    _launch("vip_cam_overlay_u8", _p(rgb), _p(map_u8), _p(table), float(alpha), n, maxH, maxW, _p(out))
    return out


def scale_add_act(x, scale=None, residual=None, act=None, act2=None):
    """act(x * scale[b,c] + residual); with ``act2`` returns ``(y, act2(y))`` from one launch.
    ``scale`` is [B, C] in the storage of ``x``, or on the fp16 storage a split gate [B, 2, C] (planes summed in fp32)."""
    B, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * Cc)
    kind = _kind(x, "scale_add_act.x")
    if scale is not None:
        _chk_kind(scale, kind, "scale_add_act.scale")
        assert scale.shape == (B, Cc) or (kind == "f16" and scale.shape == (B, 2, Cc)), scale.shape
    if residual is not None:
        _chk_kind(residual, kind, "scale_add_act.residual")
        assert residual.shape == x.shape
    out = torch.empty_like(x)
    out2 = torch.empty_like(x) if act2 is not None else None
    tail = (_p(residual), _p(out), _p(out2), B, HW, Cc, _act(act), _act(act2))
    if kind == "f16":       # this entry point alone takes the number of scale planes
        _launch("vip_scale_add_act3_f16", _p(x), _p(scale), 2 if (scale is not None and scale.dim() == 3) else 1, *tail)
    else:
        _launch_kind("scale_add_act", kind, _p(x), _p(scale), *tail)
    return out if act2 is None else (out, out2)


def window_attention(qkv, q_global, bias_table, heads: int, ws: int, scale: float):
    """GCViT window attention core on feature-map layout.  qkv ``[B,Hp,Wp,nq*C]``; q_global ``[B,ws*ws,C]`` or None."""
    kind = _kind(qkv, "window_attention.qkv")
    B, Hp, Wp, CC = qkv.shape
    nq = 2 if q_global is not None else 3
    Cc = CC // nq
    if q_global is not None:
        _chk_kind(q_global, kind, "window_attention.q_global")
        assert q_global.numel() == B * ws * ws * Cc
    assert bias_table.dtype == torch.float32 and bias_table.shape == ((2 * ws - 1) ** 2, heads)
    out = torch.empty((B, Hp, Wp, Cc), dtype=qkv.dtype, device=qkv.device)

    def prof():
        # algorithmic work of the attention core: 4*N^2*hd FLOPs and 4*N*hd fp16 elements
        # (q, k, v read + out written) per (window, head)
        nwh = B * (Hp // ws) * (Wp // ws) * heads
        N = ws * ws
        return ("window_attn_kernel", nwh * 4.0 * N * N * 32, nwh * 4.0 * N * 32 * 2,
                f"attn core ws{ws} C={Cc} heads={heads} map={Hp}x{Wp} global={int(q_global is not None)}")
    _launch_kind("window_attn_fwd", kind, _p(qkv), _p(q_global), _p(bias_table), _p(out), B, Hp, Wp, Cc, heads, ws, nq, float(scale),
                 prof=prof if kind == "f16" else None)     # the roofline counts the fp16 core only
    return out


def gcvit_attn_block(x, q_global, ln, qkv: ConvWeight, proj: ConvWeight, bias_table, heads: int, ws: int, scale: float):
    """``x + proj(window_attention(qkv(LayerNorm(x))))`` - the attention half of a GCViT block (gcvit/layers/block.py:58-79) on the
    feature-map layout ``[B, Hp, Wp, C]``; ``ln = (gamma, beta, eps)``, ``q_global`` ``[B, ws*ws, C]`` or None.  ONE launch
    (``vip_gcvit_attn_block_f16``: x in, y out, nothing in between leaves the CU) where the C ABI takes the configuration - levels 0
    and 1: 7 x 7 windows, C = 64 / 2 heads or C = 128 / 4 heads - otherwise LayerNorm, Dense, attention core, Dense + residual as four launches
    (``VIP_GCVIT_BLOCK_FUSED=0``: always; calibration / exact-weight passes too, they hook the Dense layers)."""
    B, Hp, Wp, Cc = x.shape
    nq = 2 if q_global is not None else 3
    fused = (_GCVIT_BLOCK_FUSED and not (_UNFUSED or _CALIB or _EXACT) and x.dtype == torch.float16 and x.is_contiguous()
             and qkv.w_lo is None and proj.w_lo is None and _pointwise(qkv) and _pointwise(proj)
             and qkv.cin == Cc and qkv.cout == nq * Cc and proj.cin == Cc and proj.cout == Cc
             and Hp % ws == 0 and Wp % ws == 0 and (ws != 14 or _GCVIT_BLOCK14)
             and _abi.lib().vip_gcvit_attn_block_supported(Cc, heads, ws))
    if not fused:
        y = ln_dense(x, ln, qkv)
        att = window_attention(y, q_global, bias_table, heads, ws, scale)
        return dense(att, proj, residual=x)
    _chk16(x, "gcvit_attn_block.x")
    if q_global is not None:
        _chk16(q_global, "gcvit_attn_block.q_global")
        assert q_global.numel() == B * ws * ws * Cc
    assert bias_table.dtype == torch.float32 and bias_table.shape == ((2 * ws - 1) ** 2, heads) and bias_table.is_contiguous()
    out = torch.empty_like(x)

    def prof():
        # the fused form of SURVEY.md section 8(d): per window 2 N C^2 (1 + nq) + 4 N^2 C FLOPs (= 8 N C^2 + 4 N^2 C with q, k, v) and
        # 4 N C bytes (x in, y out, fp16)
        nwin, N = B * (Hp // ws) * (Wp // ws), ws * ws
        return ("gcvit_attn_block_kernel", nwin * (2.0 * N * Cc * Cc * (1 + nq) + 4.0 * N * N * Cc), nwin * 4.0 * N * Cc,
                f"attn block ws{ws} C={Cc} heads={heads} map={Hp}x{Wp} global={int(q_global is not None)}")
    g, b, eps = _ln_args(ln)
    _launch("vip_gcvit_attn_block_f16", _p(x), _p(q_global), _p(g), _p(b), eps, _p(qkv.w), qkv.ldw, _p(qkv.bias), _p(proj.w), proj.ldw,
            _p(proj.bias), _p(bias_table), _p(out), B, Hp, Wp, Cc, heads, ws, float(scale), prof=prof)
    return out


def mhsa(qkv, heads: int, scale: float):
    """ViT attention core: qkv ``[B,N,3D]`` -> ``[B,N,D]``."""
    kind = _kind(qkv, "mhsa.qkv")
    B, N, D3 = qkv.shape
    D = D3 // 3
    out = torch.empty((B, N, D), dtype=qkv.dtype, device=qkv.device)
    _launch_kind("mhsa_fwd", kind, _p(qkv), _p(out), B, N, D, heads, float(scale))
    return out


def to_device_nhwc8(x_nhwc3: torch.Tensor, device="cuda", dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Plumbing for callers that already hold decoded float images: [B,H,W,3] float -> NHWC with the channel axis zero-padded
    to 8 (the layout vip_resize_bicubic_norm_f16 / _s32 emit), fp16 or - ``dtype=torch.float32``, the STRICT path - fp32."""
    B, H, W, Cc = x_nhwc3.shape
    dtype = dtype or torch.float16
    if dtype == PACKED:                     # the packed STRICT storage: pad in fp32, then split on the device
        return pack_h2(to_device_nhwc8(x_nhwc3, device, torch.float32))
    out = torch.zeros((B, H, W, 8), dtype=dtype, device=device)
    out[..., :Cc] = x_nhwc3.to(device=device, dtype=dtype)
    return out


def vit_tokens(patches, cls_token, pos_embed):
    """[B,NP,D] patches + cls [D] + pos [NP+1,D] -> [B,NP+1,D] (tfimm vit.py:419-426)."""
    kind = _kind(patches, "vit_tokens.patches")
    B, NP, D = patches.shape
    assert cls_token.numel() == D and pos_embed.numel() == (NP + 1) * D
    assert cls_token.dtype == pos_embed.dtype == patches.dtype, "vit_tokens: cls / pos must be stored in the activation dtype"
    out = torch.empty((B, NP + 1, D), dtype=patches.dtype, device=patches.device)
    _launch_kind("vit_tokens", kind, _p(patches), _p(cls_token), _p(pos_embed), _p(out), B, NP, D)
    return out


def cls_dense_f32(tokens, w_nc: torch.Tensor, bias: Optional[torch.Tensor]):
    """Dense head on token 0 of ``[B,N,D]`` (ViT ``head(norm(x)[:, 0])``) -> fp32 ``[B,classes]``."""
    kind = _kind(tokens, "cls_dense_f32.tokens")
    B, N, D = tokens.shape
    n_out = w_nc.shape[0]
    assert w_nc.dtype == torch.float32 and w_nc.shape == (n_out, D) and w_nc.is_contiguous()
    out = torch.empty((B, n_out), dtype=torch.float32, device=tokens.device)
    if kind != "f16":
        _launch_kind("gap_ln_dense", kind, _p(tokens), None, None, 0.0, _p(w_nc), _p(bias), _p(out), B, 1, D, D, N * D, n_out)
    else:
        _launch("vip_gap_dense_f32", _p(tokens), _p(w_nc), _p(bias), _p(out), B, 1, D, N * D, n_out)
    return out


def mul(a: torch.Tensor, b: torch.Tensor, c: int, a_off: int = 0, b_off: int = 0) -> torch.Tensor:
    """``a[..., a_off:a_off+c] * b[..., b_off:b_off+c]`` -> contiguous ``[..., c]`` (the operands are read in place as
    channel slices of their full tensors)."""
    kind = _kind(a, "mul.a")
    _chk_kind(b, kind, "mul.b")
    assert a.shape[:-1] == b.shape[:-1]
    rows = a.numel() // a.shape[-1]
    out = torch.empty((*a.shape[:-1], c), dtype=a.dtype, device=a.device)
    _launch_kind("mul", kind, _p(a), _p(b), _p(out), rows, c, a.shape[-1], a_off, b.shape[-1], b_off, c, 0)
    return out


def radix_combine(x, scale, radix: int = 2):
    """ResNeSt split-attention combine: x ``[B,H,W,radix*C]``, scale ``[B,radix*C]`` or on the fp16 storage split ``[B,2,radix*C]``
    -> ``[B,H,W,C]``."""
    B, H, W, RC = x.shape
    Cc = RC // radix
    kind = _kind(x, "radix_combine.x")
    _chk_kind(scale, kind, "radix_combine.scale")
    assert scale.shape == (B, RC) or (kind == "f16" and scale.shape == (B, 2, RC)), scale.shape
    out = torch.empty((B, H, W, Cc), dtype=x.dtype, device=x.device)
    if kind == "f16":       # this entry point alone takes the number of scale planes
        _launch("vip_radix_combine2_f16", _p(x), _p(scale), scale.dim() - 1, _p(out), B, H * W, Cc, radix)
    else:
        _launch_kind("radix_combine", kind, _p(x), _p(scale), _p(out), B, H * W, Cc, radix)
    return out


def global_local_filter(x, w3: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """HorNet ``global_local_filter`` between its two LayerNorms (kecam hornet.py:56-79) as one launch: x ``[B,H,W,S]``; channels
    ``[:S/2]`` through the 3x3 depthwise filter ``w3 [3,3,S/2]`` (zero padded, no bias), channels ``[S/2:]`` through the circular
    whole-map filter ``g [H,W,S/2]`` (``make_global_filter_weight``: rfft2 -> complex weight -> irfft2), interleaved channel by channel."""
    kind = _kind(x, "global_local_filter.x")
    B, H, W, S = x.shape
    _chk32(w3, "global_local_filter.w3")
    _chk32(g, "global_local_filter.g")
    if tuple(w3.shape) != (3, 3, S // 2) or tuple(g.shape) != (H, W, S // 2):
        raise _abi.VipError(f"global_local_filter: x {tuple(x.shape)} needs w3 (3, 3, {S // 2}) and g ({H}, {W}, {S // 2}), "
                            f"got {tuple(w3.shape)} and {tuple(g.shape)}")
    out = torch.empty_like(x)
    _launch_kind("global_local_filter_nhwc", kind, _p(x), _p(w3), _p(g), _p(out), B, H, W, S,
                 prof=lambda: ("global_local_filter_kernel", 2.0 * B * H * W * (S // 2) * (H * W + 9), 2.0 * x.numel() * x.element_size()))
    return out


def global_filter_plan(H: int, W: int, S: int):
    """dry run of ``global_local_filter``: (workgroups per image, channels of S per workgroup, LDS bytes), None when unsupported"""
    bc, lds = C.c_int(0), C.c_int(0)
    n = _abi.lib().vip_global_local_filter_plan(H, W, S, C.byref(bc), C.byref(lds))
    return (n, bc.value, lds.value) if n > 0 else None


def make_global_filter_weight(complex_weight: torch.Tensor, H: int, W: int, device="cuda", name: str = "complex_weight") -> torch.Tensor:
    """kecam ``ComplexDense`` weight ``[2, H, W // 2 + 1, half]`` (real, imaginary: hornet.py:34-42) -> the real circular filter
    ``g = irfft2(wr + j wi, s=(H, W))`` as fp32 ``[H, W, half]``, computed in float64 on the host:
    ``irfft2(rfft2(x) * Wc, s=(H, W))`` is the circular convolution of x with g.  ``irfft2`` is the numpy / pocketfft real inverse, which
    the reference's comments equate tf.signal.irfft2d to (hornet.py:69-70): the imaginary parts of the k = 0 column, and of the
    Nyquist column for even W, do not reach g.  A weight stored for another map size is refused - resizing it is the training side's
    ``load_resized_weights`` (hornet.py:44-50)."""
    cw = complex_weight.detach()
    if cw.dim() != 4 or cw.shape[0] != 2 or tuple(cw.shape[1:3]) != (H, W // 2 + 1):
        raise ValueError(f"{name}: stored for a map of {tuple(cw.shape[1:3])} (H, W // 2 + 1) frequencies, shape {tuple(cw.shape)}; "
                         f"this model's map is {H} x {W} and needs ({H}, {W // 2 + 1}) - resize the filter when the checkpoint is exported")
    wc = torch.complex(cw[0].to("cpu", torch.float64), cw[1].to("cpu", torch.float64))
    g = torch.fft.irfft2(wc, s=(H, W), dim=(0, 1))
    return g.to(torch.float32).contiguous().to(device)


SWIN_MAX_WS = 8


def swin_window_attention(qkv, v_bias, tau, bias_table, heads: int, ws: int, shift: int):
    """Swin V2 ``shifted_window_attention`` between its ``qkv`` and ``output`` Dense layers (kecam swin_transformer_v2.py:164-262) as
    one launch on the unpadded map: qkv ``[B,H,W,3C]`` (channels (q|k|v, head, 32), query / value bias already added) -> ``[B,H,W,C]``.
    ``v_bias`` fp32 ``[C]`` or None: the value of a padded token; ``tau`` fp32 ``[heads]`` (``swin_tau``); ``bias_table`` fp32
    ``[(2ws-1)^2, heads]`` (``make_swin_bias_table``); ``ws`` the window already clamped to the map, ``shift`` 0 or ``ws // 2``.
    Pad, roll, partition, mask, reverse, un-roll and crop are addressing inside the kernel (include/vipcup_hip.h has the formulas)."""
    kind = _kind(qkv, "swin_window_attention.qkv")
    B, H, W, C3 = qkv.shape
    Cc = C3 // 3
    _chk32(tau, "swin_window_attention.tau")
    _chk32(bias_table, "swin_window_attention.bias_table")
    if v_bias is not None:
        _chk32(v_bias, "swin_window_attention.v_bias")
    if C3 != 3 * Cc or tuple(tau.shape) != (heads,) or tuple(bias_table.shape) != ((2 * ws - 1) ** 2, heads) or \
            (v_bias is not None and tuple(v_bias.shape) != (Cc,)):
        raise _abi.VipError(f"swin_window_attention: qkv {tuple(qkv.shape)} with {heads} heads and ws {ws} needs tau ({heads},), bias_table "
                            f"({(2 * ws - 1) ** 2}, {heads}) and v_bias ({Cc},) or None, got {tuple(tau.shape)}, {tuple(bias_table.shape)}, "
                            f"{None if v_bias is None else tuple(v_bias.shape)}")
    out = torch.empty((B, H, W, Cc), dtype=qkv.dtype, device=qkv.device)

    def prof():
        nwh, N = B * (-(-H // ws)) * (-(-W // ws)) * heads, ws * ws
        return ("swin_attn_kernel", nwh * 4.0 * N * N * 32, B * H * W * 4.0 * Cc * 2,
                f"swin attn ws{ws} shift{shift} C={Cc} heads={heads} map={H}x{W}")
    _launch_kind("swin_attn_fwd", kind, _p(qkv), _p(v_bias), _p(tau), _p(bias_table), _p(out), B, H, W, Cc, heads, ws, shift,
                 prof=prof if kind == "f16" else None)
    return out


def swin_attn_plan(B: int, H: int, W: int, heads: int, ws: int, shift: int):
    """dry run of ``swin_window_attention``: (Hp, Wp, work items = B * windows * heads), None when the launch would be refused"""
    hp, wp, items = C.c_int(0), C.c_int(0), C.c_int(0)
    ok = _abi.lib().vip_swin_attn_plan(B, H, W, heads, ws, shift, C.byref(hp), C.byref(wp), C.byref(items))
    return (hp.value, wp.value, items.value) if ok == 1 else None


def swin_tau(scale_weight: torch.Tensor, device="cuda") -> torch.Tensor:
    """kecam ``ExpLogitScale`` (swin_transformer_v2.py:31-51): exp(min(weight, ln 100)) per head, float64 on the host -> fp32 ``[heads]``"""
    w = scale_weight.detach().to("cpu", torch.float64).reshape(-1)
    return torch.exp(torch.minimum(w, torch.log(torch.tensor(100.0, dtype=torch.float64)))).to(torch.float32).contiguous().to(device)


def make_swin_bias_table(meta1_kernel, meta1_bias, meta2_kernel, ws: int, pos_scale: int = -1, device="cuda") -> torch.Tensor:
    """The relative-position bias of ``window_mhsa_with_pair_wise_positional_embedding`` (swin_transformer_v2.py:60-108, :187-194) as
    the table the kernel indexes: fp32 ``[(2ws-1)^2, heads]``, row ``(dr + ws - 1)(2ws - 1) + (dc + ws - 1)`` for the offset (dr, dc) =
    query - key, ``16 sigmoid(meta_dense_2(relu(meta_dense_1(c))))`` with c = sign(o) log2(1 + |o|) / 3 and o = 8 (dr, dc) /
    (pos_scale - 1); ``pos_scale`` -1: the window itself.  Input-independent: float64 on the host, once per layer."""
    ps = float(ws if pos_scale == -1 else pos_scale)
    r = torch.arange(-ws + 1, ws, dtype=torch.float64)
    o = torch.stack(torch.meshgrid(r, r, indexing="ij"), -1).reshape(-1, 2) * 8.0 / (ps - 1.0)
    c = torch.sign(o) * torch.log(1.0 + o.abs()) / (torch.log(torch.tensor(2.0, dtype=torch.float64)) * 3.0)
    k1, b1, k2 = (t.detach().to("cpu", torch.float64) for t in (meta1_kernel, meta1_bias, meta2_kernel))
    t = torch.relu(c @ k1 + b1) @ k2
    return (16.0 * torch.sigmoid(t)).to(torch.float32).contiguous().to(device)


NAT_KERNEL_SIZES = (3, 5, 7)


def nat_attention(qkv, kv_pad, table, heads: int, kernel_size: int = 7):
    """kecam ``neighborhood_attention`` between its ``qkv`` and ``output`` Dense layers (nat/nat.py:65-116) as one launch on the unpadded
    map: qkv ``[B,H,W,3C]`` (channels (q|k|v, head, 32), the qkv Dense's output as it stands) -> ``[B,H,W,C]``.  Every query attends to
    the ``kernel_size`` x ``kernel_size`` block around it, clamped at the map's edge, under ``table`` fp32 ``[heads, (2K-1)^2]`` (the
    layer's ``positional_embedding``) indexed by the key-minus-query offset.  ``kv_pad`` fp32 ``[2C]`` or None (zeros): k | v of a padded
    token where the map is below the kernel - the k | v part of the qkv Dense's bias.  Patch extraction, replicate padding, the bias
    gather and the crop are addressing inside the kernel (include/vipcup_hip.h has the formulas)."""
    kind = _kind(qkv, "nat_attention.qkv")
    B, H, W, C3 = qkv.shape
    Cc = C3 // 3
    _chk32(table, "nat_attention.table")
    if kv_pad is not None:
        _chk32(kv_pad, "nat_attention.kv_pad")
    if C3 != 3 * Cc or tuple(table.shape) != (heads, (2 * kernel_size - 1) ** 2) or (kv_pad is not None and tuple(kv_pad.shape) != (2 * Cc,)):
        raise _abi.VipError(f"nat_attention: qkv {tuple(qkv.shape)} with {heads} heads and kernel_size {kernel_size} needs table "
                            f"({heads}, {(2 * kernel_size - 1) ** 2}) and kv_pad ({2 * Cc},) or None, got {tuple(table.shape)}, "
                            f"{None if kv_pad is None else tuple(kv_pad.shape)}")
    out = torch.empty((B, H, W, Cc), dtype=qkv.dtype, device=qkv.device)

    def prof():
        return ("nat_attn_kernel", B * H * W * heads * 4.0 * kernel_size ** 2 * 32, B * H * W * 4.0 * Cc * 2,
                f"nat attn k{kernel_size} C={Cc} heads={heads} map={H}x{W}")
    _launch_kind("nat_attn_fwd", kind, _p(qkv), _p(kv_pad), _p(table), _p(out), B, H, W, Cc, heads, kernel_size,
                 prof=prof if kind == "f16" else None)
    return out


def nat_attn_plan(B: int, H: int, W: int, heads: int, kernel_size: int = 7):
    """dry run of ``nat_attention``: (Hp, Wp, work items = B * 8 x 8 query tiles * heads), None when the launch would be refused"""
    hp, wp, items = C.c_int(0), C.c_int(0), C.c_int(0)
    ok = _abi.lib().vip_nat_attn_plan(B, H, W, heads, kernel_size, C.byref(hp), C.byref(wp), C.byref(items))
    return (hp.value, wp.value, items.value) if ok == 1 else None


def make_dw_weight(depthwise_kernel_hwc1: torch.Tensor, scale: Optional[torch.Tensor] = None, device="cuda") -> torch.Tensor:
    """Keras DepthwiseConv2D kernel ``[k,k,C,1]`` (optionally times a per-channel scale, e.g. a folded BN) ->
    fp32 ``[k,k,C]``.  Depthwise filters stay in fp32: with 9-49 taps per output a rounded filter is a systematic
    per-channel gain error, not noise that averages out (EfficientNet-B4: +6e-3 on the logit from this alone)."""
    w = depthwise_kernel_hwc1[..., 0].detach().to(torch.float32)
    if scale is not None:
        w = w * scale
    return w.contiguous().to(device)
