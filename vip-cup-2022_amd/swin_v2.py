"""Swin Transformer V2 on the HIP operator set - host-side mirror of kecam ``SwinTransformerV2``
(models/keras_cv_attention_models/swin_transformer_v2/swin_transformer_v2.py:298-347 the network, :265-279 the post-norm block,
:282-295 patch merging, :164-262 the shifted cosine window attention, :350-429 the twelve named constructors).

Layout: activations stay plain NHWC feature maps.  Everything between the ``qkv`` and ``output`` Dense layers of a block - zero padding
up to a multiple of the window, the half-window roll, window partition, cosine logits under the learned temperature, the
16 sigmoid(meta MLP) position bias, the -100 region mask, softmax, window reverse, un-roll and crop - is ONE launch,
``ops.swin_window_attention`` (csrc/swin_attn.hip), on the unpadded map.  The bias table and the temperature do not depend on the
input: they are built in float64 when the model is constructed.  The kernel serves windows up to 8 x 8; a stack whose clamped window
is larger (the window12 / 16 / 24 families at most input sizes) is refused by the constructor.
"""
from typing import Dict

import torch

from . import ops
from .cam import CamMixin, HeadSpec
from .pipeline import keras_predict
from .synth import ParamGen

LN_EPS = 1e-5          # common_layers.py:8,215-219
META_HIDDEN = 512      # swin_transformer_v2.py:165 meta_hidden_dim
MLP_RATIO = 4          # :266
PATCH = 4              # :304 stem_patch_size

_TINY = dict(num_blocks=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), embed_dim=96)
_SMALL = dict(num_blocks=(2, 2, 18, 2), num_heads=(3, 6, 12, 24), embed_dim=96)
_BASE = dict(num_blocks=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), embed_dim=128)
_LARGE = dict(num_blocks=(2, 2, 18, 2), num_heads=(6, 12, 24, 48), embed_dim=192)
# swin_transformer_v2.py:350-429.  ``pos_scale``: -1 (the window itself) as each constructor's default; the window16 / 24 base and large
# checkpoints fine-tuned from window12 ("imagenet22k") carry [12, 12, 12, 6] instead (:393, :402, :419, :428).  ``native_hw``: the
# constructor's default input size.
CONFIGS = {
    "swin_transformer_v2_tiny_window8": dict(_TINY, window_size=8, pos_scale=-1, native_hw=256),
    "swin_transformer_v2_tiny_window16": dict(_TINY, window_size=16, pos_scale=-1, native_hw=256),
    "swin_transformer_v2_small_window8": dict(_SMALL, window_size=8, pos_scale=-1, native_hw=256),
    "swin_transformer_v2_small_window16": dict(_SMALL, window_size=16, pos_scale=-1, native_hw=256),
    "swin_transformer_v2_base_window8": dict(_BASE, window_size=8, pos_scale=-1, native_hw=256),
    "swin_transformer_v2_base_window12": dict(_BASE, window_size=12, pos_scale=-1, native_hw=192),
    "swin_transformer_v2_base_window16": dict(_BASE, window_size=16, pos_scale=-1, native_hw=256),
    "swin_transformer_v2_base_window24": dict(_BASE, window_size=24, pos_scale=(12, 12, 12, 6), native_hw=384),
    "swin_transformer_v2_large_window12": dict(_LARGE, window_size=12, pos_scale=-1, native_hw=192),
    "swin_transformer_v2_large_window16": dict(_LARGE, window_size=16, pos_scale=(12, 12, 12, 6), native_hw=256),
    "swin_transformer_v2_large_window24": dict(_LARGE, window_size=24, pos_scale=(12, 12, 12, 6), native_hw=384),
}
# the twelfth constructor of the file is the generic one, under its own defaults (:298-313)
CONFIGS["swin_transformer_v2"] = dict(_TINY, window_size=7, pos_scale=-1, native_hw=224)


def stack_maps(input_hw, num_stacks: int = 4):
    """(H, W) of the feature map in each stack: the 4x4 stride-4 VALID stem (:318), then patch merging with an odd map padded by one
    row / column at the bottom / right (:284-287)"""
    h, w = (input_hw, input_hw) if isinstance(input_hw, int) else input_hw
    h, w = (h - PATCH) // PATCH + 1, (w - PATCH) // PATCH + 1
    out = [(h, w)]
    for _ in range(1, num_stacks):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def window_plan(window_size: int, hw, block_id: int):
    """(ws, shift) of a block (:216-220, :231, :334): the window clamped to the map, shift 0 in even blocks and int(ws * 0.5) in odd
    ones, forced to 0 when the clamped window covers the whole map.  Square maps and windows (rectangular windows are not built)."""
    h, w = hw
    if h != w:
        raise ValueError(f"SwinV2: a {h} x {w} map - only square inputs are built (rectangular windows are out of scope)")
    ws = min(window_size, h)
    shift = 0 if (block_id % 2 == 0 or ws == h) else int(ws * 0.5)
    return ws, shift


def _per_stack(v, si: int):
    return v[si] if isinstance(v, (list, tuple)) else v


def gmac_per_image(cfg: Dict, input_hw: int, classes: int = 1) -> float:
    """Algorithmic GMAC of one image, from the graph: stem 16*3*C per token; per block and token 3C^2 (qkv) + C^2 (output) + 8C^2 (MLP)
    and, per window and head, 2 * N^2 * 32 for the two attention products over the N = ws^2 slots of the PADDED map; patch merging
    4C * 2C per merged token; the head C * classes."""
    macs, c = 0.0, cfg["embed_dim"]
    maps = stack_maps(input_hw, len(cfg["num_blocks"]))
    macs += maps[0][0] * maps[0][1] * PATCH * PATCH * 3 * c
    for si, (nb, heads) in enumerate(zip(cfg["num_blocks"], cfg["num_heads"])):
        h, w = maps[si]
        if si > 0:
            macs += h * w * 4 * c * 2 * c
            c *= 2
        ws = min(cfg["window_size"], h)
        windows = (-(-h // ws)) * (-(-w // ws))
        macs += nb * (h * w * 12 * c * c + windows * heads * 2 * (ws * ws) ** 2 * 32)
    return (macs + c * classes) / 1e9


def synth_params(cfg: Dict, seed: int, classes: int = 1, input_hw=None) -> Dict[str, torch.Tensor]:
    """Synthetic checkpoint under the Keras variable names.  The two post-norm gammas of a block are drawn NON-ZERO (``zero_gamma=True``
    at :270,276 is only an initialiser - a zero gamma would leave every block dead) and the logit scale around ln 10 (:32,45).
    ``input_hw`` is accepted for symmetry with the other families; no variable of this graph depends on the input size."""
    g = ParamGen(seed)
    c = cfg["embed_dim"]
    g.conv("stem_conv", PATCH, PATCH, 3, c, bias=True, gain=1.0)
    g.ln("stem_ln", c)
    for si, (nb, heads) in enumerate(zip(cfg["num_blocks"], cfg["num_heads"])):
        st = f"stack{si + 1}_"
        if si > 0:
            g.dense(f"{st}downsample_dense", 4 * c, 2 * c, bias=False)
            c *= 2
            g.ln(f"{st}downsample_ln", c)
        for bi in range(nb):
            b = f"{st}block{bi + 1}_"
            g.dense(f"{b}attn_qkv", c, 3 * c, bias=False, gain=4.0)
            g.raw(f"{b}attn_query_bias/bias", g._n((c,), 0.3))
            g.raw(f"{b}attn_value_bias/bias", g._n((c,), 0.3))
            g.raw(f"{b}attn_scale/weight", g._n((1, heads, 1, 1), 0.3, 2.302585))          # ExpLogitScale(axis=1): [1, heads, 1, 1]
            g.dense(f"{b}attn_meta_dense_1", 2, META_HIDDEN, bias=True, gain=2.0)
            g.dense(f"{b}attn_meta_dense_2", META_HIDDEN, heads, bias=False, gain=4.0)
            g.dense(f"{b}attn_output", c, c)
            g.raw(f"{b}attn_ln/gamma", g._n((c,), 0.1, 0.5))
            g.raw(f"{b}attn_ln/beta", g._n((c,), 0.1))
            g.dense(f"{b}mlp_Dense_0", c, MLP_RATIO * c, gain=2.0)
            g.dense(f"{b}mlp_Dense_1", MLP_RATIO * c, c)
            g.raw(f"{b}mlp_ln/gamma", g._n((c,), 0.1, 0.5))
            g.raw(f"{b}mlp_ln/beta", g._n((c,), 0.1))
    g.ln("pre_output_ln", c)
    g.dense("predictions", c, classes)
    return g.p


def merge_conv_kernel(dense_kernel: torch.Tensor) -> torch.Tensor:
    """Patch merging's Dense kernel ``[4C, 2C]`` as the HWIO kernel ``[2, 2, C, 2C]`` of a 2x2 stride-2 convolution.  The reference's
    reshape / transpose / reshape (:290-292) lays the four pixels of a 2x2 patch out as channels in the order (dx, dy, c) - the COLUMN
    offset is the slow axis - so conv tap (dy, dx) takes the Dense rows (2 * dx + dy) * C + c."""
    c4, cout = dense_kernel.shape
    c = c4 // 4
    k = dense_kernel.reshape(2, 2, c, cout)           # [dx, dy, c, out]
    return k.permute(1, 0, 2, 3).contiguous()         # [dy, dx, c, out]


class _LN:
    def __init__(self, p, name, dev):
        self.g = p[f"{name}/gamma"].to(dev, torch.float32).contiguous()
        self.b = p[f"{name}/beta"].to(dev, torch.float32).contiguous()

    def __call__(self, x):
        return ops.layernorm(x, self.g, self.b, LN_EPS)


@keras_predict
class SwinV2(CamMixin):
    def __init__(self, params: Dict[str, torch.Tensor], num_blocks, num_heads, embed_dim, window_size, pos_scale=-1, input_hw=256,
                 classes: int = 1, classifier_activation: str = "default", device="cuda", native_hw=None):
        """``input_hw`` (an int or (H, W)) fixes each stack's map and with it the clamped window, the shift and the bias table of every
        block; ``native_hw`` (the reference constructor's default size) is documentation only."""
        p, dev = params, device
        self.classes, self.head_act = classes, classifier_activation
        self.maps = stack_maps(input_hw, len(num_blocks))
        for si, hw in enumerate(self.maps):
            ws = min(window_size, hw[0])
            if ws > ops.SWIN_MAX_WS:
                raise ValueError(f"SwinV2: stack{si + 1} runs {ws} x {ws} windows on its {hw[0]} x {hw[1]} map (window_size {window_size}); "
                                 f"the attention kernel serves windows up to {ops.SWIN_MAX_WS} x {ops.SWIN_MAX_WS}")
        self.stem = ops.make_conv_weight(p["stem_conv/kernel"], p["stem_conv/bias"], device=dev, pad_cin_to=8)
        self.stem_ln = _LN(p, "stem_ln", dev)
        self.stages = []
        c = embed_dim
        for si, (nb, heads) in enumerate(zip(num_blocks, num_heads)):
            st = f"stack{si + 1}_"
            down = None
            if si > 0:
                down = (ops.make_conv_weight(merge_conv_kernel(p[f"{st}downsample_dense/kernel"]), None, device=dev),
                        _LN(p, f"{st}downsample_ln", dev))
                c *= 2
            if c != heads * 32:
                raise ValueError(f"SwinV2: stack{si + 1} has {c} channels on {heads} heads; the attention kernel needs head_dim 32")
            blocks = []
            for bi in range(nb):
                b = f"{st}block{bi + 1}_"
                ws, shift = window_plan(window_size, self.maps[si], bi)
                qb, vb = p.get(f"{b}attn_query_bias/bias"), p.get(f"{b}attn_value_bias/bias")
                # the qkv Dense has no bias of its own (:171); query_bias and value_bias (:174-176) become its bias (q, 0, v)
                bias = None if qb is None else torch.cat([qb.reshape(-1), torch.zeros(c), vb.reshape(-1)]).to(torch.float32)
                blocks.append(dict(
                    heads=heads, ws=ws, shift=shift, hw=tuple(self.maps[si]),
                    qkv=ops.make_dense_weight(p[f"{b}attn_qkv/kernel"], bias, dev),
                    v_bias=None if vb is None else vb.reshape(-1).to(dev, torch.float32).contiguous(),
                    tau=ops.swin_tau(p[f"{b}attn_scale/weight"], dev),
                    table=ops.make_swin_bias_table(p[f"{b}attn_meta_dense_1/kernel"], p[f"{b}attn_meta_dense_1/bias"],
                                                   p[f"{b}attn_meta_dense_2/kernel"], ws, _per_stack(pos_scale, si), dev),
                    out=ops.make_dense_weight(p[f"{b}attn_output/kernel"], p.get(f"{b}attn_output/bias"), dev),
                    ln1=_LN(p, f"{b}attn_ln", dev), ln2=_LN(p, f"{b}mlp_ln", dev),
                    fc1=ops.make_dense_weight(p[f"{b}mlp_Dense_0/kernel"], p[f"{b}mlp_Dense_0/bias"], dev),
                    fc2=ops.make_dense_weight(p[f"{b}mlp_Dense_1/kernel"], p[f"{b}mlp_Dense_1/bias"], dev)))
            self.stages.append((down, blocks))
        self.head_ln = _LN(p, "pre_output_ln", dev)
        self.head_w = p["predictions/kernel"].t().contiguous().to(dev, torch.float32)
        self.head_b = p["predictions/bias"].to(dev, torch.float32)

    @staticmethod
    def _block(x, blk):
        """post-norm (:265-279): x + LN(attn(x)), then x + LN(mlp(x)); each LayerNorm is its own launch, then the residual add"""
        if tuple(x.shape[1:3]) != blk["hw"]:
            raise ValueError(f"SwinV2: built for a {blk['hw'][0]} x {blk['hw'][1]} map in this stack, got {x.shape[1]} x {x.shape[2]}: "
                             "construct the model with the input size it is fed (input_hw)")
        att = ops.swin_window_attention(ops.dense(x, blk["qkv"]), blk["v_bias"], blk["tau"], blk["table"], blk["heads"], blk["ws"],
                                        blk["shift"])
        x = ops.scale_add_act(blk["ln1"](ops.dense(att, blk["out"])), residual=x)
        return ops.scale_add_act(blk["ln2"](ops.mlp(x, blk["fc1"], blk["fc2"], act="gelu", ln=None)), residual=x)

    def features(self, x, collect=None):
        """x: NHWC, RGB padded to 8 channels -> the map the head pools (after pre_output_ln)"""
        assert x.shape[-1] == 8
        y = self.stem_ln(ops.conv2d(x, self.stem, stride=PATCH))
        for down, blocks in self.stages:
            if down is not None:                      # patch merging (:282-295) as a 2x2 stride-2 convolution, an odd map padded
                y = down[1](ops.conv2d(y, down[0], stride=2, pad=(0, y.shape[1] % 2, 0, y.shape[2] % 2)))
            for blk in blocks:
                y = self._block(y, blk)
            if collect is not None:
                collect.append(y)
        return self.head_ln(y)

    def head_spec(self) -> HeadSpec:
        """pre_output_ln -> avg_pool -> Dense (:341-343): the LayerNorm is per position, BEFORE the pool, so it belongs to the features"""
        return HeadSpec(self.head_w, self.head_b, None, getattr(self, "head_act", "default"))

    def logits(self, x):
        return ops.gap_dense_f32(self.features(x), self.head_w, self.head_b)

    def predict(self, x):
        return ops.head_prob(self.logits(x), getattr(self, "head_act", "default"))
