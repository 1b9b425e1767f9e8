"""Neighbourhood Attention Transformer on the HIP operator set - host-side mirror of kecam ``NAT``
(models/keras_cv_attention_models/nat/nat.py:135-179 the network, :119-132 the pre-norm block, :65-116 the neighbourhood attention,
:24-62 its position bias, :182-207 the four named constructors).

Layout: activations stay plain NHWC feature maps.  Everything between the ``qkv`` and ``output`` Dense layers of a block - the K x K
patch of every position, the replicate padding that clamps the patches at the map's edge, the gathered position bias, softmax and the
crop - is ONE launch, ``ops.nat_attention`` (csrc/nat_attn.hip), on the unpadded map.  Where a stack's map is below the kernel the layer
zero-pads the LayerNorm output BEFORE the qkv Dense (:74-77): a padded token is a real key whose k | v is the Dense's bias, handed to the
operator as ``kv_pad``.  ``attn_ln`` runs inside the qkv Dense (``ops.ln_dense``), ``mlp_ln`` inside the MLP; the layer scales of
``NAT_Small`` / ``NAT_Base`` are folded into the ``output`` Dense and the second MLP Dense.

The 3 x 3 stride-2 convolutions (two in the stem, one per downsampling) are ``conv2d_no_bias(..., padding="SAME")`` under its default
``use_torch_padding``: ZeroPadding2D(1) on every side, then a VALID convolution (common_layers.py:230-235) - pad (1, 1, 1, 1) on even and
odd maps alike, not TensorFlow's own SAME split.
"""
from typing import Dict

import torch

from . import ops
from .cam import CamMixin, HeadSpec
from .pipeline import keras_predict
from .synth import ParamGen

LN_EPS = 1e-5          # common_layers.py:8,215-219

_D = dict(out_channels=(64, 128, 256, 512), num_heads=(2, 4, 8, 16), attn_kernel_size=7, mlp_ratio=3, layer_scale=-1, native_hw=224)
# nat.py:182-207; ``native_hw``: the constructor's default input size.  ``layer_scale`` >= 0: the blocks carry 1_gamma / 2_gamma.
CONFIGS = {
    "nat_mini": dict(_D, num_blocks=(3, 4, 6, 5)),
    "nat_tiny": dict(_D, num_blocks=(3, 4, 18, 5)),
    "nat_small": dict(_D, num_blocks=(3, 4, 18, 5), num_heads=(3, 6, 12, 24), out_channels=(96, 192, 384, 768), mlp_ratio=2, layer_scale=1e-5),
    "nat_base": dict(_D, num_blocks=(3, 4, 18, 5), num_heads=(4, 8, 16, 32), out_channels=(128, 256, 512, 1024), mlp_ratio=2, layer_scale=1e-5),
}
# the fifth constructor of the file is the generic one, under its own defaults (:135-151)
CONFIGS["nat"] = dict(_D, num_blocks=(3, 4, 6, 5))

SAME_PAD = (1, 1, 1, 1)


def stack_maps(input_hw, num_stacks: int = 4):
    """(H, W) of the feature map in each stack: two 3 x 3 stride-2 convolutions in the stem, one in front of every later stack, each
    (n + 2 - 3) // 2 + 1 = (n + 1) // 2"""
    h, w = (input_hw, input_hw) if isinstance(input_hw, int) else input_hw
    h, w = (h + 1) // 2, (w + 1) // 2
    out = []
    for _ in range(num_stacks):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def gmac_per_image(cfg: Dict, input_hw, classes: int = 1) -> float:
    """Algorithmic GMAC of one image, from the graph: the stem's two convolutions 9*3*(C/2) and 9*(C/2)*C per output position; per block
    and token (4 + 2 r) C^2 for the four Dense layers and 2 K^2 C for the two attention products; 9 C_in C_out per downsampled token;
    the head C * classes."""
    chans, k2 = cfg["out_channels"], cfg["attn_kernel_size"] ** 2
    h, w = (input_hw, input_hw) if isinstance(input_hw, int) else input_hw
    maps = stack_maps(input_hw, len(cfg["num_blocks"]))
    c0 = chans[0]
    macs = ((h + 1) // 2) * ((w + 1) // 2) * 27.0 * (c0 // 2) + maps[0][0] * maps[0][1] * 9.0 * (c0 // 2) * c0
    for si, nb in enumerate(cfg["num_blocks"]):
        hw, c = maps[si][0] * maps[si][1], chans[si]
        if si > 0:
            macs += hw * 9.0 * chans[si - 1] * c
        macs += nb * hw * ((4 + 2 * cfg["mlp_ratio"]) * c * c + 2 * k2 * c)
    return (macs + chans[-1] * classes) / 1e9


def synth_params(cfg: Dict, seed: int, classes: int = 1, input_hw=None) -> Dict[str, torch.Tensor]:
    """Synthetic checkpoint under the Keras variable names.  The layer scales are drawn as TRAINED ones (the 1e-5 initialiser would mute
    every block), the position table at ten times its 0.02 initialiser so that it moves the softmax.  ``input_hw`` is accepted for
    symmetry with the other families; no variable of this graph depends on the input size."""
    g = ParamGen(seed)
    chans, K = cfg["out_channels"], cfg["attn_kernel_size"]
    g.conv("stem_1_conv", 3, 3, 3, chans[0] // 2, bias=True, gain=1.0)
    g.conv("stem_2_conv", 3, 3, chans[0] // 2, chans[0], bias=True, gain=1.0)
    g.ln("stem_ln", chans[0])
    for si, (nb, heads) in enumerate(zip(cfg["num_blocks"], cfg["num_heads"])):
        st, c = f"stack{si + 1}_", chans[si]
        if si > 0:
            g.conv(f"{st}downsample_conv", 3, 3, chans[si - 1], c, bias=False, gain=1.0)
            g.ln(f"{st}downsample_ln", c)
        for bi in range(nb):
            b = f"{st}block{bi + 1}_"
            g.ln(f"{b}attn_ln", c)
            g.dense(f"{b}attn_qkv", c, 3 * c, gain=4.0)
            g.raw(f"{b}attn_pos/positional_embedding", g._n((heads, (2 * K - 1) ** 2), 0.2))
            g.dense(f"{b}attn_output", c, c)
            g.ln(f"{b}mlp_ln", c)
            g.dense(f"{b}mlp_Dense_0", c, int(c * cfg["mlp_ratio"]), gain=2.0)
            g.dense(f"{b}mlp_Dense_1", int(c * cfg["mlp_ratio"]), c)
            if cfg["layer_scale"] >= 0:
                g.raw(f"{b}1_gamma/weight", g._u((c,), 0.1, 0.4))
                g.raw(f"{b}2_gamma/weight", g._u((c,), 0.1, 0.4))
    g.ln("pre_output_ln", chans[-1])
    g.dense("predictions", chans[-1], classes)
    return g.p


class _LN:
    def __init__(self, p, name, dev):
        self.g = p[f"{name}/gamma"].to(dev, torch.float32).contiguous()
        self.b = p[f"{name}/beta"].to(dev, torch.float32).contiguous()

    def __call__(self, x):
        return ops.layernorm(x, self.g, self.b, LN_EPS)

    @property
    def args(self):
        return (self.g, self.b, LN_EPS)


@keras_predict
class NAT(CamMixin):
    def __init__(self, params: Dict[str, torch.Tensor], num_blocks, out_channels, num_heads, attn_kernel_size=7, mlp_ratio=3, layer_scale=-1,
                 input_hw=224, classes: int = 1, classifier_activation: str = "default", device="cuda", native_hw=None):
        """``input_hw`` (an int or (H, W)) fixes each stack's map and with it whether its blocks pad; ``native_hw`` (the reference
        constructor's default size) is documentation only."""
        p, dev = params, device
        self.classes, self.head_act = classes, classifier_activation
        self.maps = stack_maps(input_hw, len(num_blocks))
        K = attn_kernel_size
        if K not in ops.NAT_KERNEL_SIZES:
            raise ValueError(f"NAT: attn_kernel_size {K}; the attention kernel serves {ops.NAT_KERNEL_SIZES}")
        self.stem1 = ops.make_conv_weight(p["stem_1_conv/kernel"], p["stem_1_conv/bias"], device=dev, pad_cin_to=8)
        self.stem2 = ops.make_conv_weight(p["stem_2_conv/kernel"], p["stem_2_conv/bias"], device=dev)
        self.stem_ln = _LN(p, "stem_ln", dev)
        self.stages = []
        for si, (nb, heads) in enumerate(zip(num_blocks, num_heads)):
            st, c = f"stack{si + 1}_", out_channels[si]
            down = None
            if si > 0:
                down = (ops.make_conv_weight(p[f"{st}downsample_conv/kernel"], None, device=dev), _LN(p, f"{st}downsample_ln", dev))
            if c != heads * 32:
                raise ValueError(f"NAT: stack{si + 1} has {c} channels on {heads} heads; the attention kernel needs head_dim 32")
            pads = self.maps[si][0] < K or self.maps[si][1] < K
            blocks = []
            for bi in range(nb):
                b = f"{st}block{bi + 1}_"
                qb = p.get(f"{b}attn_qkv/bias")
                g1, g2 = p.get(f"{b}1_gamma/weight"), p.get(f"{b}2_gamma/weight")
                one = torch.ones(c)
                g1, g2 = (one if g1 is None else g1.reshape(-1)), (one if g2 is None else g2.reshape(-1))
                blocks.append(dict(
                    heads=heads, K=K, hw=tuple(self.maps[si]),
                    ln1=_LN(p, f"{b}attn_ln", dev), ln2=_LN(p, f"{b}mlp_ln", dev),
                    qkv=ops.make_dense_weight(p[f"{b}attn_qkv/kernel"], qb, dev),
                    # a padded token's k | v: the qkv Dense of a zero row is its bias (:74-79)
                    kv_pad=(qb[c:].to(dev, torch.float32).contiguous() if (pads and qb is not None) else None),
                    table=p[f"{b}attn_pos/positional_embedding"].to(dev, torch.float32).contiguous(),
                    # ChannelAffine layer scales (:124,130) folded into the columns of each branch's last Dense
                    out=ops.make_dense_weight(p[f"{b}attn_output/kernel"] * g1[None, :], p[f"{b}attn_output/bias"] * g1, dev),
                    fc1=ops.make_dense_weight(p[f"{b}mlp_Dense_0/kernel"], p[f"{b}mlp_Dense_0/bias"], dev),
                    fc2=ops.make_dense_weight(p[f"{b}mlp_Dense_1/kernel"] * g2[None, :], p[f"{b}mlp_Dense_1/bias"] * g2, dev)))
            self.stages.append((down, blocks))
        self.head_ln = _LN(p, "pre_output_ln", dev)
        self.head_w = p["predictions/kernel"].t().contiguous().to(dev, torch.float32)
        self.head_b = p["predictions/bias"].to(dev, torch.float32)

    @staticmethod
    def _block(x, blk):
        """pre-norm (:119-132): x + gamma1 attn(LN(x)), then x + gamma2 mlp(LN(x))"""
        if tuple(x.shape[1:3]) != blk["hw"]:
            raise ValueError(f"NAT: built for a {blk['hw'][0]} x {blk['hw'][1]} map in this stack, got {x.shape[1]} x {x.shape[2]}: "
                             "construct the model with the input size it is fed (input_hw)")
        att = ops.nat_attention(ops.ln_dense(x, blk["ln1"].args, blk["qkv"]), blk["kv_pad"], blk["table"], blk["heads"], blk["K"])
        x = ops.dense(att, blk["out"], residual=x)
        return ops.mlp(x, blk["fc1"], blk["fc2"], act="gelu", residual=x, ln=blk["ln2"].args)

    def features(self, x, collect=None):
        """x: NHWC, RGB padded to 8 channels -> the map the head pools (after pre_output_ln)"""
        assert x.shape[-1] == 8
        y = ops.conv2d(ops.conv2d(x, self.stem1, stride=2, pad=SAME_PAD), self.stem2, stride=2, pad=SAME_PAD)
        y = self.stem_ln(y)
        for down, blocks in self.stages:
            if down is not None:
                y = down[1](ops.conv2d(y, down[0], stride=2, pad=SAME_PAD))
            for blk in blocks:
                y = self._block(y, blk)
            if collect is not None:
                collect.append(y)
        return self.head_ln(y)

    def head_spec(self) -> HeadSpec:
        """pre_output_ln -> avg_pool -> Dense (:173-175): the LayerNorm is per position, BEFORE the pool, so it belongs to the features"""
        return HeadSpec(self.head_w, self.head_b, None, getattr(self, "head_act", "default"))

    def logits(self, x):
        return ops.gap_dense_f32(self.features(x), self.head_w, self.head_b)

    def predict(self, x):
        return ops.head_prob(self.logits(x), getattr(self, "head_act", "default"))
