"""TEST INFRASTRUCTURE - fp32 CPU restatement of the HorNet-GF graph (kecam hornet/hornet.py:53-81 global_local_filter, :84-104 gnconv
with use_global_local_filter, :183-218 the GF constructors).  The plain layers are oracle.hornet_ref's and oracle.ops_ref's, imported; what
is added is the GF branch, with torch.fft on the CPU as the reference writes it: rfft2 -> complex weight -> irfft2 on the second half of
the channels, a bias-free 3x3 depthwise convolution on the first, concat on a new last axis + reshape.  PARITY UNPINNED like hornet_ref
(TensorFlow is not importable here): irfft2 is the numpy / pocketfft real inverse the reference's comments equate tf.signal.irfft2d to."""
import torch

from oracle import hornet_ref as HR
from oracle import ops_ref as R


def per_stack(v, n=4):
    return tuple(v) if isinstance(v, (list, tuple)) else (v,) * n


def global_local_filter(p, name, x):
    """hornet.py:53-81; x [B,H,W,S] fp32"""
    B, H, W, S = x.shape
    nn = HR._ln(p, f"{name}pre_ln", x)
    dw, ff = nn[..., :S // 2], nn[..., S // 2:]
    dw = R.dwconv2d(dw, p[f"{name}dw_conv/depthwise_kernel"], None, 1, (1, 1, 1, 1))
    cw = p[f"{name}complex_dense/complex_weight"]
    ff = torch.fft.rfft2(ff, dim=(1, 2)) * torch.complex(cw[0], cw[1])
    ff = torch.fft.irfft2(ff, s=(H, W), dim=(1, 2))
    out = torch.cat([dw.unsqueeze(-1), ff.unsqueeze(-1)], -1).reshape(B, H, W, S)
    return HR._ln(p, f"{name}post_ln", out)


def gnconv(p, name, x, gn_split, scale, use_gf):
    if not use_gf:
        return HR.gnconv(p, name, x, gn_split, scale)
    c = x.shape[-1]
    nn = HR._conv(p, f"{name}pre_conv", x)
    dims = [c // (2 ** i) for i in range(gn_split)][::-1]
    pw_first, dw_list = nn[..., :dims[0]], nn[..., dims[0]:]
    dw_list = global_local_filter(p, f"{name}gf_", dw_list) * scale
    parts = torch.split(dw_list, dims, dim=-1)
    nn = pw_first * parts[0]
    for i, dw in enumerate(parts[1:], start=1):
        nn = HR._conv(p, f"{name}pw{i}_conv", nn) * dw
    return HR._conv(p, f"{name}output_conv", nn)


def block(p, name, x, gn_split, scale, use_gf):
    a = gnconv(p, f"{name}gnconv_", HR._ln(p, f"{name}attn_ln", x), gn_split, scale, use_gf)
    x = x + a * p[f"{name}1_gamma/weight"]
    m = HR._ln(p, f"{name}mlp_ln", x)
    m = R.act(R.dense(m, p[f"{name}mlp_Dense_0/kernel"], p[f"{name}mlp_Dense_0/bias"]), "gelu")
    m = R.dense(m, p[f"{name}mlp_Dense_1/kernel"], p[f"{name}mlp_Dense_1/bias"])
    return x + m * p[f"{name}2_gamma/weight"]


def forward_features(p, x, cfg, first_strides=2, collect=None):
    use_gf = per_stack(cfg.get("use_global_local_filter", False), len(cfg["num_blocks"]))
    x = HR._ln(p, "stem_ln", HR._conv(p, "stem_conv", x, first_strides * 2))
    for si, nb in enumerate(cfg["num_blocks"]):
        st = f"stack{si + 1}_"
        if si > 0:
            x = HR._conv(p, f"{st}conv", HR._ln(p, f"{st}ln", x), 2)
        for bi in range(nb):
            x = block(p, f"{st}block{bi + 1}_", x, cfg["gn_split"][si], cfg["scale"], use_gf[si])
        if collect is not None:
            collect.append(x)
    return x


def forward_logits(p, x, cfg, first_strides=2):
    v = HR._ln(p, "pre_output_ln", R.global_avgpool(forward_features(p, x, cfg, first_strides)))
    return R.dense(v, p["predictions/kernel"], p["predictions/bias"])
