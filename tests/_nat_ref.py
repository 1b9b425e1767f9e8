"""TEST INFRASTRUCTURE - torch restatement (fp32 or fp64, whatever dtype it is handed) of the NAT graph, kecam nat/nat.py.  The attention
layer is written AS THE LAYER IS WRITTEN: zero-pad a map below the kernel, take the K x K patch of every VALID position, replicate the
first and last patch row / column K // 2 times, gather the position bias through the concatenated `bias_hh` / `bias_ww` ramps and the
reversal, softmax, crop - so it shares no addressing with csrc/nat_attn.hip, which folds all of that into index arithmetic.
`core(...)` is that layer between its `qkv` and `output` Dense layers on an explicit qkv map; `neighborhood_attention(...)` adds the two
Dense layers (and the zero padding BEFORE the qkv Dense) around it.  PARITY UNPINNED (TensorFlow is not importable here)."""
import math

import torch
import torch.nn.functional as F

LN_EPS = 1e-5


def ln(p, name, x):
    return F.layer_norm(x, x.shape[-1:], p[f"{name}/gamma"].to(x.dtype), p[f"{name}/beta"].to(x.dtype), LN_EPS)


def dense(p, name, x):
    y = x @ p[f"{name}/kernel"].to(x.dtype)
    b = p.get(f"{name}/bias")
    return y if b is None else y + b.to(x.dtype)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def bias_coords(height, width, size):
    """MultiHeadRelativePositionalKernelBias.build: [height * width, size^2] columns of `positional_embedding` for every position of the
    (padded) map - the ramp 0 .. size//2 - 1, the middle value repeated height - size + 1 times, the ramp up to size - 1, both ways,
    plus the in-block coordinate, the whole list REVERSED"""
    pos = 2 * size - 1
    idx = torch.arange(size)
    coords = (idx[:, None] * pos + idx[None, :]).reshape(-1)
    half = size // 2
    bias_hh = torch.cat([idx[:half], idx[half].repeat(height - size + 1), idx[half + 1:]])
    bias_ww = torch.cat([idx[:half], idx[half].repeat(width - size + 1), idx[half + 1:]])
    bias_hw = bias_hh[:, None] * pos + bias_ww[None, :]
    bc = (bias_hw[..., None] + coords).reshape(-1, size * size)
    return torch.flip(bc, [0])


def patches(kv, size):
    """extract_patches(sizes=size, strides=1, VALID) then the two replicate pads: [B, Hp, Wp, F] -> [B, Hp, Wp, size, size, F]"""
    B, Hp, Wp, Fc = kv.shape
    rows = torch.stack([kv[:, a:Hp - size + 1 + a] for a in range(size)], 3)                   # [B, Hp-size+1, Wp, size, F]
    pt = torch.stack([rows[:, :, b:Wp - size + 1 + b] for b in range(size)], 4)                # [B, Hp-size+1, Wp-size+1, size, size, F]
    r = (size - 1) // 2
    pt = torch.cat([pt[:, :1].repeat_interleave(r, 1), pt, pt[:, -1:].repeat_interleave(r, 1)], 1)
    return torch.cat([pt[:, :, :1].repeat_interleave(r, 2), pt, pt[:, :, -1:].repeat_interleave(r, 2)], 2)


def attend(qkv, table, heads, size):
    """nat.py:80-106 on a qkv map that already has the layer's padded size: [B, Hp, Wp, 3C] -> [B, Hp, Wp, C]"""
    B, Hp, Wp, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads
    q = qkv[..., :C].reshape(B, Hp * Wp, heads, 1, hd)
    kv = patches(qkv[..., C:], size).reshape(B, Hp * Wp, size * size, 2 * C)
    k = kv[..., :C].reshape(B, Hp * Wp, size * size, heads, hd).permute(0, 1, 3, 4, 2)         # [B, HW, heads, hd, KK]
    v = kv[..., C:].reshape(B, Hp * Wp, size * size, heads, hd).permute(0, 1, 3, 2, 4)         # [B, HW, heads, KK, hd]
    s = (q @ k) * (1.0 / (float(hd) ** 0.5))                                                   # [B, HW, heads, 1, KK]
    bias = table.to(qkv.dtype)[:, bias_coords(Hp, Wp, size)]                                   # [heads, HW, KK]
    s = s + bias.permute(1, 0, 2)[None, :, :, None, :]
    o = torch.softmax(s, -1) @ v                                                               # [B, HW, heads, 1, hd]
    return o.reshape(B, Hp, Wp, C)


def core(qkv_real, kv_pad, table, heads, size=7):
    """The layer between its two Dense layers, on an explicit map of REAL tokens: qkv_real [B, H, W, 3C].  A padded token enters the
    reference as a zero INPUT row, so its qkv row is the Dense's bias: the padding of this map holds (anything, kv_pad) - a padded token
    is never a query whose output survives the crop."""
    B, H, W, C3 = qkv_real.shape
    C = C3 // 3
    ph, pw = max(0, size - H), max(0, size - W)
    x = qkv_real
    if ph or pw:
        x = F.pad(qkv_real, (0, 0, 0, pw, 0, ph))
        if kv_pad is not None:
            fill = torch.cat([torch.zeros(C, dtype=x.dtype), kv_pad.to(x.dtype)])
            x[:, H:], x[:, :, W:] = fill, fill
    return attend(x, table, heads, size)[:, :H, :W]


def neighborhood_attention(p, name, x, heads, size):
    """nat.py:65-116 with the layer's own variables: zero-pad, qkv Dense, attention, crop, output Dense"""
    B, H, W, C = x.shape
    ph, pw = max(0, size - H), max(0, size - W)
    if ph or pw:
        x = F.pad(x, (0, 0, 0, pw, 0, ph))
    o = attend(dense(p, f"{name}qkv", x), p[f"{name}pos/positional_embedding"], heads, size)[:, :H, :W]
    return dense(p, f"{name}output", o)


def block(p, name, x, heads, size):
    a = neighborhood_attention(p, f"{name}attn_", ln(p, f"{name}attn_ln", x), heads, size)
    g1 = p.get(f"{name}1_gamma/weight")
    x = x + (a if g1 is None else a * g1.to(x.dtype))
    m = dense(p, f"{name}mlp_Dense_1", gelu(dense(p, f"{name}mlp_Dense_0", ln(p, f"{name}mlp_ln", x))))
    g2 = p.get(f"{name}2_gamma/weight")
    return x + (m if g2 is None else m * g2.to(x.dtype))


def conv3s2(p, name, x):
    """conv2d_no_bias(kernel_size=3, strides=2, padding="SAME") under its default use_torch_padding: ZeroPadding2D(1), then VALID"""
    k = p[f"{name}/kernel"].to(x.dtype).permute(3, 2, 0, 1)
    b = p.get(f"{name}/bias")
    y = F.conv2d(x.permute(0, 3, 1, 2), k, None if b is None else b.to(x.dtype), stride=2, padding=1)
    return y.permute(0, 2, 3, 1)


def forward_features(p, x, cfg, collect=None):
    """x [B, H, W, 3] -> the map the head pools (after pre_output_ln); `collect` receives each stack's output"""
    y = ln(p, "stem_ln", conv3s2(p, "stem_2_conv", conv3s2(p, "stem_1_conv", x)))
    for si, (nb, heads) in enumerate(zip(cfg["num_blocks"], cfg["num_heads"])):
        st = f"stack{si + 1}_"
        if si > 0:
            y = ln(p, f"{st}downsample_ln", conv3s2(p, f"{st}downsample_conv", y))
        for bi in range(nb):
            y = block(p, f"{st}block{bi + 1}_", y, heads, cfg["attn_kernel_size"])
        if collect is not None:
            collect.append(y)
    return ln(p, "pre_output_ln", y)


def forward_logits(p, x, cfg):
    return dense(p, "predictions", forward_features(p, x, cfg).mean((1, 2)))
