"""TEST INFRASTRUCTURE - torch restatement (fp32 or fp64, whatever dtype it is handed) of the Swin Transformer V2 graph, kecam
swin_transformer_v2/swin_transformer_v2.py.  The attention layer is written AS THE LAYER IS WRITTEN: zero-pad the map to a multiple
of the window, roll it with two cats, partition into windows, cosine attention with the position-bias MLP gathered through the
pairwise index and the [windows, N, N] mask TENSOR, reverse, un-roll, crop - so it shares no addressing with csrc/swin_attn.hip,
which folds all of that into index arithmetic.  `core(...)` is that layer between its `qkv` and `output` Dense layers on an explicit
qkv map; `window_attention(...)` adds the two Dense layers around it.  PARITY UNPINNED (TensorFlow is not importable here)."""
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


def l2_normalize(x, dim, eps=1e-6):
    """tf.nn.l2_normalize: x * rsqrt(max(sum x^2, eps))"""
    return x * torch.rsqrt(torch.clamp((x * x).sum(dim, keepdim=True), min=eps))


def tau_of(scale_weight):
    """ExpLogitScale.call: exp(min(weight, ln max_value))"""
    w = scale_weight.reshape(-1)
    return torch.exp(torch.minimum(w, torch.log(torch.tensor(100.0, dtype=w.dtype))))


def pairwise_index(wh, ww):
    """__build_pairwise_relative_position_index__: [N, N] rows of the bias table, with the layer's default "xy" meshgrid"""
    hh, ww_ = torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing="xy")
    coords = torch.stack([hh, ww_], -1).reshape(-1, 2)
    rel = coords[:, None, :] - coords[None, :, :]
    return (rel[..., 0] + wh - 1) + (rel[..., 1] + ww - 1) * (2 * wh - 1)


def gathered(table, wh, ww):
    """a bias table [(2wh-1)(2ww-1), heads] -> [heads, N, N] through the layer's pairwise index"""
    return table[pairwise_index(wh, ww)].permute(2, 0, 1)


def position_bias(k1, b1, k2, wh, ww, pos_scale=-1):
    """PairWiseRelativePositionalEmbedding + the meta MLP + gather: [heads, N, N], N = wh * ww, exactly in the reference's own index
    conventions (a meshgrid with the default "xy" indexing for the pairwise index, "ij" for the coordinate table)."""
    dt = k1.dtype
    index = pairwise_index(wh, ww)
    th, tw = torch.meshgrid(torch.arange(-wh + 1, wh), torch.arange(-ww + 1, ww), indexing="ij")
    table = torch.stack([th, tw], -1).to(dt)
    ps = [wh, ww] if pos_scale == -1 else ([pos_scale, pos_scale] if not isinstance(pos_scale, (list, tuple)) else list(pos_scale))
    table = table * 8 / torch.tensor([float(ps[0] - 1), float(ps[1] - 1)], dtype=dt)
    logc = (torch.sign(table) * torch.log(1.0 + table.abs()) / (math.log(2.0) * 3.0)).reshape(-1, 2)
    bias = torch.relu(logc @ k1 + b1) @ k2                      # [(2wh-1)(2ww-1), heads]
    bias = torch.sigmoid(bias[index]) * 16.0                    # [N, N, heads]
    return bias.permute(2, 0, 1)


def region_map(height, width, wh, ww, sh, sw):
    """WindowAttentionMask.build, first half: the nine-region label of every slot, [windows, N]"""
    hs, wsp = [0, height - wh, height - sh, height], [0, width - ww, width - sw, width]
    rows, val = [], 0
    for i in range(3):
        rows.append(torch.cat([torch.zeros(hs[i + 1] - hs[i], wsp[j + 1] - wsp[j]) + (j + val) for j in range(3)], -1))
        val += 3
    m = torch.cat(rows, 0)
    return m.reshape(height // wh, wh, width // ww, ww).permute(0, 2, 1, 3).reshape(-1, wh * ww)


def attention_mask(height, width, wh, ww, sh, sw, dtype):
    """WindowAttentionMask.build: [windows, N, N] of 0 / -100"""
    m = region_map(height, width, wh, ww, sh, sw)
    d = m[:, None, :] - m[:, :, None]
    return torch.where(d != 0, torch.tensor(-100.0), torch.tensor(0.0)).to(dtype)


def windowed(x, window_size, shift_size, attend, fill=None):
    """shifted_window_attention around `attend` ([windows * B, wh, ww, C], mask or None, (wh, ww)) -> the same shape with C_out.
    `fill` [C]: what the padding holds instead of zeros (core(): the qkv row of a zero input row)."""
    B, H, W, C = x.shape
    wh, ww = min(window_size, H), min(window_size, W)
    if wh == H and ww == W:
        shift_size = 0
    ph, pw = -(-H // wh), -(-W // ww)
    pad_h, pad_w = ph * wh - H, pw * ww - W
    if pad_h or pad_w:
        x = F.pad(x, (0, 0, 0, pad_w, 0, pad_h))
        if fill is not None:
            x[:, H:], x[:, :, W:] = fill, fill
    sh = sw = 0
    if shift_size > 0:
        sh, sw = int(wh * shift_size), int(ww * shift_size)
        x = torch.cat([x[:, sh:], x[:, :sh]], 1)
        x = torch.cat([x[:, :, sw:], x[:, :, :sw]], 2)
    Hp, Wp = x.shape[1:3]
    nn = x.reshape(B, ph, wh, pw, ww, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, wh, ww, C)
    mask = attention_mask(Hp, Wp, wh, ww, sh, sw, x.dtype) if shift_size > 0 else None
    nn = attend(nn, mask, (wh, ww))
    Co = nn.shape[-1]
    nn = nn.reshape(B, ph, pw, wh, ww, Co).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, Co)
    if shift_size > 0:
        nn = torch.cat([nn[:, -sh:], nn[:, :-sh]], 1)
        nn = torch.cat([nn[:, :, -sw:], nn[:, :, :-sw]], 2)
    return nn[:, :H, :W]


def cosine_attention(q, k, v, tau, bias, mask, heads):
    """q, k, v [G, N, C] -> [G, N, C]; tau [heads]; bias [heads, N, N]; mask [windows, N, N] or None (G = B * windows, window fastest)"""
    G, N, C = q.shape
    hd = C // heads
    q, k, v = (t.reshape(G, N, heads, hd).permute(0, 2, 1, 3) for t in (q, k, v))
    attn = l2_normalize(q, -1) @ l2_normalize(k, -1).transpose(-1, -2)
    attn = attn * tau.reshape(1, heads, 1, 1) + bias[None]
    if mask is not None:
        nw = mask.shape[0]
        attn = (attn.reshape(G // nw, nw, heads, N, N) + mask[None, :, None]).reshape(G, heads, N, N)
    out = torch.softmax(attn, -1) @ v
    return out.permute(0, 2, 1, 3).reshape(G, N, C)


def core(qkv_real, v_bias, q_bias, tau, table_fn, heads, window_size, shift_size):
    """The layer between its two Dense layers, on an explicit map of REAL tokens: qkv_real [B, H, W, 3C] holds q (query_bias included), k
    and v (value_bias included) of the real tokens.  A padded token enters the reference as a zero INPUT row, so its q = query_bias, k = 0
    and v = value_bias: that is what the padding of this map is filled with.  table_fn(wh, ww) -> bias [heads, N, N]."""
    B, H, W, C3 = qkv_real.shape
    C = C3 // 3
    fill = torch.cat([q_bias if q_bias is not None else torch.zeros(C, dtype=qkv_real.dtype), torch.zeros(C, dtype=qkv_real.dtype),
                      v_bias if v_bias is not None else torch.zeros(C, dtype=qkv_real.dtype)]).to(qkv_real.dtype)

    def attend(nn, mask, whw):
        G, wh, ww, _ = nn.shape
        q, k, v = nn.reshape(G, wh * ww, 3 * C).split(C, -1)
        return cosine_attention(q, k, v, tau, table_fn(wh, ww), mask, heads).reshape(G, wh, ww, C)

    return windowed(qkv_real, window_size, shift_size, attend, fill=fill)


def window_attention(p, name, x, heads, window_size, shift_size, pos_scale):
    """shifted_window_attention + window_mhsa_with_pair_wise_positional_embedding with the layer's own variables"""
    dt = x.dtype
    C = x.shape[-1]
    qb, vb = p.get(f"{name}query_bias/bias"), p.get(f"{name}value_bias/bias")

    def attend(nn, mask, whw):
        G, wh, ww, _ = nn.shape
        q, k, v = (nn.reshape(G, wh * ww, C) @ p[f"{name}qkv/kernel"].to(dt)).split(C, -1)
        if qb is not None:
            q, v = q + qb.reshape(-1).to(dt), v + vb.reshape(-1).to(dt)
        bias = position_bias(p[f"{name}meta_dense_1/kernel"].to(dt), p[f"{name}meta_dense_1/bias"].to(dt),
                             p[f"{name}meta_dense_2/kernel"].to(dt), wh, ww, pos_scale)
        o = cosine_attention(q, k, v, tau_of(p[f"{name}scale/weight"].to(dt)), bias, mask, heads)
        return dense(p, f"{name}output", o).reshape(G, wh, ww, C)

    return windowed(x, window_size, shift_size, attend)


def block(p, name, x, heads, window_size, shift_size, pos_scale):
    a = ln(p, f"{name}attn_ln", window_attention(p, f"{name}attn_", x, heads, window_size, shift_size, pos_scale))
    x = x + a
    m = dense(p, f"{name}mlp_Dense_1", gelu(dense(p, f"{name}mlp_Dense_0", x)))
    return x + ln(p, f"{name}mlp_ln", m)


def patch_merging(p, name, x):
    B, H, W, C = x.shape
    if H % 2 or W % 2:
        x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        H, W = x.shape[1:3]
    nn = x.reshape(-1, 2, W, C).permute(0, 2, 1, 3).reshape(B, H // 2, W // 2, 4 * C)
    return ln(p, f"{name}ln", nn @ p[f"{name}dense/kernel"].to(x.dtype))


def forward_features(p, x, cfg, collect=None):
    """x [B, H, W, 3] -> the map the head pools (after pre_output_ln); `collect` receives each stack's output"""
    dt = x.dtype
    k = p["stem_conv/kernel"].to(dt).permute(3, 2, 0, 1)
    y = F.conv2d(x.permute(0, 3, 1, 2), k, p["stem_conv/bias"].to(dt), stride=k.shape[-1]).permute(0, 2, 3, 1)
    y = ln(p, "stem_ln", y)
    for si, (nb, heads) in enumerate(zip(cfg["num_blocks"], cfg["num_heads"])):
        st = f"stack{si + 1}_"
        if si > 0:
            y = patch_merging(p, f"{st}downsample_", y)
        ps = cfg["pos_scale"][si] if isinstance(cfg["pos_scale"], (list, tuple)) else cfg["pos_scale"]
        for bi in range(nb):
            y = block(p, f"{st}block{bi + 1}_", y, heads, cfg["window_size"], 0 if bi % 2 == 0 else 0.5, ps)
        if collect is not None:
            collect.append(y)
    return ln(p, "pre_output_ln", y)


def forward_logits(p, x, cfg):
    f = forward_features(p, x, cfg)
    return dense(p, "predictions", f.mean((1, 2)))
