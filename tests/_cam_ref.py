"""Test infrastructure for the evidence maps (vipcup_amd.ops.cam / cam_compose / cam_overlay): the definition in fp64 torch.

Two independent routes to the same map:
  * ``cam_closed_form``: the closed-form gradient of a ``GAP -> [LayerNorm] -> Dense -> activation`` head, the arithmetic csrc/cam.hip
    restates in fp32;
  * ``cam_autograd``: ``torch.autograd.grad`` through the oracle's own primitives (``R.global_avgpool`` / ``R.layernorm`` / ``R.dense``),
    which is what the reference's ``tape.gradient`` computes (gradcam.py:44-55), the gradient mean taken per image.
Plus references for the full-size composition and the overlay, and ``patched()``: a CPU stand-in for ``ops.cam`` to use next to
``emul_ops.patched()``."""
import contextlib

import torch

from oracle import ops_ref as R

F64 = torch.float64


def head_probs(z, act):
    if act == "default":
        act = "sigmoid" if z.shape[1] == 1 else "softmax"
    if act == "sigmoid":
        return torch.sigmoid(z)
    if act == "softmax":
        return torch.softmax(z, dim=-1)
    assert act in ("linear", "none", None), act
    return z


def target_value(p, target):
    """the scalar per image whose gradient the map shows: "score" = ops.binary_score, an int = that class's probability"""
    if target == "score":
        return p[:, 0] if p.shape[1] == 1 else 1.0 - p[:, 0]
    return p[:, int(target)]


def head_forward(feat, w_nc, bias, ln, act):
    """feat [B,H,W,C] -> (z, p) through the oracle primitives, in feat's dtype"""
    v = R.global_avgpool(feat)
    u = v if ln is None else R.layernorm(v, ln[0].to(feat.dtype), ln[1].to(feat.dtype), float(ln[2]))
    z = R.dense(u, w_nc.to(feat.dtype).t(), None if bias is None else bias.to(feat.dtype))
    return z, head_probs(z, act)


def _finish(feat, g):
    """cam = relu(sum_c F g), peak, and kappa = max_hw sum_c |F g| / peak (the conditioning of the normalised map)"""
    cam = torch.relu((feat * g[:, None, None, :]).sum(-1))
    peak = cam.flatten(1).max(1).values
    absum = (feat * g[:, None, None, :]).abs().sum(-1).flatten(1).max(1).values
    kappa = torch.where(peak > 0, absum / peak.clamp_min(1e-300), torch.zeros_like(peak))
    return cam, peak, kappa


def cam_autograd(feat, w_nc, bias, ln=None, act="default", target="score"):
    """(cam [B,H,W], peak [B], z [B,N], kappa [B]) in fp64; g = mean_hw d target / d F per image, from autograd"""
    f = feat.detach().to(F64).requires_grad_(True)
    z, p = head_forward(f, w_nc.to(F64), None if bias is None else bias.to(F64), ln, act)
    (grad,) = torch.autograd.grad(target_value(p, target).sum(), f)          # images are independent: the sum separates them
    g = grad.mean(dim=(1, 2))
    cam, peak, kappa = _finish(f.detach(), g)
    return cam, peak, z.detach(), kappa


def cam_closed_form(feat, w_nc, bias, ln=None, act="default", target="score"):
    """the same four results from the closed form (no autograd)"""
    f, g, z = closed_form_gradient(feat, w_nc, bias, ln, act, target)
    cam, peak, kappa = _finish(f, g)
    return cam, peak, z, kappa


def abs_sum(feat, w_nc, bias, ln=None, act="default", target="score"):
    """max_hw sum_c |F g| per image: the scale the rounding error of a position's dot product is relative to (kappa = this / peak)"""
    f, g, _ = closed_form_gradient(feat, w_nc, bias, ln, act, target)
    return (f * g[:, None, None, :]).abs().sum(-1).flatten(1).max(1).values


def closed_form_gradient(feat, w_nc, bias, ln=None, act="default", target="score"):
    """(F, g [B,C] = mean_hw d target / d F, z) in fp64 from the closed form"""
    f = feat.detach().to(F64)
    w = w_nc.to(F64)
    B, H, W, C = f.shape
    N = w.shape[0]
    v = f.mean(dim=(1, 2))
    if ln is not None:
        gamma, beta, eps = ln[0].to(F64), ln[1].to(F64), float(ln[2])
        mu = v.mean(-1, keepdim=True)
        sd = torch.sqrt(((v - mu) ** 2).mean(-1, keepdim=True) + eps)
        uh = (v - mu) / sd
        u = uh * gamma + beta
    else:
        u = v
    z = u @ w.t() + (0 if bias is None else bias.to(F64))
    if act == "default":
        act = "sigmoid" if N == 1 else "softmax"
    p = head_probs(z, act)
    k = 0 if target == "score" else int(target)
    delta = torch.zeros(N, dtype=F64)
    delta[k] = 1.0
    if act == "sigmoid":
        dz = delta * (p[:, k:k + 1] * (1 - p[:, k:k + 1]))
    elif act == "softmax":
        dz = p[:, k:k + 1] * (delta - p)
    else:
        dz = delta.expand(B, N).clone()
    if target == "score" and N > 1:
        dz = -dz
    a = dz @ w
    if ln is not None:
        a = a * gamma
        a = (a - a.mean(-1, keepdim=True) - uh * (a * uh).mean(-1, keepdim=True)) / sd
    return f, a / (H * W), z


def normalise(cam, peak):
    """cam / peak, all zero where peak == 0"""
    pk = peak.reshape(-1, 1, 1)
    return torch.where(pk > 0, cam / torch.where(pk > 0, pk, torch.ones_like(pk)), torch.zeros_like(cam))


def _axis(out, inp):
    """bilinear taps of one axis: half-pixel centres, edge clamp -> (i0, i1, t) for every output index"""
    src = ((torch.arange(out, dtype=F64) + 0.5) * inp / out - 0.5).clamp_min(0.0)
    i0 = src.floor().long().clamp_max(inp - 1)
    i1 = (i0 + 1).clamp_max(inp - 1)
    return i0, i1, src - i0.to(F64)


def resize_bilinear(m, h, w):
    """m [gh, gw] fp64 -> [h, w]"""
    y0, y1, ty = _axis(h, m.shape[0])
    x0, x1, tx = _axis(w, m.shape[1])
    top = m[y0][:, x0] * (1 - tx) + m[y0][:, x1] * tx
    bot = m[y1][:, x0] * (1 - tx) + m[y1][:, x1] * tx
    return top * (1 - ty)[:, None] + bot * ty[:, None]


def compose_ref(maps, peaks, sizes_host, max_hw, weights=None):
    """fp64 [n, maxH, maxW]: mean over members of the resized normalised maps, zero outside each image"""
    M, n = len(maps), maps[0].shape[0]
    w = [1.0 / M] * M if weights is None else list(weights)
    out = torch.zeros((n, max_hw[0], max_hw[1]), dtype=F64)
    for m in range(M):
        nm = normalise(maps[m].to(F64), peaks[m].to(F64))
        for i, (h, wd) in enumerate(sizes_host):
            out[i, :h, :wd] += w[m] * resize_bilinear(nm[i], h, wd)
    return out


def to_u8(m):
    return torch.round(255.0 * m).clamp(0, 255).to(torch.uint8)


def overlay_ref(rgb, map_u8, table, alpha):
    """uint8: clip(round(rgb + alpha * table[map]))"""
    col = table.to(F64)[map_u8.long()]
    return torch.round(rgb.to(F64) + float(torch.tensor(alpha, dtype=torch.float32)) * col).clamp(0, 255).to(torch.uint8)


def cam_emul(features, w_nc, bias, ln=None, act="default", target="score"):
    """CPU stand-in for ``vipcup_amd.ops.cam``: same signature, fp32 results from the fp64 closed form"""
    cam, peak, z, _ = cam_closed_form(features.float(), w_nc, bias, ln, act, target)
    return cam.float(), peak.float(), z.float()


@contextlib.contextmanager
def patched():
    """swap ``vipcup_amd.ops.cam`` for ``cam_emul`` (use inside ``emul_ops.patched()``)"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    saved = ops.cam
    ops.cam = cam_emul
    try:
        yield
    finally:
        ops.cam = saved
