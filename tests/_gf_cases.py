"""The global-local filter (ops.global_local_filter, csrc/global_filter.hip) on operands whose result is EXACT, and on random ones.

Reference: ref64() - the two sums of include/vipcup_hip.h on double tensors with torch.roll (global half) and zero-padded shifts (local
half); fft64() is the DEFINITION, rfft2 -> complex weight -> irfft2 with torch.fft in float64.  tests/test_gf_cases_cpu.py holds the two
together on random, deliberately non-Hermitian complex weights.

EXACT rows (operands(row)): activations are integers in [-2, 2], w3 and g multiples of 1/4 in [-1, 1].  Every product and partial sum is a
multiple of 1/4 of magnitude at most 2 * H * W <= 512 (392 at 14 x 14): exact in fp32 in any order, with or without FMA, and representable in
fp16 - the three storages hold the result exactly, so a correct kernel equals ref64 BIT FOR BIT.  Structured rows:
  identity      g = a single 1 at [0][0]: the global half returns its input
  wrap-last     a single tap at [H-1][W-1]: a pure wrap of both axes
  wrap-10       a single tap at [1][0]: a pure wrap of the row axis alone
  corner-pixel  x is zero except pixel (0, W-1)
  w3-corner     w3 has only its [0][0] tap: a local half that wraps instead of zero-padding reads the far corner
BOUNDED rows (bounded_operands(row)): randn activations, a random ComplexDense weight [2, H, W // 2 + 1, half] - against fft64.

Grid of the GPU test: the maps the specialised widths serve and the maps of the generic form; S = 16, 48 (a partly filled channel block)
and the smallest S that spans three channel blocks of the kernel as built (block_channels(H): one wave = 64 // H quads of 8 channels);
B = 1 and 3."""
import zlib
from collections import namedtuple

import torch

SPECIAL_MAPS = [(6, 6), (7, 7), (12, 12), (14, 14)]                      # W a template argument
GENERIC_MAPS = [(2, 2), (3, 3), (5, 16), (16, 5), (13, 14), (16, 16)]
MAPS = SPECIAL_MAPS + GENERIC_MAPS
CHECK_MAPS = [(14, 14), (7, 7), (12, 12), (6, 6), (13, 14), (5, 16), (2, 2)]   # where ref64 is held to fft64
STRUCTURED = ("identity", "wrap-last", "wrap-10", "corner-pixel", "w3-corner")

Row = namedtuple("Row", "id B H W S kind")


def block_channels(H):
    """channels of S one workgroup owns (vip_global_local_filter_plan says the same: tests/test_gf_cases_cpu.py)"""
    return 8 * (64 // H)


def three_blocks(H):
    """the smallest supported S (a multiple of 16) that needs three workgroups per image"""
    return (2 * block_channels(H)) // 16 * 16 + 16


def _rows():
    out = []
    for H, W in MAPS:
        for S in (16, 48, three_blocks(H)):
            for B in (1, 3):
                out.append(Row(f"{H}x{W}-s{S}-b{B}", B, H, W, S, "random"))
    for H, W in ((14, 14), (7, 7), (13, 14), (5, 16)):                    # two specialised widths, two generic maps
        for kind in STRUCTURED:
            out.append(Row(f"{H}x{W}-{kind}", 2, H, W, 48, kind))
    return out


ROWS = _rows()
BOUNDED = [Row(f"bounded-{H}x{W}-s{S}", 2, H, W, S, "bounded") for (H, W), S in
           (((14, 14), 80), ((7, 7), 160), ((12, 12), 96), ((6, 6), 176), ((13, 14), 48), ((16, 16), 80), ((5, 16), 48), ((2, 2), 16))]


def _quarters(shape, gen):
    return torch.randint(-4, 5, shape, generator=gen).float() / 4


def operands(row):
    """(x [B,H,W,S], w3 [3,3,half], g [H,W,half]) as fp32 host tensors on the exact grid, seeded by the row's id"""
    gen = torch.Generator().manual_seed(zlib.crc32(row.id.encode()))
    B, H, W, S = row.B, row.H, row.W, row.S
    half = S // 2
    x = torch.randint(-2, 3, (B, H, W, S), generator=gen).float()
    w3 = _quarters((3, 3, half), gen)
    g = _quarters((H, W, half), gen)
    if row.kind in ("identity", "wrap-last", "wrap-10"):
        a, c = {"identity": (0, 0), "wrap-last": (H - 1, W - 1), "wrap-10": (1, 0)}[row.kind]
        g = torch.zeros(H, W, half)
        g[a, c] = 1.0
    elif row.kind == "corner-pixel":
        keep = x[:, 0, W - 1].clone()
        keep[keep == 0] = 1.0                                           # the pixel is live in every channel
        x = torch.zeros_like(x)
        x[:, 0, W - 1] = keep
    elif row.kind == "w3-corner":
        tap = w3[0, 0].clone()
        tap[tap == 0] = 0.75
        w3 = torch.zeros_like(w3)
        w3[0, 0] = tap
    return x, w3, g


def bounded_operands(row):
    """(x, w3, complex_weight [2, H, W // 2 + 1, half]) of a BOUNDED row: randn, nothing Hermitian about the weight"""
    gen = torch.Generator().manual_seed(zlib.crc32(row.id.encode()))
    half = row.S // 2
    x = torch.randn(row.B, row.H, row.W, row.S, generator=gen)
    w3 = torch.randn(3, 3, half, generator=gen) / 3
    cw = torch.randn(2, row.H, row.W // 2 + 1, half, generator=gen) * 0.5 ** 0.5
    return x, w3, cw


def _shift_zero(t, dy, dx):
    """out[b,h,w] = t[b,h+dy,w+dx], zero outside the map"""
    B, H, W, C = t.shape
    out = torch.zeros_like(t)
    hs, ws = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    hd, wd = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
    out[:, hs, ws] = t[:, hd, wd]
    return out


def _local(xl, w3, circular=False):
    out = torch.zeros_like(xl)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            src = torch.roll(xl, (-dy, -dx), (1, 2)) if circular else _shift_zero(xl, dy, dx)
            out = out + w3[dy + 1, dx + 1] * src
    return out


def _interleave(local, glob, swapped=False):
    pair = [glob, local] if swapped else [local, glob]
    return torch.stack(pair, -1).reshape(*local.shape[:3], 2 * local.shape[3])


MUTANTS = ("g-transposed", "shift-sign", "zero-padded-global", "circular-local", "interleave-swapped", "halves-swapped", "conjugate",
           "channel-shift")


def ref64(x, w3, g, mutant=None):
    """the operator's two sums on double tensors; ``mutant`` names one wrong reading of them (tests/test_gf_cases_cpu.py)"""
    assert mutant is None or mutant in MUTANTS
    x, w3, g = x.double(), w3.double(), g.double()
    B, H, W, S = x.shape
    half = S // 2
    xl, xg = x[..., :half], x[..., half:]
    if mutant == "halves-swapped":
        xl, xg = xg, xl
    if mutant == "g-transposed":
        g = g.transpose(0, 1) if H == W else g.reshape(W, H, half)
    if mutant == "conjugate":                                           # irfft2(conj(Wc)) is g reversed on both axes
        g = torch.roll(g.flip(0, 1), (1, 1), (0, 1))
    if mutant == "channel-shift":
        g, w3 = torch.roll(g, 1, 2), torch.roll(w3, 1, 2)
    sign = -1 if mutant == "shift-sign" else 1
    glob = torch.zeros_like(xg)
    for a in range(g.shape[0]):
        for c in range(g.shape[1]):
            if mutant == "zero-padded-global":
                src = _shift_zero(xg, -a, -c)
            else:
                src = torch.roll(xg, (sign * a, sign * c), (1, 2))     # out[h, w] = in[(h - a) mod H, (w - c) mod W]
            glob = glob + g[a, c] * src
    return _interleave(_local(xl, w3, circular=mutant == "circular-local"), glob, swapped=mutant == "interleave-swapped")


def filter64(cw, H, W):
    """ComplexDense weight [2, H, W // 2 + 1, half] -> g [H, W, half] in float64"""
    return torch.fft.irfft2(torch.complex(cw[0].double(), cw[1].double()), s=(H, W), dim=(0, 1))


def fft64(x, w3, cw):
    """the definition (kecam hornet.py:56-79): rfft2 -> complex weight -> irfft2 on the second half of the channels, float64"""
    x, w3 = x.double(), w3.double()
    B, H, W, S = x.shape
    half = S // 2
    wc = torch.complex(cw[0].double(), cw[1].double())
    glob = torch.fft.irfft2(torch.fft.rfft2(x[..., half:], dim=(1, 2)) * wc, s=(H, W), dim=(1, 2))
    return _interleave(_local(x[..., :half], w3), glob)
