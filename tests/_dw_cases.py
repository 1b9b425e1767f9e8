"""Every depthwise kernel of the three storages at the paddings the models hand it, on operands whose result is EXACT.

Operands (operands(row)): x holds integers in [-2, 2], the filter taps are multiples of 1/4 in [-1, 1] (another filter per channel), the
bias is a multiple of 1/4 in [-2, 2].  Every product and every partial sum is then a multiple of 1/4 below 2^11 / 4 (at most 49 * 2 + 2
= 100), so the sums are exact in fp32 in ANY order, with or without FMA, and the result is exactly representable in fp16: the fp16
storage, the packed (hi, lo) storage (lo = 0) and the fp32 storage all hold it exactly.  With act in {None, "relu"} a correct kernel
equals ref64() - the oracle's dwconv2d and act on double tensors - BIT FOR BIT: no tolerance, a quiet channel or a border row is held
as hard as the global maximum.  tests/test_dw_cases_cpu.py checks those claims, the dispatch and that the operands tell a wrong
padding / filter layout / border apart, without a GPU; tests/test_gpu_dw.py runs the rows.

A row names the kernel that must serve it; reaches(row) proves that from the project's own dry runs (nothing is launched):
  f16  dwconv_tile_kernel      stride 1: ops.dwconv_tile_plan(...)[0] > 0                                  (csrc/dwconv.hip)
  f16  dwconv_kernel           stride 2: the tile plan declines the stride, <3,2,2> / <5,2,2> remain       (csrc/pointwise.hip)
  f16  dwconv_tile_kernel/pool vip_dwconv2d_pool_parts(...) > 0                                            (POOL rows)
  h2   dwconv_lds_h2_kernel    stride 1, default switch: vip_dwconv2d_s1_supported_h2(...) == 1            (csrc/dwconv_lds_h2.hip)
  h2   dwconv_tile_h2_kernel   the same shapes with ops._DW_H2_LDS = 0: ops.dwconv_tile_plan(packed=True)  (csrc/dwconv.hip)
  h2   sdwconv_kernel          stride 2: both stride-1 kernels decline                                     (csrc/strict_ops.hip)
  s32  sdwconv_kernel          every call of the fp32 storage, stride 1 and 2
The LDS-staged kernel declines only tensors of 4 GiB and more (pick_config always finds a lane packing for k <= 7), so no small shape
reaches the tile twin by rejection: its rows run with the documented switch at 0.  The stride-1 sdwconv_kernel<SH2> sits behind
VIP_DW_H2_TILE=0, which is read once per process: not covered here.

Register tiles T x TW of the tile kernels (vip_dwconv_tiled): k = 3: 2 x 4, k = 5: 2 x 2, k = 7: 2 x 4; the plain kernels take TW = 2
output columns per thread at stride 2 and 4 at stride 1.  Channel chunks: 8 channels (fp16), 4 channels (strict)."""
import zlib
from collections import namedtuple

import torch

from oracle import ops_ref as R

TILE = {3: (2, 4), 5: (2, 2), 7: (2, 4)}

Row = namedtuple("Row", "id storage kernel B H W C k stride pad act nonlinear what")
Geom = namedtuple("Geom", "id B H W C k stride pad act nonlinear what")

# ---- stride 1: the symmetric pad, VALID and shifted pads; Ho, Wo no multiples of T, TW; the channel counts of the tile kernels ----------
_S1 = [
    Geom("k3-c8-sym", 2, 7, 9, 8, 3, 1, (1, 1, 1, 1), None, "gelu",
         "C = 8: one chunk per block (cb = 1), 256 tiles per block; 7 x 9 outputs: tile tails on both axes"),
    Geom("k3-c40-valid", 2, 9, 11, 40, 3, 1, (0, 0, 0, 0), "relu", None,
         "VALID: pt = pl = 0, 7 x 9 outputs; C = 40: cb = 5, 51 tiles per block, one idle lane (fp16), cb = 10 (strict)"),
    Geom("k3-c136-shift", 2, 7, 10, 136, 3, 1, (0, 2, 2, 0), None, None,
         "shifted pad: all of the vertical pad below, all of the horizontal pad left; C = 136: the second channel block holds one "
         "8-channel chunk (fp16) / two 4-channel chunks (strict)"),
    Geom("k5-c96-shift", 2, 8, 8, 96, 5, 1, (1, 2, 2, 1), None, "silu",
         "shifted pad (1,2,2,1), 7 x 7 outputs; C = 96: cb = 12 with 252 live lanes (fp16), cb = 24 (strict)"),
    Geom("k5-c136-sym", 2, 7, 5, 136, 5, 1, (2, 2, 2, 2), "relu", None,
         "7 x 5 outputs: a tail tile in both axes of the 2 x 2 register tile; second channel block nearly empty"),
    Geom("k5-c40-valid", 2, 9, 11, 40, 5, 1, (0, 0, 0, 0), None, None, "VALID, 5 x 7 outputs; C = 40 is no multiple of 16"),
    Geom("k7-c96-small", 2, 5, 6, 96, 7, 1, (3, 3, 3, 3), None, "gelu",
         "a map smaller than the filter: every window reaches the padding on all four sides; 5 x 6 outputs"),
    Geom("k7-c136-valid", 2, 11, 13, 136, 7, 1, (0, 0, 0, 0), "relu", None, "VALID, 5 x 7 outputs, two channel blocks"),
    Geom("k7-c40-shift", 3, 9, 7, 40, 7, 1, (2, 4, 1, 5), None, None, "shifted pad (2,4,1,5), 9 x 7 outputs, three images"),
]
# ---- uneven XCD bands: gridDim.x >= 8 with 9 ... 15 tile groups - chunk = ceil(groups / 8), the last bands empty ---------------------------
_XCD_F16 = Geom("k3-c64-xcd", 3, 19, 35, 64, 3, 1, (1, 1, 1, 1), "relu", None,
                "90 tiles per image in groups of 32: 9 groups - bands of 2, 2, 2, 2, 1 groups and three empty bands")
_XCD_H2 = Geom("k3-c64-xcd", 2, 19, 35, 64, 3, 1, (1, 1, 1, 1), "relu", None,
               "180 tiles in groups of 16: 12 groups - six bands of 2 groups and two empty bands")
XCD_GROUPS = range(9, 16)

# ---- stride 2, TF SAME (kecam_models.EfficientNet._pad): every parity of H, W; Wo odd - the two-column thread tile has a tail ------------
_S2 = [
    Geom("k3-s2-even", 3, 10, 14, 40, 3, 2, (0, 1, 0, 1), None, "silu", "even map: (0,1,0,1), 5 x 7 outputs; more than one block"),
    Geom("k3-s2-odd", 2, 9, 13, 8, 3, 2, (1, 1, 1, 1), "relu", None, "odd map: (1,1,1,1), 5 x 7 outputs; C = 8"),
    Geom("k3-s2-mixed", 2, 10, 13, 24, 3, 2, (0, 1, 1, 1), None, None, "H even, W odd: (0,1,1,1)"),
    Geom("k5-s2-even", 3, 10, 14, 40, 5, 2, (1, 2, 1, 2), "relu", "silu", "even map: (1,2,1,2), 5 x 7 outputs; more than one block"),
    Geom("k5-s2-odd", 2, 9, 13, 16, 5, 2, (2, 2, 2, 2), None, None, "odd map: (2,2,2,2), 5 x 7 outputs"),
    Geom("k5-s2-mixed", 2, 10, 13, 136, 5, 2, (1, 2, 2, 2), None, None, "H even, W odd: (1,2,2,2); C = 136"),
]
# the fp32 storage has one kernel: a stride-1 row per k (4 output columns per thread: Wo = 9, 7, 6 leave a tail) next to the stride-2 rows
_S1_S32 = ("k3-c8-sym", "k3-c40-valid", "k5-c96-shift", "k7-c96-small", "k7-c40-shift")


def _rows():
    out = []
    for g in _S1 + [_XCD_F16]:
        out.append(Row(f"f16-tile-{g.id}", "f16", "dwconv_tile_kernel", *g[1:]))
    for g in _S1:
        out.append(Row(f"h2-lds-{g.id}", "h2", "dwconv_lds_h2_kernel", *g[1:]))
    for g in _S1 + [_XCD_H2]:
        out.append(Row(f"h2-tile-{g.id}", "h2", "dwconv_tile_h2_kernel", *g[1:]))
    for g in _S1:
        if g.id in _S1_S32:
            out.append(Row(f"s32-plain-{g.id}", "s32", "sdwconv_kernel", *g[1:]))
    for g in _S2:
        out.append(Row(f"f16-plain-{g.id}", "f16", "dwconv_kernel", *g[1:]))
        out.append(Row(f"h2-plain-{g.id}", "h2", "sdwconv_kernel", *g[1:]))
        out.append(Row(f"s32-plain-{g.id}", "s32", "sdwconv_kernel", *g[1:]))
    return out


ROWS = _rows()
NONLINEAR = [r for r in ROWS if r.nonlinear]
# the matrix-core experiment (VIP_DW_MFMA=1, experimental builds only) takes k = 5 / 7, stride 1, C % 16 == 0 of the fp16 storage
MFMA = [r for r in ROWS if r.kernel == "dwconv_tile_kernel" and r.k in (5, 7) and r.C % 16 == 0]

# ---- the pooling forms (ops.dwconv2d_se): the map and per-group partial sums of it ------------------------------------------------------------
_POOL = [
    Geom("pool-k3-c64-19x35", 2, 19, 35, 64, 3, 1, (1, 1, 1, 1), "relu", None,
         "90 tiles per image in 3 image-aligned groups of 32: six idle slots in the last group; tile tails on both axes"),
    Geom("pool-k5-c128-12x12-valid", 3, 12, 12, 128, 5, 1, (0, 0, 0, 0), None, None, "VALID: 8 x 8 outputs, 16 tiles in one full group"),
    Geom("pool-k7-c96-14x12", 2, 14, 12, 96, 7, 1, (3, 3, 3, 3), "relu", None, "21 tiles = one group of cb 12's 21 slots"),
]
POOL = ([Row(f"f16-{g.id}", "f16", "dwconv_tile_kernel/pool", *g[1:]) for g in _POOL]
        + [Row(f"h2-{g.id}", "h2", "dwconv_lds_h2_kernel/pool", *g[1:]) for g in _POOL])

EXACT_ACTS = (None, "relu")


def out_hw(row):
    pt, pb, pl, pr = row.pad
    return (row.H + pt + pb - row.k) // row.stride + 1, (row.W + pl + pr - row.k) // row.stride + 1


def operands(row):
    """(x [B,H,W,C], w [k,k,C,1], bias [C]) as fp32 host tensors on the exact grid, seeded by the row's id"""
    g = torch.Generator().manual_seed(zlib.crc32(row.id.encode()))
    x = torch.randint(-2, 3, (row.B, row.H, row.W, row.C), generator=g).float()
    w = torch.randint(-4, 5, (row.k, row.k, row.C, 1), generator=g).float() / 4
    b = torch.randint(-8, 9, (row.C,), generator=g).float() / 4
    return x, w, b


def ref64(x, w, b, stride, pad, act):
    """the oracle's depthwise convolution and activation on double tensors"""
    return R.act(R.dwconv2d(x.double(), w.double(), None if b is None else b.double(), stride, pad), act)


def reaches(row, ops):
    """None when the project's dry runs send the row to the kernel it names, else what they say instead.  Launches nothing."""
    lib = ops._abi.lib()
    B, H, W, C, k, s, pad = row.B, row.H, row.W, row.C, row.k, row.stride, row.pad
    Ho, Wo = out_hw(row)
    f16_tile = lib.vip_dwconv2d_tile_plan(B, H, W, C, k, s, Ho, Wo, 0, None, None)
    h2_tile = lib.vip_dwconv2d_tile_plan_h2(B, H, W, C, k, s, pad[0], pad[2], Ho, Wo, None, None)
    lds = s == 1 and lib.vip_dwconv2d_s1_supported_h2(B, H, W, C, k, Ho, Wo) == 1
    plain = (k, s) in ((3, 1), (3, 2), (5, 1), (5, 2), (7, 1))            # the instantiations of dwconv_kernel / sdwconv_kernel
    checks = {
        ("f16", "dwconv_tile_kernel"): s == 1 and ops.dwconv_tile_plan(B, H, W, C, k, pad=pad) is not None and f16_tile > 0,
        ("f16", "dwconv_kernel"): s == 2 and f16_tile == 0 and plain,
        ("f16", "dwconv_tile_kernel/pool"): lib.vip_dwconv2d_pool_parts(B, H, W, C, k, s, Ho, Wo) > 0,
        ("h2", "dwconv_lds_h2_kernel"): lds and 0 < ops._DW_H2_LDS <= k,
        ("h2", "dwconv_lds_h2_kernel/pool"): lds and 0 < ops._DW_H2_LDS <= k and lib.vip_dwconv2d_s1_pool_parts_h2(B, H, W, C, k, Ho, Wo) > 0,
        ("h2", "dwconv_tile_h2_kernel"): s == 1 and h2_tile > 0,          # the kernel of ops.dwconv2d once ops._DW_H2_LDS is 0
        ("h2", "sdwconv_kernel"): s == 2 and not lds and h2_tile == 0 and plain,
        ("s32", "sdwconv_kernel"): plain,
    }
    ok = checks[(row.storage, row.kernel)]
    return None if ok else f"{row.id}: f16 tile plan {f16_tile}, h2 tile plan {h2_tile}, lds {lds}, plain instantiation {plain}"
