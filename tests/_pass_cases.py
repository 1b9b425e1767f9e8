"""Shapes that push the PERSISTENT kernels past their first grid pass: launches whose grid is capped, so that a workgroup handles several
units of work in a loop and carries device-side state from one unit to the next.  What a "pass" is, per family:

  fused MLP (csrc/mlp_fused.hip, csrc/mlp_h2.hip)    unit = a tile of tokens, walked `tile += gridDim.x`; pass p of a workgroup is its tile
                                                     `blockIdx.x + p * workgroups`.  The streamed / packed kernels keep a double-buffered
                                                     LDS ring of weight slices running ACROSS tiles (the last slice of a tile prefetches
                                                     slice 0 of the next, `buf` is never reset: with an odd hidden / 32 every following
                                                     tile starts on the other buffer).
  depthwise tile kernel (csrc/dwconv.hip)            unit = a tile group (256 / cb tiles); at the cap (2048 / channel blocks workgroups
                                                     per channel block) every XCD walks one contiguous band of groups.  The pooling form
                                                     reuses its LDS reduction area from group to group.
  LDS-staged packed depthwise (dwconv_lds_h2.hip)    unit = an item (region group x 16-channel block); each of min(2 x CUs, items)
                                                     workgroups takes a contiguous run and ping-pongs descriptor slots where the run
                                                     crosses from one region group into the next.
  elementwise (grid_for / sgrid)                     unit = a block of 256 items (8 or 4 channels each), 8192 blocks at the most.

The dry runs (ops.mlp_plan, ops.dwconv_tile_plan, ops.dwconv_lds_plan: the launchers' own geometry functions, nothing is launched)
confirm the regime of every row before any GPU time is spent: tests/test_pass_plan_cpu.py for the depthwise tile kernel (host arithmetic),
tests/test_gpu_passes.py for the rest (they ask the device for its CU count).  Token counts and LDS batches are sized FROM the plan's
workgroup count G, so the rows stay in their regime on a part with another CU count; the absolute sizes in the comments assume 256 CUs.
The sizes are inherent: one full pass has to be filled before a second exists.  A change of the launch geometry that moves a row out
of its regime fails those assertions: re-derive the shape then, never the expectation."""
from collections import namedtuple

BIG_M = 1 << 22          # a token count far beyond every cap: its plan's workgroup count is the cap G itself

# ---- fused MLP, fp16 storage ----------------------------------------------------------------------------------------------------------
# M = tile_rows * full(G) + tail: full(G) whole tiles and one ragged one; tile_rows and G from ops.mlp_plan(BIG_M, C, hidden)
MlpRow = namedtuple("MlpRow", "id C hidden full tail ln res min_passes what")

MLP_F16 = [
    MlpRow("resident-c96", 96, 384, lambda G: G + 77, 37, True, True, 2,
           "mlp_fused_kernel, 512-token tiles: 78 workgroups take a second tile (the last one 37 rows), the others stop after one"),
    MlpRow("resident-c64-three", 64, 192, lambda G: 2 * G + 5, 1, False, False, 3,
           "mlp_fused_kernel: a third, partial pass whose last tile holds a single row; no LayerNorm, no residual"),
    MlpRow("stream-h768", 192, 768, lambda G: G + 77, 37, True, True, 2,
           "mlp_stream_kernel, 256-token tiles, nq = 24: the wrap-around prefetch of slice 0 feeds a second tile"),
    MlpRow("stream-h96-odd", 192, 96, lambda G: 2 * G + 5, 1, False, True, 3,
           "mlp_stream_kernel, nq = 3 (odd): the ring parity flips between tiles - the second tile starts on buffer 1, the third on 0"),
    MlpRow("stream-h416", 192, 416, lambda G: G + 3, 200, True, False, 2,
           "mlp_stream_kernel, nq = 13 (odd): only 4 workgroups go round again, the last of them on a 200-row tile"),
]

# ---- fused MLP, packed strict storage: one row per instantiation the host picks ---------------------------------------------------------
MLP_H2 = [
    MlpRow("h2-c96-8w", 96, 384, lambda G: G + 77, 37, True, True, 2,
           "mlp_h2_kernel<3, 8>: 256-token tiles, two workgroups per CU; nq = 12"),
    MlpRow("h2-c64-4w-odd", 64, 160, lambda G: G + 77, 37, True, True, 2,
           "mlp_h2_kernel<2, 4>: 128-token tiles, four workgroups per CU; nq = 5 (odd): the second tile starts on buffer 1"),
    MlpRow("h2-c128-4w", 128, 256, lambda G: G + 77, 37, False, False, 2,
           "mlp_h2_kernel<4, 4>: 128-token tiles, two workgroups per CU; no LayerNorm, no residual"),
]


def mlp_rows(row, tile_rows, G):
    """token count of an MLP row for the plan's tile size and workgroup cap"""
    return tile_rows * row.full(G) + row.tail


# ---- fp16 depthwise tile kernel (stride 1) --------------------------------------------------------------------------------------------
# groups / cap in (1.25, 1.4); `geom`: what the row's description claims about the launch, held against the plan
DwRow = namedtuple("DwRow", "id B H W C k pad act pooled geom what")

DW_TILE = [
    DwRow("k7-c96-29x27", 532, 29, 27, 96, 7, (3, 3, 3, 3), "gelu", False, dict(cb=12, tiles_per_block=21, channel_blocks=1, cap=2048),
          "cb 12 leaves 4 idle lanes per block; tile tails on both axes (15 x 7 tiles of 2 x 4); 2 660 groups against 2 048"),
    DwRow("k3-c1152-7x7", 600, 7, 7, 1152, 3, (1, 1, 1, 1), "gelu", False, dict(cb=16, tiles_per_block=16, channel_blocks=9, cap=228),
          "9 channel blocks: the cap is 228, no multiple of 8 - uneven XCD bands (29 or 28 workgroups over bands of 38 or 34 groups)"),
    DwRow("k5-c240-13x12-asym", 520, 13, 12, 240, 5, (1, 3, 2, 2), "gelu", False, dict(cb=16, tiles_per_block=16, channel_blocks=2, cap=1024),
          "the second channel block holds 14 of 16 chunks; asymmetric padding; 1 365 groups against 1 024"),
    DwRow("pool-k3-c64-56x56", 200, 56, 56, 64, 3, (1, 1, 1, 1), "gelu", True, dict(cb=8, tiles_per_block=32, channel_blocks=1, cap=2048),
          "the pooling form (ops.dwconv2d_se): 13 image-aligned groups per image, 2 600 against 2 048 - the LDS reduction area is reused "
          "from group to group and the last group of an image parks 24 of its 32 tile slots below the map"),
]
POOL_CR = 16            # squeeze width of the pooled rows' gate

# a shape tests/test_gpu_ops.py::test_dwconv runs (B = 2, H x (H + 1)): a single pass - the gap this table closes
DW_SINGLE_PASS = [(2, 14, 15, 64, 3), (2, 12, 13, 40, 5), (2, 11, 12, 96, 7)]

# ---- LDS-staged packed depthwise --------------------------------------------------------------------------------------------------------
# items / workgroups >= 2.5 and no integer; B = base_B * G / 512 (G = workgroups of the plan at base_B: 2 x CUs)
LdsRow = namedtuple("LdsRow", "id base_B H W C k act pooled geom what")

DW_LDS = [
    LdsRow("14x14-c72-k5", 560, 14, 14, 72, 5, "silu", False, dict(img=2, channel_blocks=5),
           "two images share a wave; 5 channel blocks, the last half empty; runs of 2.7 items cross from one region group into the next"),
    LdsRow("56x56-c24-k3", 128, 56, 56, 24, 3, "silu", False, dict(img=8, rgy=7, rgx=7, channel_blocks=2),
           "49 regions per image, 8 of them per wave; the second channel block half empty"),
    LdsRow("pool-14x14-c72-k5", 560, 14, 14, 72, 5, "silu", True, dict(img=2, channel_blocks=5),
           "the pooling form (ops.dwconv2d_se in strict mode) at the first shape: partial sums per sub-region across the slot ping-pong"),
]


def lds_batch(row, G):
    return max(1, (row.base_B * G + 256) // 512)


# ---- capped elementwise grid ------------------------------------------------------------------------------------------------------------
# scale_add_act with a gate (split on the fp16 storage), a residual and a second output
ELEMENTWISE = (40, 28, 28, 672)          # 21.1 M elements: 2.63 M 8-channel items against 8192 x 256 (1.26 passes), 2.5 passes of 4-channel ones
ELEMENTWISE_CAP = 8192 * 256             # grid_for (pointwise.hip) / sgrid (strict_ops.hip): blocks x items per block
