"""Input pipeline — the MI355X counterpart of dataset/dataset.py (``build_decoder.decode`` :22-39,
``build_dataset`` :64-102) and of the TTA ops of dataset/augment.py (:115-120, :142-182).

Differences from the reference, by design: every JPEG is entropy-decoded ONCE on the
host (C++ threads inside libvipcup_hip.so) and turned into RGB once on the GPU; each member resolution
(200, 224, ...) is then one resize launch on the resident uint8 pixels — the reference re-reads and
re-decodes the files for every model.
"""
import ctypes as C
import math
import os
import re
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi
from .chain import chain_noise_seeds, parse_chain, parse_chains  # noqa: F401  (the chain grammar: torch-free, re-exported here)
from .ops import _launch, _p

_TABLE_DEV: Dict[int, torch.Tensor] = {}


def bicubic_table(device) -> torch.Tensor:
    key = torch.device(device).index or 0
    if key not in _TABLE_DEV:
        host = np.zeros((1025 * 2,), dtype=np.float32)
        _abi.check(_abi.lib().vip_bicubic_table_f32(host.ctypes.data_as(C.c_void_p)), "vip_bicubic_table_f32")
        _TABLE_DEV[key] = torch.from_numpy(host).to(device)
    return _TABLE_DEV[key]


# per image, JPEG, PNG and WebP (csrc/png_host.cpp and csrc/webp_host.cpp read the same variable); the task's images are 200 x 200
MAX_JPEG_PIXELS = int(os.environ.get("VIP_MAX_JPEG_PIXELS", str(64 << 20)))


def _raw_args(raws: Sequence[bytes], threads: int):
    """What every batched host call takes: the files as arrays of pointers and lengths (and the buffers that keep the pointers good),
    and the thread count, ``threads`` <= 0 standing for one per CPU up to 16."""
    if threads <= 0:
        threads = min(16, os.cpu_count() or 1)
    n = len(raws)
    bufs = [np.frombuffer(b, dtype=np.uint8) for b in raws]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in raws])
    return bufs, ptrs, lens, threads


def entropy_decode(jpegs: Sequence[bytes], threads: int = 0, pinned: bool = False):
    """Host stage: list of JPEG byte strings -> (desc array (ctypes), coef int16 numpy array); with ``pinned`` the
    coefficients come back as a page-locked torch tensor instead (torch caches such buffers), so that the H2D copy in
    ``decode_entropy`` is asynchronous and runs at PCIe rate.
    Raises VipError for streams outside the supported Huffman subset (SOF0/1/2, 8-bit, 1 or 3 components) (the reference raises too: TF)."""
    lib = _abi.lib()
    n = len(jpegs)
    bufs, ptrs, lens, threads = _raw_args(jpegs, threads)
    desc = (_abi.JpegDesc * n)()
    total = 0
    tmp = _abi.JpegDesc()
    need = C.c_size_t(0)
    for i in range(n):
        _abi.check(lib.vip_jpeg_probe_h(ptrs[i], lens[i], C.byref(tmp), C.byref(need)), "vip_jpeg_probe_h")
        if tmp.width * tmp.height > MAX_JPEG_PIXELS:      # a corrupt header can claim 65535 x 65535: do not allocate for it
            raise _abi.VipError(f"jpeg {i}: {tmp.width}x{tmp.height} exceeds VIP_MAX_JPEG_PIXELS={MAX_JPEG_PIXELS}")
        total += need.value
    coef_t = torch.empty((max(total, 1),), dtype=torch.int16, pin_memory=True) if pinned else None
    coef = coef_t.numpy() if pinned else np.empty((max(total, 1),), dtype=np.int16)
    used = C.c_size_t(0)
    st = lib.vip_jpeg_entropy_decode_h(ptrs, lens, n, desc, coef.ctypes.data_as(C.c_void_p), coef.size, C.byref(used),
                                       threads)
    _abi.check(st, "vip_jpeg_entropy_decode_h")
    return desc, (coef_t[:used.value] if pinned else coef[:used.value])


class DecodedBatch:
    """uint8 RGB pixels of a batch, resident on the GPU: ``rgb [n,maxH,maxW,3]``, ``sizes [n,2]`` (h,w)."""

    def __init__(self, rgb: torch.Tensor, sizes: torch.Tensor, sizes_host: List[Tuple[int, int]]):
        self.rgb, self.sizes, self.sizes_host = rgb, sizes, sizes_host

    def __len__(self):
        return self.rgb.shape[0]

    def resized(self, out_h: int, out_w: int, c_out: int = 8, dtype: torch.dtype = torch.float16) -> torch.Tensor:
        """cast -> tf.image.resize(bicubic) -> /255 (dataset/dataset.py:31-38) -> NHWC, channels padded; fp16, or with
        ``dtype=torch.float32`` (the STRICT path) the unrounded fp32 values the reference's pipeline produces."""
        n, maxH, maxW, _ = self.rgb.shape
        from . import ops
        if dtype == ops.PACKED:                      # packed STRICT storage: the fp32 pipeline values, split once on the device
            return ops.pack_h2(self.resized(out_h, out_w, c_out, torch.float32))
        out = torch.empty((n, out_h, out_w, c_out), dtype=dtype, device=self.rgb.device)
        fn = {torch.float16: "vip_resize_bicubic_norm_f16", torch.float32: "vip_resize_bicubic_norm_s32"}[dtype]
        _launch(fn, _p(self.rgb), _p(self.sizes), _p(bicubic_table(self.rgb.device)), n, maxH, maxW, _p(out), out_h, out_w, c_out)
        return out

    def tiles(self, tab_d: torch.Tensor, lo: int, hi: int, tile: int, out_hw: int, c_out: int = 8,
              dtype: torch.dtype = torch.float16) -> torch.Tensor:
        """Tiles ``tab_d[lo:hi]`` of this batch (``tab_d``: the device copy of ``tile_plan``'s ``tab``, int32 ``[T, 4]``) as network
        inputs ``[hi - lo, out_hw, out_hw, c_out]``: every ``tile x tile`` crop treated as an image of its own and sent through
        dataset/dataset.py:31-38 - exactly the values ``DecodedBatch(crop).resized(out_hw, out_hw, c_out, dtype)`` gives, the bicubic
        taps clamped at the tile's edge.  One launch (``vip_tile_resize_bicubic_norm_*``), no intermediate uint8 batch."""
        n, maxH, maxW, _ = self.rgb.shape
        from . import ops
        if dtype == ops.PACKED:
            return ops.pack_h2(self.tiles(tab_d, lo, hi, tile, out_hw, c_out, torch.float32))
        if tab_d.dtype != torch.int32 or tab_d.dim() != 2 or tab_d.shape[1] != 4 or not tab_d.is_contiguous() or \
                tab_d.device != self.rgb.device:
            raise ValueError(f"tiles: tab_d must be a contiguous int32 [T, 4] tensor on {self.rgb.device}, got {tab_d.dtype} "
                             f"{tuple(tab_d.shape)} on {tab_d.device}")
        if not 0 <= lo < hi <= tab_d.shape[0]:
            raise ValueError(f"tiles: rows {lo}:{hi} of a table of {tab_d.shape[0]}")
        if not 1 <= int(tile) <= min(maxH, maxW):
            raise ValueError(f"tiles: tile {tile} does not fit the batch's {maxH} x {maxW} slots")
        src = self.rgb if self.rgb.is_contiguous() else self.rgb.contiguous()
        out = torch.empty((hi - lo, out_hw, out_hw, c_out), dtype=dtype, device=self.rgb.device)
        fn = {torch.float16: "vip_tile_resize_bicubic_norm_f16", torch.float32: "vip_tile_resize_bicubic_norm_s32"}[dtype]
        _launch(fn, _p(src), _p(tab_d[lo:hi]), _p(bicubic_table(self.rgb.device)), hi - lo, maxH, maxW, int(tile), _p(out), out_hw, out_hw,
                c_out)
        return out

    def mean_colour(self) -> torch.Tensor:
        """uint8 ``[n, 4]`` on the device: (r, g, b, 0), each image's mean colour over its own ``h x w`` pixels, per channel
        ``(sum + h * w // 2) // (h * w)`` in 64-bit integers (``vip_image_mean_u8``; the padding of the slots is not read)"""
        n, maxH, maxW, _ = self.rgb.shape
        src = self.rgb if self.rgb.is_contiguous() else self.rgb.contiguous()
        out = torch.empty((n, 4), dtype=torch.uint8, device=self.rgb.device)
        _launch("vip_image_mean_u8", _p(src), _p(self.sizes), n, maxH, maxW, _p(out))
        return out

    def occluded(self, tab_d: torch.Tensor, lo: int, hi: int, fill_d: torch.Tensor, out_h: int, out_w: int, c_out: int = 8,
                 dtype: torch.dtype = torch.float16) -> torch.Tensor:
        """Variants ``tab_d[lo:hi]`` of this batch (``tab_d``: the device copy of ``occlusion_plan``'s ``tab``, int32 ``[V, 8]`` = (image, y0,
        x0, y1, x1, 0, 0, 0)) as network inputs ``[hi - lo, out_h, out_w, c_out]``: the image with the pixels of the rectangle replaced by
        its row of ``fill_d`` (uint8 ``[n, 4]``, e.g. ``mean_colour()``) and sent through dataset/dataset.py:31-38 - exactly the values
        ``resized(out_h, out_w, c_out, dtype)`` gives for an occluded copy of the pixels.  One launch
        (``vip_occlude_resize_bicubic_norm_*``): the replacement happens as the resize reads each tap, no uint8 copy is made."""
        n, maxH, maxW, _ = self.rgb.shape
        from . import ops
        if dtype == ops.PACKED:
            return ops.pack_h2(self.occluded(tab_d, lo, hi, fill_d, out_h, out_w, c_out, torch.float32))
        if dtype not in (torch.float16, torch.float32):
            raise ValueError(f"occluded: dtype {dtype}: expected torch.float16, torch.float32 or the packed strict storage")
        if tab_d.dtype != torch.int32 or tab_d.dim() != 2 or tab_d.shape[1] != 8 or not tab_d.is_contiguous() or \
                tab_d.device != self.rgb.device:
            raise ValueError(f"occluded: tab_d must be a contiguous int32 [V, 8] tensor on {self.rgb.device}, got {tab_d.dtype} "
                             f"{tuple(tab_d.shape)} on {tab_d.device}")
        if not 0 <= lo < hi <= tab_d.shape[0]:
            raise ValueError(f"occluded: rows {lo}:{hi} of a table of {tab_d.shape[0]}")
        if fill_d.dtype != torch.uint8 or tuple(fill_d.shape) != (n, 4) or not fill_d.is_contiguous() or fill_d.device != self.rgb.device:
            raise ValueError(f"occluded: fill_d must be a contiguous uint8 [{n}, 4] tensor on {self.rgb.device}, got {fill_d.dtype} "
                             f"{tuple(fill_d.shape)} on {fill_d.device}")
        src = self.rgb if self.rgb.is_contiguous() else self.rgb.contiguous()
        out = torch.empty((hi - lo, out_h, out_w, c_out), dtype=dtype, device=self.rgb.device)
        fn = {torch.float16: "vip_occlude_resize_bicubic_norm_f16", torch.float32: "vip_occlude_resize_bicubic_norm_s32"}[dtype]
        _launch(fn, _p(src), _p(self.sizes), _p(fill_d), _p(tab_d[lo:hi]), _p(bicubic_table(self.rgb.device)), n, hi - lo, maxH, maxW,
                _p(out), int(out_h), int(out_w), c_out)
        return out


def _int_arg(name: str, v, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{name} {v!r}: expected an integer in {lo}..{hi}")
    return int(v)


def _tile_args(tile, stride, max_tiles) -> Tuple[int, int, int]:
    tile = _int_arg("tile", tile, 16, 1024)
    stride = tile if stride is None else _int_arg("stride", stride, 1, tile)
    return tile, stride, _int_arg("max_tiles", max_tiles, 1, 4096)


def _tile_positions(length: int, tile: int, n: int) -> List[int]:
    """``n`` tile origins along an axis of ``length`` >= ``tile``: the first at 0, the last at ``length - tile``, the others spaced evenly
    between them (rounded to the nearest pixel, halves up) - so whatever overlap or gap there is, is spread over the whole axis"""
    if n <= 1:
        return [0]
    return [(2 * k * (length - tile) + (n - 1)) // (2 * (n - 1)) for k in range(n)]


def tile_grid(h: int, w: int, tile: int = 200, stride: Optional[int] = None, max_tiles: int = 256) -> Tuple[List[int], List[int]]:
    """Where the ``tile x tile`` crops of an ``h x w`` image start: ``(ys, xs)``, the grid is their product.  Per axis of length L
    ``ceil((L - tile) / stride) + 1`` tiles (``stride`` defaults to ``tile``), placed by ``_tile_positions``: the image is covered edge to
    edge and neighbours never lie further apart than ``stride``.  While the grid holds more than ``max_tiles`` the larger count (rows on a
    tie) drops by one and that axis is laid out again: the grid is then an evenly spaced sample of the image with gaps.  An image
    smaller than a tile in either direction has no tiles: ``([], [])``.  Pure host arithmetic."""
    tile, stride, max_tiles = _tile_args(tile, stride, max_tiles)
    h, w = int(h), int(w)
    if h < tile or w < tile:
        return [], []
    ny, nx = -(-(h - tile) // stride) + 1, -(-(w - tile) // stride) + 1
    while ny * nx > max_tiles:
        if ny >= nx:
            ny -= 1
        else:
            nx -= 1
    return _tile_positions(h, tile, ny), _tile_positions(w, tile, nx)


class TilePlan:
    """What ``tile_plan`` returns; unpacks as ``tab, seg = tile_plan(...)``.  ``tab`` int32 ``[T, 4]`` = (image, y0, x0, 0) in image
    order, then row-major; ``seg`` int32 ``[n + 1]``: the tiles of image i are ``tab[seg[i]:seg[i + 1]]``.  Per image also ``sizes`` (h, w),
    ``grids`` (ny, nx) - (0, 0) for an image that is not tiled - and ``thinned`` (``max_tiles`` removed rows or columns: the grid has
    gaps, or less overlap than ``stride`` asks for); and the settings ``tile``, ``stride``, ``max_tiles``."""

    def __init__(self, tab, seg, sizes, grids, thinned, tile, stride, max_tiles):
        self.tab, self.seg, self.sizes, self.grids, self.thinned = tab, seg, sizes, grids, thinned
        self.tile, self.stride, self.max_tiles = tile, stride, max_tiles

    def __iter__(self):
        return iter((self.tab, self.seg))


def tile_plan(sizes_host: Sequence[Tuple[int, int]], tile: int = 200, stride: Optional[int] = None, max_tiles: int = 256) -> TilePlan:
    """The tiles of a batch of images of ``sizes_host`` = [(h, w)]: ``tile_grid`` per image, ``max_tiles`` per image.  An image that IS one
    tile (``tile x tile`` exactly: the challenge's own 200 x 200 files) is left out like one that is too small - its only tile would be
    the plain input again.  A pure function of its arguments: every rank derives the same plan from the same sizes."""
    tile, stride, max_tiles = _tile_args(tile, stride, max_tiles)
    rows: List[Tuple[int, int, int, int]] = []
    seg, grids, thinned = [0], [], []
    for i, (h, w) in enumerate(sizes_host):
        ys, xs = ([], []) if (int(h), int(w)) == (tile, tile) else tile_grid(h, w, tile, stride, max_tiles)
        rows += [(i, y, x, 0) for y in ys for x in xs]
        seg.append(len(rows))
        grids.append((len(ys), len(xs)))
        thinned.append(bool(ys) and len(ys) * len(xs) < (-(-(int(h) - tile) // stride) + 1) * (-(-(int(w) - tile) // stride) + 1))
    tab = np.asarray(rows, dtype=np.int32).reshape(-1, 4)
    return TilePlan(tab, np.asarray(seg, dtype=np.int32), [(int(h), int(w)) for h, w in sizes_host], grids, thinned, tile, stride,
                    max_tiles)


class OcclusionPlan:
    """What ``occlusion_plan`` returns; unpacks as ``tab, seg = occlusion_plan(...)``.  ``tab`` int32 ``[V, 8]`` = (image, y0, x0, y1, x1, 0,
    0, 0): the pixel rectangle each variant hides, in image order, then window row-major ``(wy, wx)``; ``seg`` int32 ``[n + 1]``: the
    variants of image i are ``tab[seg[i]:seg[i + 1]]``.  Per image also ``sizes`` (h, w); ``skipped``: the indices of the images without
    variants (lower or narrower than ``grid`` pixels); and the settings ``grid`` and ``window``."""

    def __init__(self, tab, seg, sizes, skipped, grid, window):
        self.tab, self.seg, self.sizes, self.skipped, self.grid, self.window = tab, seg, sizes, skipped, grid, window

    def __iter__(self):
        return iter((self.tab, self.seg))


def occlusion_bounds(length: int, grid: int) -> List[int]:
    """the ``grid + 1`` cell edges along an axis of ``length`` pixels: cell g covers ``[b[g], b[g + 1])``, ``b[g] = (g * length) // grid``"""
    return [(g * int(length)) // int(grid) for g in range(int(grid) + 1)]


def occlusion_plan(sizes_host: Sequence[Tuple[int, int]], grid: int = 8, window: int = 2) -> OcclusionPlan:
    """The occlusion variants of a batch of images of ``sizes_host`` = [(h, w)]: every image is divided into ``grid x grid`` cells
    (``occlusion_bounds`` per axis) and a window of ``window x window`` cells is placed at every cell offset ``0 .. grid - window`` in both
    axes - ``(grid - window + 1)^2`` variants per image, each hiding the pixels of its window.  An image with ``h < grid`` or
    ``w < grid`` (a cell would be empty) has no variants and is listed in ``skipped``.  Integer arithmetic only, a pure function of its
    arguments: every rank derives the same plan from the same sizes."""
    grid = _int_arg("grid", grid, 2, 32)
    window = _int_arg("window", window, 1, grid)
    rows: List[Tuple[int, ...]] = []
    seg, skipped = [0], []
    for i, (h, w) in enumerate(sizes_host):
        h, w = int(h), int(w)
        if h < grid or w < grid:
            skipped.append(i)
        else:
            by, bx = occlusion_bounds(h, grid), occlusion_bounds(w, grid)
            rows += [(i, by[wy], bx[wx], by[wy + window], bx[wx + window], 0, 0, 0)
                     for wy in range(grid - window + 1) for wx in range(grid - window + 1)]
        seg.append(len(rows))
    tab = np.asarray(rows, dtype=np.int32).reshape(-1, 8)
    return OcclusionPlan(tab, np.asarray(seg, dtype=np.int32), [(int(h), int(w)) for h, w in sizes_host], skipped, grid, window)


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


class HostStage:
    """What the host stage of a format other than JPEG returns (``FORMATS`` lists them): ``desc`` (ctypes array of the format's
    descriptor), ``stream`` (what the device half reads: a uint8 numpy array, or a page-locked torch tensor; aligned to the format's
    word and a whole number of them) and ``scratch_bytes``, the size of the device buffer the format's kernels need besides (0: none)."""

    def __init__(self, desc, stream, scratch_bytes=0):
        self.desc, self.stream, self.scratch_bytes = desc, stream, scratch_bytes

    def __len__(self):
        return len(self.desc)


class PngStage(HostStage):
    """What ``inflate_pngs`` returns: ``desc`` (ctypes array of PngDesc) and the still-filtered scanlines of the batch
    (uint8 numpy array, or a page-locked torch tensor), padded to whole 4-byte words (the device kernel reads words)."""


class WebpStage(HostStage):
    """What ``entropy_decode_webps`` returns: ``desc`` (ctypes array of WebpDesc) and the batch's still-transformed ARGB
    words with the transforms' data (uint8 numpy array, or a page-locked torch tensor; 4-byte aligned)."""


class Vp8Stage(HostStage):
    """What ``entropy_decode_vp8s`` returns: ``desc`` (ctypes array of Vp8Desc), the batch's macroblock records and dequantised
    coefficients (uint8 numpy array, or a page-locked torch tensor; 8-byte aligned, only what the images used) and
    ``scratch_bytes``, the size of the device buffer their Y / U / V planes need."""


class Format(NamedTuple):
    """One row of ``FORMATS``: all that tells the staged path of one input format from that of another."""
    word: str                    # what the format's messages call an image: "<word> image K: ..."
    desc: type                   # its descriptor in _abi
    probe: str                   # C symbol: one file -> size, and the stream bytes it may need
    batch: str                   # C symbol: the files of a batch -> descriptors and stream (C++ threads)
    align: int                   # the stream's word in bytes: the buffer is aligned to it and holds whole words
    trim: bool                   # the batch call packs the stream: only what it used is kept (and copied to the device)
    scratch: Optional[str]       # C symbol that sizes the device scratch buffer of the launch, None: the launch takes none
    launch: str                  # C symbol of the device half
    stage: type                  # what the host stage returns
    bare: bool                   # host_decode returns a batch of this format alone as ``stage`` itself, not as a MixedStage of one part


# The input formats other than JPEG, by the name ``_batch_kinds`` gives their files and ``MixedStage`` gives its attributes.  A fifth
# format is a row here, its signature in ``_batch_kinds``, its descriptor in _abi.py and a pair of public one-line bindings below.
FORMATS: Dict[str, Format] = {
    "png": Format("png", _abi.PngDesc, "vip_png_probe_h", "vip_png_inflate_h", 4, False, None, "vip_png_unfilter_rgb_u8", PngStage, False),
    "webp": Format("webp", _abi.WebpDesc, "vip_webp_probe_h", "vip_webp_entropy_h", 4, False, None, "vip_webp_inverse_rgb_u8", WebpStage, True),
    "vp8": Format("webp", _abi.Vp8Desc, "vip_vp8_probe_h", "vip_vp8_entropy_h", 8, True, "vip_vp8_scratch_bytes",
                  "vip_vp8_reconstruct_rgb_u8", Vp8Stage, True),
}


class MixedStage:
    """``host_decode`` of a batch that is not all JPEG and not all WebP: the PNG subset (if any) inflated, the JPEG subset
    (if any) entropy-decoded, the lossless WebP subset (if any) entropy-decoded, the lossy WebP subset (only with the
    ``lossy_webp`` switch on) token-decoded, and where each image of the batch sits in them: ``jpeg_idx`` / ``jpeg`` and, per row
    of ``FORMATS``, ``png_idx`` / ``png``, ``webp_idx`` / ``webp``, ``vp8_idx`` / ``vp8`` (the stage is None where the list is empty)."""

    n: int
    jpeg_idx: List[int]
    jpeg: Optional[tuple]
    png_idx: List[int]
    png: Optional[PngStage]
    webp_idx: List[int]
    webp: Optional[WebpStage]
    vp8_idx: List[int]
    vp8: Optional[Vp8Stage]

    def __init__(self, n, where, staged):
        """``where``, ``staged``: batch positions and stage (or None) by kind, "jpeg" and every key of ``FORMATS``"""
        self.n = n
        for kind, idx in where.items():
            setattr(self, kind + "_idx", idx)
            setattr(self, kind, staged[kind])

    def __len__(self):
        return self.n

    def subsets(self):
        """(batch positions, stage) of every subset other than the JPEG one that is there, in the order of ``FORMATS``"""
        return [(getattr(self, kind + "_idx"), getattr(self, kind)) for kind in FORMATS if getattr(self, kind) is not None]


def _remap_index(msg: str, index: Optional[Sequence[int]]) -> str:
    if index is None:
        return msg
    return re.sub(r"(png|webp) image (\d+)", lambda m: f"{m.group(1)} image {index[int(m.group(2))]}", msg)


def _host_stage(row: Format, raws: Sequence[bytes], threads: int = 0, pinned: bool = False,
                index: Optional[Sequence[int]] = None) -> HostStage:
    """The host stage of every format of ``FORMATS``: probe each file (size, pixel cap, stream bytes), allocate the batch's stream -
    page-locked with ``pinned`` - and fill it with one batched call (C++ threads, the GIL is released inside the ctypes call).
    ``index``: the batch position of every file, used in error messages."""
    lib = _abi.lib()
    n = len(raws)
    bufs, ptrs, lens, threads = _raw_args(raws, threads)
    probe = getattr(lib, row.probe)
    desc = (row.desc * n)()
    total = 0
    tmp = row.desc()
    need = C.c_size_t(0)
    for i in range(n):
        where = i if index is None else index[i]
        st = probe(ptrs[i], lens[i], C.byref(tmp), C.byref(need))
        if st != 0:
            raise _abi.VipError(f"{row.word} image {where}: {row.probe} failed with vip_status {st}: "
                                f"{lib.vip_last_error().decode('utf-8', 'replace')}")
        if tmp.width * tmp.height > MAX_JPEG_PIXELS:
            raise _abi.VipError(f"{row.word} image {where}: {tmp.width}x{tmp.height} exceeds VIP_MAX_JPEG_PIXELS={MAX_JPEG_PIXELS}")
        total += need.value
    # whole words, and one more so that the buffer is never empty.  One rule for all: the lossless WebP path used to add its word without
    # rounding, and rounds nothing now either, since parse_header in csrc/webp_host.cpp sets *stream_bytes = words * 4
    size = (total + row.align - 1) // row.align * row.align + row.align
    stream_t = torch.empty((size,), dtype=torch.uint8, pin_memory=True) if pinned else None
    stream = stream_t.numpy() if pinned else np.empty((size // row.align,), dtype=f"u{row.align}").view(np.uint8)
    used = C.c_size_t(0)
    st = getattr(lib, row.batch)(ptrs, lens, n, desc, stream.ctypes.data_as(C.c_void_p), stream.size, C.byref(used), threads)
    if st != 0:
        msg = _remap_index(lib.vip_last_error().decode("utf-8", "replace"), index)
        raise _abi.VipError(f"{row.batch} failed with vip_status {st}: {msg}")
    scratch = C.c_size_t(0)
    if row.scratch is not None:
        _abi.check(getattr(lib, row.scratch)(desc, n, C.byref(scratch)), row.scratch)
    out = stream_t if pinned else stream
    if row.trim:
        out = out[:max(int(used.value), row.align)]       # what was not used is not copied to the device
    return row.stage(desc, out, int(scratch.value))


def _stage_into(stage: HostStage, slots: Sequence[int], n: int, rgb: torch.Tensor, device) -> None:
    """Launch the device half of ``stage``'s format for its images, image k writing batch row ``slots[k]`` of ``rgb``."""
    row = next(r for r in FORMATS.values() if isinstance(stage, r.stage))
    maxH, maxW = int(rgb.shape[1]), int(rgb.shape[2])
    full = (row.desc * n)()                           # the other rows get all-zero descriptors: no pass, nothing written
    for k, i in enumerate(slots):
        full[i] = stage.desc[k]
    desc_d = torch.from_numpy(np.frombuffer(bytes(full), dtype=np.uint8).copy()).to(device)
    if isinstance(stage.stream, torch.Tensor):        # page-locked: asynchronous copy
        stream_d = stage.stream.to(device, non_blocking=True)
    else:
        stream_d = torch.from_numpy(stage.stream).to(device)
    if row.scratch is None:
        _launch(row.launch, _p(stream_d), _p(desc_d), n, _p(rgb), maxH, maxW)
    else:
        scratch = torch.empty((stage.scratch_bytes,), dtype=torch.uint8, device=device)      # every byte is written before it is read
        _launch(row.launch, _p(stream_d), stream_d.numel(), _p(desc_d), n, _p(scratch), scratch.numel(), _p(rgb), maxH, maxW)


def _decoded(sizes_host: List[Tuple[int, int]], device, fill) -> DecodedBatch:
    """The frame of every device half: zeroed pixels large enough for images of ``sizes_host`` [(h, w)], ``fill(rgb)`` launches what
    writes them, and the batch is what comes out."""
    maxH = max(h for h, _ in sizes_host)
    maxW = max(w for _, w in sizes_host)
    rgb = torch.zeros((len(sizes_host), maxH, maxW, 3), dtype=torch.uint8, device=device)
    fill(rgb)
    sizes = torch.tensor(sizes_host, dtype=torch.int32, device=device)
    return DecodedBatch(rgb, sizes, sizes_host)


def _decode_stage(staged: HostStage, device) -> DecodedBatch:
    n = len(staged.desc)
    return _decoded([(int(d.height), int(d.width)) for d in staged.desc], device, lambda rgb: _stage_into(staged, range(n), n, rgb, device))


def inflate_pngs(pngs: Sequence[bytes], threads: int = 0, pinned: bool = False,
                 index: Optional[Sequence[int]] = None) -> PngStage:
    """Host stage of the PNG path, the twin of ``entropy_decode``: chunk walk + CRC checks + inflate (C++ threads, the
    GIL is released inside the ctypes call) into the still-filtered scanline stream of the batch.  ``index``: the batch
    position of every PNG, used in error messages.  Raises VipError (naming the image) for a stream that is not a valid
    PNG or whose size exceeds VIP_MAX_JPEG_PIXELS."""
    return _host_stage(FORMATS["png"], pngs, threads, pinned, index)


def decode_png_stage(staged: PngStage, device="cuda") -> DecodedBatch:
    """Device half of the PNG path, the twin of ``decode_entropy``: ``staged`` = ``inflate_pngs(...)``.  Undoes the
    scanline filters and expands to 8-bit RGB like ``tf.image.decode_png(channels=3)`` (dataset/dataset.py:30): gray
    1/2/4 bits by bit replication, palette through PLTE (an index past it is black), alpha dropped (tRNS ignored), 16-bit
    samples reduced to round(v / 257) (libpng ``png_set_scale_16``), Adam7 passes scattered to their pixels."""
    return _decode_stage(staged, device)


def entropy_decode_webps(webps: Sequence[bytes], threads: int = 0, pinned: bool = False,
                         index: Optional[Sequence[int]] = None) -> WebpStage:
    """Host stage of the lossless WebP path, the twin of ``inflate_pngs``: container walk + everything serial in the VP8L
    streams (prefix codes, LZ77, colour cache, the transforms' sub-images; C++ threads, the GIL is released inside the
    ctypes call).  ``index``: the batch position of every WebP, used in error messages.  Raises VipError (naming the
    image) for a lossy or animated file, a damaged stream, or a size beyond VIP_MAX_JPEG_PIXELS."""
    return _host_stage(FORMATS["webp"], webps, threads, pinned, index)


def decode_webp_stage(staged: WebpStage, device="cuda") -> DecodedBatch:
    """Device half of the lossless WebP path, the twin of ``decode_png_stage``: ``staged`` = ``entropy_decode_webps(...)``.
    Undoes the VP8L transforms (predictor, cross-colour, subtract-green, colour indexing) in the reverse of the order
    read and drops alpha: the RGB of libwebp's decoder, bit for bit."""
    return _decode_stage(staged, device)


def lossy_webp_enabled(lossy_webp: Optional[bool] = None) -> bool:
    """The lossy WebP switch: the keyword when it is given, else the ``VIP_WEBP_LOSSY`` knob (default 0), read per call."""
    if lossy_webp is not None:
        return bool(lossy_webp)
    return os.environ.get("VIP_WEBP_LOSSY", "0") == "1"


def webp_is_lossy(raw: bytes) -> bool:
    """True when the first image chunk of a RIFF / WEBP file is ``VP8 `` (a lossy key frame), from the chunk tags alone.  Anything
    else - ``VP8L``, animation, a damaged container - is left to the lossless path and its messages."""
    pos, end = 12, min(len(raw), 8 + int.from_bytes(raw[4:8], "little"))
    while pos + 8 <= end:
        tag = raw[pos:pos + 4]
        if tag == b"VP8 ":
            return True
        if tag in (b"VP8L", b"ANIM", b"ANMF"):
            return False
        size = int.from_bytes(raw[pos + 4:pos + 8], "little")
        pos += 8 + size + (size & 1)
    return False


def entropy_decode_vp8s(webps: Sequence[bytes], threads: int = 0, pinned: bool = False,
                        index: Optional[Sequence[int]] = None) -> Vp8Stage:
    """Host stage of the lossy WebP path, the twin of ``entropy_decode_webps``: container walk, the VP8 key frame's header,
    per-macroblock modes and residual tokens (the boolean decoder; C++ threads, the GIL is released inside the ctypes call),
    dequantised as libwebp does.  ``index``: the batch position of every file, used in error messages.  Raises VipError
    (naming the image) for an animated file, an inter frame, a damaged stream, or a size beyond VIP_MAX_JPEG_PIXELS."""
    return _host_stage(FORMATS["vp8"], webps, threads, pinned, index)


def decode_vp8_stage(staged: Vp8Stage, device="cuda") -> DecodedBatch:
    """Device half of the lossy WebP path, the twin of ``decode_webp_stage``: ``staged`` = ``entropy_decode_vp8s(...)``.
    Intra prediction + inverse WHT / DCT, the in-loop filter, fancy chroma upsampling and YUV -> RGB; alpha dropped: the
    RGB of libwebp's decoder, bit for bit."""
    return _decode_stage(staged, device)


def image_format(raw: bytes, i: int = 0) -> str:
    """"jpeg", "png" or "webp", from the magic bytes (not the file name); anything else raises VipError naming image ``i``."""
    if raw[:2] == b"\xff\xd8":
        return "jpeg"
    if raw[:8] == PNG_SIGNATURE:
        return "png"
    if raw[:4] == b"RIFF" and raw[8:12] == b"WEBP":
        return "webp"
    raise _abi.VipError(f"image {i}: neither a JPEG (FF D8), a PNG (89 50 4E 47 0D 0A 1A 0A) nor a WebP (RIFF....WEBP) signature")


def _batch_kinds(raws: Sequence[bytes], lossy_webp: Optional[bool] = None) -> List[str]:
    """"jpeg" or the key in ``FORMATS`` of every image of a batch: ``image_format``, and with the lossy WebP switch on (``lossy_webp``;
    ``None``: the ``VIP_WEBP_LOSSY`` knob) the WebPs split by their chunk tags into "webp" (lossless) and "vp8" (lossy)."""
    kinds = [image_format(r, i) for i, r in enumerate(raws)]
    if "webp" in kinds and lossy_webp_enabled(lossy_webp):
        kinds = ["vp8" if k == "webp" and webp_is_lossy(r) else k for k, r in zip(kinds, raws)]
    return kinds


def host_decode(raws: Sequence[bytes], threads: int = 0, pinned: bool = False, lossy_webp: Optional[bool] = None):
    """Host stage of ``decode_images``: picks the format of every image by its magic bytes.  An all-JPEG batch returns
    exactly what ``entropy_decode`` returns (same calls, same buffers), an all-WebP batch a ``WebpStage``; anything else
    returns a ``MixedStage``.  Animated WebPs are refused here, before any launch, and so are lossy ones unless the switch
    is on (``lossy_webp``; ``None``: the ``VIP_WEBP_LOSSY`` knob, default 0): then the WebPs are split by their chunk tags, an
    all-lossy batch returns a ``Vp8Stage`` and a ``MixedStage`` carries the lossy subset as ``vp8``.  With the switch off
    the calls made are exactly those made before the switch existed."""
    kinds = _batch_kinds(raws, lossy_webp)
    if kinds.count("jpeg") == len(kinds):            # the common batch: nothing more is done for it here (this runs beside the launching thread)
        return entropy_decode(raws, threads, pinned)
    for kind, row in FORMATS.items():
        if row.bare and kinds.count(kind) == len(kinds):
            return _host_stage(row, raws, threads, pinned)
    order = list(FORMATS)
    order.insert(1, "jpeg")          # the subsets are staged in the order they always were: which of two damaged files is reported hangs on it
    where = {kind: [i for i, k in enumerate(kinds) if k == kind] for kind in order}
    staged = {}
    for kind, idx in where.items():
        sub = [raws[i] for i in idx]
        if not idx:
            staged[kind] = None
        elif kind == "jpeg":
            staged[kind] = entropy_decode(sub, threads, pinned)
        else:
            staged[kind] = _host_stage(FORMATS[kind], sub, threads, pinned, index=idx)
    return MixedStage(len(raws), where, staged)


def decode_staged(staged, device="cuda") -> DecodedBatch:
    """Device half of ``decode_images``: ``staged`` = ``host_decode(...)`` (or ``entropy_decode`` / ``inflate_pngs`` /
    ``entropy_decode_webps``).  In a mixed batch the PNG and WebP kernels write straight into the batch's pixels and the
    JPEG subset, decoded as ``decode_entropy`` does, is copied into its rows."""
    if isinstance(staged, tuple):
        return decode_entropy(staged, device)
    if isinstance(staged, HostStage):
        return _decode_stage(staged, device)
    n = staged.n
    sizes_host: List[Tuple[int, int]] = [(0, 0)] * n
    for idx, sub in staged.subsets():
        for k, i in enumerate(idx):
            d = sub.desc[k]
            sizes_host[i] = (int(d.height), int(d.width))
    jb = None
    if staged.jpeg is not None:
        jb = decode_entropy(staged.jpeg, device)
        for k, i in enumerate(staged.jpeg_idx):
            sizes_host[i] = jb.sizes_host[k]

    def fill(rgb):
        for idx, sub in staged.subsets():
            _stage_into(sub, idx, n, rgb, device)
        if jb is not None:
            rows = torch.tensor(staged.jpeg_idx, dtype=torch.long, device=device)
            rgb[rows, :jb.rgb.shape[1], :jb.rgb.shape[2]] = jb.rgb
    return _decoded(sizes_host, device, fill)


def as_batch(staged) -> DecodedBatch:
    """What the scoring entry points accept, as a ``DecodedBatch``: an already decoded batch is returned as it is, the raw byte
    strings of the images go through ``decode_images`` and a host stage (``host_decode(...)`` and its kin) through ``decode_staged``."""
    if isinstance(staged, DecodedBatch):
        return staged
    if isinstance(staged, (list, tuple)) and len(staged) and isinstance(staged[0], (bytes, bytearray)):
        return decode_images(staged)
    return decode_staged(staged)


def decode_images(raws: Sequence[bytes], device="cuda", threads: int = 0, lossy_webp: Optional[bool] = None) -> DecodedBatch:
    """``build_decoder(ext=...)`` for a batch of JPEG, PNG and / or lossless WebP byte strings (dataset/dataset.py:22-30),
    the format of each image picked from its content; with the ``lossy_webp`` switch on (see ``host_decode``) lossy WebP too."""
    return decode_staged(host_decode(raws, threads, lossy_webp=lossy_webp), device)


def decode_jpegs(jpegs: Sequence[bytes], device="cuda", threads: int = 0) -> DecodedBatch:
    """``tf.image.decode_jpeg(channels=3)`` for a batch (dataset/dataset.py:24-28)."""
    return decode_entropy(entropy_decode(jpegs, threads), device)


def decode_entropy(host_stage, device="cuda") -> DecodedBatch:
    """Device half of ``decode_jpegs``: ``host_stage`` = ``entropy_decode(...)`` (which may have run on another thread
    while the GPU was busy with the previous batch)."""
    desc, coef = host_stage
    n = len(desc)
    max_blocks = max(sum(d.blocks_w[c] * d.blocks_h[c] for c in range(d.ncomp)) for d in desc)
    if isinstance(coef, torch.Tensor):     # page-locked tensor from entropy_decode(pinned=True): asynchronous copy, and the
        coef_d = coef.to(device, non_blocking=True)   # caching host allocator keeps the buffer until the copy has run
    else:
        coef_d = torch.from_numpy(coef).to(device)
    desc_bytes = np.frombuffer(bytes(desc), dtype=np.uint8)
    desc_d = torch.from_numpy(desc_bytes.copy()).to(device)
    planes = torch.empty((coef_d.numel(),), dtype=torch.uint8, device=device)
    return _decoded([(int(d.height), int(d.width)) for d in desc], device,
                    lambda rgb: _launch("vip_jpeg_idct_rgb_u8", _p(coef_d), _p(desc_d), n, max_blocks, _p(planes), _p(rgb),
                                        int(rgb.shape[1]), int(rgb.shape[2])))


SUBSAMPLINGS = {"4:2:0": 420, "420": 420, 420: 420, "4:4:4": 444, "444": 444, 444: 444}


def quality_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """libjpeg's ``jpeg_set_quality(quality, force_baseline)`` tables: (luma, chroma), uint16 [64], natural order (host)."""
    luma, chroma = np.zeros((64,), np.uint16), np.zeros((64,), np.uint16)
    st = _abi.lib().vip_jpeg_quality_tables_h(int(quality), luma.ctypes.data_as(C.c_void_p), chroma.ctypes.data_as(C.c_void_p))
    _abi.check(st, "vip_jpeg_quality_tables_h")
    return luma, chroma


def encode_layout(sizes_host: Sequence[Tuple[int, int]], quality: int, subsampling="4:2:0"):
    """Host: the descriptors of a batch re-saved as JPEG at ``quality`` / ``subsampling`` - what ``entropy_decode`` would return for the
    files - as ``(desc (ctypes array, coef_off absolute), total int16 coefficients, max_blocks)``.  ``sizes_host`` = [(h, w)]."""
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling {subsampling!r}: expected '4:2:0' or '4:4:4'")
    lib = _abi.lib()
    desc = (_abi.JpegDesc * len(sizes_host))()
    need = C.c_size_t(0)
    done: Dict[Tuple[int, int], Tuple[_abi.JpegDesc, int]] = {}     # a batch holds few distinct sizes
    total = max_blocks = 0
    for i, (h, w) in enumerate(sizes_host):
        if (h, w) not in done:
            tmp = _abi.JpegDesc()
            st = lib.vip_jpeg_encode_layout_h(int(w), int(h), SUBSAMPLINGS[subsampling], int(quality), C.byref(tmp), C.byref(need))
            _abi.check(st, "vip_jpeg_encode_layout_h")
            done[(h, w)] = (tmp, int(need.value))
        tmp, elems = done[(h, w)]
        C.memmove(C.byref(desc[i]), C.byref(tmp), C.sizeof(_abi.JpegDesc))
        for c in range(3):
            desc[i].coef_off[c] += total
        total += elems
        max_blocks = max(max_blocks, elems // 64)
    return desc, total, max_blocks


def recompress(batch: DecodedBatch, quality: int, subsampling: str = "4:2:0") -> DecodedBatch:
    """The batch as it would come back from a JPEG save at ``quality`` (1..100) and a load - dataset/augment.py:110-113 ``JpegCompress``
    (``tf.image.random_jpeg_quality``) at a fixed quality, each image re-saved at its own size: forward colour conversion, chroma
    downsampling, DCT and quantisation on the GPU (``vip_jpeg_fdct_quant_u8``), then the decoder's own ``vip_jpeg_idct_rgb_u8``.  The
    pixels are those of libjpeg(-turbo) writing and reading the file, bit for bit (the entropy coder in between is lossless and is
    skipped).  Returns a new batch of the same sizes; ``batch`` is not touched.  Runs on the current stream; only the descriptors
    (a few hundred bytes per image) come from the host."""
    n, maxH, maxW, _ = batch.rgb.shape
    device = batch.rgb.device
    desc, total, max_blocks = encode_layout(batch.sizes_host, quality, subsampling)
    desc_d = torch.from_numpy(np.frombuffer(bytes(desc), dtype=np.uint8).copy()).to(device)
    coef = torch.empty((total,), dtype=torch.int16, device=device)
    planes = torch.empty((total,), dtype=torch.uint8, device=device)
    rgb = torch.zeros_like(batch.rgb)
    src = batch.rgb if batch.rgb.is_contiguous() else batch.rgb.contiguous()
    _launch("vip_jpeg_fdct_quant_u8", _p(src), _p(desc_d), n, max_blocks, _p(planes), _p(coef), maxH, maxW)
    _launch("vip_jpeg_idct_rgb_u8", _p(coef), _p(desc_d), n, max_blocks, _p(planes), _p(rgb), maxH, maxW)
    return DecodedBatch(rgb, batch.sizes, list(batch.sizes_host))


class WebpEncoded:
    """What ``webp_encode`` leaves on the device: ``desc`` (ctypes array of Vp8Desc, host) and ``desc_d``, ``stream`` (uint8: per image
    the macroblock records and the dequantised coefficients, the layout of ``entropy_decode_vp8s``), ``levels`` (int16 ``[macroblocks
    of the batch, 25, 16]``, raster order), ``scratch`` (uint8: the planes before the loop filter) and ``params`` (Vp8EncParams)."""

    def __init__(self, desc, desc_d, stream, levels, scratch, params):
        self.desc, self.desc_d, self.stream, self.levels, self.scratch, self.params = desc, desc_d, stream, levels, scratch, params


def webp_encode_params(quality: int) -> "_abi.Vp8EncParams":
    """Host: what ``quality`` (1..100) stands for in the lossy WebP re-save - quantiser index, steps, loop-filter level, mode bias"""
    params = _abi.Vp8EncParams()
    _abi.check(_abi.lib().vip_vp8_encode_params_h(_int_arg("quality", quality, 1, 100), C.byref(params)), "vip_vp8_encode_params_h")
    return params


def webp_encode(batch: DecodedBatch, quality: int) -> WebpEncoded:
    """The encoder half of ``webp_recompress``: one launch (``vip_vp8_encode_rgb_u8``) that leaves the batch's macroblock records,
    coefficients, levels and unfiltered planes on the device.  Argument checks run before any launch."""
    quality = _int_arg("quality", quality, 1, 100)
    if not isinstance(batch, DecodedBatch):
        raise ValueError(f"webp_encode: expected a DecodedBatch, got {type(batch).__name__}")
    n, maxH, maxW, _ = batch.rgb.shape
    device = batch.rgb.device
    lib = _abi.lib()
    sizes = np.ascontiguousarray(np.array(batch.sizes_host, dtype=np.int32).reshape(n, 2))
    desc = (_abi.Vp8Desc * n)()
    stream_bytes, scratch_bytes = C.c_size_t(0), C.c_size_t(0)
    _abi.check(lib.vip_vp8_encode_layout_h(sizes.ctypes.data_as(C.c_void_p), n, quality, desc, C.byref(stream_bytes), C.byref(scratch_bytes)),
               "vip_vp8_encode_layout_h")
    params = webp_encode_params(quality)
    desc_d = torch.from_numpy(np.frombuffer(bytes(desc), dtype=np.uint8).copy()).to(device)
    stream = torch.empty((stream_bytes.value,), dtype=torch.uint8, device=device)
    scratch = torch.empty((scratch_bytes.value,), dtype=torch.uint8, device=device)
    levels = torch.empty((sum(d.mb_w * d.mb_h for d in desc), 25, 16), dtype=torch.int16, device=device)
    src = batch.rgb if batch.rgb.is_contiguous() else batch.rgb.contiguous()
    _launch("vip_vp8_encode_rgb_u8", _p(src), _p(desc_d), n, maxH, maxW, quality, _p(stream), stream.numel(), _p(levels), levels.numel(),
            _p(scratch), scratch.numel())
    return WebpEncoded(desc, desc_d, stream, levels, scratch, params)


def webp_recompress(batch: DecodedBatch, quality: int) -> DecodedBatch:
    """The batch as it would come back from a lossy WebP save at ``quality`` (1..100) and a load, each image re-saved at its own size:
    what a CDN or a messenger does to an upload today.  The encoder is the project's own (include/vipcup_hip.h states its rules: libwebp's
    colour conversion and quality curve, mode decision by prediction error, no segments) and stops in front of the entropy coder, which
    is lossless; the decoder half is the lossy WebP input path's loop filter and RGB output, unchanged.  The pixels are those libwebp
    decodes from the file these decisions make, bit for bit.  Returns a new batch of the same sizes; ``batch`` is not touched.  Runs on
    the current stream; only the descriptors come from the host."""
    enc = webp_encode(batch, quality)
    n, maxH, maxW, _ = batch.rgb.shape
    rgb = torch.zeros_like(batch.rgb)
    _launch("vip_vp8_reconstruct_stages_rgb_u8", _p(enc.stream), enc.stream.numel(), _p(enc.desc_d), n, _p(enc.scratch), enc.scratch.numel(),
            _p(rgb), maxH, maxW, 2 | 4)                 # VIP_VP8_STAGE_FILTER | VIP_VP8_STAGE_OUTPUT: the reconstruction stands already
    return DecodedBatch(rgb, batch.sizes, list(batch.sizes_host))


RESAMPLE_FILTERS = {"bilinear": 0, "bicubic": 1, "lanczos": 2}      # VIP_RESAMPLE_* (include/vipcup_hip.h)
_RESAMPLE_TABLES: Dict[Tuple[int, int, str], Tuple[np.ndarray, np.ndarray, int]] = {}
_RESAMPLE_TILE: List[int] = []


def resample_coeffs(in_size: int, out_size: int, filter: str = "bicubic") -> Tuple[np.ndarray, np.ndarray, int]:
    """Host: the integer tables of one axis of an antialiased 8-bit resize, ``(bounds int32 [out, 2] = (first tap, taps), k int32
    [out, ksize], ksize)`` (``vip_resample_coeffs_h``), cached per ``(in, out, filter)`` - a batch holds few sizes."""
    if filter not in RESAMPLE_FILTERS:
        raise ValueError(f"filter {filter!r}: expected one of {', '.join(RESAMPLE_FILTERS)}")
    key = (int(in_size), int(out_size), filter)
    if key not in _RESAMPLE_TABLES:
        lib = _abi.lib()
        ksize = C.c_int(0)
        st = lib.vip_resample_coeffs_h(key[0], key[1], RESAMPLE_FILTERS[filter], None, 0, None, 0, C.byref(ksize))
        _abi.check(st, "vip_resample_coeffs_h")
        bounds = np.zeros((key[1], 2), np.int32)
        k = np.zeros((key[1], ksize.value), np.int32)
        st = lib.vip_resample_coeffs_h(key[0], key[1], RESAMPLE_FILTERS[filter], bounds.ctypes.data_as(C.c_void_p), bounds.size,
                                       k.ctypes.data_as(C.c_void_p), k.size, C.byref(ksize))
        _abi.check(st, "vip_resample_coeffs_h")
        if len(_RESAMPLE_TABLES) >= 256:                  # sizes keep coming (a folder of arbitrary images): start over
            _RESAMPLE_TABLES.clear()
        _RESAMPLE_TABLES[key] = (bounds, k, int(ksize.value))
    return _RESAMPLE_TABLES[key]


def scaled_size(h: int, w: int, percent: int) -> Tuple[int, int]:
    """the size ``rescale`` gives an ``h x w`` image: each side times percent / 100, rounded half up, at least 1"""
    return max(1, int(h * percent / 100 + 0.5)), max(1, int(w * percent / 100 + 0.5))


def rescale(batch: DecodedBatch, percent: int, filter: str = "bicubic") -> DecodedBatch:
    """The batch as an image editor or an upload would resize it: every image to ``percent`` % of its own size (``scaled_size``) with
    an antialiased ``filter`` (bilinear, bicubic or lanczos: the support widens with the shrink factor), integer arithmetic and a uint8
    result - Pillow's ``Image.resize``, bit for bit (``vip_resample_rgb_u8``, one launch).  This is the first half of the challenge's
    "resized and then JPEG-compressed"; ``recompress`` is the second.  Not the network-input resize (``DecodedBatch.resized``).
    Returns a new batch at the new sizes, pixels outside an image 0; ``batch`` is not touched.  Runs on the current stream; only the
    coefficient tables and their offsets (a few KiB per distinct size) come from the host.  ``percent`` = 100 returns the pixels unchanged."""
    if isinstance(percent, bool) or not isinstance(percent, (int, np.integer)) or not 10 <= int(percent) <= 400:
        raise ValueError(f"percent {percent!r}: expected an integer in 10..400")
    if filter not in RESAMPLE_FILTERS:
        raise ValueError(f"filter {filter!r}: expected one of {', '.join(RESAMPLE_FILTERS)}")
    percent = int(percent)
    new_sizes = [scaled_size(h, w, percent) for h, w in batch.sizes_host]
    for i, (h, w) in enumerate(new_sizes):
        if h * w > MAX_JPEG_PIXELS:
            raise _abi.VipError(f"image {i}: {w}x{h} after a {percent} % resize exceeds VIP_MAX_JPEG_PIXELS={MAX_JPEG_PIXELS}")
    maxHo, maxWo = max(h for h, _ in new_sizes), max(w for _, w in new_sizes)
    rgb = torch.zeros((len(batch), maxHo, maxWo, 3), dtype=torch.uint8, device=batch.rgb.device)
    return _resample_into(batch, new_sizes, filter, rgb)


def resample_plan(sizes_host: Sequence[Tuple[int, int]], new_sizes: Sequence[Tuple[int, int]], filter: str):
    """Host: what ``vip_resample_rgb_u8`` needs besides the pixels - ``(image_tab int32 [n, 8], tables int32, total tiles, widest
    vertical window)`` for images of ``sizes_host`` = [(h, w)] going to ``new_sizes``; the tables of a size pair appear once."""
    if not _RESAMPLE_TILE:
        shape = (C.c_int * 3)()
        st = _abi.lib().vip_resample_tile_shape(C.byref(shape, 0), C.byref(shape, 4), C.byref(shape, 8))
        _abi.check(st, "vip_resample_tile_shape")
        _RESAMPLE_TILE.extend(int(v) for v in shape)
    tile_rows, tile_bytes, _ = _RESAMPLE_TILE
    parts: List[np.ndarray] = []
    placed: Dict[Tuple[int, int], Tuple[int, int, int]] = {}        # (in, out) -> (bounds offset, coefficient offset, ksize)
    used = 0

    def place(n_in, n_out):
        nonlocal used
        if n_in == n_out:
            return 0, 0, 0                                           # skipped pass: the kernel does not read its tables
        if (n_in, n_out) not in placed:
            bounds, k, ksize = resample_coeffs(n_in, n_out, filter)
            placed[(n_in, n_out)] = (used, used + bounds.size, ksize)
            parts.extend((bounds.reshape(-1), k.reshape(-1)))
            used += bounds.size + k.size
        return placed[(n_in, n_out)]

    tab = np.zeros((len(sizes_host), 8), np.int32)
    tiles, max_window = 0, 1
    for i, ((h, w), (ho, wo)) in enumerate(zip(sizes_host, new_sizes)):
        tiles_x = -(-wo * 3 // tile_bytes)
        tab[i] = (tiles, tiles_x) + place(w, wo) + place(h, ho)
        tiles += tiles_x * -(-ho // tile_rows)
        max_window = max(max_window, min(int(tab[i, 7]), h))
    tables = np.concatenate(parts) if parts else np.zeros((1,), np.int32)
    return tab, tables, tiles, max_window


def _slot_pair(batch: DecodedBatch, rgb: torch.Tensor, sizes_host) -> Tuple[torch.Tensor, int, int]:
    """What every ``_..._into`` launch starts with: ``rgb`` is checked to be a destination [n, H, W, 3] for ``batch`` (contiguous uint8 on the
    batch's device) whose slots hold images of ``sizes_host``; returns the batch's pixels, contiguous, and ``(H, W)``."""
    assert rgb.is_contiguous() and rgb.dtype == torch.uint8 and rgb.shape[0] == batch.rgb.shape[0] and rgb.shape[3] == 3 and \
        rgb.device == batch.rgb.device
    assert all(1 <= h <= rgb.shape[1] and 1 <= w <= rgb.shape[2] for h, w in sizes_host)
    return (batch.rgb if batch.rgb.is_contiguous() else batch.rgb.contiguous()), int(rgb.shape[1]), int(rgb.shape[2])


def _blank_like(batch: DecodedBatch) -> torch.Tensor:
    """the zeroed destination of a perturbation that keeps every image's size: the batch's slots, contiguous"""
    return torch.zeros_like(batch.rgb, memory_format=torch.contiguous_format)


def _resample_into(batch: DecodedBatch, new_sizes: List[Tuple[int, int]], filter: str, rgb: torch.Tensor) -> DecodedBatch:
    """``rescale``'s launch: image i of ``batch`` resampled to ``new_sizes[i]`` = (h, w) into its slot of ``rgb`` [n, maxHo, maxWo, 3]
    (contiguous uint8 on the batch's device; only the pixels of the images are written)."""
    n, maxH, maxW, _ = batch.rgb.shape
    device = batch.rgb.device
    src, maxHo, maxWo = _slot_pair(batch, rgb, new_sizes)
    tab, tables, tiles, max_window = resample_plan(batch.sizes_host, new_sizes, filter)
    tab_d = torch.from_numpy(tab).to(device)
    tables_d = torch.from_numpy(tables).to(device)
    sizes = torch.tensor(new_sizes, dtype=torch.int32, device=device)
    _launch("vip_resample_rgb_u8", _p(src), _p(batch.sizes), maxH, maxW, _p(rgb), _p(sizes), maxHo, maxWo, _p(tab_d), _p(tables_d), n,
            tiles, max_window)
    return DecodedBatch(rgb, sizes, list(new_sizes))


_BLUR_WEIGHTS: Dict[Tuple[int, int], np.ndarray] = {}
_BLUR_WEIGHTS_DEV: Dict[Tuple[int, int, int], torch.Tensor] = {}


def _blur_args(sigma, radius) -> Tuple[int, int]:
    """``(round(sigma * 10), radius)`` of a valid ``blur`` call: sigma a multiple of 0.1 in 0.3..5.0, radius None or an integer in 1..15"""
    ok = not isinstance(sigma, bool) and isinstance(sigma, (int, float, np.integer, np.floating)) and np.isfinite(sigma)
    tenths = int(round(float(sigma) * 10)) if ok else 0
    if not ok or not 3 <= tenths <= 50 or abs(float(sigma) * 10 - tenths) > 1e-6:
        raise ValueError(f"sigma {sigma!r}: expected a multiple of 0.1 in 0.3..5.0")
    return tenths, (blur_radius(tenths / 10) if radius is None else _int_arg("radius", radius, 1, 15))


def blur_radius(sigma: float) -> int:
    """the default radius of ``blur``: three sigma, ``max(1, ceil(3 * sigma))``"""
    return max(1, int(np.ceil(3 * float(sigma))))


def blur_weights(sigma: float, radius: Optional[int] = None) -> np.ndarray:
    """Host: the ``2 * radius + 1`` integer weights of one axis of ``blur`` (``vip_blur_weights_h``: a sampled Gaussian normalised in
    double precision, 16 fractional bits, non-negative, summing to exactly 65536), int32, read-only, cached per ``(sigma, radius)``."""
    key = _blur_args(sigma, radius)
    if key not in _BLUR_WEIGHTS:
        w = np.zeros((2 * key[1] + 1,), np.int32)
        _abi.check(_abi.lib().vip_blur_weights_h(key[0] / 10, key[1], w.ctypes.data_as(C.c_void_p), w.size), "vip_blur_weights_h")
        w.setflags(write=False)
        _BLUR_WEIGHTS[key] = w
    return _BLUR_WEIGHTS[key]


def blur(batch: DecodedBatch, sigma: float, radius: Optional[int] = None) -> DecodedBatch:
    """The batch under a Gaussian blur of ``sigma`` pixels (a multiple of 0.1 in 0.3..5.0) cut off at ``radius`` (1..15; default
    ``blur_radius(sigma)``) - dataset/augment.py:131-140 ``Blur``'s ``gaussian_filter2d``, which is ``blur(batch, 1.0, 1)``.  Every image
    is filtered at its own size, each channel separately, edges mirrored without repeating the edge sample (tfa's REFLECT); integer
    arithmetic with 16-bit weights and an 8.8 intermediate, at most one level from the rounded exact convolution
    (``vip_blur_gauss_rgb_u8``, one launch).  Returns a new batch of the same sizes, pixels outside an image 0; ``batch`` is not touched.
    Runs on the current stream; only the weights (at most 31 integers, cached on the device) come from the host."""
    key = _blur_args(sigma, radius)
    return _filter_into(batch, _blank_like(batch), "gauss", key)


def median(batch: DecodedBatch, k: int) -> DecodedBatch:
    """The batch under a ``k x k`` median filter (``k`` 3 or 5) - dataset/augment.py:131-140 ``Blur``'s ``median_filter2d``, which is
    ``median(batch, 3)``.  Every image at its own size, each channel separately, edges mirrored without repeating the edge sample; exact
    (``vip_median_rgb_u8``, one launch).  Returns a new batch of the same sizes, pixels outside an image 0; ``batch`` is not touched."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) not in (3, 5):
        raise ValueError(f"k {k!r}: expected 3 or 5")
    return _filter_into(batch, _blank_like(batch), "median", int(k))


def sharpen_amount(percent: int) -> int:
    """The gain ``vip_sharpen_rgb_u8`` takes for ``percent`` (an integer in 1..500): ``a = round(256 percent / 100)`` in exact integer
    arithmetic (64 percent / 25 never meets a tie): 1 -> 3, 100 -> 256, 500 -> 1280"""
    return (256 * _int_arg("percent", percent, 1, 500) + 50) // 100


def sharpen(batch: DecodedBatch, percent: int, sigma: float = 1.0, radius: Optional[int] = None, threshold: int = 0) -> DecodedBatch:
    """The batch under an unsharp mask, the sharpening a platform adds after a downscale: with ``B = blur(batch, sigma, radius)`` (its
    uint8 pixels, bit for bit) and ``d = X - B``, every sample becomes ``clamp(X + ((a d + 128) >> 8), 0, 255)`` where ``|d| >
    threshold`` and stays ``X`` elsewhere; ``a = sharpen_amount(percent)``, ``percent`` an integer in 1..500, ``threshold`` an integer in
    0..255, ``sigma`` and ``radius`` as for ``blur``.  Integer arithmetic, at most one level from ``round(X + percent / 100 (X - B))``
    clamped (``vip_sharpen_rgb_u8``: ONE launch, the blurred image never reaches global memory).  Pillow's ``UnsharpMask`` blurs with
    a box approximation of the Gaussian: close to this, not bit for bit.  Returns a new batch of the same sizes, pixels outside an
    image 0; ``batch`` is not touched.  Runs on the current stream; only the weights (cached on the device) come from the host."""
    a = sharpen_amount(percent)
    key = _blur_args(sigma, radius) + (a, _int_arg("threshold", threshold, 0, 255))
    return _filter_into(batch, _blank_like(batch), "sharpen", key)


def _filter_into(batch: DecodedBatch, rgb: torch.Tensor, kind: str, arg) -> DecodedBatch:
    """``blur``'s (``kind`` "gauss", ``arg`` = (round(sigma * 10), radius)), ``median``'s (``kind`` "median", ``arg`` = k) and
    ``sharpen``'s (``kind`` "sharpen", ``arg`` = (round(sigma * 10), radius, ``sharpen_amount``, threshold)) launch:
    image i of ``batch`` filtered into its slot of ``rgb`` [n, H, W, 3] (contiguous uint8 on the batch's device, slots at least as large
    as the images; only the pixels of the images are written)."""
    n, maxH, maxW, _ = batch.rgb.shape
    device = batch.rgb.device
    src, dstH, dstW = _slot_pair(batch, rgb, batch.sizes_host)
    if kind in ("gauss", "sharpen"):
        dkey = (device.index or 0,) + tuple(arg[:2])
        if dkey not in _BLUR_WEIGHTS_DEV:
            _BLUR_WEIGHTS_DEV[dkey] = torch.from_numpy(blur_weights(arg[0] / 10, arg[1]).copy()).to(device)
        if kind == "gauss":
            _launch("vip_blur_gauss_rgb_u8", _p(src), _p(batch.sizes), maxH, maxW, _p(rgb), dstH, dstW,
                    _p(_BLUR_WEIGHTS_DEV[dkey]), int(arg[1]), n)
        else:
            _launch("vip_sharpen_rgb_u8", _p(src), _p(batch.sizes), maxH, maxW, _p(rgb), dstH, dstW,
                    _p(_BLUR_WEIGHTS_DEV[dkey]), int(arg[1]), int(arg[2]), int(arg[3]), n)
    else:
        _launch("vip_median_rgb_u8", _p(src), _p(batch.sizes), maxH, maxW, _p(rgb), dstH, dstW, int(arg), n)
    return DecodedBatch(rgb, batch.sizes, list(batch.sizes_host))


WARP_FILLS = {"black": 0, "mirror": 1}                 # VIP_WARP_FILL_* (include/vipcup_hip.h)


def warp_matrix(a: float, b: float, tx: float, c: float, d: float, ty: float) -> List[int]:
    """The inverse map ``(X, Y) -> (a X + b Y + tx, c X + d Y + ty)`` (output point to source point, pixel-edge coordinates: pixel x
    covers [x, x + 1)) as the six integers of ``warp``: coefficients ``floor(v * 2^24 + 0.5)``, offsets ``floor(v * 2^25 + 0.5)``."""
    vals = [float(v) for v in (a, b, tx, c, d, ty)]
    if not all(math.isfinite(v) and abs(v) < 2.0 ** 31 for v in vals):
        raise ValueError(f"warp_matrix {vals!r}: expected six finite numbers below 2^31")
    return [math.floor(v * (2.0 ** 25 if k % 3 == 2 else 2.0 ** 24) + 0.5) for k, v in enumerate(vals)]


def _fill_arg(fill, allowed) -> str:
    if not isinstance(fill, str) or fill not in allowed:
        raise ValueError(f"fill {fill!r}: expected one of {', '.join(allowed)}")
    return fill


def warp(batch: DecodedBatch, xforms, out_sizes: Sequence[Tuple[int, int]], fill: str = "black") -> DecodedBatch:
    """The general geometric transform: image i of the batch under the inverse affine map ``xforms[i]`` (int64 ``[n, 6]``, one
    ``warp_matrix`` per image) into an image of ``out_sizes[i]`` = (h, w), bilinear taps in integer arithmetic
    (``vip_warp_affine_rgb_u8``, one launch; the arithmetic is stated in include/vipcup_hip.h).  ``fill``: ``"black"`` - a tap outside
    the image is 0 (tfa's ``constant``, the reference's ``CFG.fill_mode``) - or ``"mirror"`` (reflect without repeating the edge sample).
    Returns a new batch at ``out_sizes``, pixels outside an image 0; ``batch`` is not touched.  Runs on the current stream; only the
    transforms and sizes (56 bytes per image) come from the host."""
    _fill_arg(fill, WARP_FILLS)
    xf = np.asarray(xforms)
    if xf.dtype != np.int64 or xf.ndim != 2 or xf.shape[1] != 6:
        raise ValueError(f"xforms: expected an int64 [n, 6] array, got {xf.dtype} {tuple(xf.shape)}")
    sizes = []
    for i, s in enumerate(out_sizes):
        if len(s) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1 for v in s):
            raise ValueError(f"out_sizes[{i}] {s!r}: expected (height, width), positive integers")
        sizes.append((int(s[0]), int(s[1])))
    if len(sizes) != xf.shape[0] or len(sizes) != len(batch):
        raise ValueError(f"warp: {len(batch)} images, {xf.shape[0]} transforms, {len(sizes)} output sizes")
    for i, (h, w) in enumerate(sizes):
        if h * w > MAX_JPEG_PIXELS:
            raise _abi.VipError(f"image {i}: {w}x{h} after the warp exceeds VIP_MAX_JPEG_PIXELS={MAX_JPEG_PIXELS}")
    rgb = torch.zeros((len(batch), max(h for h, _ in sizes), max(w for _, w in sizes), 3), dtype=torch.uint8, device=batch.rgb.device)
    return _warp_into(batch, np.ascontiguousarray(xf), sizes, WARP_FILLS[fill], rgb)


def _warp_into(batch: DecodedBatch, xf: np.ndarray, out_sizes: List[Tuple[int, int]], fill: int, rgb: torch.Tensor) -> DecodedBatch:
    """``warp``'s launch: image i of ``batch`` warped to ``out_sizes[i]`` = (h, w) into its slot of ``rgb`` [n, H, W, 3] (contiguous uint8
    on the batch's device, slots at least as large as the output sizes; only the pixels of the images are written)."""
    n, maxH, maxW, _ = batch.rgb.shape
    device = batch.rgb.device
    src, dstH, dstW = _slot_pair(batch, rgb, out_sizes)
    sizes = torch.tensor(out_sizes, dtype=torch.int32, device=device)
    xf_d = torch.from_numpy(xf).to(device)
    _launch("vip_warp_affine_rgb_u8", _p(src), _p(batch.sizes), maxH, maxW, _p(rgb), _p(sizes), dstH, dstW,
            _p(xf_d), int(fill), n)
    return DecodedBatch(rgb, sizes, list(out_sizes))


def flip(batch: DecodedBatch, axis: str) -> DecodedBatch:
    """The batch mirrored left-right (``axis`` "h") or top-bottom ("v") - dataset/augment.py:115-120 ``RandomFlip`` on the decoded
    pixels at their own size; an exact copy (``warp`` with whole-pixel coordinates).  Returns a new batch; ``batch`` is not touched."""
    if not isinstance(axis, str) or axis not in ("h", "v"):
        raise ValueError(f"axis {axis!r}: expected 'h' or 'v'")
    xf = [warp_matrix(-1, 0, w, 0, 1, 0) if axis == "h" else warp_matrix(1, 0, 0, 0, -1, h) for h, w in batch.sizes_host]
    return warp(batch, np.array(xf, np.int64).reshape(-1, 6), list(batch.sizes_host), "black")


def crop(batch: DecodedBatch, percent: int, origin: str = "centre") -> DecodedBatch:
    """The batch cropped to ``percent`` % (an integer in 50..99) of each side (``scaled_size``), taken from the middle - at
    ``((h - h') // 2, (w - w') // 2)`` - or with ``origin="topleft"`` at (0, 0), which keeps the pixels on the 8 x 8 grid of a JPEG
    source.  An exact copy.  Returns a new batch at the new sizes; ``batch`` is not touched."""
    percent = _int_arg("percent", percent, 50, 99)
    if not isinstance(origin, str) or origin not in ("centre", "topleft"):
        raise ValueError(f"origin {origin!r}: expected 'centre' or 'topleft'")
    sizes = [scaled_size(h, w, percent) for h, w in batch.sizes_host]
    xf = [warp_matrix(1, 0, (w - ww) // 2 if origin == "centre" else 0, 0, 1, (h - hh) // 2 if origin == "centre" else 0)
          for (h, w), (hh, ww) in zip(batch.sizes_host, sizes)]
    return warp(batch, np.array(xf, np.int64).reshape(-1, 6), sizes, "black")


def _rotate_args(degrees, fill) -> Tuple[int, str]:
    """``(round(degrees * 10), fill)`` of a valid ``rotate`` call"""
    ok = not isinstance(degrees, bool) and isinstance(degrees, (int, float, np.integer, np.floating)) and np.isfinite(degrees)
    tenths = int(round(float(degrees) * 10)) if ok else 0
    if not ok or tenths == 0 or not -450 <= tenths <= 450 or abs(float(degrees) * 10 - tenths) > 1e-6:
        raise ValueError(f"degrees {degrees!r}: expected a non-zero multiple of 0.1 in -45..45")
    return tenths, _fill_arg(fill, ("crop", "mirror", "black"))


def rotated_rect(h: int, w: int, degrees: float) -> Tuple[int, int]:
    """``(h', w')``: the largest axis-aligned rectangle, centred, that lies inside an ``h x w`` image rotated by ``degrees`` - what is
    left after an editor's "straighten"; each side floored, at least 1."""
    t = math.radians(float(degrees))
    s, c = abs(math.sin(t)), abs(math.cos(t))
    long_side, short_side = max(h, w), min(h, w)
    if short_side <= 2.0 * s * c * long_side or s == c:   # half-constrained: two corners touch the long sides
        x = 0.5 * short_side
        wr, hr = (x / s, x / c) if w >= h else (x / c, x / s)
    else:
        wr, hr = (w * c - h * s) / (c * c - s * s), (h * c - w * s) / (c * c - s * s)
    return max(1, int(math.floor(hr))), max(1, int(math.floor(wr)))


def rotate(batch: DecodedBatch, degrees: float, fill: str = "crop") -> DecodedBatch:
    """The batch rotated counter-clockwise by ``degrees`` (a non-zero multiple of 0.1 in -45..45; Pillow's direction) about each
    image's centre, bilinear - dataset/augment.py:68-107 ``ShiftScaleShearRotate``'s ``tfa.image.rotate`` on the decoded pixels at
    their own size.  ``fill``: ``"crop"`` (what an editor's "straighten" does) outputs the largest axis-aligned rectangle inside the
    rotated image (``rotated_rect``), so no tap leaves the image (taps are mirrored, which only matters for 1-pixel axes); ``"black"``
    (the reference's constant fill) and ``"mirror"`` keep the size.  At most 1 level from Pillow's ``Image.rotate(BILINEAR)``.
    Returns a new batch; ``batch`` is not touched."""
    tenths, fill = _rotate_args(degrees, fill)
    t = math.radians(tenths / 10)
    a, b, c, d = math.cos(t), -math.sin(t), math.sin(t), math.cos(t)
    sizes = [rotated_rect(h, w, tenths / 10) if fill == "crop" else (h, w) for h, w in batch.sizes_host]
    xf = [warp_matrix(a, b, w / 2 - a * ww / 2 - b * hh / 2, c, d, h / 2 - c * ww / 2 - d * hh / 2)   # output centre -> source centre
          for (h, w), (hh, ww) in zip(batch.sizes_host, sizes)]
    return warp(batch, np.array(xf, np.int64).reshape(-1, 6), sizes, "black" if fill == "black" else "mirror")


GRAY_Q16 = (19595, 38470, 7471)                        # Pillow's convert("L"): (R 19595 + G 38470 + B 7471 + 32768) >> 16
YIQ = ((0.299, 0.587, 0.114), (0.596, -0.274, -0.322), (0.211, -0.523, 0.312))     # NTSC: RGB -> (Y, I, Q)
COLOUR_M_MAX, COLOUR_O_MAX = 1 << 18, 1 << 25          # the bounds of vip_colour_rgb_u8 (include/vipcup_hip.h)
_LUT_DEV: Dict[Tuple[int, bytes], torch.Tensor] = {}    # (device, table bytes) -> the table on that device, the last _LUT_DEV_MAX used
_LUT_DEV_MAX = 32


def _q16(x) -> np.ndarray:
    """``floor(x * 65536 + 0.5)`` in float64, as int64"""
    return np.floor(np.asarray(x, np.float64) * 65536.0 + 0.5).astype(np.int64)


def _ints(name: str, v, shape, bound: int) -> np.ndarray:
    """``v`` as an int64 array of ``shape`` whose entries are integers of magnitude at most ``bound``; None: zeros"""
    if v is None:
        return np.zeros(shape, np.int64)
    try:
        arr = np.asarray(v)
    except ValueError:
        arr = np.zeros((0,))
    if arr.shape != shape or arr.dtype.kind not in "iu":
        raise ValueError(f"{name} {v!r}: expected {' x '.join(str(s) for s in shape)} integers")
    arr = arr.astype(np.int64)
    if (np.abs(arr) > bound).any():
        raise ValueError(f"{name}: {int(arr.flat[int(np.abs(arr).argmax())])} is outside -{bound}..{bound}")
    return arr


def _colour_coef(M, K, O, lut) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """the 15 int32 of ``vip_colour_rgb_u8`` (M row by row, K, O) and the table as 256 uint8 or None, validated"""
    if M is None:
        raise ValueError("M None: expected 3 x 3 integers")
    coef = np.concatenate([_ints("M", M, (3, 3), COLOUR_M_MAX).ravel(), _ints("K", K, (3,), COLOUR_M_MAX),
                           _ints("O", O, (3,), COLOUR_O_MAX)]).astype(np.int32)
    if lut is not None:
        lut = _ints("lut", lut, (256,), 255)
        if (lut < 0).any():
            raise ValueError(f"lut: {int(lut.min())} is outside 0..255")
        lut = lut.astype(np.uint8)
    return coef, lut


def colour(batch: DecodedBatch, M, K=None, O=None, lut=None, mean: Optional[torch.Tensor] = None) -> DecodedBatch:
    """The general colour transform: every pixel (R, G, B) of image i becomes, per output channel c and in 32-bit integers,
    ``v = clamp((M[c][0] R + M[c][1] G + M[c][2] B + K[c] mean_i[c] + O[c] + 32768) >> 16, 0, 255)`` and then ``lut[v]`` when a table is
    given (``vip_colour_rgb_u8``, one launch; include/vipcup_hip.h).  ``M`` 3 x 3 and ``K`` Q16 integers of magnitude at most 2^18,
    ``O`` Q16 integers of magnitude at most 2^25, ``lut`` 256 integers in 0..255; ``mean_i`` is the image's own rounded mean colour,
    ``batch.mean_colour()`` - computed here only when some ``K`` is not 0 and ``mean`` (that tensor, from an earlier call) is not given.
    Returns a new batch of the same sizes, pixels outside an image 0; ``batch`` is not touched.  Runs on the current stream; the
    coefficients travel as kernel arguments, a table is copied to the device once and cached (the 32 tables used last)."""
    coef, lut = _colour_coef(M, K, O, lut)
    return _colour_into(batch, coef, lut, mean, _blank_like(batch))


def _colour_into(batch: DecodedBatch, coef: np.ndarray, lut: Optional[np.ndarray], mean: Optional[torch.Tensor],
                 rgb: torch.Tensor) -> DecodedBatch:
    """``colour``'s launch: image i of ``batch`` into its slot of ``rgb`` [n, H, W, 3] (contiguous uint8 on the batch's device, slots at
    least as large as the images; only the pixels of the images are written)."""
    n, maxH, maxW, _ = batch.rgb.shape
    device = batch.rgb.device
    assert coef.dtype == np.int32 and coef.shape == (15,) and coef.flags.c_contiguous
    src, dstH, dstW = _slot_pair(batch, rgb, batch.sizes_host)
    if coef[9:12].any():
        if mean is None:
            mean = batch.mean_colour()
        assert mean.dtype == torch.uint8 and tuple(mean.shape) == (n, 4) and mean.is_contiguous() and mean.device == device
    else:
        mean = None
    lut_d = None
    if lut is not None:
        key = (torch.cuda.current_device() if device.index is None else device.index, lut.tobytes())
        lut_d = _LUT_DEV.pop(key, None)
        if lut_d is None:
            lut_d = torch.from_numpy(lut.copy()).to(device)
        _LUT_DEV[key] = lut_d                           # most recently used last
        while len(_LUT_DEV) > _LUT_DEV_MAX:
            del _LUT_DEV[next(iter(_LUT_DEV))]
    _launch("vip_colour_rgb_u8", _p(src), _p(batch.sizes), maxH, maxW, _p(rgb), dstH, dstW,
            coef.ctypes.data_as(C.c_void_p), _p(mean), _p(lut_d), n)
    return DecodedBatch(rgb, batch.sizes, list(batch.sizes_host))


def _identity_q16() -> np.ndarray:
    return np.eye(3, dtype=np.int64) << 16


def colour_gray():
    """``(M, K, O, lut)`` of ``gray``: every output channel Pillow's ``convert("L")`` luma, ``(19595 R + 38470 G + 7471 B + 32768) >> 16``"""
    return np.array([GRAY_Q16] * 3, np.int64), None, None, None


def colour_bgr():
    """``(M, K, O, lut)`` of ``bgr``: the channels reversed, an exact copy"""
    return _identity_q16()[::-1].copy(), None, None, None


def colour_hue(degrees: int):
    """``(M, K, O, lut)`` of ``hue``: ``M = q(inv(T) R(theta) T)``, ``T`` the NTSC YIQ matrix, ``R`` the rotation of the (I, Q) plane by
    ``degrees`` (a non-zero integer in -180..180), ``q(x) = floor(x * 65536 + 0.5)`` - the LINEAR form of a hue shift"""
    d = _int_arg("degrees", degrees, -180, 180)
    if d == 0:
        raise ValueError(f"degrees {degrees!r}: expected a non-zero integer in -180..180")
    T = np.array(YIQ, np.float64)
    t = np.deg2rad(np.float64(d))
    R = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(t), -np.sin(t)], [0.0, np.sin(t), np.cos(t)]], np.float64)
    return _q16(np.linalg.inv(T) @ R @ T), None, None, None


def _percent_not_100(name: str, percent) -> float:
    p = _int_arg(name, percent, 0, 200)
    if p == 100:
        raise ValueError(f"{name} {percent!r}: expected an integer in 0..200 other than 100")
    return p / 100.0


def colour_saturation(percent: int):
    """``(M, K, O, lut)`` of ``saturation``: ``M = q(f I + (1 - f) [w; w; w])`` with ``f = percent / 100`` (an integer in 0..200, not
    100) and ``w`` the luma weights (19595, 38470, 7471) / 65536 - a blend with the gray image, the LINEAR form; 0 is ``colour_gray``"""
    f = _percent_not_100("percent", percent)
    w = np.array(GRAY_Q16, np.float64) / 65536.0
    return _q16(f * np.eye(3) + (1.0 - f) * np.tile(w, (3, 1))), None, None, None


def colour_contrast(percent: int):
    """``(M, K, O, lut)`` of ``contrast``: ``M = q(f I)``, ``K = q(1 - f)`` on every channel, ``f = percent / 100`` (an integer in
    0..200, not 100): ``(x - mean_c) f + mean_c`` with the image's own per-channel mean, ``tf.image.adjust_contrast``"""
    f = _percent_not_100("percent", percent)
    return _q16(f * np.eye(3)), _q16([1.0 - f] * 3), None, None


def colour_brightness(percent: int):
    """``(M, K, O, lut)`` of ``brightness``: the identity and ``O = q(percent / 100 * 255)`` (a non-zero integer in -50..50): a delta in
    units of full scale, ``tf.image.adjust_brightness``"""
    p = _int_arg("percent", percent, -50, 50)
    if p == 0:
        raise ValueError(f"percent {percent!r}: expected a non-zero integer in -50..50")
    return _identity_q16(), None, _q16([p / 100.0 * 255.0] * 3), None


def _gamma_hundredths(g) -> int:
    ok = not isinstance(g, bool) and isinstance(g, (int, float, np.integer, np.floating)) and np.isfinite(g)
    hundredths = int(round(float(g) * 100)) if ok else 0
    if not ok or not 50 <= hundredths <= 200 or hundredths == 100 or abs(float(g) * 100 - hundredths) > 1e-6:
        raise ValueError(f"gamma {g!r}: expected a decimal in 0.50..2.00 with at most two fractional digits, other than 1")
    return hundredths


def colour_gamma(g: float):
    """``(M, K, O, lut)`` of ``gamma``: the identity and ``lut[v] = floor(255 (v / 255) ** g + 0.5)`` (``g`` in 0.50..2.00 with two
    decimals, not 1; below 1 brightens), ``tf.image.adjust_gamma``"""
    g = _gamma_hundredths(g) / 100.0
    lut = np.floor(255.0 * (np.arange(256, dtype=np.float64) / 255.0) ** g + 0.5).astype(np.int64)
    return _identity_q16(), None, None, lut


def gray(batch: DecodedBatch) -> DecodedBatch:
    """The batch as gray images in three equal channels - dataset/augment.py:142-146 ``RandomGray`` on the decoded pixels at their own
    size, with Pillow's integer luma.  (``apply_augment``'s ``gray`` flag works on resized float inputs; this output can go into
    ``recompress``.)  Returns a new batch; ``batch`` is not touched."""
    return colour(batch, *colour_gray())


def bgr(batch: DecodedBatch) -> DecodedBatch:
    """The batch with red and blue exchanged - dataset/augment.py:148-151 ``RandomBGR``; an exact copy.  Returns a new batch."""
    return colour(batch, *colour_bgr())


def hue(batch: DecodedBatch, degrees: int) -> DecodedBatch:
    """The batch with its chroma rotated by ``degrees`` (``colour_hue``: a rotation in the YIQ plane, not ``tf.image``'s HSV round
    trip; gray pixels stay as they are) - dataset/augment.py:122-129 ``RandomJitter``.  Returns a new batch."""
    return colour(batch, *colour_hue(degrees))


def saturation(batch: DecodedBatch, percent: int) -> DecodedBatch:
    """The batch at ``percent`` % of its saturation (``colour_saturation``: a blend with the luma image, not ``tf.image``'s HSV round
    trip; 0 is ``gray``, above 100 clips) - dataset/augment.py:122-129.  Returns a new batch."""
    return colour(batch, *colour_saturation(percent))


def contrast(batch: DecodedBatch, percent: int, mean: Optional[torch.Tensor] = None) -> DecodedBatch:
    """The batch at ``percent`` % of its contrast about each image's own mean colour (``colour_contrast``; the mean is
    ``batch.mean_colour()``, or ``mean`` when the caller has it already) - dataset/augment.py:122-129.  Returns a new batch."""
    return colour(batch, *colour_contrast(percent), mean=mean)


def brightness(batch: DecodedBatch, percent: int) -> DecodedBatch:
    """The batch with ``percent`` % of full scale added to every sample (``colour_brightness``) - dataset/augment.py:122-129.  Returns
    a new batch."""
    return colour(batch, *colour_brightness(percent))


def gamma(batch: DecodedBatch, g: float) -> DecodedBatch:
    """The batch under ``out = 255 (in / 255) ** g`` through a 256-entry table (``colour_gamma``).  Returns a new batch."""
    return colour(batch, *colour_gamma(g))


NOISE_KINDS = {"gaussian": 0, "mono": 1, "speckle": 2, "impulse": 3}       # the modes of vip_noise_rgb_u8 (include/vipcup_hip.h)
_NOISE_TABLE: List[np.ndarray] = []
_NOISE_TABLE_DEV: Dict[int, torch.Tensor] = {}


def noise_table() -> np.ndarray:
    """The Q12 inverse normal CDF of ``vip_noise_rgb_u8``: int32 ``[4097]`` (read-only), ``T[i] = round(4096 Phi^-1(i / 4096))`` for
    0 < i < 4096 in float64 (the lower half computed, the upper half its mirror image), ``T[0] = -16384``, ``T[4096] = 16384``.
    Built once; ``noise`` keeps one copy per device."""
    if not _NOISE_TABLE:
        from statistics import NormalDist
        inv = NormalDist().inv_cdf
        t = np.zeros(4097, np.int32)
        for i in range(1, 2049):
            t[i] = math.floor(4096.0 * inv(i / 4096.0) + 0.5)
            t[4096 - i] = -t[i]
        t[0], t[4096] = -16384, 16384
        t.setflags(write=False)
        _NOISE_TABLE.append(t)
    return _NOISE_TABLE[0]


def _tenths(name: str, v, lo: int, hi: int) -> int:
    """``v`` as tenths: a number in lo / 10 .. hi / 10 with at most one fractional digit"""
    ok = not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
    tenths = int(round(float(v) * 10)) if ok else 0
    if not ok or not lo <= tenths <= hi or abs(float(v) * 10 - tenths) > 1e-6:
        raise ValueError(f"{name} {v!r}: expected a number in {lo / 10}..{hi / 10} with at most one fractional digit")
    return tenths


def noise_amount(kind: str, amount) -> int:
    """The integer ``vip_noise_rgb_u8`` takes for ``amount`` in the user's units, in exact integer arithmetic: ``a = round(256 sigma)``
    for "gaussian" and "mono" (sigma in levels, 0.5..50.0 in steps of 0.1), ``a = round(256 P / 100)`` for "speckle" (an integer
    percent in 1..50), ``thr = round(P / 100 * 2^32)`` for "impulse" (percent, 0.1..50.0 in steps of 0.1).  None of them meets a tie."""
    if kind not in NOISE_KINDS:
        raise ValueError(f"kind {kind!r}: expected one of {', '.join(NOISE_KINDS)}")
    if kind == "speckle":
        return (256 * _int_arg("percent", amount, 1, 50) + 50) // 100
    if kind == "impulse":
        return ((_tenths("percent", amount, 1, 500) << 32) + 500) // 1000
    return (256 * _tenths("sigma", amount, 5, 500) + 5) // 10


def noise_keys(names: Sequence[str]) -> List[int]:
    """One generator key per file: ``zlib.crc32`` of the basename's UTF-8 bytes - a file keeps its noise whatever directory it is read
    from, wherever it stands in the CSV and whatever batch or rank it falls into"""
    import zlib
    return [zlib.crc32(os.path.basename(str(name)).encode("utf-8")) & 0xFFFFFFFF for name in names]


def _noise_keys_arg(keys, n: int) -> np.ndarray:
    """``keys`` as uint32 ``[n]``; None: 0..n-1"""
    if keys is None:
        return np.arange(n, dtype=np.uint32)
    try:
        arr = np.asarray(keys)
    except ValueError:
        arr = np.zeros((0,))
    if arr.shape != (n,) or arr.dtype.kind not in "iu" or (n and (int(arr.min()) < 0 or int(arr.max()) > 0xFFFFFFFF)):
        raise ValueError(f"keys {keys!r}: expected {n} integers in 0..2^32-1, one per image")
    return arr.astype(np.uint32)


def noise(batch: DecodedBatch, kind: str, amount, seed: int = 0, keys=None) -> DecodedBatch:
    """Noise on every image of the batch (``vip_noise_rgb_u8``, one launch; include/vipcup_hip.h has the arithmetic): ``kind``
    "gaussian" (``amount`` = sigma in levels, an independent sample per channel), "mono" (one sample on all three channels), "speckle"
    (``amount`` = percent: every sample is multiplied by 1 + P / 100 z) or "impulse" (``amount`` = percent of the pixels that turn black
    or white); ranges as ``noise_amount``.  The random field is Philox4x32-10 of the pixel's position in its own image under the key
    (``seed``, ``keys[i]``): ``seed`` an integer in 0..2^32-1, ``keys`` one such integer per image (None: 0..n-1; ``noise_keys`` makes
    them from file names) or the int32 device tensor an earlier ``noise_keys_device`` returned.  The same image with the same seed and
    key gets the same pixels in any batch.  Returns a new batch of the same sizes, pixels outside an image 0; ``batch`` is not touched.
    Runs on the current stream."""
    a = noise_amount(kind, amount)
    seed = _int_arg("seed", seed, 0, 0xFFFFFFFF)
    keys_d = keys if isinstance(keys, torch.Tensor) else noise_keys_device(batch, keys)
    return _noise_into(batch, NOISE_KINDS[kind], a, seed, keys_d, _blank_like(batch))


def noise_keys_device(batch: DecodedBatch, keys=None) -> torch.Tensor:
    """``keys`` (as for ``noise``) on the batch's device: int32 ``[n]`` holding the 32-bit words, for several ``noise`` calls on one batch"""
    host = _noise_keys_arg(keys, len(batch))
    return torch.from_numpy(host.view(np.int32).copy()).to(batch.rgb.device)


def _noise_into(batch: DecodedBatch, mode: int, a: int, seed: int, keys_d: torch.Tensor, rgb: torch.Tensor,
                placement: Optional[int] = None) -> DecodedBatch:
    """``noise``'s launch: image i of ``batch`` into its slot of ``rgb`` [n, H, W, 3] (contiguous uint8 on the batch's device, slots at
    least as large as the images; only the pixels of the images are written).  ``placement``: None, or the table placement of
    ``vip_noise_rgb_u8_placed`` (tools/bench_noise.py)."""
    n, maxH, maxW, _ = batch.rgb.shape
    device = batch.rgb.device
    src, dstH, dstW = _slot_pair(batch, rgb, batch.sizes_host)
    if keys_d.dtype != torch.int32 or tuple(keys_d.shape) != (n,) or not keys_d.is_contiguous() or keys_d.device != device:
        raise ValueError(f"keys: expected a contiguous int32 [{n}] tensor on {device}, got {keys_d.dtype} {tuple(keys_d.shape)} on "
                         f"{keys_d.device}")
    table_d = None
    if mode != NOISE_KINDS["impulse"]:                  # the impulses read no table
        key = torch.cuda.current_device() if device.index is None else device.index
        if key not in _NOISE_TABLE_DEV:
            _NOISE_TABLE_DEV[key] = torch.from_numpy(noise_table().copy()).to(device)
        table_d = _NOISE_TABLE_DEV[key]
    args = (_p(src), _p(batch.sizes), maxH, maxW, _p(rgb), dstH, dstW, mode, a, seed, _p(keys_d), _p(table_d))
    if placement is None:
        _launch("vip_noise_rgb_u8", *args, n)
    else:
        _launch("vip_noise_rgb_u8_placed", *args, int(placement), n)
    return DecodedBatch(rgb, batch.sizes, list(batch.sizes_host))


def gaussian_noise(batch: DecodedBatch, sigma: float, seed: int = 0, keys=None) -> DecodedBatch:
    """The batch with Gaussian noise of standard deviation ``sigma`` levels (0.5..50.0 in steps of 0.1) added to every channel
    independently, rounded and clamped: sensor-like noise.  ``noise(batch, "gaussian", ...)``.  Returns a new batch."""
    return noise(batch, "gaussian", sigma, seed, keys)


def mono_noise(batch: DecodedBatch, sigma: float, seed: int = 0, keys=None) -> DecodedBatch:
    """The batch with ONE Gaussian sample of standard deviation ``sigma`` per pixel added to all three channels: luminance noise, the
    chroma untouched up to the clamp.  ``noise(batch, "mono", ...)``.  Returns a new batch."""
    return noise(batch, "mono", sigma, seed, keys)


def speckle(batch: DecodedBatch, percent: int, seed: int = 0, keys=None) -> DecodedBatch:
    """The batch with every sample multiplied by ``1 + percent / 100 * z``, z standard normal per channel (an integer percent in
    1..50): multiplicative noise, strongest in the highlights.  ``noise(batch, "speckle", ...)``.  Returns a new batch."""
    return noise(batch, "speckle", percent, seed, keys)


def impulse(batch: DecodedBatch, percent: float, seed: int = 0, keys=None) -> DecodedBatch:
    """The batch with ``percent`` % of its pixels (0.1..50.0 in steps of 0.1) replaced by black or white, half each: salt and pepper.
    ``noise(batch, "impulse", ...)``.  Returns a new batch."""
    return noise(batch, "impulse", percent, seed, keys)


TONE_MODES = {"autocontrast": 0, "autocontrast_luma": 1, "equalize": 2, "clahe": 3}     # VIP_TONE_* (include/vipcup_hip.h)
TONE_MAX_GRID = 16
# the tiles over which the histogram launch of the three whole-image modes spreads an image (their sum is the image's histogram
# whatever the grid): more workgroups per image against more histograms to write and add up (README.md has the measurement)
_TONE_GLOBAL_GRID = 4


def tone_grid(h: int, w: int, grid: int = 8) -> Tuple[int, int]:
    """``(gy, gx)``, the tiles of an ``h x w`` image under ``clahe(..., grid=grid)``: per axis ``min(grid, max(1, side // 16))``, so that a
    tile is at least 16 pixels wide; tile k of an axis covers ``occlusion_bounds(side, g)[k:k + 2]``.  Pure host arithmetic."""
    grid = _int_arg("grid", grid, 1, TONE_MAX_GRID)
    return min(grid, max(1, int(h) // 16)), min(grid, max(1, int(w) // 16))


def _tone_args(mode, arg, grid) -> Tuple[int, int, int]:
    """``(mode, parameter, grid)`` as the entry points take them, validated"""
    if not isinstance(mode, str) or mode not in TONE_MODES:
        raise ValueError(f"mode {mode!r}: expected one of {', '.join(TONE_MODES)}")
    grid = _int_arg("grid", grid, 1, TONE_MAX_GRID)
    if mode == "equalize":
        if arg is not None:
            raise ValueError(f"arg {arg!r}: equalize takes no argument (None)")
        return TONE_MODES[mode], 0, grid
    if mode == "clahe":
        return TONE_MODES[mode], _tenths("limit", arg, 10, 99), grid
    return TONE_MODES[mode], _int_arg("cutoff", arg, 0, 49), grid


def tone_histograms(batch: DecodedBatch, grid: int, channels: int) -> torch.Tensor:
    """int32 ``[n, slots, channels, 256]`` on the device: per image and tile of ``tone_grid(h, w, grid)`` (tile ``(ky, kx)`` in slot
    ``ky * gx + kx``; ``slots`` = the batch's largest ``gy * gx``, the others zero) the histogram of R, G and B (``channels`` 3) or of the
    luma (1).  ``vip_tone_hist_u8``, one launch on the current stream; the padding of the slots is not read."""
    grid = _int_arg("grid", grid, 1, TONE_MAX_GRID)
    if channels not in (1, 3):
        raise ValueError(f"channels {channels!r}: expected 3 (R, G, B) or 1 (luma)")
    n, maxH, maxW, _ = batch.rgb.shape
    slots = max(min(grid, max(1, h // 16)) * min(grid, max(1, w // 16)) for h, w in set(batch.sizes_host))      # tone_grid, per distinct size
    src = batch.rgb if batch.rgb.is_contiguous() else batch.rgb.contiguous()
    hist = torch.empty((n, slots, channels, 256), dtype=torch.int32, device=batch.rgb.device)
    _launch("vip_tone_hist_u8", _p(src), _p(batch.sizes), n, maxH, maxW, grid, channels, _p(hist), slots)
    return hist


def tone_tables(hist: torch.Tensor, mode: str, arg=None) -> torch.Tensor:
    """The uint8 tables of ``mode`` from ``tone_histograms``' int32 ``[n, slots, C, 256]`` (C = 3 for "autocontrast" and "equalize", 1
    for "autocontrast_luma" and "clahe"): ``[n, C, 256]`` from the sum of an image's slots, for "clahe" ``[n, slots, 256]``, one table per
    tile.  ``vip_tone_lut_u8``, one launch on the current stream."""
    m, param, _ = _tone_args(mode, arg, 1)
    c = 3 if m in (0, 2) else 1
    if hist.dtype != torch.int32 or hist.dim() != 4 or hist.shape[2] != c or hist.shape[3] != 256 or not hist.is_contiguous() or \
            not 1 <= hist.shape[1] <= TONE_MAX_GRID ** 2 or hist.shape[0] < 1:
        raise ValueError(f"hist: expected a contiguous int32 [n, 1..{TONE_MAX_GRID ** 2}, {c}, 256] tensor for {mode}, got {hist.dtype} "
                         f"{tuple(hist.shape)}")
    n, slots = int(hist.shape[0]), int(hist.shape[1])
    lut = torch.empty((n, slots if m == 3 else c, 256), dtype=torch.uint8, device=hist.device)
    _launch("vip_tone_lut_u8", _p(hist), n, slots, m, param, _p(lut))
    return lut


def tone(batch: DecodedBatch, mode: str, arg=None, grid: int = 8) -> DecodedBatch:
    """A tone curve MEASURED from each image's own histogram, on the decoded pixels at their own size (include/vipcup_hip.h has the
    arithmetic).  ``mode`` "autocontrast" (``arg`` = cutoff, an integer percent 0..49: Pillow's ``ImageOps.autocontrast`` per channel, bit
    for bit), "autocontrast_luma" (one table from the luma's histogram on all three channels: ``preserve_tone=True``), "equalize" (``arg``
    None: ``ImageOps.equalize``, bit for bit) or "clahe" (``arg`` = clip limit 1.0..9.9 in steps of 0.1, ``grid`` 1..16 tiles per axis, at
    least 16 pixels each - ``tone_grid``: contrast-limited equalisation of the luma per tile, the tile tables blended bilinearly, the
    chroma kept; ``grid`` is validated and otherwise unused in the other modes).  Three launches on the current stream - histograms,
    tables, pixels - with no host round trip.  Returns a new batch of the same sizes, pixels outside an image 0; ``batch`` is not
    touched."""
    _, _, grid = _tone_args(mode, arg, grid)              # every argument is checked before the first launch
    return _tone_into(batch, mode, arg, grid, _blank_like(batch))


def _tone_into(batch: DecodedBatch, mode: str, arg, grid: int, rgb: torch.Tensor, placement: Optional[int] = None) -> DecodedBatch:
    """``tone``'s launches: image i of ``batch`` into its slot of ``rgb`` [n, H, W, 3] (contiguous uint8 on the batch's device, slots at
    least as large as the images; only the pixels of the images are written).  ``placement``: None, or the table placement of
    ``vip_tone_apply_rgb_u8_placed`` (tools/bench_tone.py)."""
    m = TONE_MODES[mode]
    n, maxH, maxW, _ = batch.rgb.shape
    src, dstH, dstW = _slot_pair(batch, rgb, set(batch.sizes_host))
    g = grid if m == 3 else _TONE_GLOBAL_GRID
    hist = tone_histograms(batch, g, 3 if m in (0, 2) else 1)
    lut = tone_tables(hist, mode, arg)
    args = (_p(src), _p(batch.sizes), maxH, maxW, _p(rgb), dstH, dstW, _p(lut), m, g, int(hist.shape[1]))
    if placement is None:
        _launch("vip_tone_apply_rgb_u8", *args, n)
    else:
        _launch("vip_tone_apply_rgb_u8_placed", *args, int(placement), n)
    return DecodedBatch(rgb, batch.sizes, list(batch.sizes_host))


def autocontrast(batch: DecodedBatch, cutoff: int, luma: bool = False) -> DecodedBatch:
    """The batch with every image's levels stretched to the full range after ``cutoff`` % of its pixels (an integer in 0..49) are cut
    off either end of the histogram - per channel (Pillow's ``ImageOps.autocontrast(cutoff=...)``), or with ``luma`` one curve from the
    luma on all three channels (``preserve_tone=True``).  ``tone(batch, "autocontrast" / "autocontrast_luma", cutoff)``.  Returns a new
    batch."""
    if not isinstance(luma, (bool, np.bool_)):
        raise ValueError(f"luma {luma!r}: expected a bool")
    return tone(batch, "autocontrast_luma" if luma else "autocontrast", cutoff)


def equalize(batch: DecodedBatch) -> DecodedBatch:
    """The batch with every image's histogram flattened per channel (Pillow's ``ImageOps.equalize``).  ``tone(batch, "equalize")``.
    Returns a new batch."""
    return tone(batch, "equalize")


def clahe(batch: DecodedBatch, limit: float, grid: int = 8) -> DecodedBatch:
    """The batch with its local contrast lifted tile by tile: contrast-limited adaptive equalisation of the luma with clip limit
    ``limit`` (1.0..9.9 in steps of 0.1) on ``tone_grid(h, w, grid)`` tiles, the chroma kept - the "HDR look" of an enhance button.
    ``tone(batch, "clahe", limit, grid)``.  Returns a new batch."""
    return tone(batch, "clahe", limit, grid)


# what apply_step reads from its options: apply_chain's keywords but noise_keys
STEP_OPTIONS = ("subsampling", "resize_filter", "blur_radius", "crop_origin", "rotate_fill", "sharpen_sigma", "sharpen_radius", "sharpen_threshold",
                "noise_seed", "clahe_grid")


def apply_step(batch: DecodedBatch, kind: str, arg, options, mean: Optional[torch.Tensor] = None, keys=None, seed: Optional[int] = None) -> DecodedBatch:
    """The batch after ONE perturbation: ``(kind, arg)`` as ``parse_step`` gives it, through the ``pipeline`` function of its family with
    that family's entry of ``options`` (a mapping with ``apply_chain``'s keywords).  The one place where a step kind meets its function:
    a row of ``ensemble.stress_batch`` and a step of ``apply_chain`` are this call.  ``mean``: the batch's mean colour for a ``contrast``
    step (None: measured here); ``keys``: as for ``noise``; ``seed``: a noise step's seed when it is not ``options["noise_seed"]``."""
    if kind in NOISE_KINDS:
        return noise(batch, kind, arg, options["noise_seed"] if seed is None else seed, keys)
    if kind in TONE_MODES:
        return tone(batch, kind, arg, options["clahe_grid"])
    if kind == "recompress":
        return recompress(batch, arg, options["subsampling"])
    if kind == "webp_recompress":
        return webp_recompress(batch, arg)
    if kind == "rescale":
        return rescale(batch, arg, options["resize_filter"])
    if kind == "blur":
        return blur(batch, arg, options["blur_radius"])
    if kind == "crop":
        return crop(batch, arg, options["crop_origin"])
    if kind == "rotate":
        return rotate(batch, arg, options["rotate_fill"])
    if kind == "sharpen":
        return sharpen(batch, arg, options["sharpen_sigma"], options["sharpen_radius"], options["sharpen_threshold"])
    if kind == "contrast":
        return contrast(batch, arg) if mean is None else contrast(batch, arg, mean)
    if kind in ("gray", "bgr"):
        return gray(batch) if kind == "gray" else bgr(batch)
    one_argument = {"median": median, "flip": flip, "hue": hue, "saturation": saturation, "brightness": brightness, "gamma": gamma}
    if kind not in one_argument:
        raise ValueError(f"chain step kind {kind!r}: not a step of parse_chain")
    return one_argument[kind](batch, arg)


def apply_chain(batch: DecodedBatch, steps, *, subsampling: str = "4:2:0", resize_filter: str = "bicubic", blur_radius: Optional[int] = None,
                crop_origin: str = "centre", rotate_fill: str = "crop", sharpen_sigma: float = 1.0, sharpen_radius: Optional[int] = None,
                sharpen_threshold: int = 0, noise_seed: int = 0, noise_keys=None, clahe_grid: int = 8) -> DecodedBatch:
    """The batch after the ``steps`` of a stress chain (``parse_chain(text)``, or the chain's text), applied left to right to the decoded
    pixels at their own size, each through the ``pipeline`` function of its family with that family's options (``apply_step``):
    ``recompress`` (``subsampling``), ``rescale`` (``resize_filter``), ``blur`` (``blur_radius``), ``crop`` (``crop_origin``), ``rotate``
    (``rotate_fill``), ``sharpen`` (``sharpen_sigma``, ``sharpen_radius``, ``sharpen_threshold``).  A ``contrast`` step takes the mean
    colour of the batch as it reaches that step.  A noise step uses ``noise_keys`` (as for ``noise``: one integer per image, None:
    0..n-1, or ``noise_keys_device``'s tensor) and positions in the image as it reaches that step; the k-th noise step of the chain draws
    from seed ``(noise_seed + k) mod 2^32`` (``chain_noise_seeds``).  A tone step (``autocontrast``, ``autocontrast_luma``, ``equalize``,
    ``clahe`` with ``clahe_grid`` tiles per axis) measures the batch as it reaches that step.  Intermediate batches are dropped as the
    chain proceeds.  Returns a new batch; ``batch`` is not touched."""
    options = dict(locals())                            # the keywords above, by name
    steps = parse_chain(steps) if isinstance(steps, str) else list(steps)
    seeds = chain_noise_seeds(steps, _int_arg("noise_seed", noise_seed, 0, 0xFFFFFFFF))
    options["clahe_grid"] = _int_arg("clahe_grid", clahe_grid, 1, TONE_MAX_GRID)
    keys_d = None
    cur = batch
    for (kind, arg), seed in zip(steps, seeds):
        if seed is not None and keys_d is None:         # once per chain: no step changes the number of images
            keys_d = noise_keys if isinstance(noise_keys, torch.Tensor) else noise_keys_device(batch, noise_keys)
        cur = apply_step(cur, kind, arg, options, keys=keys_d, seed=seed)
    return cur


def apply_augment(x: torch.Tensor, hflip, vflip, gray) -> torch.Tensor:
    """Deterministic form of dataset/augment.py ``apply_augment`` (:153-182): per-image flags instead of the
    reference's TF RNG draws (p=0.8 gate, hflip .5, vflip .5, gray .3) — the caller owns the randomness."""
    B, H, W, Cc = x.shape
    flags = (torch.as_tensor(hflip, dtype=torch.int32) | (torch.as_tensor(vflip, dtype=torch.int32) << 1) |
             (torch.as_tensor(gray, dtype=torch.int32) << 2)).to(x.device)
    assert flags.numel() == B
    from . import ops
    if x.dtype == ops.PACKED:                        # flips / grey on the joined fp32 values, split again
        return ops.pack_h2(apply_augment(ops.unpack_h2(x), hflip, vflip, gray))
    out = torch.empty_like(x)
    fn = "vip_tta_augment_s32" if x.dtype == torch.float32 else "vip_tta_augment_f16"
    _launch(fn, _p(x), _p(out), _p(flags), B, H, W, Cc)
    return out


class Dataset:
    """What ``build_dataset`` returns: an iterable of batches with the stream semantics of the reference's tf.data chain
    ``from_tensor_slices(paths).map(decode)[.cache()][.repeat()][.shuffle(buf, seed)][.map(augment)].batch(bs, drop_remainder).prefetch()``
    (dataset/dataset.py:87-101).  Element k of the stream is image ``k % n`` (pass ``k // n``) unless shuffled; batches run across
    the repeat boundary exactly as ``repeat()`` before ``batch()`` makes them.  Each batch is an fp16 NHWC tensor
    ``[bs, H, W, 8]`` resident on the GPU (channels 3..7 zero), or ``(batch, labels)`` when labels were given."""

    def __init__(self, paths, labels, batch_size, cache, decode_fn, augment_fn, img_size, augment, repeat, shuffle,
                 drop_remainder, seed, num_classes, device, threads, dtype=torch.float16):
        self.dtype = dtype
        self.paths = [os.fspath(p) for p in paths]
        self.labels = None if labels is None else np.asarray(labels)
        self.batch_size, self.cache, self.decode_fn, self.augment_fn = int(batch_size), bool(cache), decode_fn, augment_fn
        self.img_size = (int(img_size[0]), int(img_size[1]))
        self.augment, self.repeat, self.shuffle, self.drop_remainder = bool(augment), bool(repeat), int(shuffle or 0), bool(drop_remainder)
        self.seed, self.num_classes, self.device, self.threads = int(seed), int(num_classes), device, threads
        self._cached: Dict[int, torch.Tensor] = {}      # image index -> [H, W, 8] fp16 (``cache=True``: decoded once, kept in HBM)
        self._flags: Dict[int, np.ndarray] = {}         # pass -> bool [n, 3] apply_augment draws

    def __len__(self):
        """batches in one pass (tf.data cardinality of the un-repeated dataset)"""
        n, bs = len(self.paths), self.batch_size
        return n // bs if self.drop_remainder else -(-n // bs)

    def _order(self):
        """stream of (image index, pass) - repeat(), then a buffered shuffle like tf.data's (uniform pick from a buffer)"""
        n = len(self.paths)

        def base():
            t = 0
            while True:
                for i in range(n):
                    yield i, t
                t += 1
                if not self.repeat:
                    return
        if not self.shuffle:
            yield from base()
            return
        rng = np.random.default_rng(self.seed)
        buf = []
        for item in base():
            buf.append(item)
            if len(buf) >= self.shuffle:
                yield buf.pop(int(rng.integers(len(buf))))
        while buf:
            yield buf.pop(int(rng.integers(len(buf))))

    def _host_stage(self, items):
        """read + entropy-decode / inflate the images of one batch that are not cached (runs on the read-ahead thread)"""
        todo = [i for i, _ in items if i not in self._cached]
        todo = list(dict.fromkeys(todo))
        if not todo:
            return todo, None
        if self.decode_fn is not None:                      # caller-supplied decoder: path -> float [H, W, 3] in [0, 1]
            return todo, [np.asarray(self.decode_fn(self.paths[i]), dtype=np.float32) for i in todo]
        raws = []
        for i in todo:
            with open(self.paths[i], "rb") as f:            # tf.io.read_file (dataset.py:24)
                raws.append(f.read())
        return todo, host_decode(raws, self.threads, pinned=torch.cuda.is_available())

    def _device_stage(self, items, staged):
        from . import ops
        todo, host = staged
        fresh: Dict[int, torch.Tensor] = {}
        if todo:
            if self.decode_fn is not None:
                x = ops.to_device_nhwc8(torch.from_numpy(np.stack(host)), self.device, self.dtype)
            else:
                x = decode_staged(host, self.device).resized(self.img_size[0], self.img_size[1], dtype=self.dtype)
            fresh = {i: x[j] for j, i in enumerate(todo)}
            if self.cache:
                self._cached.update(fresh)
        src = self._cached if self.cache else fresh
        batch = torch.stack([src[i] if i in src else fresh[i] for i, _ in items])
        if self.augment:
            if self.augment_fn is not None:
                batch = self.augment_fn(batch)
            else:       # apply_augment (dataset/augment.py:153-182): seeded draws per (pass, image) - TF's RNG stream is not reproducible
                from .ensemble import tta_flags_pass
                need = {t for _, t in items}                # the draws of a pass are a function of (seed, pass): built once per pass
                for t in need:
                    if t not in self._flags:
                        self._flags[t] = tta_flags_pass(len(self.paths), t, self.seed)
                sel = np.stack([self._flags[t][i] for i, t in items])
                # trimmed only AFTER the batch is assembled and never below what it used: a batch may span many passes (fewer images
                # than batch_size / 5) or straddle the restart of a second predict() - a repeating dataset walks the passes in order
                for t in sorted(self._flags):
                    if len(self._flags) <= max(4, len(need)):
                        break
                    if t not in need:
                        del self._flags[t]
                batch = apply_augment(batch, sel[:, 0], sel[:, 1], sel[:, 2])
        if self.labels is None:
            return batch
        lab = torch.as_tensor(self.labels[[i for i, _ in items]])
        if self.num_classes > 1:                            # decode_with_labels (dataset.py:41-46)
            lab = torch.nn.functional.one_hot(lab.long().reshape(-1), self.num_classes)
        return batch, lab.to(torch.float32)

    def __iter__(self):
        from concurrent.futures import ThreadPoolExecutor

        def batches():
            cur = []
            for item in self._order():
                cur.append(item)
                if len(cur) == self.batch_size:
                    yield cur
                    cur = []
            if cur and not self.drop_remainder:
                yield cur
        it = batches()
        with ThreadPoolExecutor(max_workers=1) as pool:     # prefetch(AUTO): the host stage of batch i+1 under the GPU work of batch i
            nxt_items = next(it, None)
            nxt = pool.submit(self._host_stage, nxt_items) if nxt_items is not None else None
            while nxt_items is not None:
                items, staged = nxt_items, nxt.result()
                nxt_items = next(it, None)
                nxt = pool.submit(self._host_stage, nxt_items) if nxt_items is not None else None
                yield self._device_stage(items, staged)


def build_dataset(paths, labels=None, batch_size=32, cache=True, decode_fn=None, augment_fn=None, dim=[200, 200],
                  augment=True, repeat=True, shuffle=1024, cache_dir="", drop_remainder=False, CFG=None,
                  device="cuda", threads: int = 0) -> Dataset:
    """Same signature and stream semantics as the reference's ``build_dataset`` (dataset/dataset.py:64-102); the call
    in main.py:89-98 works unchanged.  Like the reference, the image size comes from ``CFG.img_size`` (``dim`` is only the
    fallback when no CFG is passed), ``CFG.seed`` seeds the shuffle, ``CFG.num_classes`` the label encoding; ``CFG.is_train``
    is set as a side effect (:73).  ``cache`` keeps the decoded, resized batch elements resident in HBM (tf.data's in-memory
    cache); ``cache_dir`` is created when given (:70-71) but nothing is written to it."""
    from . import ops
    if cache_dir != "" and cache is True:
        os.makedirs(cache_dir, exist_ok=True)
    img_size = tuple(dim)
    seed, num_classes = 42, 1
    mode = None
    if CFG is not None:
        CFG.is_train = labels is not None
        img_size = tuple(getattr(CFG, "img_size", dim))
        seed = int(getattr(CFG, "seed", 42))
        num_classes = int(getattr(CFG, "num_classes", 1))
        mode = getattr(CFG, "precision", None)
    # batches are stored in the precision mode's activation dtype: fp16 ("fast"), fp32 ("strict": CFG.precision or ops.PRECISION)
    return Dataset(paths, labels, batch_size, cache, decode_fn, augment_fn, img_size, augment, repeat, shuffle,
                   drop_remainder, seed, num_classes, device, threads, ops.act_dtype(mode))


def predict_dataset(predict_batch, dataset, steps=None, verbose=0, precision=None) -> np.ndarray:
    """``tf.keras.Model.predict(dataset, steps)`` (main.py:109): run ``predict_batch`` over ``ceil(steps)`` batches of the
    iterable (Keras' data handler keeps stepping while ``step < steps``, so the reference's fractional
    ``steps = max(tta * n / batch, 1)`` means its ceiling; ``None`` = until the dataset ends) and return the concatenated
    predictions as a numpy array ``[sum of batch sizes, C]`` - the caller slices off what the repeat padded (main.py:110).
    ``precision`` "strict" (the model's): the packed storage's status word is read once, after the last batch and before the copy to the
    host (``ops.h2_check``: it raises when an activation left the fp16 range and names ``--precision f32``)."""
    import itertools
    import math
    limit = None if steps is None else int(math.ceil(float(steps)))
    outs = []
    # islice stops BEFORE asking the dataset for batch number `limit` (a plain `break` after enumerate would already have pulled it:
    # one more read + Huffman decode + H2D + IDCT + resize per predict call)
    for k, batch in enumerate(dataset if limit is None else itertools.islice(dataset, limit)):
        x = batch[0] if isinstance(batch, (tuple, list)) else batch
        outs.append(predict_batch(x))
        if verbose:
            print(f"{k + 1}/{limit if limit is not None else '?'} batches", end="\r", flush=True)
    if verbose:
        print()
    if not outs:
        return np.zeros((0, 1), dtype=np.float32)
    if precision == "strict":
        from . import ops
        ops.h2_check("predict(dataset)")
    return torch.cat([o.float() for o in outs], 0).cpu().numpy()


def keras_predict(cls):
    """Class decorator: ``model.predict`` keeps taking a resident batch tensor (-> tensor) and ALSO takes what
    ``tf.keras.Model.predict`` takes in main.py:109 - a dataset iterable plus ``steps`` / ``verbose`` (-> numpy ``[n, C]``)."""
    batch_predict = cls.predict

    def checked(self, t):
        prec = getattr(self, "precision", None)           # set by zoo.construct; absent on hand-built models (no check)
        from . import ops
        if prec is not None and t.dtype != ops.act_dtype(prec):
            raise _abi.VipError(f"{type(self).__name__}.predict: a {prec} model got a {t.dtype} batch "
                                "(DecodedBatch.resized(..., dtype=...) / build_dataset with CFG.precision pick the input dtype)")
        return batch_predict(self, t)

    def predict(self, x, steps=None, verbose=0, **_keras_kwargs):
        if isinstance(x, torch.Tensor):
            return checked(self, x)
        return predict_dataset(lambda t: checked(self, t), x, steps, verbose, precision=getattr(self, "precision", None))
    predict.__doc__ = batch_predict.__doc__
    cls.predict = predict
    return cls


def calibration_batch(n: int = 16, seed: int = 20221, device="cuda") -> DecodedBatch:
    """A fixed, seeded batch of synthetic 200x200 RGB images (smooth colour field + pixel noise: the statistics of the
    synthetic test set, SURVEY.md §8d, from a different seed) for ops.calibration().  With real checkpoints pass a
    few real images through ``decode_jpegs`` instead - the correction only needs typical per-channel means."""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn((n, 3, 8, 8), generator=g) * 48.0 + 128.0
    field = torch.nn.functional.interpolate(low.clamp(0, 255), size=(200, 200), mode="bicubic", align_corners=False)
    img = (field + torch.randn((n, 3, 200, 200), generator=g) * 12.0).clamp(0, 255).to(torch.uint8)
    rgb = img.permute(0, 2, 3, 1).contiguous().to(device)
    sizes = torch.tensor([[200, 200]] * n, dtype=torch.int32, device=device)
    return DecodedBatch(rgb, sizes, [(200, 200)] * n)
