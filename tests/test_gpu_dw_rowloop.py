"""The addressing of the register-tiled fp16 depthwise kernel (dwconv_tile_kernel, csrc/dwconv.hip) where tests/_dw_cases.py does not aim:
the kernel decides once per tile which of its patch columns lie inside the image and then walks the rows with one running byte offset,
so a wrong column mask, a row base that is not rebuilt, an offset that wraps or an out-of-range value that comes back into range all
show up as a wrong border, a wrong image or a wrong channel.  Operands are those of tests/_dw_cases.py (integers times quarter-valued
taps: every fp32 sum is exact in any order), the reference is its ref64, the comparison is torch.equal - no tolerance anywhere.
  * maps narrower than one register patch and just wider, at the symmetric pad, the TensorFlow SAME pad of an even map and VALID, with
    8 and 24 channels (1 and 3 chunks: 256 and 85 tiles a workgroup, a wave holds many tiles) and 2 and 3 images (a wave straddles images);
  * C = 200: channel blocks of 16 and 9 chunks, plain and pooling form (idle lanes parked on a tile below the image), partial sums too;
  * an input of 2.2 GB: byte offsets above 2^31 in the last image, a band of its rows against the reference of that band alone.
Every plain case runs through ops.dwconv2d; the pooling form has no other door than the entry point ops.dwconv2d_se calls."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _dw_cases as T  # noqa: E402
from tests import test_gpu_passes as P  # noqa: E402
from tests.test_gpu_dw import _assert_equal  # noqa: E402
from tests.test_gpu_ops import dev  # noqa: E402

_ops = P._ops

# map sizes around the patch: k = 7 reads 10 columns and 8 rows per tile, k = 5 reads 6 x 6, k = 3 reads 6 x 4
SIZES = {7: ((1, 3, 4, 5, 7, 9), (1, 2, 3, 9)), 5: ((1, 2, 3, 5), (1, 2, 3, 5)), 3: ((1, 2, 3, 5), (1, 2, 3, 5))}     # k: (W, H)
# symmetric; TensorFlow SAME of an even map at stride 2 (k = 3: (0,1,0,1), k = 5: (1,2,1,2), continued to k = 7), here at stride 1; VALID
PADS = {"sym": lambda k: (k // 2,) * 4, "tfsame": lambda k: ((k - 2) // 2, k // 2) * 2, "valid": lambda k: (0, 0, 0, 0)}


def _row(name, B, H, W, Cc, k, pad, act):
    return T.Row(name, "f16", "dwconv_tile_kernel", B, H, W, Cc, k, 1, pad, act, None, "")


def _small_rows(k, padname, Cc, B):
    pad = PADS[padname](k)
    rows = []
    for W in SIZES[k][0]:
        for H in SIZES[k][1]:
            row = _row(f"rowloop-k{k}-{padname}-c{Cc}-b{B}-{H}x{W}", B, H, W, Cc, k, pad, "relu" if (H + W) % 2 else None)
            if min(T.out_hw(row)) >= 1:
                rows.append(row)
    return rows


def test_pads_are_the_ones_named():
    assert PADS["tfsame"](3) == (0, 1, 0, 1) and PADS["tfsame"](5) == (1, 2, 1, 2) and PADS["tfsame"](7) == (2, 3, 2, 3)
    assert PADS["sym"](7) == (3, 3, 3, 3) and PADS["valid"](5) == (0, 0, 0, 0)
    # VALID keeps the maps at least as large as the filter, the other pads keep nearly all of them
    assert [len(_small_rows(k, "valid", 8, 2)) for k in (3, 5, 7)] == [4, 1, 2]
    assert [len(_small_rows(k, "sym", 8, 2)) for k in (3, 5, 7)] == [16, 16, 24]
    assert [len(_small_rows(k, "tfsame", 8, 2)) for k in (3, 5, 7)] == [9, 9, 15]


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("Cc", [8, 24])
@pytest.mark.parametrize("padname", list(PADS))
@pytest.mark.parametrize("k", [3, 5, 7])
def test_small_maps_exact(k, padname, Cc, B, report):
    """column validity differs between the lanes of one wave: every map size of the k, one launch each"""
    ops = _ops()
    rows = _small_rows(k, padname, Cc, B)
    assert rows
    for row in rows:
        assert ops.dwconv_tile_plan(row.B, row.H, row.W, row.C, k, pad=row.pad) is not None, row.id
        x, w, b = T.operands(row)
        got = ops.dwconv2d(dev(x), ops.make_dw_weight(w), b.cuda(), k, 1, row.pad, act=row.act)
        _assert_equal(row.id, got.cpu().double(), T.ref64(x, w, b, 1, row.pad, row.act))
    report(f"[dw rowloop] k{k} pad {padname} C{Cc} B{B}: {len(rows)} maps from {rows[0].H}x{rows[0].W} to {rows[-1].H}x{rows[-1].W} bit-exact")


def _vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


# 15 tiles of the 2 x 4 (k = 3, 7) / 2 x 2 (k = 5) register tile in the 16 slots of a group: one slot idle besides the idle chunks
@pytest.mark.parametrize("k,H,W", [(3, 6, 20), (5, 6, 10), (7, 6, 20)])
def test_partly_filled_channel_block_exact(k, H, W, report):
    """C = 200 is 25 chunks: a channel block of 16 and one of 9, whose 7 idle lanes per tile leave the plain kernel and, in the pooling
    form, run a tile below the image on a clamped chunk - nothing of theirs may reach the map or the partial sums"""
    ops = _ops()
    lib = ops._abi.lib()
    B, Cc, pad = 2, 200, (k // 2,) * 4
    row = _row(f"rowloop-c200-k{k}", B, H, W, Cc, k, pad, "relu")
    plan = ops.dwconv_tile_plan(B, H, W, Cc, k, pad=pad)
    assert plan is not None and plan[2]["cb"] == 16 and plan[2]["channel_blocks"] == 2, plan
    x, w, b = T.operands(row)
    ref = T.ref64(x, w, b, 1, pad, row.act)
    xd, wd, bd = dev(x), ops.make_dw_weight(w), b.cuda()
    plain = ops.dwconv2d(xd, wd, bd, k, 1, pad, act=row.act)
    _assert_equal(f"{row.id} plain", plain.cpu().double(), ref)
    parts = lib.vip_dwconv2d_pool_parts(B, H, W, Cc, k, 1, H, W)
    assert parts == 1, parts
    y = torch.full((B, H, W, Cc), float("nan"), dtype=torch.float16, device="cuda")
    partials = torch.full((B, parts, Cc), float("nan"), dtype=torch.float32, device="cuda")
    st = lib.vip_dwconv2d_pool_nhwc_f16(_vp(xd), _vp(wd), _vp(bd), _vp(y), _vp(partials), parts, B, H, W, Cc, k, 1, pad[0], pad[2], H, W,
                                        ops._act(row.act), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, lib.vip_last_error()
    torch.cuda.synchronize()
    _assert_equal(f"{row.id} pooling form", y.cpu().double(), ref)
    assert 4 * ref.abs().sum((1, 2)).max().item() < 2 ** 24              # quarter units: every fp32 partial sum is exact
    sums, want = partials.sum(1).cpu().double(), ref.sum((1, 2))
    assert torch.equal(sums, want), f"{row.id}: {int((sums != want).sum())} of {want.numel()} pooled sums differ"
    report(f"[dw rowloop] {row.id}: {B}x{H}x{W}x{Cc} plain and pooling form bit-exact, {parts} partial row per image exact")


BIG = (12, 300, 300, 1024)      # 2 211 840 000 bytes of fp16: the last image starts below 2^31 and ends above it
BAND = 6                        # output rows checked at the top of the first image and at the bottom of the last


@pytest.fixture(scope="module")
def big_x():
    """integers in [-2, 2] as in tests/_dw_cases.py, drawn on the device (the host generator would take longer than the whole file)"""
    g = torch.Generator(device="cuda").manual_seed(20221)
    x = torch.randint(-2, 3, BIG, generator=g, device="cuda", dtype=torch.int8).to(torch.float16)
    yield x
    del x
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [3, 5, 7])
def test_offsets_above_2_31_exact(k, big_x, report):
    ops = _ops()
    B, H, W, Cc = BIG
    p = k // 2
    assert 2 ** 31 < big_x.numel() * 2 < 2 ** 32 and (B - 1) * H * W * Cc * 2 < 2 ** 31
    assert ((B - 1) * H + H - BAND - p) * W * Cc * 2 > 2 ** 31           # every input row of the last band lies above 2^31
    assert ops.dwconv_tile_plan(B, H, W, Cc, k) is not None
    _, w, b = T.operands(_row(f"rowloop-big-k{k}", 1, 1, 1, Cc, k, (p,) * 4, None))
    got = ops.dwconv2d(big_x, ops.make_dw_weight(w), b.cuda(), k, 1, (p,) * 4)
    assert got.shape == big_x.shape
    # the band's own convolution: its p halo rows inside the image are real rows, the image border is padding
    top = T.ref64(big_x[0, :BAND + p].cpu().float()[None], w, b, 1, (p, 0, p, p), None)
    _assert_equal(f"k{k}: first {BAND} rows of the first image", got[0, :BAND].cpu().double()[None], top)
    bottom = T.ref64(big_x[B - 1, H - BAND - p:].cpu().float()[None], w, b, 1, (0, p, p, p), None)
    _assert_equal(f"k{k}: last {BAND} rows of the last image", got[B - 1, H - BAND:].cpu().double()[None], bottom)
    report(f"[dw rowloop] k{k} {B}x{H}x{W}x{Cc} ({big_x.numel() * 2 / 2 ** 30:.2f} GiB): first and last {BAND} rows bit-exact")
