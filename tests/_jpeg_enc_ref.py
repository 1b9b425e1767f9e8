"""NumPy restatement of the forward half of a baseline JPEG save, up to (and not including) entropy coding: the test suite's oracle for
csrc/jpeg_encode.hip.  Written from ITU-T T.81 and the published behaviour of libjpeg's compressor with its defaults (jccolor.c,
jcprepct.c, jcsample.c, jfdctint.c, jcdctmgr.c, jccoefct.c, jcparam.c); tests/test_jpeg_recompress_cpu.py checks it, coefficient by
coefficient, against the files Pillow (libjpeg-turbo) writes.  Everything is integer arithmetic.

    quality_tables(q)                    -> (luma [64], chroma [64]) uint16, natural (row-major) order
    layout(w, h, subsampling)            -> per component (hsamp, vsamp, blocks_w, blocks_h), blocks padded to whole MCUs
    coefficients(rgb, q, subsampling)    -> three int16 arrays [blocks_h, blocks_w, 64], natural order
and the two helpers the tests share: pil_jpeg (the arbiter's file) and content (test images of any size).
"""
import io
import os

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_SUB = {"4:2:0": 2, "4:4:4": 0}          # Pillow's ``subsampling`` argument

# T.81 Annex K, tables K.1 and K.2, natural order
BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    dtype=np.int64)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99],
    dtype=np.int64)

SUBSAMPLINGS = {"4:2:0": 2, "4:4:4": 1}


def quality_tables(q: int):
    """jpeg_set_quality(q, force_baseline = TRUE): jpeg_quality_scaling + jpeg_add_quant_table (jcparam.c)"""
    if not 1 <= q <= 100:
        raise ValueError(f"quality {q} outside 1..100")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint16) for base in (BASE_LUMA, BASE_CHROMA))


def layout(w: int, h: int, subsampling: str = "4:2:0"):
    s = SUBSAMPLINGS[subsampling]
    mx, my = -(-w // (8 * s)), -(-h // (8 * s))
    return [(s, s, mx * s, my * s), (1, 1, mx, my), (1, 1, mx, my)]


def _fix(x):
    return int(x * 65536 + 0.5)


def rgb_to_ycc(rgb):
    """jccolor.c rgb_ycc_convert: 16 fractional bits; the chroma rounding constant is ONE_HALF - 1 on top of the 128 offset"""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    half = 1 << 15
    y = (_fix(0.29900) * r + _fix(0.58700) * g + _fix(0.11400) * b + half) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.50000) * b + (128 << 16) + half - 1) >> 16
    cr = (_fix(0.50000) * r - _fix(0.41869) * g - _fix(0.08131) * b + (128 << 16) + half - 1) >> 16
    return y, cb, cr


def _pad_replicate(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def component_planes(rgb, subsampling="4:2:0"):
    """The sample planes the DCT reads, [8 * real block rows, 8 * real block columns] per component (dummy blocks excluded).
    Full-size components: last column / row replicated.  h2v2 (jcsample.c): the input columns are replicated out to twice the output
    width BEFORE the 2x2 sums (bias 1, 2, 1, 2 along the row); the rows are replicated to an even count before, and the last OUTPUT row
    is replicated after (jcprepct.c pre_process_data)."""
    h, w = rgb.shape[:2]
    y, cb, cr = rgb_to_ycc(rgb)
    s = SUBSAMPLINGS[subsampling]
    planes = [_pad_replicate(y, -(-h // 8) * 8, -(-w // 8) * 8)]
    for c in (cb, cr):
        if s == 1:
            planes.append(_pad_replicate(c, -(-h // 8) * 8, -(-w // 8) * 8))
            continue
        dw, dh = -(-w // 2), -(-h // 2)
        ow, oh = -(-dw // 8) * 8, -(-dh // 8) * 8
        full = _pad_replicate(c, 2 * dh, 2 * ow)
        bias = np.tile(np.array([1, 2], dtype=np.int64), ow // 2)[None, :]
        down = (full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2] + bias) >> 2
        planes.append(_pad_replicate(down, oh, ow))
    return planes


CONST_BITS, PASS1_BITS = 13, 2
F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865 = 2446, 3196, 4433, 6270
F_0_899976223, F_1_175875602, F_1_501321110, F_1_847759065 = 7373, 9633, 12299, 15137
F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = 16069, 16819, 20995, 25172


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """one pass of jfdctint.c jpeg_fdct_islow over the LAST axis of d [..., 8]"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << PASS1_BITS, (t10 - t11) << PASS1_BITS
        sh = CONST_BITS - PASS1_BITS
    else:
        out[0], out[4] = _descale(t10 + t11, PASS1_BITS), _descale(t10 - t11, PASS1_BITS)
        sh = CONST_BITS + PASS1_BITS
    z1 = (t12 + t13) * F_0_541196100
    out[2] = _descale(z1 + t13 * F_0_765366865, sh)
    out[6] = _descale(z1 + t12 * (-F_1_847759065), sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175875602
    t4, t5, t6, t7 = t4 * F_0_298631336, t5 * F_2_053119869, t6 * F_3_072711026, t7 * F_1_501321110
    z1, z2, z3, z4 = z1 * -F_0_899976223, z2 * -F_2_562915447, z3 * -F_1_961570560, z4 * -F_0_390180644
    z3, z4 = z3 + z5, z4 + z5
    out[7] = _descale(t4 + z1 + z3, sh)
    out[5] = _descale(t5 + z2 + z4, sh)
    out[3] = _descale(t6 + z2 + z3, sh)
    out[1] = _descale(t7 + z1 + z4, sh)
    return np.stack(out, axis=-1)


def fdct_quantise(plane, qt):
    """plane [8 bh, 8 bw] samples 0..255 -> [bh, bw, 64] int16: level shift, ISLOW forward DCT (outputs scaled by 8), and the
    quantisation of jcdctmgr.c: divisor = 8 * table entry, magnitude rounded to nearest, sign restored"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    blk = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128          # [bh, bw, row, col]
    blk = _fdct_1d(blk, True)                                                               # rows
    blk = _fdct_1d(blk.swapaxes(-1, -2), False).swapaxes(-1, -2)                            # columns
    assert np.abs(blk).max() < 2 ** 31
    div = qt.astype(np.int64).reshape(8, 8) * 8
    mag = (np.abs(blk) + (div >> 1)) // div
    return (np.sign(blk) * mag).astype(np.int16).reshape(bh, bw, 64)


def coefficients(rgb, quality: int, subsampling: str = "4:2:0"):
    """What the file's entropy-coded segment holds.  Blocks that only pad the last MCU column / row are the DUMMY blocks of jccoefct.c
    compress_data: all AC zero, DC copied from the block before them in the MCU - to the right of the image the block on their left; below
    it the last block of the MCU's row above (for both blocks of the dummy row)."""
    h, w = rgb.shape[:2]
    luma, chroma = quality_tables(quality)
    planes = component_planes(rgb, subsampling)
    out = []
    for (hs, vs, bw, bh), plane, qt in zip(layout(w, h, subsampling), planes, (luma, chroma, chroma)):
        real = fdct_quantise(plane, qt)
        rh, rw = real.shape[:2]
        full = np.zeros((bh, bw, 64), dtype=np.int16)
        full[:rh, :rw] = real
        assert bw - rw in (0, 1) and bh - rh in (0, 1) and (hs == 2 or (bw == rw and bh == rh))
        if bw > rw:
            full[:rh, rw, 0] = full[:rh, rw - 1, 0]
        if bh > rh:
            full[rh, :, 0] = np.repeat(full[rh - 1, 1::2, 0], 2)
        out.append(full)
    return out


def pil_jpeg(px: np.ndarray, quality: int, sampling: str) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, format="JPEG", quality=quality, subsampling=PIL_SUB[sampling])
    return buf.getvalue()


def content(kind, w: int, h: int) -> np.ndarray:
    """[h, w, 3] uint8: synthetic images (tools/make_synth) or a photograph of tests/golden, tiled where the size asks for more"""
    from PIL import Image
    from tools.make_synth import synth_pixels
    if isinstance(kind, int):
        tiles = [[synth_pixels(kind + 2 * r + c) for c in range(2)] for r in range(2)]
        src = np.concatenate([np.concatenate(row, axis=1) for row in tiles], axis=0)
    else:
        src = np.asarray(Image.open(os.path.join(_ROOT, "tests", "golden", kind)).convert("RGB"))
    reps = (-(-h // src.shape[0]), -(-w // src.shape[1]), 1)
    return np.ascontiguousarray(np.tile(src, reps)[:h, :w])
