"""CPU: the host half of the recompression stress test (csrc/jpeg_encode.hip: quality tables, encode layout), the NumPy restatement of
the forward JPEG path (tests/_jpeg_enc_ref.py, the suite's oracle for the GPU stage) and ``ensemble.stress_table``.

The arbiter is Pillow, which tests/test_oracle_jpeg.py pins as libjpeg-turbo: a file saved with ``quality=q`` runs libjpeg's
``jpeg_set_quality(q, TRUE)``, the ISLOW forward DCT and, when no ``subsampling`` is given, libjpeg's default 4:2:0 (checked below on
the written file's frame header).  4:4:4 is asked for with ``subsampling=0``; 4:2:0 is passed as ``subsampling=2`` so that a Pillow whose
default differed would still write libjpeg's.  Every comparison is exact."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _jpeg_enc_ref as R  # noqa: E402
from tests._jpeg_enc_ref import content, pil_jpeg  # noqa: E402

SIZES = [(1, 1), (8, 8), (17, 13), (33, 250), (200, 200), (256, 192)]          # (width, height)
SAMPLINGS = ["4:2:0", "4:4:4"]
ABI_SUB = {"4:2:0": 420, "4:4:4": 444}
PHOTOS = ["ref_cat.jpg", "ref_dog.jpg", "ref_dog_cat.jpg"]


def _lib():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    return _abi, _abi.lib()


def _probe(raw: bytes):
    _abi, lib = _lib()
    d, need = _abi.JpegDesc(), C.c_size_t(0)
    buf = np.frombuffer(raw, dtype=np.uint8)
    _abi.check(lib.vip_jpeg_probe_h(buf.ctypes.data, len(raw), C.byref(d), C.byref(need)), "vip_jpeg_probe_h")
    return d, int(need.value)


def test_pillow_default_is_libjpegs_420():
    """no ``subsampling`` argument -> 2x2, 1x1, 1x1 in the frame header, libjpeg's default; 0 -> 1x1 three times"""
    px = content(1, 64, 48)
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, format="JPEG", quality=75)
    d, _ = _probe(buf.getvalue())
    assert (list(d.hsamp), list(d.vsamp)) == ([2, 1, 1], [2, 1, 1])
    assert buf.getvalue() == pil_jpeg(px, 75, "4:2:0")
    d, _ = _probe(pil_jpeg(px, 75, "4:4:4"))
    assert (list(d.hsamp), list(d.vsamp)) == ([1, 1, 1], [1, 1, 1])


@pytest.mark.parametrize("q", [1, 10, 25, 49, 50, 51, 75, 85, 90, 95, 100])
def test_quality_tables_equal_pillows(q):
    _abi, lib = _lib()
    d, _ = _probe(pil_jpeg(content(0, 16, 16), q, "4:2:0"))
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    assert lib.vip_jpeg_quality_tables_h(q, luma.ctypes.data, chroma.ctypes.data) == 0
    assert np.array_equal(luma, np.array(d.qt[0][:], dtype=np.uint16)), q
    assert np.array_equal(chroma, np.array(d.qt[1][:], dtype=np.uint16)) and np.array_equal(chroma, np.array(d.qt[2][:], dtype=np.uint16)), q
    rl, rc = R.quality_tables(q)                                   # the restatement agrees too
    assert np.array_equal(rl, luma) and np.array_equal(rc, chroma)


@pytest.mark.parametrize("q", [0, 101, -5])
def test_quality_outside_1_100_is_refused(q):
    _abi, lib = _lib()
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    assert lib.vip_jpeg_quality_tables_h(q, luma.ctypes.data, chroma.ctypes.data) == -1 and b"1..100" in lib.vip_last_error()
    d, need = _abi.JpegDesc(), C.c_size_t(0)
    assert lib.vip_jpeg_encode_layout_h(8, 8, 420, q, C.byref(d), C.byref(need)) == -1
    assert lib.vip_jpeg_quality_tables_h(50, None, chroma.ctypes.data) == -1


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_layout_equals_the_probe_of_pillows_file(size, sampling):
    _abi, lib = _lib()
    w, h = size
    for q in (75, 30):
        want, want_elems = _probe(pil_jpeg(content(3, w, h), q, sampling))
        got, need = _abi.JpegDesc(), C.c_size_t(0)
        assert lib.vip_jpeg_encode_layout_h(w, h, ABI_SUB[sampling], q, C.byref(got), C.byref(need)) == 0
        assert (got.width, got.height, got.ncomp, got.rgb_coded) == (w, h, 3, 0) == (want.width, want.height, want.ncomp, want.rgb_coded)
        for f in ("hsamp", "vsamp", "blocks_w", "blocks_h", "coef_off"):
            assert list(getattr(got, f)) == list(getattr(want, f)), (f, size, sampling)
        assert bytes(got.qt) == bytes(want.qt)
        assert need.value == want_elems
        assert [tuple(v) for v in zip(got.hsamp, got.vsamp, got.blocks_w, got.blocks_h)] == R.layout(w, h, sampling)


def test_encode_layout_refusals(monkeypatch):
    _abi, lib = _lib()
    d, need = _abi.JpegDesc(), C.c_size_t(0)
    assert lib.vip_jpeg_encode_layout_h(65535, 65535, 420, 75, C.byref(d), C.byref(need)) == -1            # over the default 64 Mi pixel cap
    assert b"VIP_MAX_JPEG_PIXELS" in lib.vip_last_error()
    monkeypatch.setenv("VIP_MAX_JPEG_PIXELS", "10000")
    assert lib.vip_jpeg_encode_layout_h(100, 100, 420, 75, C.byref(d), C.byref(need)) == 0
    assert lib.vip_jpeg_encode_layout_h(101, 100, 420, 75, C.byref(d), C.byref(need)) == -1
    monkeypatch.delenv("VIP_MAX_JPEG_PIXELS")
    assert lib.vip_jpeg_encode_layout_h(0, 8, 420, 75, C.byref(d), C.byref(need)) == -1
    assert lib.vip_jpeg_encode_layout_h(8, 65536, 420, 75, C.byref(d), C.byref(need)) == -1
    assert lib.vip_jpeg_encode_layout_h(8, 8, 422, 75, C.byref(d), C.byref(need)) == -1 and b"420 or 444" in lib.vip_last_error()
    assert lib.vip_jpeg_encode_layout_h(8, 8, 420, 75, None, C.byref(need)) == -1
    # the device entry point checks its arguments before any HIP call
    p = C.c_void_p(64)
    assert lib.vip_jpeg_fdct_quant_u8(None, p, 1, 1, p, p, 8, 8, None) == -1
    assert lib.vip_jpeg_fdct_quant_u8(p, p, 0, 1, p, p, 8, 8, None) == -1
    assert lib.vip_jpeg_fdct_quant_u8(p, p, 1, 1, C.c_void_p(72), p, 8, 8, None) == -2


def _host_coefficients(raw: bytes):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    desc, coef = pipeline.entropy_decode([raw], threads=1)
    d = desc[0]
    return [coef[d.coef_off[c]:d.coef_off[c] + d.blocks_w[c] * d.blocks_h[c] * 64].reshape(d.blocks_h[c], d.blocks_w[c], 64)
            for c in range(3)]


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_pillows_coefficients(size, sampling):
    """tests/_jpeg_enc_ref.coefficients == the entropy decode of the file Pillow writes from the same pixels, synthetic and photographic"""
    w, h = size
    for kind in [7] + PHOTOS:
        px = content(kind, w, h)
        for q in (30, 75, 95, 100):
            want = _host_coefficients(pil_jpeg(px, q, sampling))
            got = R.coefficients(px, q, sampling)
            for c in range(3):
                assert got[c].shape == want[c].shape, (kind, q, c)
                assert np.array_equal(got[c], want[c]), (kind, size, sampling, q, c, int((got[c] != want[c]).sum()))


@pytest.mark.parametrize("photo", PHOTOS)
def test_restatement_on_whole_photographs(photo):
    px = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", photo)).convert("RGB"))
    for sampling in SAMPLINGS:
        for q in (30, 95):
            want = _host_coefficients(pil_jpeg(px, q, sampling))
            got = R.coefficients(px, q, sampling)
            assert all(np.array_equal(g, w_) for g, w_ in zip(got, want)), (photo, sampling, q)


def test_restatement_gray_image_has_neutral_chroma():
    """R = G = B: Cb = Cr = 128 exactly (the chroma rounding constant is ONE_HALF - 1, so the tables' rounding errors do not tip it)"""
    g = content(5, 40, 24)[..., :1].repeat(3, axis=2)
    y, cb, cr = R.rgb_to_ycc(g)
    assert np.array_equal(y, g[..., 0]) and (cb == 128).all() and (cr == 128).all()
    coef = R.coefficients(g, 75, "4:2:0")
    assert not coef[1].any() and not coef[2].any()


# ---- stress_table -----------------------------------------------------------------------------------------------------------------------
def test_stress_table_rules():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    thr = np.float32(ensemble.THR)
    up = np.nextafter(thr, np.float32(1.0))
    names = ["b.jpg", "a.jpg", "c.jpg", "a.jpg", "d.jpg"]
    qs = [90, 70, 50]
    # [1 + Q, M = 2, n = 5]; both members equal unless said otherwise
    s = np.zeros((4, 2, 5), dtype=np.float32)
    s[0] = [[0.9, 0.2, thr, 0.6, 0.1]] * 2            # a.jpg: rows 1 and 3 -> mean 0.4 -> 0;  c.jpg exactly AT the threshold -> 0 (strict >)
    s[1] = [[0.8, 0.2, up, 0.6, 0.1]] * 2             # q90: c.jpg one ulp above the threshold -> 1: a flip
    s[2] = [[0.4, 0.9, thr, 0.7, 0.1]] * 2            # q70: b.jpg flips to 0; a.jpg rows 0.9 / 0.7 -> 0.8 -> flips to 1; c.jpg back at thr -> 0
    s[3] = [[0.3, 0.2, 0.9, 0.6, 0.1]] * 2            # q50: b.jpg still flipped, a.jpg back, c.jpg flips
    s[3, 0, 4], s[3, 1, 4] = 0.0, 0.99                # d.jpg: the members disagree, mean 0.495 > thr -> flips at 50 only
    table, summary = ensemble.stress_table(names, s, qs)
    assert table["filename"] == ["a.jpg", "b.jpg", "c.jpg", "d.jpg"]                      # sorted, duplicates merged (aggregate's rule)
    for k in range(4):                                                                    # every row IS aggregate's
        uniq, p, dec = ensemble.aggregate(names, s[k])
        got_p, got_d = (table["p"], table["decision"]) if k == 0 else (table["p_q"][:, k - 1], table["decision_q"][:, k - 1])
        assert uniq == table["filename"] and np.array_equal(p, got_p) and np.array_equal(dec, got_d)
    assert np.allclose(table["p"], [0.4, 0.9, float(thr), 0.1]) and table["decision"].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert table["decision_q"].tolist() == [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 1.0], [0.0, 0.0, 1.0]]
    assert table["stable"].tolist() == [False, False, False, False]
    assert table["flips_at"] == [70, 70, 90, 50]                                         # the HIGHEST differing quality
    assert summary["flips"] == {"90": 1, "70": 2, "50": 3} and summary["n_stable"] == 0 and summary["n_files"] == 4
    assert summary["flip_rate"] == {"90": 0.25, "70": 0.5, "50": 0.75}
    want = np.abs(table["p_q"].astype(np.float64) - table["p"].astype(np.float64)[:, None]).mean(axis=0)
    assert [summary["mean_abs_dp"][str(q)] for q in qs] == pytest.approx(want.tolist(), abs=0, rel=1e-12)
    # a stable file: no flips_at
    table, summary = ensemble.stress_table(["x", "y"], np.array([[[0.9, 0.1]], [[0.6, 0.2]]], dtype=np.float32), [80])
    assert table["stable"].tolist() == [True, True] and table["flips_at"] == [None, None]
    assert summary["flips"] == {"80": 0} and summary["flip_rate"] == {"80": 0.0} and summary["n_stable"] == 2
    assert summary["mean_abs_dp"]["80"] == pytest.approx((0.3 + 0.1) / 2, rel=1e-6)


class _FakeDist:
    """all_gather_into_tensor over payloads recorded in a first pass (the ranks run one after the other in this process)"""

    def __init__(self):
        self.payloads, self.calls, self.replay = [], 0, False

    def all_gather_into_tensor(self, out, mine):
        self.calls += 1
        if not self.replay:
            self.payloads.append(mine.clone())
            out.zero_()
        else:
            out.copy_(__import__("torch").cat(self.payloads))


@pytest.mark.parametrize("world,n", [(1, 5), (2, 7), (4, 3), (3, 10)])
def test_gather_stress_rows_one_collective(world, n):
    """every rank's [Q, M, n_local] rows, kept per batch, arrive as [Q, M, n] through ONE all-gather (shards of unequal or zero length)"""
    import torch
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    Q, M = 3, 2
    full = torch.arange(Q * M * n, dtype=torch.float32).reshape(Q, M, n) / 7.0
    kept = []
    for r in range(world):
        lo, hi = ensemble.shard_bounds(n, r, world)
        kept.append([full[:, :, b:min(b + 2, hi)].clone() for b in range(lo, hi, 2)])
    fake = _FakeDist()
    for r in range(world):
        ensemble.gather_stress_rows(kept[r], Q, M, n, r, world, fake if world > 1 else None)
    fake.replay, fake.calls = True, 0
    for r in range(world):
        got = ensemble.gather_stress_rows(kept[r], Q, M, n, r, world, fake if world > 1 else None)
        assert got.shape == (Q, M, n) and np.array_equal(got, full.numpy())
    assert fake.calls == (world if world > 1 else 0)
