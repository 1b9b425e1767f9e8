"""CPU: the sharpening stress test's host side - the integer restatement of the unsharp mask (tests/_sharpen_ref.py, the suite's oracle for
``vip_sharpen_rgb_u8``) against the rounded float64 formula, its threshold, ``pipeline.sharpen_amount``, the argument checks of the
Python layer and of the entry point, and the refusals of ``main.py``.

Bound.  The kernel's gain is ``a / 256`` with ``a = round(256 P / 100)``: ``|a / 256 - P / 100| <= 1 / 512``, and ``|d| <= 255``, so before
rounding the integer form is within 255 / 512 < 0.5 level of ``X + P / 100 d``; both sides round to nearest and clamp (monotone), so the
results differ by at most ONE level.  Both sides use the same uint8 blurred image ``B``."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _blur_ref as B  # noqa: E402
from tests import _sharpen_ref as S  # noqa: E402

SIZES = [(1, 1), (2, 3), (7, 5), (17, 31), (65, 129)]                                         # (height, width)
PERCENTS = [1, 50, 150, 500]
SIGMAS = [0.3, 1.0, 5.0]


def _inputs():
    from tests._jpeg_enc_ref import content
    out = [content(31 + k, w, h) for k, (h, w) in enumerate(SIZES)]
    out[4] = B.two_level(4, *SIZES[4])                                                        # 0 / 255: the largest steps, both clamps
    return out


def test_restatement_is_within_one_level_of_the_exact_formula(report):
    samples = differ = 0
    for px in _inputs():
        for sigma in SIGMAS:
            for pc in PERCENTS:
                got = S.sharpen(px, pc, sigma).astype(np.int64)
                want = S.exact_sharpen(px, pc, sigma).astype(np.int64)
                d = np.abs(got - want)
                assert got.shape == px.shape and d.max() <= 1, (px.shape, pc, sigma, int(d.max()))
                samples += d.size
                differ += int((d != 0).sum())
    report(f"[sharpen cpu] integer unsharp mask vs rounded float64: {differ} of {samples} samples differ, all by one level")


def test_both_clamps_are_hit_on_the_two_level_image():
    px = _inputs()[4]
    for sigma in SIGMAS:
        x = px.astype(np.int64)
        raw = x + ((S.amount(500) * (x - B.gauss(px, sigma).astype(np.int64)) + 128) >> 8)    # before the clamp
        assert (raw < 0).any() and (raw > 255).any(), sigma
        out = S.sharpen(px, 500, sigma)
        assert (out[raw < 0] == 0).all() and (out[raw > 255] == 255).all()


def test_threshold():
    for px in _inputs():
        assert np.array_equal(S.sharpen(px, 200, 1.0, None, 255), px)                         # |d| <= 255 always
    px = _inputs()[3]
    d = px.astype(np.int64) - B.gauss(px, 1.0).astype(np.int64)
    out = S.sharpen(px, 150, 1.0, None, 3)
    quiet = np.abs(d) <= 3
    assert quiet.any() and (~quiet).any()
    assert np.array_equal(out[quiet], px[quiet]) and (out[~quiet] != px[~quiet]).any()
    assert np.array_equal(out[~quiet], S.sharpen(px, 150, 1.0, None, 0)[~quiet])


def test_sharpen_amount():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    assert [pipeline.sharpen_amount(pc) for pc in (1, 100, 500)] == [3, 256, 1280]
    for pc in range(1, 501):
        assert pipeline.sharpen_amount(pc) == S.amount(pc) == int(np.floor(256 * pc / 100 + 0.5))
        assert abs(pipeline.sharpen_amount(pc) / 256 - pc / 100) <= 1 / 512
    for pc in (0, 501, -1, 1.0, "100", None, True):
        with pytest.raises(ValueError, match="1..500"):
            pipeline.sharpen_amount(pc)


def test_sharpen_checks_its_arguments_without_a_gpu(monkeypatch):
    """percent, sigma, radius and threshold are validated before the batch is looked at, the library loaded or anything launched"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    touched = []
    monkeypatch.setattr(pipeline, "_launch", lambda *a, **k: touched.append(a))
    monkeypatch.setattr(_abi, "lib", lambda: touched.append("lib"))
    for pc in (0, 501, -5, 1.5, "100", None, True):
        with pytest.raises(ValueError, match="1..500"):
            pipeline.sharpen(None, pc)
    for sigma in (0.2, 5.1, 1.25, 0, None, True):
        with pytest.raises(ValueError, match="multiple of 0.1 in 0.3..5.0"):
            pipeline.sharpen(None, 100, sigma)
    for r in (0, 16, -1, 2.0, True):
        with pytest.raises(ValueError, match="1..15"):
            pipeline.sharpen(None, 100, 1.0, r)
    for t in (256, -1, 3.0, "3", None, True):
        with pytest.raises(ValueError, match="0..255"):
            pipeline.sharpen(None, 100, 1.0, None, t)
    assert not touched


def test_entry_point_checks_its_arguments_before_any_work():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    lib = _abi.lib()
    p, q = C.c_void_p(1 << 20), C.c_void_p(1 << 24)
    fn = lib.vip_sharpen_rgb_u8
    assert fn(None, p, 8, 8, q, 8, 8, p, 3, 256, 0, 1, None) == -1 and b"null" in lib.vip_last_error()
    assert fn(p, p, 8, 8, q, 8, 8, None, 3, 256, 0, 1, None) == -1
    assert fn(p, p, 8, 8, q, 8, 0, p, 3, 256, 0, 1, None) == -1 and b"size" in lib.vip_last_error()
    assert fn(p, p, 8, 8, q, 8, 8, p, 3, 256, 0, 0, None) == -1
    assert fn(p, C.c_void_p(66), 8, 8, q, 8, 8, p, 3, 256, 0, 1, None) == -2
    assert fn(p, p, 8, 8, q, 8, 8, C.c_void_p(66), 3, 256, 0, 1, None) == -2
    assert fn(p, p, 8, 8, p, 8, 8, p, 3, 256, 0, 1, None) == -1 and b"overlap" in lib.vip_last_error()
    for r in (0, 16):
        assert fn(p, p, 8, 8, q, 8, 8, p, r, 256, 0, 1, None) == -1 and b"radius" in lib.vip_last_error()
    for a in (0, 1281, -256):
        assert fn(p, p, 8, 8, q, 8, 8, p, 3, a, 0, 1, None) == -1 and b"amount_q8" in lib.vip_last_error()
    for t in (-1, 256):
        assert fn(p, p, 8, 8, q, 8, 8, p, 3, 256, t, 1, None) == -1 and b"threshold" in lib.vip_last_error()


# ---- CLI refusals: everything is refused before torch is imported ---------------------------------------------------------------------------
REFUSALS = [
    (["--stress-sharpen", "150"], "--stress-sharpen needs --stress-out"),
    (["--stress-sharpen", "0", "--stress-out", "S"], "integer percents in 1..500"),
    (["--stress-sharpen", "501", "--stress-out", "S"], "integer percents in 1..500"),
    (["--stress-sharpen", "50,1.5", "--stress-out", "S"], "integer percents in 1..500"),
    (["--stress-sharpen", "50,,80", "--stress-out", "S"], "integer percents in 1..500"),
    (["--stress-sharpen", "150,50,150", "--stress-out", "S"], "each listed once"),
    (["--stress-sharpen-sigma", "2", "--stress-out", "S"], "need --stress-sharpen"),
    (["--stress-sharpen-sigma", "2", "--stress-blur", "1", "--stress-out", "S"], "need --stress-sharpen"),
    (["--stress-sharpen-sigma", "2", "--stress-chain", "r50+q80", "--stress-out", "S"], "need --stress-sharpen"),
    (["--stress-sharpen-radius", "2", "--stress-out", "S"], "need --stress-sharpen"),
    (["--stress-sharpen-threshold", "2", "--stress-out", "S"], "need --stress-sharpen"),
    (["--stress-sharpen", "150", "--stress-sharpen-sigma", "0.2", "--stress-out", "S"], "sigma in 0.3..5.0"),
    (["--stress-sharpen", "150", "--stress-sharpen-sigma", "1.25", "--stress-out", "S"], "sigma in 0.3..5.0"),
    (["--stress-sharpen", "150", "--stress-sharpen-radius", "16", "--stress-out", "S"], "integer in 1..15"),
    (["--stress-sharpen", "150", "--stress-sharpen-threshold", "256", "--stress-out", "S"], "integer in 0..255"),
    (["--stress-sharpen", "150", "--stress-out", "S", "--tta", "2"], "--stress-sharpen works with --shard images and --tta 1 only"),
    (["--stress-sharpen", "150", "--stress-out", "S", "--shard", "members"], "--stress-sharpen works with --shard images and --tta 1 only"),
    (["--stress-sharpen", "150", "--stress-out", "S", "--shard", "hybrid"], "--stress-sharpen works with --shard images and --tta 1 only"),
    (["--stress-sharpen", "150", "--stress-out", "S", "--heatmaps", "H"], "--stress-sharpen and --heatmaps cannot be combined"),
    (["--stress-sharpen", "150", "--stress-out", "S", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-sharpen", "150", "--stress-out", "S", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
]


@pytest.mark.parametrize("extra,message", REFUSALS, ids=lambda v: "".join(v) if isinstance(v, list) else None)
def test_cli_refuses_before_scoring(tmp_path, extra, message):
    (tmp_path / "test.csv").write_text("filename\nimg_00000.jpg\n")
    paths = {"S": "stress.csv", "H": "maps", "T": "tiles.csv"}
    extra = [str(tmp_path / paths[t]) if t in paths else t for t in extra]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "vip-cup-2022_amd", "main.py"), str(tmp_path / "test.csv"), str(tmp_path / "o.csv"),
                        "--synthetic", *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and message in (r.stderr + r.stdout), r.stderr[-400:]
    assert sorted(os.listdir(tmp_path)) == ["test.csv"] and "MODEL(" not in r.stdout
