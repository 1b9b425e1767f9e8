"""CPU: the geometric stress tests' host side - the integer restatement of the affine warp (tests/_warp_ref.py, the suite's oracle for
csrc/warp.hip) against a float64 bilinear and against Pillow's ``Image.rotate``, flips and crops against numpy slicing, ``rotated_rect``,
``pipeline.warp_matrix`` against the restatement's quantisation, argument checks of the Python layers and of the C entry point,
``stress_labels`` / ``stress_table`` with ``flip`` / ``crop`` / ``rot`` labels, and the refusals of ``main.py``.

Bounds.  Against the exact bilinear value the integer warp is off by at most 0.5 (the final rounding) + 2 * 255 / 1024 = 0.498 (each
axis' weight is truncated to 10 bits, i.e. is short by less than 1 / 1024 of a difference of at most 255 levels) + about 0.02 (the
coefficients are rounded to 2^-25 of a pixel per unit of u = 2 x + 1 <= 400, which moves a coordinate by at most 400 * 2^-25 + 2^-26
of a pixel, times at most 255 levels per pixel, on both axes): less than 1.02 levels.  Pillow rounds the same exact value to the
nearest level, so the two integers differ by at most 1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _warp_ref as W  # noqa: E402

SIZES = [(37, 53), (129, 64), (200, 200)]                                                     # (height, width)
ANGLES = [0.5, -3, 7.5, 12.3, 45, -45]


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _ramp(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([xx * 255 // (w - 1), yy * 255 // (h - 1), (xx + yy) * 255 // (h + w - 2)], axis=2).astype(np.uint8)


def _inputs():
    for k, (h, w) in enumerate(SIZES):
        yield _noise(40 + k, h, w)
        yield _ramp(h, w)


def test_restatement_against_float64_bilinear_and_pillow(report):
    worst_exact = worst_pil = 0.0
    for px in _inputs():
        h, w = px.shape[:2]
        for deg in ANGLES:
            f = W.rotate_xf(h, w, deg)
            q = W.quantise(*f)
            inside = W.taps_inside(q, h, w, h, w, margin=1)
            assert inside.sum() > h * w // 4
            got = W.warp(px, q, h, w, "black").astype(np.float64)
            d_exact = float(np.abs(got - W.exact_bilinear(px, *f, h, w))[inside].max())
            pil = np.asarray(Image.fromarray(px).rotate(deg, resample=Image.BILINEAR)).astype(np.float64)
            d_pil = float(np.abs(got - pil)[inside].max())
            worst_exact, worst_pil = max(worst_exact, d_exact), max(worst_pil, d_pil)
            assert d_exact < 1.02, ((h, w), deg, d_exact)
            assert d_pil <= 1, ((h, w), deg, d_pil)
            # the fill decides the taps outside only
            assert np.array_equal(W.warp(px, q, h, w, "mirror")[inside], got[inside].astype(np.uint8))
    report(f"[warp cpu] integer warp vs float64 bilinear: max {worst_exact:.4f} levels (bound 1.02); vs Pillow rotate(BILINEAR): "
           f"max {worst_pil:.0f} (bound 1)")


def test_flips_and_crops_are_exact_copies():
    for px in (_noise(7, 37, 53), _noise(8, 64, 129), _noise(9, 1, 7), _noise(10, 7, 1), _noise(11, 1, 1)):
        h, w = px.shape[:2]
        for fill in ("black", "mirror"):
            assert np.array_equal(W.warp(px, W.quantise(*W.flip_xf(h, w, "h")), h, w, fill), px[:, ::-1])
            assert np.array_equal(W.warp(px, W.quantise(*W.flip_xf(h, w, "v")), h, w, fill), px[::-1])
            for pc in (50, 77, 99):
                for origin in ("centre", "topleft"):
                    y0, x0, hh, ww = W.crop_box(h, w, pc, origin)
                    assert 0 <= y0 and y0 + hh <= h and 0 <= x0 and x0 + ww <= w
                    assert (y0, x0) == ((0, 0) if origin == "topleft" else ((h - hh) // 2, (w - ww) // 2))
                    assert np.array_equal(W.warp(px, W.quantise(*W.crop_xf(y0, x0)), hh, ww, fill), px[y0:y0 + hh, x0:x0 + ww])
    assert W.crop_box(37, 53, 50) == (9, 13, 19, 27) and W.crop_box(200, 200, 99, "topleft") == (0, 0, 198, 198)


def test_fills_outside_the_image():
    px = _noise(12, 5, 6)
    shift = W.quantise(1, 0, -2, 0, 1, 3)                   # output (x, y) <- source (x - 2, y + 3)
    black, mirror = W.warp(px, shift, 5, 6, "black"), W.warp(px, shift, 5, 6, "mirror")
    assert not black[:, :2].any() and not black[2:].any() and np.array_equal(black[:2, 2:], px[3:, :4])
    assert np.array_equal(mirror, px[[3, 4, 3, 2, 1]][:, [2, 1, 0, 1, 2, 3]])
    half = W.warp(px, W.quantise(1, 0, -0.5, 0, 1, 0), 5, 6, "black")      # half a pixel: the first column is half black
    assert np.array_equal(half[:, 0], (px[:, 0].astype(np.int64) * 512 * 1024 + (1 << 19)) >> 20)


def test_rotated_rect_keeps_every_tap_inside():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    for h in range(2, 41):
        for w in range(2, 41):
            for deg in (0.1, -0.1, 7.5, -7.5, 44.9, -44.9, 45, -45):
                hh, ww = W.rotated_rect(h, w, deg)
                assert 1 <= hh <= h and 1 <= ww <= w and pipeline.rotated_rect(h, w, deg) == (hh, ww)
                q = W.quantise(*W.rotate_xf(h, w, deg, hh, ww))
                assert W.taps_inside(q, hh, ww, h, w).all(), (h, w, deg, hh, ww)
    # 1-pixel axes stay defined; a square at 45 degrees keeps side / sqrt 2
    assert W.rotated_rect(1, 7, 7.5) == (1, 3) and W.rotated_rect(7, 1, -45) == (1, 1) and W.rotated_rect(1, 1, 45) == (1, 1)
    assert W.rotated_rect(200, 200, 45) == (141, 141) and W.rotated_rect(200, 200, 7.5) == (178, 178)
    assert W.rotated_rect(100, 300, 45) == (70, 70) and W.rotated_rect(300, 100, 45) == (70, 70)       # half-constrained
    for args in ((1, 7, 7.5), (7, 1, -45), (1, 1, 45), (200, 200, 45), (100, 300, 45), (64, 300, -12.3)):
        assert pipeline.rotated_rect(*args) == W.rotated_rect(*args)


def test_warp_matrix_equals_the_restatements_quantisation():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    rng = np.random.default_rng(3)
    for _ in range(200):
        f = tuple(float(v) for v in rng.uniform(-3, 3, 6) * [1, 1, 300, 1, 1, 300])
        assert pipeline.warp_matrix(*f) == W.quantise(*f).tolist()
    assert pipeline.warp_matrix(1, 0, 0, 0, -1, 200) == [1 << 24, 0, 0, 0, -(1 << 24), 200 << 25]
    assert pipeline.warp_matrix(0.5 + 2.0 ** -25, -2.0 ** -25, 0.25, 0, 0, -0.75) == [(1 << 23) + 1, 0, 1 << 23, 0, 0, -(3 << 23)]   # halves go up
    for deg in ANGLES:
        f = W.rotate_xf(129, 64, deg, 100, 50)
        assert pipeline.warp_matrix(*f) == W.quantise(*f).tolist()
    for bad in (float("nan"), float("inf"), 2.0 ** 31):
        with pytest.raises(ValueError, match="finite"):
            pipeline.warp_matrix(1, 0, bad, 0, 1, 0)


def test_geometry_checks_its_arguments_without_a_gpu(monkeypatch):
    """axis, percent, origin, degrees, fill and the transforms are validated before the batch is looked at or anything launched"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    touched = []
    monkeypatch.setattr(pipeline, "_launch", lambda *a, **k: touched.append(a))
    monkeypatch.setattr(_abi, "lib", lambda: touched.append("lib"))
    for axis in ("x", "hv", "", None, 0, True):
        with pytest.raises(ValueError, match="expected 'h' or 'v'"):
            pipeline.flip(None, axis)
    for pc in (49, 100, 0, -80, 80.0, "80", None, True):
        with pytest.raises(ValueError, match="50..99"):
            pipeline.crop(None, pc)
    for origin in ("center", "top", None, 0):
        with pytest.raises(ValueError, match="'centre' or 'topleft'"):
            pipeline.crop(None, 80, origin)
    for deg in (0, 0.0, 45.1, -45.1, 90, 7.55, 0.04, "7.5", None, True, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="non-zero multiple of 0.1 in -45..45"):
            pipeline.rotate(None, deg)
    for fill in ("constant", "reflect", None, 0):
        with pytest.raises(ValueError, match="crop, mirror, black"):
            pipeline.rotate(None, 7.5, fill)
    ident = np.array([[1 << 24, 0, 0, 0, 1 << 24, 0]], np.int64)
    for fill in ("crop", "reflect", None, 1):
        with pytest.raises(ValueError, match="black, mirror"):
            pipeline.warp(None, ident, [(4, 4)], fill)
    for xf in (ident.astype(np.int32), ident.astype(np.float64), ident[0], ident[:, :5], ident.tolist() + [[0.5] * 6]):
        with pytest.raises(ValueError, match=r"int64 \[n, 6\]"):
            pipeline.warp(None, xf, [(4, 4)])
    for sizes in ([(0, 4)], [(4, -1)], [(4.0, 4)], [(4,)], [(True, 4)]):
        with pytest.raises(ValueError, match="positive integers"):
            pipeline.warp(None, ident, sizes)
    with pytest.raises(ValueError, match="1 images, 1 transforms, 2 output sizes"):
        pipeline.warp([0], ident, [(4, 4), (4, 4)])
    assert not touched
    assert pipeline._rotate_args(7.5, "crop") == (75, "crop") and pipeline._rotate_args(-45, "black") == (-450, "black")
    assert pipeline._rotate_args(np.float32(12.5), "mirror") == (125, "mirror") and pipeline._rotate_args(1, "crop") == (10, "crop")


def test_warp_refuses_an_output_above_the_pixel_cap(monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    touched = []
    monkeypatch.setattr(pipeline, "_launch", lambda *a, **k: touched.append(a))
    monkeypatch.setattr(pipeline, "MAX_JPEG_PIXELS", 1000)
    with pytest.raises(_abi.VipError, match="VIP_MAX_JPEG_PIXELS=1000"):
        pipeline.warp([0], np.array([[1 << 24, 0, 0, 0, 1 << 24, 0]], np.int64), [(40, 26)])
    assert not touched


def test_entry_point_refuses_bad_arguments_before_it_launches():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    lib = _abi.lib()
    p, q, s = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 28)
    f = lib.vip_warp_affine_rgb_u8
    for k in (0, 1, 4, 5, 8):                                 # every pointer
        args = [p, s, 8, 8, q, s, 8, 8, s, 0, 1, None]
        args[k] = None
        assert f(*args) == -1 and b"null pointer" in lib.vip_last_error()
    for k in (2, 3, 6, 7, 10):                                # n and every slot side
        for v in (0, -1):
            args = [p, s, 8, 8, q, s, 8, 8, s, 0, 1, None]
            args[k] = v
            assert f(*args) == -1 and b"bad size" in lib.vip_last_error()
    for fill in (2, -1, 7):
        assert f(p, s, 8, 8, q, s, 8, 8, s, fill, 1, None) == -1 and b"fill" in lib.vip_last_error()
    assert f(p, s, 8, 8, p, s, 8, 8, s, 0, 1, None) == -1 and b"overlap" in lib.vip_last_error()
    assert f(p, s, 8, 8, C.c_void_p((1 << 20) + 191), s, 9, 9, s, 1, 1, None) == -1 and b"overlap" in lib.vip_last_error()
    assert f(p, C.c_void_p((1 << 28) + 2), 8, 8, q, s, 8, 8, s, 0, 1, None) == -2
    assert f(p, s, 8, 8, q, C.c_void_p((1 << 28) + 1), 8, 8, s, 0, 1, None) == -2
    assert f(p, s, 8, 8, q, s, 8, 8, C.c_void_p((1 << 28) + 4), 0, 1, None) == -2 and b"8-byte" in lib.vip_last_error()


# ---- ensemble -----------------------------------------------------------------------------------------------------------------------------
def test_stress_labels_order():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    assert ensemble.stress_labels([75], flips=["h"], crops=[80], rotations=[7.5]) == \
        ["q75", "fliph", "fliph_q75", "crop80", "crop80_q75", "rot075", "rot075_q75"]
    assert ensemble.stress_labels([90, 70], [50], [1.0], [3], flips=("v", "h"), crops=(60, 99), rotations=(12.3, -45, 0.1, -0.5)) == \
        ["q90", "q70", "r50", "r50_q90", "r50_q70", "b10", "b10_q90", "b10_q70", "m3", "m3_q90", "m3_q70",
         "fliph", "fliph_q90", "fliph_q70", "flipv", "flipv_q90", "flipv_q70", "crop99", "crop99_q90", "crop99_q70",
         "crop60", "crop60_q90", "crop60_q70", "rotm450", "rotm450_q90", "rotm450_q70", "rotm005", "rotm005_q90", "rotm005_q70",
         "rot001", "rot001_q90", "rot001_q70", "rot123", "rot123_q90", "rot123_q70"]
    assert ensemble.stress_labels([], rotations=[45, -7.5]) == ["rotm075", "rot450"] and ensemble.stress_labels([], flips=["v"]) == ["flipv"]
    assert ensemble.stress_labels([], crops=[50], crop_origin="topleft", rotate_fill="black") == ["crop50"]
    # empty new lists: the earlier results
    for args in (([90, 70],), ([], []), ([90, 70], [150, 50]), ([80], [50], [1.0], [3]), ([], (), [2.5, 0.5], [5, 3])):
        assert ensemble.stress_labels(*args, flips=(), crops=(), rotations=()) == ensemble.stress_labels(*args)
    assert ensemble.stress_labels([80], [50], [1.0], [3]) == ["q80", "r50", "r50_q80", "b10", "b10_q80", "m3", "m3_q80"]
    assert ensemble.stress_labels([90, 70]) == ["q90", "q70"] and ensemble.stress_labels([], []) == []


def test_stress_table_with_geometry_labels():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    names = ["b.jpg", "a.jpg", "c.jpg", "a.jpg", "d.jpg"]
    labels = ensemble.stress_labels([75], flips=["h"], crops=[80], rotations=[-7.5])
    assert labels == ["q75", "fliph", "fliph_q75", "crop80", "crop80_q75", "rotm075", "rotm075_q75"]
    s = np.zeros((8, 2, 5), dtype=np.float32)                 # [1 + V, M = 2, n = 5]; a.jpg is rows 1 and 3
    s[0] = [[0.9, 0.2, 0.3, 0.6, 0.1]] * 2                    # a 0.4 -> 0, b 0.9 -> 1, c 0.3 -> 0, d 0.1 -> 0
    s[1] = [[0.4, 0.2, 0.3, 0.6, 0.1]] * 2                    # q75: b flips
    s[2] = [[0.9, 0.2, 0.3, 0.6, 0.1]] * 2                    # fliph: nothing flips
    s[3] = [[0.9, 0.9, 0.3, 0.7, 0.1]] * 2                    # fliph_q75: a -> 0.8 flips
    s[4] = [[0.9, 0.2, 0.3, 0.6, 0.9]] * 2                    # crop80: d flips
    s[5] = [[0.2, 0.2, 0.9, 0.6, 0.1]] * 2                    # crop80_q75: b and c flip
    s[6] = [[0.9, 0.2, 0.3, 0.6, 0.1]] * 2                    # rotm075: nothing flips
    s[7] = [[0.1, 0.9, 0.9, 0.9, 0.9]] * 2                    # rotm075_q75: everything flips
    table, summary = ensemble.stress_table(names, s, labels)
    assert table["filename"] == ["a.jpg", "b.jpg", "c.jpg", "d.jpg"] and table["labels"] == labels
    for k in range(8):                                        # every row IS aggregate's
        uniq, p, dec = ensemble.aggregate(names, s[k])
        got_p, got_d = (table["p"], table["decision"]) if k == 0 else (table["p_q"][:, k - 1], table["decision_q"][:, k - 1])
        assert uniq == table["filename"] and np.array_equal(p, got_p) and np.array_equal(dec, got_d)
    assert table["stable"].tolist() == [False] * 4 and table["flips_at"] == [None, 75, None, None]      # flips_at: the plain q rows only
    assert table["flips"] == ["fliph_q75;rotm075_q75", "q75;crop80_q75;rotm075_q75", "crop80_q75;rotm075_q75", "crop80;rotm075_q75"]
    assert summary["variants"] == labels and summary["qualities"] == [75] and summary["n_stable"] == 0 and summary["n_files"] == 4
    assert summary["flips"] == {"q75": 1, "fliph": 0, "fliph_q75": 1, "crop80": 1, "crop80_q75": 2, "rotm075": 0, "rotm075_q75": 4}
    assert list(summary["mean_abs_dp"]) == labels and summary["flip_rate"]["rotm075_q75"] == 1.0
    table, summary = ensemble.stress_table(names, s[[0, 2, 4]], ["fliph", "crop80"])                   # geometry only: no q rows
    assert table["flips_at"] == [None] * 4 and table["flips"] == ["", "", "", "crop80"] and summary["qualities"] == []


# ---- CLI refusals: everything is refused before torch is imported ---------------------------------------------------------------------------
REFUSALS = [
    (["--stress-flip", "h"], "--stress-flip needs --stress-out"),
    (["--stress-crop", "80"], "--stress-crop needs --stress-out"),
    (["--stress-rotate", "7.5"], "--stress-rotate needs --stress-out"),
    (["--stress-crop-origin", "topleft", "--stress-flip", "h", "--stress-out", "S"], "--stress-crop-origin needs --stress-crop"),
    (["--stress-rotate-fill", "black", "--stress-crop", "80", "--stress-out", "S"], "--stress-rotate-fill needs --stress-rotate"),
    (["--stress-flip", "x", "--stress-out", "S"], "expected h, v or h,v"),
    (["--stress-flip", "h,,v", "--stress-out", "S"], "expected h, v or h,v"),
    (["--stress-crop", "49", "--stress-out", "S"], "integer percents in 50..99"),
    (["--stress-crop", "80,100", "--stress-out", "S"], "integer percents in 50..99"),
    (["--stress-crop", "80.5", "--stress-out", "S"], "integer percents in 50..99"),
    (["--stress-rotate", "0", "--stress-out", "S"], "non-zero angles in -45..45"),
    (["--stress-rotate=-45.1", "--stress-out", "S"], "non-zero angles in -45..45"),
    (["--stress-rotate", "7.55", "--stress-out", "S"], "non-zero angles in -45..45"),
    (["--stress-rotate", "3,,5", "--stress-out", "S"], "non-zero angles in -45..45"),
    (["--stress-flip", "h", "--stress-out", "S", "--tta", "2"], "--stress-flip works with --shard images and --tta 1 only"),
    (["--stress-crop", "80", "--stress-out", "S", "--shard", "members"], "--stress-crop works with --shard images and --tta 1 only"),
    (["--stress-rotate=-3,7.5", "--stress-out", "S", "--shard", "hybrid"], "--stress-rotate works with --shard images and --tta 1 only"),
    (["--stress-flip", "v", "--stress-out", "S", "--heatmaps", "H"], "--stress-flip and --heatmaps cannot be combined"),
    (["--stress-crop", "80", "--stress-out", "S", "--heatmaps", "H"], "--stress-crop and --heatmaps cannot be combined"),
    (["--stress-rotate", "7.5", "--stress-out", "S", "--heatmaps", "H"], "--stress-rotate and --heatmaps cannot be combined"),
    (["--stress-flip", "h", "--stress-out", "S", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-crop", "80", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-rotate", "7.5", "--stress-out", "S", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-flip", "h", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--stress-crop", "80", "--stress-out", "S", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--stress-rotate", "7.5", "--stress-out", "S", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
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
