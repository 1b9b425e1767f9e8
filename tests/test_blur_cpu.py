"""CPU: the smoothing stress tests' host side - the integer restatement of the Gaussian blur and the median (tests/_blur_ref.py, the
suite's oracle for csrc/blur.hip) against scipy.ndimage, ``vip_blur_weights_h`` against the restatement's weights, the 5 x 5 selection
network of csrc/blur.hip on every 0 / 1 input, argument checks of the Python layers, ``stress_labels`` / ``stress_table`` with ``b`` / ``m``
labels, and the refusals of ``main.py``.

Bounds.  The integer blur rounds its horizontal pass once to 1 / 256 level (2^-9 level, carried through weights that sum to 1) and its
weights are off by at most (2 R + 1) * 2^-16 in total per axis, the centre included ((2 R + 1) * 2^-16 * 255 <= 0.121 level at R = 15):
before the final rounding it is within 0.002 + 2 * 0.121 < 0.25 level of the exact convolution, so the rounded results differ by at most
ONE level, and only where the exact value lies that close to a rounding boundary.  The share of such samples is bounded by the
specification at 1 %; it measures 0.125 % on these inputs."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _blur_ref as B  # noqa: E402

SIZES = [(1, 1), (2, 3), (7, 5), (17, 31), (65, 129), (33, 200)]                               # (height, width)
GAUSS = [(0.3, None), (0.5, None), (1.0, None), (2.5, None), (5.0, None), (1.0, 1)]           # (sigma, radius; None = three sigma)


def _inputs():
    from tests._jpeg_enc_ref import content
    for k, (h, w) in enumerate(SIZES):
        yield content(31 + k, w, h)
        yield B.two_level(200 + k, h, w)


def test_mirror_is_reflect_without_the_edge_sample():
    assert B.mirror(np.arange(-7, 9), 4).tolist() == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert B.mirror(np.arange(-3, 4), 1).tolist() == [0] * 7
    assert B.mirror(np.arange(-4, 6), 2).tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    for n in (1, 2, 3, 5, 8):                               # numpy's 'reflect' padding is the same rule, repeated for short axes
        want = np.pad(np.arange(n), 17, mode="reflect")
        assert np.array_equal(B.mirror(np.arange(-17, n + 17), n), want), n


def test_gaussian_restatement_is_within_one_level_of_scipy(report):
    samples = differ = 0
    for px in _inputs():
        for sigma, r in GAUSS:
            got = B.gauss(px, sigma, r).astype(np.int64)
            want = np.floor(B.exact_gauss(px, sigma, r) + 0.5).astype(np.int64)
            d = np.abs(got - want)
            assert got.shape == px.shape and d.max() <= 1, (px.shape, sigma, r, int(d.max()))
            samples += d.size
            differ += int((d != 0).sum())
    report(f"[blur cpu] integer Gaussian vs rounded float64 scipy: {differ} of {samples} samples differ ({100.0 * differ / samples:.4f} %), "
           "all by one level")
    assert differ <= 0.01 * samples, (differ, samples)


@pytest.mark.parametrize("k", [3, 5])
def test_median_restatement_equals_scipy(k):
    from scipy import ndimage
    for px in _inputs():
        want = np.stack([ndimage.median_filter(px[..., c], size=k, mode="mirror") for c in range(3)], axis=2)
        assert np.array_equal(B.median(px, k), want), (px.shape, k)


def test_selection_network_of_the_kernel_finds_the_median_of_every_binary_input():
    """the 99 exchanges of csrc/blur.hip's 5 x 5 median, read from the source: a network of min / max exchanges that leaves the median of
    every 0 / 1 input in wire 12 does so for every input (the zero-one principle)"""
    src = open(os.path.join(ROOT, "vip-cup-2022_amd", "csrc", "blur.hip")).read()
    body = re.search(r"NET\[99\]\[2\] = \{(.*?)\};", src, re.S).group(1)
    net = [(int(a), int(b)) for a, b in re.findall(r"\{(\d+), *(\d+)\}", body)]
    assert len(net) == 99 and all(0 <= a < b < 25 for a, b in net)
    popcount = np.array([bin(v).count("1") for v in range(1 << 13)], dtype=np.uint8)
    bad = 0
    for base in range(0, 1 << 25, 1 << 22):
        x = np.arange(base, base + (1 << 22), dtype=np.uint32)
        p = [((x >> i) & 1).astype(np.uint8) for i in range(25)]
        for a, b in net:
            p[a], p[b] = p[a] & p[b], p[a] | p[b]
        bad += int((p[12] != (popcount[x & 0x1FFF] + popcount[x >> 13] >= 13)).sum())
    assert bad == 0


# ---- vip_blur_weights_h -----------------------------------------------------------------------------------------------------------------
def test_library_weights_equal_the_restatement():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    lib = _abi.lib()
    cases = 0
    for tenths in range(3, 51):
        sigma = tenths / 10
        assert pipeline.blur_radius(sigma) == B.radius(sigma) == max(1, -(-3 * tenths // 10))
        for r in (B.radius(sigma), 1, 15):
            w = np.full((2 * r + 2,), -7, np.int32)
            assert lib.vip_blur_weights_h(sigma, r, w.ctypes.data_as(C.c_void_p), w.size) == 0, lib.vip_last_error()
            want = B.weights(sigma, r)
            assert np.array_equal(w[:-1], want) and w[-1] == -7, (sigma, r)
            assert int(w[:-1].sum()) == 65536 and (w[:-1] >= 0).all() and np.array_equal(w[:-1], w[:-1][::-1]), (sigma, r)
            cached = pipeline.blur_weights(sigma, r)
            assert np.array_equal(cached, want) and cached.dtype == np.int32 and pipeline.blur_weights(sigma, r) is cached
            cases += 1
        assert np.array_equal(pipeline.blur_weights(sigma), B.weights(sigma))
    assert cases == 48 * 3


def test_weight_arguments_are_checked_before_any_work():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    lib = _abi.lib()
    w = np.full((31,), -7, np.int32)
    pw = w.ctypes.data_as(C.c_void_p)
    for sigma in (0.29, 5.01, 0.0, -1.0, float("nan"), float("inf")):
        assert lib.vip_blur_weights_h(sigma, 3, pw, w.size) == -1
        assert b"sigma" in lib.vip_last_error() and (w == -7).all()
    for r in (0, -1, 16, 100):
        assert lib.vip_blur_weights_h(1.0, r, pw, w.size) == -1
        assert b"radius" in lib.vip_last_error() and (w == -7).all()
    assert lib.vip_blur_weights_h(1.0, 3, pw, 6) == -1
    assert b"too short" in lib.vip_last_error() and (w == -7).all()
    assert lib.vip_blur_weights_h(1.0, 3, None, 7) == -1
    assert lib.vip_blur_weights_h(1.0, 3, pw, 7) == 0 and (w[7:] == -7).all() and np.array_equal(w[:7], B.weights(1.0, 3))
    # the device entry points refuse bad arguments before they launch anything
    p, q = C.c_void_p(1 << 20), C.c_void_p(1 << 24)
    assert lib.vip_blur_gauss_rgb_u8(None, p, 8, 8, q, 8, 8, p, 3, 1, None) == -1
    assert lib.vip_blur_gauss_rgb_u8(p, p, 8, 8, q, 8, 0, p, 3, 1, None) == -1
    assert lib.vip_blur_gauss_rgb_u8(p, p, 8, 8, q, 8, 8, p, 16, 1, None) == -1 and b"radius" in lib.vip_last_error()
    assert lib.vip_blur_gauss_rgb_u8(p, p, 8, 8, q, 8, 8, p, 0, 1, None) == -1
    assert lib.vip_blur_gauss_rgb_u8(p, p, 8, 8, q, 8, 8, None, 3, 1, None) == -1
    assert lib.vip_blur_gauss_rgb_u8(p, p, 8, 8, p, 8, 8, p, 3, 1, None) == -1 and b"overlap" in lib.vip_last_error()
    assert lib.vip_blur_gauss_rgb_u8(p, p, 8, 8, C.c_void_p((1 << 20) + 191), 9, 9, p, 3, 1, None) == -1 and b"overlap" in lib.vip_last_error()
    assert lib.vip_blur_gauss_rgb_u8(p, C.c_void_p(66), 8, 8, q, 8, 8, p, 3, 1, None) == -2
    for k in (1, 2, 4, 7, 0, -3):
        assert lib.vip_median_rgb_u8(p, p, 8, 8, q, 8, 8, k, 1, None) == -1 and b"3 or 5" in lib.vip_last_error()
    assert lib.vip_median_rgb_u8(p, p, 8, 8, p, 8, 8, 3, 1, None) == -1 and b"overlap" in lib.vip_last_error()
    assert lib.vip_median_rgb_u8(p, None, 8, 8, q, 8, 8, 3, 1, None) == -1
    assert lib.vip_median_rgb_u8(p, p, 8, 8, q, 8, 8, 3, 0, None) == -1


# ---- Python layers ------------------------------------------------------------------------------------------------------------------------
def test_blur_and_median_check_their_arguments_without_a_gpu(monkeypatch):
    """sigma, radius and k are validated before the batch is looked at, the library loaded or anything launched"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    touched = []
    monkeypatch.setattr(pipeline, "_launch", lambda *a, **k: touched.append(a))
    monkeypatch.setattr(_abi, "lib", lambda: touched.append("lib"))
    for sigma in (0.2, 0.29, 5.1, 1.25, 0.35, 0, -1.0, "1.0", None, True, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="multiple of 0.1 in 0.3..5.0"):
            pipeline.blur(None, sigma)
        with pytest.raises(ValueError, match="multiple of 0.1 in 0.3..5.0"):
            pipeline.blur_weights(sigma)
    for r in (0, 16, -1, 2.0, "3", True):
        with pytest.raises(ValueError, match="1..15"):
            pipeline.blur(None, 1.0, r)
    for k in (1, 2, 4, 7, 3.0, "3", None, True):
        with pytest.raises(ValueError, match="expected 3 or 5"):
            pipeline.median(None, k)
    assert not touched
    assert [pipeline.blur_radius(s) for s in (0.3, 0.5, 1.0, 1.1, 2.5, 5.0)] == [1, 2, 3, 4, 8, 15]
    assert pipeline._blur_args(0.3, None) == (3, 1) and pipeline._blur_args(1, 1) == (10, 1) and pipeline._blur_args(np.float32(2.5), 15) == (25, 15)


def test_stress_labels_order():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    assert ensemble.stress_labels([80], [50], [1.0], [3]) == ["q80", "r50", "r50_q80", "b10", "b10_q80", "m3", "m3_q80"]
    assert ensemble.stress_labels([90, 70], (), [2.5, 0.5, 1], [5, 3]) == \
        ["q90", "q70", "b05", "b05_q90", "b05_q70", "b10", "b10_q90", "b10_q70", "b25", "b25_q90", "b25_q70",
         "m3", "m3_q90", "m3_q70", "m5", "m5_q90", "m5_q70"]
    assert ensemble.stress_labels([], [], [5.0, 0.3]) == ["b03", "b50"] and ensemble.stress_labels([], medians=[5]) == ["m5"]
    # the earlier call forms give the earlier results
    assert ensemble.stress_labels([90, 70]) == ["q90", "q70"] and ensemble.stress_labels([], []) == []
    assert ensemble.stress_labels([90, 70], [150, 50]) == ["q90", "q70", "r150", "r150_q90", "r150_q70", "r50", "r50_q90", "r50_q70"]
    assert ensemble.stress_labels([], [50]) == ["r50"]


def test_stress_table_with_blur_and_median_labels():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    names = ["b.jpg", "a.jpg", "c.jpg", "a.jpg", "d.jpg"]
    labels = ["q90", "q70", "b10", "b10_q90", "b10_q70", "m3", "m3_q90", "m3_q70"]
    s = np.zeros((9, 2, 5), dtype=np.float32)                 # [1 + V, M = 2, n = 5]; a.jpg is rows 1 and 3
    s[0] = [[0.9, 0.2, 0.3, 0.6, 0.1]] * 2                    # a 0.4 -> 0, b 0.9 -> 1, c 0.3 -> 0, d 0.1 -> 0
    s[1] = [[0.8, 0.2, 0.3, 0.6, 0.1]] * 2                    # q90: nothing flips
    s[2] = [[0.4, 0.2, 0.3, 0.6, 0.1]] * 2                    # q70: b flips
    s[3] = [[0.9, 0.9, 0.3, 0.7, 0.1]] * 2                    # b10: a -> 0.8 flips
    s[4] = [[0.2, 0.2, 0.9, 0.6, 0.1]] * 2                    # b10_q90: b and c flip
    s[5] = [[0.2, 0.9, 0.9, 0.9, 0.1]] * 2                    # b10_q70: a, b and c flip
    s[6] = [[0.9, 0.2, 0.3, 0.6, 0.9]] * 2                    # m3: d flips
    s[7] = [[0.9, 0.2, 0.3, 0.6, 0.1]] * 2                    # m3_q90: nothing flips
    s[8] = [[0.1, 0.2, 0.3, 0.6, 0.1]] * 2                    # m3_q70: b flips
    table, summary = ensemble.stress_table(names, s, labels)
    assert table["filename"] == ["a.jpg", "b.jpg", "c.jpg", "d.jpg"] and table["labels"] == labels
    for k in range(9):                                        # every row IS aggregate's
        uniq, p, dec = ensemble.aggregate(names, s[k])
        got_p, got_d = (table["p"], table["decision"]) if k == 0 else (table["p_q"][:, k - 1], table["decision_q"][:, k - 1])
        assert uniq == table["filename"] and np.array_equal(p, got_p) and np.array_equal(dec, got_d)
    assert table["stable"].tolist() == [False, False, False, False]                 # over ALL variants
    assert table["flips_at"] == [None, 70, None, None]                              # the unsmoothed q rows only
    assert table["flips"] == ["b10;b10_q70", "q70;b10_q90;b10_q70;m3_q70", "b10_q90;b10_q70", "m3"]
    assert summary["variants"] == labels and summary["qualities"] == [90, 70] and summary["n_stable"] == 0 and summary["n_files"] == 4
    assert summary["flips"] == {"q90": 0, "q70": 1, "b10": 1, "b10_q90": 2, "b10_q70": 3, "m3": 1, "m3_q90": 0, "m3_q70": 1}
    assert summary["flip_rate"]["b10_q70"] == 0.75 and summary["flip_rate"]["m3_q90"] == 0.0
    want = np.abs(table["p_q"].astype(np.float64) - table["p"].astype(np.float64)[:, None]).mean(axis=0)
    assert list(summary["mean_abs_dp"]) == labels
    assert [summary["mean_abs_dp"][v] for v in labels] == pytest.approx(want.tolist(), rel=1e-12)
    # smoothing only: no q rows, so flips_at is empty everywhere
    table, summary = ensemble.stress_table(names, s[[0, 3, 6]], ["b10", "m3"])
    assert table["flips_at"] == [None] * 4 and table["flips"] == ["b10", "", "", "m3"] and table["stable"].tolist() == [False, True, True, False]
    assert summary["qualities"] == [] and summary["variants"] == ["b10", "m3"] and summary["flips"] == {"b10": 1, "m3": 1}


# ---- CLI refusals: everything is refused before torch is imported ---------------------------------------------------------------------------
REFUSALS = [
    (["--stress-blur", "1"], "--stress-blur needs --stress-out"),
    (["--stress-median", "3"], "--stress-median needs --stress-out"),
    (["--stress-blur-radius", "2", "--stress-out", "S"], "--stress-blur-radius needs --stress-blur"),
    (["--stress-blur-radius", "2", "--stress-median", "3", "--stress-out", "S"], "--stress-blur-radius needs --stress-blur"),
    (["--stress-blur", "1", "--stress-blur-radius", "16", "--stress-out", "S"], "integer in 1..15"),
    (["--stress-blur", "1", "--stress-blur-radius", "0", "--stress-out", "S"], "integer in 1..15"),
    (["--stress-blur", "0.2", "--stress-out", "S"], "sigmas in 0.3..5.0"),
    (["--stress-blur", "1,5.1", "--stress-out", "S"], "sigmas in 0.3..5.0"),
    (["--stress-blur", "1.25", "--stress-out", "S"], "sigmas in 0.3..5.0"),
    (["--stress-blur", "1,,2", "--stress-out", "S"], "sigmas in 0.3..5.0"),
    (["--stress-blur", "one", "--stress-out", "S"], "sigmas in 0.3..5.0"),
    (["--stress-median", "4", "--stress-out", "S"], "each 3 or 5"),
    (["--stress-median", "3,7", "--stress-out", "S"], "each 3 or 5"),
    (["--stress-median", "3.0", "--stress-out", "S"], "each 3 or 5"),
    (["--stress-blur", "1", "--stress-out", "S", "--tta", "2"], "--stress-blur works with --shard images and --tta 1 only"),
    (["--stress-median", "3", "--stress-out", "S", "--tta", "2"], "--stress-median works with --shard images and --tta 1 only"),
    (["--stress-blur", "1", "--stress-out", "S", "--shard", "members"], "--stress-blur works with --shard images and --tta 1 only"),
    (["--stress-median", "3", "--stress-out", "S", "--shard", "members"], "--stress-median works with --shard images and --tta 1 only"),
    (["--stress-median", "5", "--stress-out", "S", "--shard", "hybrid"], "--stress-median works with --shard images and --tta 1 only"),
    (["--stress-blur", "1", "--stress-out", "S", "--heatmaps", "H"], "--stress-blur and --heatmaps cannot be combined"),
    (["--stress-median", "3", "--stress-out", "S", "--heatmaps", "H"], "--stress-median and --heatmaps cannot be combined"),
    (["--stress-blur", "1", "--stress-out", "S", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-median", "3", "--stress-out", "S", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-blur", "1", "--stress-out", "S", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--stress-median", "3", "--stress-out", "S", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--stress-blur", "1", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-median", "3", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
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
