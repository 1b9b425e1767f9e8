"""CPU: the colour stress tests without a GPU - the numpy restatement of csrc/colour.hip (tests/_colour_ref.py) against Pillow and
against the float64 formula it approximates, ``pipeline``'s constructors against the restatement's, the argument checks of ``pipeline``
and of the entry point, ``stress_labels`` / ``stress_table`` with colour labels, and ``main.py``'s refusals.

The bound on the restatement's distance from the rounded float64 formula is derived, not measured: 0.5 from the final rounding, at most
3 * 255 * 2^-17 < 0.006 from rounding the three matrix coefficients to Q16 (and as much again from K and O), and - for contrast only -
0.5 |1 - f| <= 0.5 from the image mean rounded to an integer; together below 1.02, and two integers that far apart differ by at most 1."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _colour_ref as R  # noqa: E402


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _gradient(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(h + w - 2, 1)], axis=2).astype(np.uint8)


def _grays(h, w):
    v = (np.arange(h * w) % 256).astype(np.uint8).reshape(h, w)
    return np.stack([v, v, v], axis=2)


def _inputs():
    return [_noise(1, 37, 53), _grays(16, 32), _gradient(40, 61), np.full((5, 5, 3), 255, np.uint8), np.zeros((3, 4, 3), np.uint8)]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_gray_equals_pillow_and_bgr_is_the_reversal():
    for px in _inputs():
        got = R.apply(px, *R.gray())
        want = np.asarray(Image.fromarray(px).convert("L"))
        assert np.array_equal(got[..., 0], want) and np.array_equal(got[..., 1], want) and np.array_equal(got[..., 2], want)
        assert np.array_equal(R.apply(px, *R.bgr()), px[..., ::-1])
    assert [a.tolist() if a is not None else None for a in R.saturation(0)] == [a.tolist() if a is not None else None for a in R.gray()]


def test_hue_and_saturation_leave_gray_pixels_alone():
    px = _grays(16, 32)
    for d in (1, -1, 30, -30, 90, -90, 180):
        assert np.array_equal(R.apply(px, *R.hue(d)), px), d
    for pc in R.SATURATIONS:
        assert np.array_equal(R.apply(px, *R.saturation(pc)), px), pc


@pytest.mark.parametrize("kind,args", [("hue", R.HUES), ("saturation", R.SATURATIONS), ("contrast", R.CONTRASTS),
                                       ("brightness", R.BRIGHTNESSES)])
def test_restatement_is_within_one_level_of_the_float64_formula(kind, args, report):
    real = {"hue": R.hue_real, "saturation": R.saturation_real, "contrast": R.contrast_real, "brightness": R.brightness_real}[kind]
    worst = 0
    for arg in args:
        for px in _inputs():
            d = int(np.abs(R.apply(px, *R.variant(kind, arg)).astype(np.int64) - R.exact(px, *real(arg)).astype(np.int64)).max())
            worst = max(worst, d)
            assert d <= 1, (kind, arg, px.shape, d)
    report(f"colour restatement vs float64 formula: {kind}: worst {worst} level(s) over {args}")


def test_every_hue_matrix_fits_the_entry_points_bound():
    worst = max(int(np.abs(R.hue(d)[0]).max()) for d in range(-180, 181) if d)
    assert worst < 1 << 18, worst
    for kind, args in (("saturation", range(0, 201)), ("contrast", range(0, 201)), ("brightness", range(-50, 51))):
        for arg in args:
            M, K, O, _ = R.variant(kind, arg)
            assert np.abs(M).max() <= 1 << 18 and (K is None or np.abs(K).max() <= 1 << 18) and (O is None or np.abs(O).max() <= 1 << 25)


def test_gamma_tables():
    lut = R.gamma(2.0)[3]
    assert lut[0] == 0 and lut[255] == 255 and lut[128] == 64
    for g in R.GAMMAS + [0.51, 1.99, 1.01]:
        lut = R.gamma(g)[3]
        assert lut.shape == (256,) and lut[0] == 0 and lut[255] == 255 and (np.diff(lut) >= 0).all(), g
    assert (R.gamma(0.8)[3] >= np.arange(256)).all() and (R.gamma(1.25)[3] <= np.arange(256)).all()     # below 1 brightens


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(np.asarray(x), np.asarray(y)))
               for x, y in zip(a, b)) and len(a) == len(b) == 4


def test_pipeline_constructors_equal_the_restatements():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    assert _same(pipeline.colour_gray(), R.gray()) and _same(pipeline.colour_bgr(), R.bgr())
    for d in range(-180, 181):
        if d:
            assert _same(pipeline.colour_hue(d), R.hue(d)), d
    for pc in range(0, 201):
        if pc != 100:
            assert _same(pipeline.colour_saturation(pc), R.saturation(pc)), pc
            assert _same(pipeline.colour_contrast(pc), R.contrast(pc)), pc
    for pc in range(-50, 51):
        if pc:
            assert _same(pipeline.colour_brightness(pc), R.brightness(pc)), pc
    for hh in range(50, 201):
        if hh != 100:
            assert _same(pipeline.colour_gamma(hh / 100), R.gamma(hh / 100)), hh
    assert _same(pipeline.colour_saturation(0), pipeline.colour_gray())
    assert pipeline.colour_contrast(150)[1].tolist() == [-32768] * 3 and pipeline.colour_brightness(10)[2].tolist() == [1671168] * 3


def test_colour_checks_its_arguments_without_a_gpu(monkeypatch):
    """coefficients, tables and the named variants' arguments are validated before the batch is looked at or anything launched"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    touched = []
    monkeypatch.setattr(pipeline, "_launch", lambda *a, **k: touched.append(a))
    monkeypatch.setattr(_abi, "lib", lambda: touched.append("lib"))
    ident = [[65536, 0, 0], [0, 65536, 0], [0, 0, 65536]]
    for M in (None, [[1, 2, 3]], [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], np.eye(3), [[1, 0], [0, 1]], "M", [[1, 2, 3], [4, 5], [6]]):
        with pytest.raises(ValueError, match="3 x 3 integers"):
            pipeline.colour(None, M)
    big = [[(1 << 18) + 1, 0, 0], [0, 65536, 0], [0, 0, 65536]]
    with pytest.raises(ValueError, match="M: 262145 is outside -262144..262144"):
        pipeline.colour(None, big)
    with pytest.raises(ValueError, match="K: -262145 is outside"):
        pipeline.colour(None, ident, K=[0, -(1 << 18) - 1, 0])
    with pytest.raises(ValueError, match="O: 33554433 is outside -33554432..33554432"):
        pipeline.colour(None, ident, O=[0, 0, (1 << 25) + 1])
    for K in ([1, 2], [0.5, 0, 0], 7):
        with pytest.raises(ValueError, match="K .*expected 3 integers"):
            pipeline.colour(None, ident, K=K)
    for lut in (list(range(255)), np.arange(256) / 2, "lut"):
        with pytest.raises(ValueError, match="expected 256 integers"):
            pipeline.colour(None, ident, lut=lut)
    with pytest.raises(ValueError, match="lut: 256 is outside"):
        pipeline.colour(None, ident, lut=list(range(1, 257)))
    with pytest.raises(ValueError, match="lut: -1 is outside 0..255"):
        pipeline.colour(None, ident, lut=[-1] + [0] * 255)
    for d in (0, 181, -181, 30.0, "30", None, True):
        with pytest.raises(ValueError, match="degrees .*-180..180"):
            pipeline.hue(None, d)
    for fn in (pipeline.saturation, pipeline.contrast):
        for pc in (100, -1, 201, 50.0, "50", None, True):
            with pytest.raises(ValueError, match="percent .*0..200"):
                fn(None, pc)
    for pc in (0, 51, -51, 10.0, "10", None, True):
        with pytest.raises(ValueError, match="percent .*-50..50"):
            pipeline.brightness(None, pc)
    for g in (1, 1.0, 0.49, 2.01, 0.805, "0.8", None, True, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gamma .*0.50..2.00"):
            pipeline.gamma(None, g)
    assert not touched


def test_entry_point_refuses_bad_arguments_before_it_launches():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    lib = _abi.lib()
    f = lib.vip_colour_rgb_u8
    p, q, s, m = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 28), C.c_void_p(1 << 29)

    def coef(**kw):
        v = np.zeros(15, np.int32)
        v[[0, 4, 8]] = 65536
        for k, x in kw.items():
            v[int(k[1:])] = x
        return v

    ok = coef()
    cp = lambda v: v.ctypes.data_as(C.c_void_p)           # noqa: E731
    for k in (0, 1, 4, 7):                                    # every required pointer
        args = [p, s, 8, 8, q, 8, 8, cp(ok), None, None, 1, None]
        args[k] = None
        assert f(*args) == -1 and b"null pointer" in lib.vip_last_error(), k
    for k in (2, 3, 5, 6, 10):                                # n and every slot side
        for v in (0, -1):
            args = [p, s, 8, 8, q, 8, 8, cp(ok), None, None, 1, None]
            args[k] = v
            assert f(*args) == -1 and b"bad size" in lib.vip_last_error(), (k, v)
    assert f(p, s, 8, 8, p, 8, 8, cp(ok), None, None, 1, None) == -1 and b"overlap" in lib.vip_last_error()
    assert f(p, s, 8, 8, C.c_void_p((1 << 20) + 191), 9, 9, cp(ok), None, None, 1, None) == -1 and b"overlap" in lib.vip_last_error()
    for k, lim in [(c, 1 << 18) for c in range(12)] + [(c, 1 << 25) for c in range(12, 15)]:
        for sign in (1, -1):
            bad = coef(**{f"c{k}": sign * (lim + 1)})
            assert f(p, s, 8, 8, q, 8, 8, cp(bad), m, None, 1, None) == -1 and b"coefficient" in lib.vip_last_error(), (k, sign)
    for k in (9, 10, 11):                                     # a K without the means
        assert f(p, s, 8, 8, q, 8, 8, cp(coef(**{f"c{k}": 1})), None, None, 1, None) == -1 and b"mean_u8" in lib.vip_last_error()
    assert f(p, C.c_void_p((1 << 28) + 2), 8, 8, q, 8, 8, cp(ok), None, None, 1, None) == -2 and b"4-byte" in lib.vip_last_error()
    assert f(p, s, 8, 8, q, 8, 8, cp(coef(c9=1)), C.c_void_p((1 << 29) + 1), None, 1, None) == -2 and b"4-byte" in lib.vip_last_error()


# ---- ensemble -----------------------------------------------------------------------------------------------------------------------------
def test_stress_labels_order():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    assert ensemble.stress_labels([75], gray=True, hues=[30], contrasts=[150]) == \
        ["q75", "gray", "gray_q75", "hue030", "hue030_q75", "con150", "con150_q75"]
    got = ensemble.stress_labels([90, 70], [50], [1.0], [3], flips=["h"], rotations=[-3], gammas=[1.25, 0.8], brightnesses=[10, -10, 5],
                                 contrasts=[150, 50], saturations=[150, 0, 50], hues=[30, -30, 180, -5], bgr=True, gray=True)
    variants = ["r50", "b10", "m3", "fliph", "rotm030", "gray", "bgr", "huem030", "huem005", "hue030", "hue180", "sat000", "sat050", "sat150",
                "con050", "con150", "brim10", "bri05", "bri10", "gam080", "gam125"]
    assert got == ["q90", "q70"] + [v + s for v in variants for s in ("", "_q90", "_q70")]
    assert ensemble.stress_labels([], bgr=True, gammas=[2, 0.5]) == ["bgr", "gam050", "gam200"]
    assert ensemble.stress_labels([], brightnesses=[-50, 50]) == ["brim50", "bri50"] and ensemble.stress_labels([], hues=[-180]) == ["huem180"]
    # the new keywords left out or empty: the earlier lists
    none = dict(gray=False, bgr=False, hues=(), saturations=(), contrasts=(), brightnesses=(), gammas=())
    for args, kw in ((([90, 70],), {}), (([], []), {}), (([80], [50], [1.0], [3]), {}), (([75],), dict(flips=["h"], crops=[80], rotations=[7.5]))):
        assert ensemble.stress_labels(*args, **kw, **none) == ensemble.stress_labels(*args, **kw)
    assert ensemble.stress_labels([75], flips=["h"], crops=[80], rotations=[7.5]) == \
        ["q75", "fliph", "fliph_q75", "crop80", "crop80_q75", "rot075", "rot075_q75"]
    assert ensemble.stress_labels([80], [50], [1.0], [3]) == ["q80", "r50", "r50_q80", "b10", "b10_q80", "m3", "m3_q80"]
    assert ensemble.stress_labels([90, 70]) == ["q90", "q70"] and ensemble.stress_labels([], []) == []


def test_stress_table_with_colour_labels():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    names = ["b.jpg", "a.jpg", "c.jpg", "a.jpg", "d.jpg"]
    labels = ensemble.stress_labels([75], gray=True, saturations=[50], brightnesses=[-10])
    assert labels == ["q75", "gray", "gray_q75", "sat050", "sat050_q75", "brim10", "brim10_q75"]
    s = np.zeros((8, 2, 5), dtype=np.float32)                 # [1 + V, M = 2, n = 5]; a.jpg is rows 1 and 3
    s[0] = [[0.9, 0.2, 0.3, 0.6, 0.1]] * 2                    # a 0.4 -> 0, b 0.9 -> 1, c 0.3 -> 0, d 0.1 -> 0
    s[1] = [[0.4, 0.2, 0.3, 0.6, 0.1]] * 2                    # q75: b flips
    s[2] = [[0.9, 0.2, 0.3, 0.6, 0.1]] * 2                    # gray: nothing flips
    s[3] = [[0.9, 0.9, 0.3, 0.7, 0.1]] * 2                    # gray_q75: a -> 0.8 flips
    s[4] = [[0.9, 0.2, 0.3, 0.6, 0.9]] * 2                    # sat050: d flips
    s[5] = [[0.2, 0.2, 0.9, 0.6, 0.1]] * 2                    # sat050_q75: b and c flip
    s[6] = [[0.9, 0.2, 0.3, 0.6, 0.1]] * 2                    # brim10: nothing flips
    s[7] = [[0.1, 0.9, 0.9, 0.9, 0.9]] * 2                    # brim10_q75: everything flips
    table, summary = ensemble.stress_table(names, s, labels)
    assert table["filename"] == ["a.jpg", "b.jpg", "c.jpg", "d.jpg"] and table["labels"] == labels
    for k in range(8):                                        # every row IS aggregate's
        uniq, p, dec = ensemble.aggregate(names, s[k])
        got_p, got_d = (table["p"], table["decision"]) if k == 0 else (table["p_q"][:, k - 1], table["decision_q"][:, k - 1])
        assert uniq == table["filename"] and np.array_equal(p, got_p) and np.array_equal(dec, got_d)
    assert table["stable"].tolist() == [False] * 4 and table["flips_at"] == [None, 75, None, None]      # flips_at: the plain q rows only
    assert table["flips"] == ["gray_q75;brim10_q75", "q75;sat050_q75;brim10_q75", "sat050_q75;brim10_q75", "sat050;brim10_q75"]
    assert summary["variants"] == labels and summary["qualities"] == [75] and summary["n_stable"] == 0 and summary["n_files"] == 4
    assert summary["flips"] == {"q75": 1, "gray": 0, "gray_q75": 1, "sat050": 1, "sat050_q75": 2, "brim10": 0, "brim10_q75": 4}
    table, summary = ensemble.stress_table(names, s[[0, 2, 4]], ["gray", "sat050"])                    # colour only: no q rows
    assert table["flips_at"] == [None] * 4 and table["flips"] == ["", "", "", "sat050"] and summary["qualities"] == []
    assert table["stable"].tolist() == [True, True, True, False]


# ---- CLI refusals: everything is refused before torch is imported or a model is built --------------------------------------------------------
REFUSALS = [
    (["--stress-gray"], "--stress-gray needs --stress-out"),
    (["--stress-bgr"], "--stress-bgr needs --stress-out"),
    (["--stress-hue", "30"], "--stress-hue needs --stress-out"),
    (["--stress-saturation", "50"], "--stress-saturation needs --stress-out"),
    (["--stress-contrast", "150"], "--stress-contrast needs --stress-out"),
    (["--stress-brightness", "10"], "--stress-brightness needs --stress-out"),
    (["--stress-gamma", "0.8"], "--stress-gamma needs --stress-out"),
    (["--stress-hue", "0", "--stress-out", "S"], "--stress-hue '0': expected a comma-separated list of non-zero integer degrees in -180..180"),
    (["--stress-hue", "181", "--stress-out", "S"], "--stress-hue '181'"),
    (["--stress-hue=-181,30", "--stress-out", "S"], "non-zero integer degrees in -180..180"),
    (["--stress-hue", "7.5", "--stress-out", "S"], "non-zero integer degrees in -180..180"),
    (["--stress-hue", "30,,60", "--stress-out", "S"], "non-zero integer degrees in -180..180"),
    (["--stress-saturation", "100", "--stress-out", "S"], "--stress-saturation '100': expected a comma-separated list of integer percents in 0..200 other than 100"),
    (["--stress-saturation", "50,201", "--stress-out", "S"], "integer percents in 0..200 other than 100"),
    (["--stress-saturation=-5", "--stress-out", "S"], "integer percents in 0..200 other than 100"),
    (["--stress-contrast", "100", "--stress-out", "S"], "--stress-contrast '100'"),
    (["--stress-contrast", "x", "--stress-out", "S"], "integer percents in 0..200 other than 100"),
    (["--stress-brightness", "0", "--stress-out", "S"], "--stress-brightness '0': expected a comma-separated list of non-zero integer percents in -50..50"),
    (["--stress-brightness", "51", "--stress-out", "S"], "non-zero integer percents in -50..50"),
    (["--stress-gamma", "3", "--stress-out", "S"], "--stress-gamma '3': expected a comma-separated list of decimals in 0.50..2.00"),
    (["--stress-gamma", "1", "--stress-out", "S"], "decimals in 0.50..2.00"),
    (["--stress-gamma", "1.00", "--stress-out", "S"], "decimals in 0.50..2.00"),
    (["--stress-gamma", "0.805", "--stress-out", "S"], "decimals in 0.50..2.00"),
    (["--stress-gamma", "0.49", "--stress-out", "S"], "decimals in 0.50..2.00"),
    (["--stress-gray", "--stress-out", "S", "--tta", "2"], "--stress-gray works with --shard images and --tta 1 only"),
    (["--stress-hue", "30", "--stress-out", "S", "--shard", "members"], "the colour stress tests under member sharding or TTA are not implemented"),
    (["--stress-gamma", "0.8", "--stress-out", "S", "--shard", "hybrid"], "--stress-gamma works with --shard images and --tta 1 only"),
    (["--stress-gray", "--stress-out", "S", "--heatmaps", "H"], "--stress-gray and --heatmaps cannot be combined"),
    (["--stress-saturation", "50", "--stress-out", "S", "--heatmaps", "H"], "--stress-saturation and --heatmaps cannot be combined"),
    (["--stress-contrast", "50", "--stress-out", "S", "--heatmaps", "H"], "--stress-contrast and --heatmaps cannot be combined"),
    (["--stress-bgr", "--stress-out", "S", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-hue", "30", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-gamma", "0.8", "--stress-out", "S", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-gray", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--stress-brightness=-10,10", "--stress-out", "S", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--stress-contrast", "50", "--stress-out", "S", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
]


@pytest.mark.parametrize("extra,message", REFUSALS, ids=lambda v: "".join(v) if isinstance(v, list) else None)
def test_cli_refuses_before_scoring(tmp_path, monkeypatch, extra, message):
    """in-process: the refusals come before main.py imports torch or looks at a file, so nothing is built and nothing written"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import main as cli
    from vipcup_amd import zoo
    monkeypatch.setattr(zoo, "build_member", lambda *a, **k: pytest.fail("a member was built"))
    (tmp_path / "test.csv").write_text("filename\nimg_00000.jpg\n")
    paths = {"S": "stress.csv", "H": "maps", "T": "tiles.csv"}
    extra = [str(tmp_path / paths[t]) if t in paths else t for t in extra]
    with pytest.raises(SystemExit) as e:
        cli.main([str(tmp_path / "test.csv"), str(tmp_path / "o.csv"), "--synthetic", *extra])
    assert message in str(e.value), str(e.value)
    assert sorted(os.listdir(tmp_path)) == ["test.csv"]
