"""CPU: the tone perturbations' host side - the numpy restatement (tests/_tone_ref.py) against Pillow's ``ImageOps.autocontrast`` (also
``preserve_tone=True``) and ``ImageOps.equalize`` bit for bit, the float64 auto-contrast table for every pair of levels, the CLAHE grid,
bounds and redistribution, the chain grammar of the tone steps, ``stress_labels`` with the tone rows, and the refusals of ``pipeline``
and ``main.py``."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _tone_ref as ref  # noqa: E402

CUTOFFS = (0, 1, 2, 5, 10, 25, 49)
SIZES = [(1, 1), (1, 7), (2, 2), (5, 9), (13, 4), (16, 16), (37, 53), (60, 60), (59, 23), (200, 200)]
SIX = {(37, 53): (2, 3), (200, 200): (8, 8), (15, 300): (1, 8), (129, 64): (8, 4), (16, 16): (1, 1), (1, 1): (1, 1)}


def _images():
    """(name, uint8 [h, w, 3]): random, low-range, narrow Gaussian and flat content at every size of SIZES"""
    rng = np.random.default_rng(20221)
    out = []
    for h, w in SIZES:
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out.append((f"random{h}x{w}", a))
        out.append((f"low{h}x{w}", (a // 3 + 40).astype(np.uint8)))
        out.append((f"narrow{h}x{w}", np.clip(rng.normal(110, 6, (h, w, 3)), 0, 255).astype(np.uint8)))
        out.append((f"flat{h}x{w}", np.full((h, w, 3), 77, np.uint8)))
    return out


IMAGES = _images()


@pytest.mark.parametrize("luma", [False, True], ids=["ac", "acl"])
def test_autocontrast_equals_pillow(luma):
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    for name, a in IMAGES:
        for c in CUTOFFS:
            want = np.asarray(ImageOps.autocontrast(Image.fromarray(a, "RGB"), cutoff=c, preserve_tone=luma))
            got = ref.tone(a, "autocontrast_luma" if luma else "autocontrast", c)
            assert np.array_equal(got, want), (name, c)


def test_equalize_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    for name, a in IMAGES:
        want = np.asarray(ImageOps.equalize(Image.fromarray(a, "RGB")))
        assert np.array_equal(ref.tone(a, "equalize"), want), name
    # step = 1: table entries above 255 are cut at 255, as Image.point does
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (20, 20, 3), dtype=np.uint8)
    want = np.asarray(ImageOps.equalize(Image.fromarray(a, "RGB")))
    assert np.array_equal(ref.tone(a, "equalize"), want)


def test_autocontrast_table_for_every_pair_of_levels():
    """Pillow's expression, restated here on its own, for all 32 640 pairs; and the integer form is NOT it"""
    pairs, tables = ref.autocontrast_tables_all_pairs()
    assert pairs.shape == (32640, 2) and tables.shape == (32640, 256)
    row = {(int(lo), int(hi)): k for k, (lo, hi) in enumerate(pairs)}
    for lo in range(255):
        for hi in range(lo + 1, 256):
            scale = 255.0 / (hi - lo)
            offset = -lo * scale
            want = []
            for ix in range(256):
                v = int(ix * scale + offset)
                want.append(0 if v < 0 else 255 if v > 255 else v)
            assert ref.autocontrast_table_lo_hi(lo, hi) == want == tables[row[lo, hi]].tolist(), (lo, hi)
            h = np.zeros(256, np.int64)
            h[lo], h[hi] = 3, 5
            if (lo + hi) % 16 == 0:                          # the table found from a histogram: a sample of the pairs
                assert ref.autocontrast_table(h, 0) == want, (lo, hi)
    lo, hi, i = pairs[:, :1], pairs[:, 1:], np.arange(256)[None, :]
    differ = int((np.clip(((i - lo) * 255) // (hi - lo), 0, 255) != tables).sum())
    assert differ == 12094 and tables.size == 8355840


def test_autocontrast_table_equals_pillows_for_every_pair_of_levels():
    """Pillow itself: a ramp of all 256 levels whose histogram is taken under a mask that shows the levels lo and hi only comes back as
    the whole table of (lo, hi)"""
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    ramp = Image.fromarray(np.arange(256, dtype=np.uint8)[None, :], "L")
    pairs, tables = ref.autocontrast_tables_all_pairs()
    shown = np.zeros((1, 256), np.uint8)
    for (lo, hi), want in zip(pairs, tables):
        shown[0, lo] = shown[0, hi] = 255
        got = np.asarray(ImageOps.autocontrast(ramp, cutoff=0, mask=Image.fromarray(shown, "L")))[0]
        shown[0, lo] = shown[0, hi] = 0
        assert np.array_equal(got, want), (lo, hi)


def test_grid_and_bounds():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    for (h, w), want in SIX.items():
        assert pipeline.tone_grid(h, w, 8) == want == ref.grid(h, w, 8), (h, w)
        for side, g in ((h, want[0]), (w, want[1])):
            b = ref.bounds(side, g)
            assert b == pipeline.occlusion_bounds(side, g) and b[0] == 0 and b[-1] == side
            assert all(b[k + 1] - b[k] >= (16 if g > 1 else 1) for k in range(g))
    assert pipeline.tone_grid(200, 200, 3) == (3, 3) and pipeline.tone_grid(200, 40, 16) == (12, 2) and pipeline.tone_grid(15, 31, 1) == (1, 1)
    for bad in (0, 17, 2.0, True, None):
        with pytest.raises(ValueError, match="grid"):
            pipeline.tone_grid(200, 200, bad)


def test_axis_neighbours():
    for side, g in ((37, 2), (53, 3), (200, 8), (300, 8), (129, 8), (16, 1), (1, 1), (64, 4)):
        b = ref.bounds(side, g)
        k0, k1, wq = ref.axis_neighbours(side, g)
        assert ((0 <= wq) & (wq <= 255)).all() and (k0 <= k1).all() and (k1 - k0 <= 1).all() and (np.diff(k0) >= 0).all()
        assert k0[0] == 0 and k1[-1] == g - 1
        for k in range(g):                                   # nearest its own tile's centre a pixel takes at least half from that tile
            x = (b[k] + b[k + 1]) // 2
            assert k in (k0[x], k1[x])
            assert (256 - wq[x] if k0[x] == k else wq[x]) >= 128 or k0[x] == k1[x]


def test_clahe_redistribution_keeps_the_area():
    rng = np.random.default_rng(5)
    cases = [rng.integers(0, 40, 256), np.bincount(np.clip(rng.normal(110, 5, 625), 0, 255).astype(int), minlength=256),
             np.eye(256, dtype=np.int64)[7] * 40000, np.ones(256, np.int64), np.eye(256, dtype=np.int64)[255]]
    for h in cases:
        A = int(np.sum(h))
        for tt in (10, 20, 57, 99):
            h2 = ref.clahe_redistribute(h, tt)
            assert sum(h2) == A and min(h2) >= 0
            t = ref.clahe_table(h, tt)
            assert t[255] == 255 and all(t[i] <= t[i + 1] for i in range(255))


def test_clahe_on_one_tile_is_a_plain_table():
    rng = np.random.default_rng(6)
    a = np.clip(rng.normal(120, 30, (16, 16, 3)), 0, 255).astype(np.uint8)
    assert ref.grid(16, 16) == (1, 1)
    Y = ref.luma(a)
    for tt in (10, 20, 99):
        T = np.array(ref.clahe_table(ref.hist256(Y), tt), np.int64)
        want = np.clip(a.astype(np.int64) + (T[Y] - Y)[..., None], 0, 255).astype(np.uint8)
        assert np.array_equal(ref.clahe(a, tt), want)
    one = np.array([[[10, 200, 30]]], np.uint8)
    assert ref.clahe(one, 20).shape == (1, 1, 3)


def test_tile_histograms_add_up():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    for G in (1, 2, 8):
        h3, h1 = ref.tile_histograms(a, G, 3), ref.tile_histograms(a, G, 1)
        assert np.array_equal(h3.sum(0), np.stack([ref.hist256(a[..., c]) for c in range(3)]))
        assert np.array_equal(h1.sum(0)[0], ref.hist256(ref.luma(a)))


# ---- chain grammar ------------------------------------------------------------------------------------------------------------------
STEPS = [("ac00", ("autocontrast", 0)), ("ac02", ("autocontrast", 2)), ("ac49", ("autocontrast", 49)), ("acl00", ("autocontrast_luma", 0)),
         ("acl49", ("autocontrast_luma", 49)), ("eq", ("equalize", None)), ("clahe10", ("clahe", 1.0)), ("clahe20", ("clahe", 2.0)),
         ("clahe99", ("clahe", 9.9))]


def test_tone_steps_parse_in_both_positions():
    from vipcup_amd import chain
    for token, want in STEPS:
        assert chain.parse_chain(f"{token}+q75") == [want, ("recompress", 75)], token
        assert chain.parse_chain(f"q90+{token}") == [("recompress", 90), want], token
    assert [k for k, _ in chain.parse_chain("r50+clahe20+q75")] == ["rescale", "clahe", "recompress"]
    assert chain.chain_kinds(["eq+q80", "r50+acl02"]) == {"equalize", "recompress", "rescale", "autocontrast_luma"}
    assert chain.chain_noise_seeds(chain.parse_chain("n030+eq+n030"), 4) == [4, None, 5]


@pytest.mark.parametrize("token", ["ac50", "ac5", "clahe09", "clahe100", "eq1", "acl", "ac", "acl50", "acl2", "clahe", "clahe2.0", "EQ", "ac002"])
def test_tone_steps_refused(token):
    from vipcup_amd import chain
    for text in (f"{token}+q80", f"q80+{token}"):
        with pytest.raises(ValueError) as e:
            chain.parse_chain(text)
        assert repr(token) in str(e.value), str(e.value)


def test_one_step_chains_name_the_flag():
    from vipcup_amd import chain
    for token, flag in (("ac02", "--stress-autocontrast"), ("acl02", "--stress-autocontrast-luma"), ("eq", "--stress-equalize"),
                        ("clahe20", "--stress-clahe")):
        with pytest.raises(ValueError) as e:
            chain.parse_chain(token)
        assert str(e.value).endswith(f"{flag} gives"), str(e.value)


# ---- stress_labels ------------------------------------------------------------------------------------------------------------------
def test_stress_labels_with_tone_rows():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    got = ensemble.stress_labels([90, 70], sharpens=[150], chains=["eq+q80"], autocontrasts=[5, 2], autocontrast_lumas=[2], equalize=True,
                                 clahes=[4.0, 2], clahe_grid=3)
    tone = ["ac02", "ac05", "acl02", "eq", "clahe20", "clahe40"]
    assert got == ["q90", "q70", "shp150", "shp150_q90", "shp150_q70"] + [x for v in tone for x in (v, f"{v}_q90", f"{v}_q70")] + ["eq+q80"]
    assert ensemble.stress_labels([], equalize=True, clahes=[9.9, 1.0]) == ["eq", "clahe10", "clahe99"]
    assert ensemble.stress_labels([80], autocontrasts=[0]) == ["q80", "ac00", "ac00_q80"]
    full = dict(scales=[50], blurs=[1.0], medians=[3], flips=["h"], crops=[90], rotations=[7.5], gray=True, hues=[30], impulses=[1], sharpens=[80],
                chains=["r50+q75"])
    base = ensemble.stress_labels([80], **full)
    assert ensemble.stress_labels([80], **full, autocontrasts=(), autocontrast_lumas=(), equalize=False, clahes=(), clahe_grid=8) == base
    assert base[-3:] == ["shp080", "shp080_q80", "r50+q75"]
    assert ensemble.stress_labels([80], **full, equalize=True)[-5:] == ["shp080", "shp080_q80", "eq", "eq_q80", "r50+q75"]


# ---- refusals before any launch -----------------------------------------------------------------------------------------------------
def test_pipeline_checks_before_any_launch(monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    touched = []
    monkeypatch.setattr(pipeline, "_launch", lambda *a, **k: touched.append(a))
    monkeypatch.setattr(_abi, "lib", lambda: touched.append("lib"))
    for bad in (-1, 50, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="cutoff"):
            pipeline.autocontrast(None, bad)
        with pytest.raises(ValueError, match="cutoff"):
            pipeline.autocontrast(None, bad, luma=True)
        with pytest.raises(ValueError, match="cutoff"):
            pipeline.tone(None, "autocontrast", bad)
    with pytest.raises(ValueError, match="luma"):
        pipeline.autocontrast(None, 2, luma=1)
    for bad in (0.9, 10.0, 2.05, True, None, "2", float("nan")):
        with pytest.raises(ValueError, match="limit"):
            pipeline.clahe(None, bad)
    for bad in (0, 17, 8.0, True, None):
        with pytest.raises(ValueError, match="grid"):
            pipeline.clahe(None, 2.0, bad)
        with pytest.raises(ValueError, match="grid"):
            pipeline.tone(None, "equalize", None, bad)
        with pytest.raises(ValueError, match="clahe_grid"):
            pipeline.apply_chain(None, "clahe20+q80", clahe_grid=bad)
    with pytest.raises(ValueError, match="no argument"):
        pipeline.tone(None, "equalize", 3)
    for bad in ("posterize", "eq", None, 3):
        with pytest.raises(ValueError, match="mode"):
            pipeline.tone(None, bad, 2)
    with pytest.raises(ValueError, match="'ac50'"):
        pipeline.apply_chain(None, "ac50+q80")
    with pytest.raises(ValueError, match="'clahe09'"):
        pipeline.apply_chain(None, "q80+clahe09")
    with pytest.raises(ValueError, match="not a step"):
        pipeline.apply_chain(None, [("posterize", 3)])
    with pytest.raises(ValueError, match="channels"):
        pipeline.tone_histograms(None, 8, 2)
    assert not touched


# ---- CLI refusals: everything is refused before torch is imported -------------------------------------------------------------------
REFUSALS = [
    (["--stress-autocontrast", "2,2", "--stress-out", "S"], "each listed once"),
    (["--stress-autocontrast-luma", "5,2,5", "--stress-out", "S"], "each listed once"),
    (["--stress-clahe", "2,2.0", "--stress-out", "S"], "each listed once"),
    (["--stress-autocontrast", "50", "--stress-out", "S"], "0..49"),
    (["--stress-autocontrast-luma", "-1", "--stress-out", "S"], "0..49"),
    (["--stress-clahe", "0.9", "--stress-out", "S"], "1.0..9.9"),
    (["--stress-clahe", "2.05", "--stress-out", "S"], "1.0..9.9"),
    (["--stress-clahe-grid", "4"], "--stress-clahe-grid needs --stress-clahe"),
    (["--stress-equalize", "--stress-out", "S", "--stress-clahe-grid", "4"], "--stress-clahe-grid needs --stress-clahe"),
    (["--stress-chain", "eq+q80", "--stress-out", "S", "--stress-clahe-grid", "4"], "--stress-clahe-grid needs --stress-clahe"),
    (["--stress-clahe", "2", "--stress-out", "S", "--stress-clahe-grid", "17"], "integer in 1..16"),
    (["--stress-chain", "clahe20+q80", "--stress-out", "S", "--stress-clahe-grid", "0"], "integer in 1..16"),
    (["--stress-equalize"], "--stress-equalize needs --stress-out"),
    (["--stress-clahe", "2"], "--stress-clahe needs --stress-out"),
    (["--stress-autocontrast", "2", "--stress-out", "S", "--shard", "members"], "--stress-autocontrast works with --shard images and --tta 1 only"),
    (["--stress-autocontrast-luma", "2", "--stress-out", "S", "--shard", "hybrid"],
     "--stress-autocontrast-luma works with --shard images and --tta 1 only"),
    (["--stress-equalize", "--stress-out", "S", "--tta", "2"], "--stress-equalize works with --shard images and --tta 1 only"),
    (["--stress-clahe", "2", "--stress-out", "S", "--heatmaps", "H"], "--stress-clahe and --heatmaps cannot be combined"),
    (["--stress-equalize", "--stress-out", "S", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-clahe", "2", "--stress-out", "S", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--stress-chain", "ac50+q80", "--stress-out", "S"], "chain step 'ac50'"),
    (["--stress-chain", "eq", "--stress-out", "S"], "--stress-equalize gives"),
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


def test_cli_accepts_the_grid_with_a_clahe_step(tmp_path):
    """--stress-clahe-grid goes with --stress-clahe or a chain that holds a clahe step: the run gets past every refusal"""
    (tmp_path / "test.csv").write_text("filename\nimg_00000.jpg\n")
    for extra in (["--stress-clahe", "2,4.5", "--stress-autocontrast", "0,2", "--stress-autocontrast-luma", "49", "--stress-equalize"],
                  ["--stress-chain", "r50+clahe20+q75"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "vip-cup-2022_amd", "main.py"), str(tmp_path / "test.csv"), str(tmp_path / "o.csv"),
                            "--synthetic", "--stress-out", str(tmp_path / "stress.csv"), *extra, "--stress-clahe-grid", "3", "--ckpt-cfg",
                            str(tmp_path / "none.json")], capture_output=True, text=True, timeout=300)
        out = r.stderr + r.stdout
        assert r.returncode != 0 and ("no GPU visible" in out or "none.json" in out), out[-600:]
        assert "needs --stress" not in out and "need --stress" not in out and "expected" not in out
