"""CPU: stress chains' host side - the grammar of ``--stress-chain`` (``pipeline.parse_chain`` / ``parse_chains``), the seeds of a chain's
noise steps, ``stress_labels`` / ``stress_table`` with ``shp`` and chain labels, and the refusals of ``main.py``."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EVERY_STEP = [("q80", ("recompress", 80)), ("q100", ("recompress", 100)), ("q1", ("recompress", 1)), ("r50", ("rescale", 50)),
              ("r400", ("rescale", 400)), ("r10", ("rescale", 10)), ("b10", ("blur", 1.0)), ("b03", ("blur", 0.3)), ("b50", ("blur", 5.0)),
              ("m3", ("median", 3)), ("m5", ("median", 5)), ("fliph", ("flip", "h")), ("flipv", ("flip", "v")), ("crop90", ("crop", 90)),
              ("crop50", ("crop", 50)), ("rot075", ("rotate", 7.5)), ("rotm123", ("rotate", -12.3)), ("rot450", ("rotate", 45.0)),
              ("gray", ("gray", None)), ("bgr", ("bgr", None)), ("hue030", ("hue", 30)), ("huem180", ("hue", -180)),
              ("sat000", ("saturation", 0)), ("sat150", ("saturation", 150)), ("con050", ("contrast", 50)), ("con200", ("contrast", 200)),
              ("bri10", ("brightness", 10)), ("brim05", ("brightness", -5)), ("gam080", ("gamma", 0.8)), ("gam125", ("gamma", 1.25)),
              ("n030", ("gaussian", 3.0)), ("n005", ("gaussian", 0.5)), ("nm030", ("mono", 3.0)), ("spk05", ("speckle", 5)),
              ("imp010", ("impulse", 1.0)), ("imp500", ("impulse", 50.0)), ("shp080", ("sharpen", 80)), ("shp500", ("sharpen", 500)),
              ("shp001", ("sharpen", 1))]


def _pipeline():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    return pipeline


def test_every_step_kind_in_canonical_spelling():
    pipeline = _pipeline()
    for token, want in EVERY_STEP:
        assert pipeline.parse_chain(f"{token}+q75") == [want, ("recompress", 75)], token
        assert pipeline.parse_chain(f"q90+{token}") == [("recompress", 90), want], token
    eight = "r50+shp080+crop95+n030+gray+b10+fliph+q75"
    assert [k for k, _ in pipeline.parse_chain(eight)] == ["rescale", "sharpen", "crop", "gaussian", "gray", "blur", "flip", "recompress"]
    assert pipeline.parse_chain("r400+r50+r50") == [("rescale", 400), ("rescale", 50), ("rescale", 50)]     # 100 %: within 10..400
    assert pipeline.parse_chain("r20+r50") == [("rescale", 20), ("rescale", 50)]                              # exactly 10 %
    assert pipeline.parse_chain("r200+r200") == [("rescale", 200), ("rescale", 200)]                          # exactly 400 %


def test_steps_match_the_whole_token():
    pipeline = _pipeline()
    want = {"nm030": ("mono", 3.0), "bgr": ("bgr", None), "bri10": ("brightness", 10), "b10": ("blur", 1.0), "m3": ("median", 3)}
    for token, step in want.items():
        assert pipeline.parse_chain(f"{token}+{token}") == [step, step]
    for token in ("nm03", "bgr1", "b10x", "xb10", "m33", "m4", "n030 ", " q80", "Q80", "q80_q70", "r50_q80", "fliphv", "grayy", "b1.0"):
        with pytest.raises(ValueError) as e:
            pipeline.parse_chain(f"{token}+q80")
        assert repr(token) in str(e.value), (token, str(e.value))


REFUSED = [("q80", "--stress-jpeg"), ("shp150", "--stress-sharpen"), ("nm030", "--stress-noise-mono"), ("gray", "--stress-gray"),
           ("+".join(["q80"] * 9), "9 steps"), ("r400+r200", "800 %"), ("r10+r50", "5 %"), ("r100+q80", "'r100'"), ("q0+q80", "'q0'"),
           ("q101+q80", "'q101'"), ("q080+q80", "'q080'"), ("r50+b02", "'b02'"), ("r50+b51", "'b51'"), ("rot000+q80", "'rot000'"),
           ("rot451+q80", "'rot451'"), ("shp000+q80", "'shp000'"), ("shp501+q80", "'shp501'"), ("hue30+q80", "'hue30'"),
           ("hue000+q80", "'hue000'"), ("sat100+q80", "'sat100'"), ("con100+q80", "'con100'"), ("bri00+q80", "'bri00'"),
           ("gam100+q80", "'gam100'"), ("n004+q80", "'n004'"), ("spk51+q80", "'spk51'"), ("imp000+q80", "'imp000'"),
           ("crop49+q80", "'crop49'"), ("r9+q80", "'r9'"), ("r401+q80", "'r401'"), ("r50++q80", "''"), ("+q80", "''"), ("q80+", "''"),
           ("", "''"), ("sharpen+q80", "'sharpen'"), ("r50+jpeg75", "'jpeg75'")]


@pytest.mark.parametrize("text,message", REFUSED, ids=[t[0][:24] or "empty" for t in REFUSED])
def test_parse_chain_refuses(text, message):
    pipeline = _pipeline()
    with pytest.raises(ValueError) as e:
        pipeline.parse_chain(text)
    assert message in str(e.value), str(e.value)


def test_chain_lists():
    pipeline = _pipeline()
    assert pipeline.parse_chains("r50+shp080+q75,q90+crop95+q75") == ["r50+shp080+q75", "q90+crop95+q75"]          # the order given
    assert pipeline.parse_chains("q90+q75") == ["q90+q75"]
    with pytest.raises(ValueError, match="listed twice"):
        pipeline.parse_chains("r50+q80,q90+q75,r50+q80")
    with pytest.raises(ValueError, match="''"):
        pipeline.parse_chains("r50+q80,")
    with pytest.raises(ValueError, match="--stress-resize"):
        pipeline.parse_chains("r50+q80,r50")
    sixteen = [f"r50+q{q}" for q in range(60, 76)]
    assert pipeline.parse_chains(",".join(sixteen)) == sixteen
    with pytest.raises(ValueError, match="at most 16"):
        pipeline.parse_chains(",".join(sixteen + ["r50+q76"]))


def test_noise_step_seeds():
    pipeline = _pipeline()
    steps = pipeline.parse_chain("n030+r50+n030")
    assert pipeline.chain_noise_seeds(steps, 7) == [7, None, 8]
    assert pipeline.chain_noise_seeds(pipeline.parse_chain("n030+q75"), 7) == [7, None]                # the field of the row n030
    assert pipeline.chain_noise_seeds(pipeline.parse_chain("r50+nm030+spk05+imp010+q75"), 0) == [None, 0, 1, 2, None]
    assert pipeline.chain_noise_seeds(pipeline.parse_chain("n030+n030+n030"), 0xFFFFFFFE) == [0xFFFFFFFE, 0xFFFFFFFF, 0]      # mod 2^32
    assert pipeline.chain_noise_seeds(pipeline.parse_chain("r50+q75")) == [None, None]


def test_apply_chain_checks_before_any_launch(monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    touched = []
    monkeypatch.setattr(pipeline, "_launch", lambda *a, **k: touched.append(a))
    monkeypatch.setattr(_abi, "lib", lambda: touched.append("lib"))
    with pytest.raises(ValueError, match="'hue30'"):
        pipeline.apply_chain(None, "hue30+q80")
    with pytest.raises(ValueError, match="noise_seed"):
        pipeline.apply_chain(None, "n030+q80", noise_seed=-1)
    with pytest.raises(ValueError, match="not a step"):
        pipeline.apply_chain(None, [("posterize", 3)])
    assert not touched


def test_stress_labels_with_sharpen_and_chains():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    chain = "r50+shp080+q75"
    got = ensemble.stress_labels([90, 70], noises=[3], sharpens=[150, 50], chains=[chain])
    assert got == ["q90", "q70", "n030", "n030_q90", "n030_q70", "shp050", "shp050_q90", "shp050_q70", "shp150", "shp150_q90", "shp150_q70", chain]
    assert ensemble.stress_labels([80], sharpens=[150]) == ["q80", "shp150", "shp150_q80"]
    assert ensemble.stress_labels([], sharpens=[5], sharpen_sigma=2.5, sharpen_radius=3, sharpen_threshold=4) == ["shp005"]
    assert ensemble.stress_labels([80], chains=["q90+crop95+q75", chain]) == ["q80", "q90+crop95+q75", chain]      # the order given, no _q rows
    full = dict(scales=[50], blurs=[1.0], medians=[3], flips=["h"], crops=[90], rotations=[7.5], gray=True, hues=[30], impulses=[1])
    base = ensemble.stress_labels([80], **full)
    assert ensemble.stress_labels([80], **full, sharpens=(), chains=()) == base                                  # unchanged when both are empty
    assert ensemble.stress_labels([80], **full, sharpens=[150], chains=[chain]) == base + ["shp150", "shp150_q80", chain]


def test_stress_table_with_a_chain_label():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    names = ["b.jpg", "a.jpg", "c.jpg"]
    labels = ["q90", "shp150", "shp150_q90", "q90+crop95+q75", "r50+shp080+q75"]
    s = np.zeros((6, 1, 3), dtype=np.float32)
    s[0] = [[0.9, 0.2, 0.3]]                                  # b 1, a 0, c 0
    s[1] = [[0.9, 0.2, 0.3]]                                  # q90: nothing flips
    s[2] = [[0.9, 0.9, 0.3]]                                  # shp150: a flips
    s[3] = [[0.9, 0.2, 0.3]]
    s[4] = [[0.1, 0.2, 0.3]]                                  # q90+crop95+q75: b flips - a chain that starts with a q step
    s[5] = [[0.9, 0.2, 0.9]]                                  # r50+shp080+q75: c flips
    table, summary = ensemble.stress_table(names, s, labels)
    assert table["filename"] == ["a.jpg", "b.jpg", "c.jpg"] and table["labels"] == labels
    assert table["stable"].tolist() == [False, False, False]                       # the chains count
    assert table["flips"] == ["shp150", "q90+crop95+q75", "r50+shp080+q75"]
    assert table["flips_at"] == [None, None, None]                                 # the plain q rows only
    assert summary["qualities"] == [90] and summary["variants"] == labels and summary["n_stable"] == 0
    assert summary["flips"] == {"q90": 0, "shp150": 1, "shp150_q90": 0, "q90+crop95+q75": 1, "r50+shp080+q75": 1}
    s[1] = [[0.1, 0.2, 0.3]]                                  # now q90 flips b too
    table, _ = ensemble.stress_table(names, s, labels)
    assert table["flips_at"] == [None, 90, None] and table["flips"][1] == "q90;q90+crop95+q75"
    # chains alone
    table, summary = ensemble.stress_table(names, s[[0, 4]], ["q90+crop95+q75"])
    assert table["flips_at"] == [None] * 3 and table["stable"].tolist() == [True, False, True] and summary["qualities"] == []


# ---- CLI refusals: everything is refused before torch is imported ---------------------------------------------------------------------------
REFUSALS = [
    (["--stress-chain", "r50+q80"], "--stress-chain needs --stress-out"),
    (["--stress-chain", "r50+q80", "--stress-out", "S", "--heatmaps", "H"], "--stress-chain and --heatmaps cannot be combined"),
    (["--stress-chain", "r50+q80", "--stress-out", "S", "--shard", "members"], "--stress-chain works with --shard images and --tta 1 only"),
    (["--stress-chain", "r50+q80", "--stress-out", "S", "--shard", "hybrid"], "--stress-chain works with --shard images and --tta 1 only"),
    (["--stress-chain", "r50+q80", "--stress-out", "S", "--tta", "2"], "--stress-chain works with --shard images and --tta 1 only"),
    (["--stress-chain", "r50+q80", "--stress-out", "S", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-chain", "r50+q80", "--stress-out", "S", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--stress-chain", "q80", "--stress-out", "S"], "--stress-jpeg gives"),
    (["--stress-chain", "r50+hue30", "--stress-out", "S"], "chain step 'hue30'"),
    (["--stress-chain", "r400+r200", "--stress-out", "S"], "10..400 %"),
    (["--stress-chain", "r50+q80,r50+q80", "--stress-out", "S"], "listed twice"),
    (["--stress-chain", "r50+q80", "--stress-out", "S", "--stress-crop-origin", "topleft"], "--stress-crop-origin needs --stress-crop"),
    (["--stress-chain", "r50+q80", "--stress-out", "S", "--stress-rotate-fill", "black"], "--stress-rotate-fill needs --stress-rotate"),
    (["--stress-chain", "crop95+q80", "--stress-out", "S", "--stress-resize-filter", "lanczos"], "--stress-resize-filter needs --stress-resize"),
    (["--stress-chain", "r50+q80", "--stress-out", "S", "--stress-blur-radius", "2"], "--stress-blur-radius needs --stress-blur"),
    (["--stress-chain", "r50+b10", "--stress-out", "S", "--stress-blur-radius", "16"], "integer in 1..15"),
    (["--stress-chain", "r50+q80", "--stress-out", "S", "--stress-noise-seed", "3"], "--stress-noise-seed needs"),
    (["--stress-chain", "r50+b10", "--stress-out", "S", "--stress-subsampling", "444"], "--stress-subsampling need"),
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


def test_cli_accepts_the_options_of_a_chains_steps(tmp_path):
    """the option flags go with a chain that holds the step they govern: the run gets past every refusal, to the GPU check or beyond"""
    (tmp_path / "test.csv").write_text("filename\nimg_00000.jpg\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "vip-cup-2022_amd", "main.py"), str(tmp_path / "test.csv"), str(tmp_path / "o.csv"),
                        "--synthetic", "--stress-out", str(tmp_path / "stress.csv"), "--stress-chain",
                        "r50+b10+crop95+rot030+shp150+n030+q75", "--stress-resize-filter", "lanczos", "--stress-blur-radius", "2",
                        "--stress-crop-origin", "topleft", "--stress-rotate-fill", "black", "--stress-sharpen-sigma", "0.8",
                        "--stress-sharpen-radius", "2", "--stress-sharpen-threshold", "3", "--stress-noise-seed", "5",
                        "--stress-subsampling", "444", "--ckpt-cfg", str(tmp_path / "none.json")], capture_output=True, text=True, timeout=300)
    out = r.stderr + r.stdout
    assert r.returncode != 0 and ("no GPU visible" in out or "none.json" in out), out[-600:]
    assert "needs --stress" not in out and "need --stress" not in out and "expected" not in out
