"""GPU: stress chains - ``stress_batch(chains=...)`` / ``pipeline.apply_chain`` against the rows that exist already (the chain ``X+q80`` IS
the row ``X_q80``), against the ``pipeline`` calls applied by hand, and ``main.py --stress-chain`` against plain runs on the files a user
would make on the CPU from the restatements, step by step.  Every comparison is exact: every step is integer arithmetic held to its own
reference elsewhere, and the member passes see the same pixels in the same batch positions."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _parity as P  # noqa: E402
from tests import _resample_ref as R  # noqa: E402
from tests import _sharpen_ref as S  # noqa: E402
from tests import _warp_ref as W  # noqa: E402
from tests._jpeg_enc_ref import pil_jpeg  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402

SEED = 5


def _write_set(d, n):
    names = []
    for i in P.e2e_image_ids(n):
        name = f"img_{i:05d}.jpg"
        (d / name).write_bytes(synth_jpeg(i))
        names.append(name)
    (d / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
    return names


def _one_member():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import zoo
    return [(zoo.MEMBERS["resnet_rs50"], zoo.FoldMean([P.gpu_member("resnet_rs50")[1]]))]


def test_a_chain_of_one_step_and_a_resave_is_the_existing_row(tmp_path):
    """every step kind's wiring, the noise keys, the noise seed and the contrast mean, pinned against rows held to their own references"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, pipeline
    names = _write_set(tmp_path, 3)
    members = _one_member()
    raws = [(tmp_path / n).read_bytes() for n in names]
    steps = ["r50", "b10", "m3", "fliph", "crop90", "rot075", "gray", "con150", "n030", "imp010", "shp150"]
    chains = [f"{x}+q80" for x in steps]
    rows, labels = ensemble.stress_batch(raws, members, [80], scales=[50], blurs=[1.0], medians=[3], flips=["h"], crops=[90], rotations=[7.5],
                                         gray=True, contrasts=[150], noises=[3], impulses=[1], noise_seed=SEED,
                                         noise_keys=pipeline.noise_keys(names), sharpens=[150], chains=chains)
    assert labels == ["q80"] + [v for x in steps for v in (x, f"{x}_q80")] + chains and rows.shape == (1 + len(labels), 1, 3)
    for x, chain in zip(steps, chains):
        a, b = rows[1 + labels.index(f"{x}_q80")], rows[1 + labels.index(chain)]
        assert torch.equal(a, b), (chain, (a - b).abs().max().item())
        assert not torch.equal(b, rows[0]), chain
    # the rows in front of the chains are those of the call without them
    old, old_labels = ensemble.stress_batch(raws, members, [80], scales=[50], sharpens=[150])
    assert old_labels == ["q80", "r50", "r50_q80", "shp150", "shp150_q80"]
    assert torch.equal(old[:4], rows[:4]) and torch.equal(old[4:], rows[1 + labels.index("shp150"):3 + labels.index("shp150")])


def test_chains_equal_the_pipeline_calls_applied_by_hand(tmp_path):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, pipeline
    names = _write_set(tmp_path, 3)
    members = _one_member()
    raws = [(tmp_path / n).read_bytes() for n in names]
    keys = pipeline.noise_keys(names)
    chains = ["r50+shp080+crop95+q75", "q90+crop95+q75", "n030+r50+n030"]
    rows, labels = ensemble.stress_batch(raws, members, [], subsampling="4:4:4", resize_filter="lanczos", crop_origin="topleft",
                                         sharpen_sigma=0.8, sharpen_radius=2, sharpen_threshold=2, noise_seed=SEED, noise_keys=keys,
                                         chains=chains)
    assert labels == chains and rows.shape == (4, 1, 3)
    batch = pipeline.decode_images(raws)
    by_hand = [
        pipeline.recompress(pipeline.crop(pipeline.sharpen(pipeline.rescale(batch, 50, "lanczos"), 80, 0.8, 2, 2), 95, "topleft"), 75, "4:4:4"),
        pipeline.recompress(pipeline.crop(pipeline.recompress(batch, 90, "4:4:4"), 95, "topleft"), 75, "4:4:4"),
        pipeline.gaussian_noise(pipeline.rescale(pipeline.gaussian_noise(batch, 3.0, SEED, keys), 50, "lanczos"), 3.0, SEED + 1, keys),
    ]
    for k, (chain, want) in enumerate(zip(chains, by_hand)):
        assert torch.equal(rows[1 + k], ensemble._score_batch(want, members)), chain
        assert not torch.equal(rows[1 + k], rows[0]), chain
    assert torch.equal(rows[0], ensemble._score_batch(batch, members))
    # the pixels of the noise chain: the second noise step draws from seed + 1 on the resized batch, not from the first step's field
    options = dict(subsampling="4:4:4", resize_filter="lanczos", blur_radius=None, crop_origin="topleft", rotate_fill="crop", sharpen_sigma=0.8,
                   sharpen_radius=2, sharpen_threshold=2, noise_seed=SEED, noise_keys=keys)
    got = pipeline.apply_chain(batch, pipeline.parse_chain(chains[2]), **options)
    small = pipeline.rescale(pipeline.gaussian_noise(batch, 3.0, SEED, keys), 50, "lanczos")
    assert got.sizes_host == small.sizes_host and torch.equal(got.rgb, pipeline.gaussian_noise(small, 3.0, SEED + 1, keys).rgb)
    assert not torch.equal(got.rgb, pipeline.gaussian_noise(small, 3.0, SEED, keys).rgb)
    for chain, want in zip(chains[:2], by_hand[:2]):
        got = pipeline.apply_chain(batch, chain, **options)               # the chain's text works too
        assert got.sizes_host == want.sizes_host and torch.equal(got.rgb, want.rgb), chain


# ---- CLI --------------------------------------------------------------------------------------------------------------------------------
def _two_members(tmp_path, keys=("resnet_rs50", "convnext_tiny_in22k")):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import zoo
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS[k].ckpt_name, [zoo.MEMBERS[k].input_hw] * 2, 0] for k in keys]))
    return ["--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "4"]


def _load(raw: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))


def _resized(px, percent, filter):
    return R.resize(px, *R.scaled_size(px.shape[0], px.shape[1], percent), filter)


def _cropped(px, percent, origin):
    y0, x0, hh, ww = W.crop_box(px.shape[0], px.shape[1], percent, origin)
    return W.warp(px, W.quantise(*W.crop_xf(y0, x0)), hh, ww, "black")


def _downscale_sharpen_resave(px):
    """r50+shp150+q75 on the CPU, in that order of steps: the file a messenger would hand on"""
    return pil_jpeg(S.sharpen(_resized(px, 50, "bicubic"), 150), 75, "4:2:0")


def _double_compression(px):
    """q90+crop95+q75 with the crop at the top left: a second JPEG of a re-saved, cropped image"""
    return pil_jpeg(_cropped(_load(pil_jpeg(px, 90, "4:2:0")), 95, "topleft"), 75, "4:2:0")


def _plain(scores_csv, out_csv):
    import pandas as pd
    from vipcup_amd import ensemble
    s = pd.read_csv(scores_csv)
    members = [c for c in s.columns if c not in ("filename", "ensemble_mean")]
    uniq, p, dec = ensemble.aggregate(s.filename.tolist(), np.stack([s[m].to_numpy(np.float32) for m in members]))
    o = pd.read_csv(out_csv)
    assert o.filename.tolist() == uniq and np.array_equal(o.logit.to_numpy(np.float32), dec)
    return uniq, p, dec


def test_cli_chains_end_to_end(tmp_path, report):
    """--stress-chain r50+shp150+q75,q90+crop95+q75: the CSVs of a plain run unchanged, every chain column == a plain run on the files
    made on the CPU step by step; the chains count for stable and flips, not for flips_at"""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import main as cli
    names = _write_set(tmp_path, 4)
    extra = _two_members(tmp_path)
    chains = [("r50+shp150+q75", _downscale_sharpen_resave), ("q90+crop95+q75", _double_compression)]
    labels = [c for c, _ in chains]
    csv = str(tmp_path / "test.csv")
    cli.main([csv, str(tmp_path / "o0.csv"), "--scores-out", str(tmp_path / "s0.csv"), *extra])
    cli.main([csv, str(tmp_path / "o1.csv"), "--scores-out", str(tmp_path / "s1.csv"), *extra, "--stress-chain", ",".join(labels),
              "--stress-resize-filter", "bicubic", "--stress-crop-origin", "topleft", "--stress-out", str(tmp_path / "stress.csv")])
    assert (tmp_path / "o0.csv").read_bytes() == (tmp_path / "o1.csv").read_bytes()
    assert (tmp_path / "s0.csv").read_bytes() == (tmp_path / "s1.csv").read_bytes()
    table = pd.read_csv(tmp_path / "stress.csv", dtype={"flips_at": str, "flips": str}, keep_default_na=False)
    assert list(table.columns) == ["filename", "p", "decision"] + [f"p_{v}" for v in labels] + [f"decision_{v}" for v in labels] + \
        ["stable", "flips_at", "flips"]
    assert table.filename.tolist() == sorted(names)
    uniq, p, dec = _plain(tmp_path / "s0.csv", tmp_path / "o0.csv")
    assert np.array_equal(table.p.to_numpy(np.float32), p) and np.array_equal(table.decision.to_numpy(np.float32), dec)
    for k, (label, make) in enumerate(chains):
        d = tmp_path / f"chain{k}"
        d.mkdir()
        for name in names:
            (d / name).write_bytes(make(_load((tmp_path / name).read_bytes())))
        (d / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
        cli.main([str(d / "test.csv"), str(d / "o.csv"), "--scores-out", str(d / "s.csv"), *extra])
        uq, pq, dq = _plain(d / "s.csv", d / "o.csv")
        got_p, got_d = table[f"p_{label}"].to_numpy(np.float32), table[f"decision_{label}"].to_numpy(np.float32)
        report(f"[chain cli] {label}: max|p - p(files)| {float(np.abs(got_p - pq).max()):.3e}, "
               f"mean|p - p0| {float(np.abs(got_p - p).mean()):.3e}, flips {int((got_d != dec).sum())}/{len(uniq)}")
        assert uq == uniq and np.array_equal(got_p, pq), (label, np.abs(got_p - pq).max())
        assert np.array_equal(got_d, dq), label
    dv = np.stack([table[f"decision_{v}"].to_numpy(np.float32) for v in labels], axis=1)
    differs = dv != dec[:, None]
    assert table.stable.tolist() == [int(not r.any()) for r in differs]
    assert table.flips.tolist() == [";".join(v for v, f in zip(labels, r) if f) for r in differs]
    assert table.flips_at.tolist() == [""] * len(uniq)                     # no plain q row: the chains never count here
    info = json.loads((tmp_path / "stress.json").read_text())
    assert info["variants"] == labels and info["qualities"] == [] and info["n_stable"] == int(table.stable.sum())
    assert list(info["flips"]) == labels and [info["flips"][v] for v in labels] == [int(differs[:, k].sum()) for k in range(len(labels))]
    s = info["settings"]
    assert s["chains"] == labels and s["qualities"] == [] and s["subsampling"] == "4:2:0" and len(s["members"]) == 2
    assert s["resize_filter"] == "bicubic" and s["crop_origin"] == "topleft"
    assert s["sharpen_percents"] == [] and s["sharpen_sigma"] == 1.0 and s["sharpen_radius"] is None and s["sharpen_threshold"] == 0


def test_cli_every_family_end_to_end(tmp_path):
    """one value of every stress flag, every option off its default and two chains in ONE run, two batches: the CSVs of a plain run
    unchanged, the table's columns and the settings, and every column == ``stress_batch`` called with the same keywords on each batch"""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, pipeline, zoo
    from vipcup_amd import main as cli
    names = [f"img_{i:05d}.jpg" for i in range(100, 104)]                  # 200 x 200 each
    for i, name in zip(range(100, 104), names):
        (tmp_path / name).write_bytes(synth_jpeg(i))
    (tmp_path / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS["resnet_rs50"].ckpt_name, [zoo.MEMBERS["resnet_rs50"].input_hw] * 2, 0]]))
    extra = ["--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "2", "--precision", "fast"]
    chains = ["n030+q75", "r50+con120+q75"]
    csv = str(tmp_path / "test.csv")
    cli.main([csv, str(tmp_path / "o0.csv"), "--scores-out", str(tmp_path / "s0.csv"), *extra])
    cli.main([csv, str(tmp_path / "o1.csv"), "--scores-out", str(tmp_path / "s1.csv"), *extra, "--stress-out", str(tmp_path / "stress.csv"),
              "--stress-jpeg", "80", "--stress-subsampling", "444", "--stress-resize", "50", "--stress-resize-filter", "lanczos",
              "--stress-blur", "1", "--stress-blur-radius", "2", "--stress-median", "3", "--stress-flip", "h", "--stress-crop", "90",
              "--stress-crop-origin", "topleft", "--stress-rotate", "7.5", "--stress-rotate-fill", "black", "--stress-gray", "--stress-bgr",
              "--stress-hue", "30", "--stress-saturation", "50", "--stress-contrast", "150", "--stress-brightness=-10", "--stress-gamma", "0.8",
              "--stress-noise", "3", "--stress-noise-mono", "3", "--stress-speckle", "20", "--stress-impulse", "1", "--stress-noise-seed", "9",
              "--stress-sharpen", "150", "--stress-sharpen-sigma", "0.8", "--stress-sharpen-radius", "2", "--stress-sharpen-threshold", "3",
              "--stress-autocontrast", "2", "--stress-autocontrast-luma", "1", "--stress-equalize", "--stress-clahe", "2",
              "--stress-clahe-grid", "4", "--stress-chain", ",".join(chains)])
    assert (tmp_path / "o0.csv").read_bytes() == (tmp_path / "o1.csv").read_bytes()
    assert (tmp_path / "s0.csv").read_bytes() == (tmp_path / "s1.csv").read_bytes()
    labels = ["q80", "r50", "r50_q80", "b10", "b10_q80", "m3", "m3_q80", "fliph", "fliph_q80", "crop90", "crop90_q80", "rot075", "rot075_q80",
              "gray", "gray_q80", "bgr", "bgr_q80", "hue030", "hue030_q80", "sat050", "sat050_q80", "con150", "con150_q80", "brim10", "brim10_q80",
              "gam080", "gam080_q80", "n030", "n030_q80", "nm030", "nm030_q80", "spk20", "spk20_q80", "imp010", "imp010_q80", "shp150",
              "shp150_q80", "ac02", "ac02_q80", "acl01", "acl01_q80", "eq", "eq_q80", "clahe20", "clahe20_q80", "n030+q75", "r50+con120+q75"]
    table = pd.read_csv(tmp_path / "stress.csv", dtype={"flips_at": str, "flips": str}, keep_default_na=False)
    assert list(table.columns) == ["filename", "p", "decision"] + [f"p_{v}" for v in labels] + [f"decision_{v}" for v in labels] + \
        ["stable", "flips_at", "flips"]
    assert table.filename.tolist() == names
    info = json.loads((tmp_path / "stress.json").read_text())
    assert info["variants"] == labels
    assert info["settings"] == {
        "qualities": [80], "subsampling": "4:4:4", "threshold": 0.487, "precision": "fast", "batch_size": 2, "n_images": 4,
        "members": ["resnet_rs50"], "scales": [50], "resize_filter": "lanczos", "blur_sigmas": [1.0], "blur_radius": 2, "medians": [3],
        "flips": ["h"], "crops": [90], "crop_origin": "topleft", "rotations": [7.5], "rotate_fill": "black", "gray": True, "bgr": True,
        "hues": [30], "saturations": [50], "contrasts": [150], "brightnesses": [-10], "gammas": [0.8], "noise_sigmas": [3.0],
        "noise_mono_sigmas": [3.0], "speckles": [20], "impulses": [1.0], "noise_seed": 9, "sharpen_percents": [150], "sharpen_sigma": 0.8,
        "sharpen_radius": 2, "sharpen_threshold": 3, "autocontrast_cutoffs": [2], "autocontrast_luma_cutoffs": [1], "equalize": True,
        "clahe_limits": [2.0], "clahe_grid": 4, "chains": chains}
    keywords = dict(subsampling="4:4:4", scales=[50], resize_filter="lanczos", blurs=[1.0], blur_radius=2, medians=[3], flips=["h"], crops=[90],
                    crop_origin="topleft", rotations=[7.5], rotate_fill="black", gray=True, bgr=True, hues=[30], saturations=[50],
                    contrasts=[150], brightnesses=[-10], gammas=[0.8], noises=[3.0], mono_noises=[3.0], speckles=[20], impulses=[1.0],
                    noise_seed=9, sharpens=[150], sharpen_sigma=0.8, sharpen_radius=2, sharpen_threshold=3, autocontrasts=[2],
                    autocontrast_lumas=[1], equalize=True, clahes=[2.0], clahe_grid=4, chains=chains)
    members = _one_member()
    for b0 in (0, 2):                                                      # the second batch: noise keys by file, not by batch position
        batch = names[b0:b0 + 2]
        rows, got = ensemble.stress_batch([(tmp_path / n).read_bytes() for n in batch], members, [80], noise_keys=pipeline.noise_keys(batch),
                                          **keywords)
        assert got == labels
        rows = rows.cpu().numpy()
        assert np.array_equal(table.p.to_numpy(np.float32)[b0:b0 + 2], ensemble.aggregate(batch, rows[0])[1])
        for k, v in enumerate(labels):
            want = ensemble.aggregate(batch, rows[1 + k])[1]
            assert np.array_equal(table[f"p_{v}"].to_numpy(np.float32)[b0:b0 + 2], want), (v, b0)
