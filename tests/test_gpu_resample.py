"""GPU: the resize stress test - csrc/resample.hip (``pipeline.rescale``) against the integer restatement of tests/_resample_ref.py and
against Pillow's ``Image.resize`` directly, pixel by pixel, and ``main.py --stress-resize`` against plain runs on the files Pillow makes.
Every comparison is exact: tables and passes are integer arithmetic, and the member passes see the same pixels in the same batch positions."""
import functools
import io
import json
import os
import subprocess
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
from tests._jpeg_enc_ref import content, pil_jpeg  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402

SIZES = [(1, 1), (2, 3), (7, 5), (17, 31), (65, 129), (33, 200), (200, 200), (256, 192)]      # (height, width)
PERCENTS = [25, 50, 75, 90, 110, 150, 200]
_WANT = {}


@functools.lru_cache(maxsize=None)
def _images():
    out = [content(31 + k, w, h) for k, (h, w) in enumerate(SIZES)]
    out[3] = R.two_level(3, *SIZES[3])                                                  # 0 / 255: overshoot and the clamp
    out[4] = R.two_level(4, *SIZES[4])
    out[5] = np.ascontiguousarray(out[5][..., :1].repeat(3, axis=2))                    # R = G = B
    for px in out:
        px.setflags(write=False)
    return tuple(out)


def _want(i, percent, filter):
    """the restatement's pixels of image i, computed once and checked against Pillow itself"""
    key = (i, percent, filter)
    if key not in _WANT:
        px = _images()[i]
        ho, wo = R.scaled_size(px.shape[0], px.shape[1], percent)
        want = R.resize(px, ho, wo, filter)
        assert np.array_equal(want, R.pil_resize(px, ho, wo, filter)), ("restatement != Pillow", key)
        want.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def _batch(imgs, pad: int = 0):
    """a DecodedBatch holding ``imgs`` in slots of the largest size (+ pad), the rest of every slot filled with noise"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    sizes = [(im.shape[0], im.shape[1]) for im in imgs]
    maxH, maxW = max(h for h, _ in sizes) + pad, max(w for _, w in sizes) + pad
    rgb = np.random.default_rng(5).integers(0, 256, (len(imgs), maxH, maxW, 3), dtype=np.uint8)
    for i, im in enumerate(imgs):
        rgb[i, :im.shape[0], :im.shape[1]] = im
    return pipeline.DecodedBatch(torch.from_numpy(rgb).cuda(), torch.tensor(sizes, dtype=torch.int32, device="cuda"), sizes)


@pytest.mark.parametrize("filter", R.FILTERS)
def test_rescale_equals_restatement_and_pillow(filter):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    imgs = _images()
    for pad in (0, 3):                                    # pad 3: slot rows at an odd pitch
        batch = _batch(imgs, pad)
        before = batch.rgb.clone()
        for percent in PERCENTS:
            out = pipeline.rescale(batch, percent, filter)
            again = pipeline.rescale(batch, percent, filter)
            torch.cuda.synchronize()
            assert out.rgb.data_ptr() != batch.rgb.data_ptr() and torch.equal(out.rgb, again.rgb), "rescale is not bit-repeatable"
            got = out.rgb.cpu().numpy()
            inside = np.zeros(got.shape[:3], bool)
            for i, im in enumerate(imgs):
                want = _want(i, percent, filter)
                ho, wo = want.shape[:2]
                assert out.sizes_host[i] == (ho, wo) == pipeline.scaled_size(im.shape[0], im.shape[1], percent)
                bad = int((got[i, :ho, :wo] != want).any(axis=2).sum())
                assert bad == 0, f"image {i} {SIZES[i]} -> {(ho, wo)} {percent} % {filter} pad {pad}: {bad} pixels differ"
                inside[i, :ho, :wo] = True
            assert out.sizes.cpu().tolist() == [list(s) for s in out.sizes_host]
            assert got.shape[1:3] == (max(s[0] for s in out.sizes_host), max(s[1] for s in out.sizes_host))
            assert not got[~inside].any(), f"{percent} % {filter} pad {pad}: pixels outside an image are not 0"
        assert torch.equal(batch.rgb, before), "rescale changed its input"


@pytest.mark.parametrize("percent,filter", [(10, "lanczos"), (10, "bilinear"), (400, "bicubic")])
def test_rescale_at_the_ends_of_the_range(percent, filter):
    """10 %: a tile's vertical window (16 output rows x 10 + 2 x 30 taps) is taller than what the kernel holds on chip, so it works
    through the tile in groups of rows; sides that shrink to one sample; 400 %: many tiles per image"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    imgs = _images()
    out = pipeline.rescale(_batch(imgs, 3), percent, filter)
    got = out.rgb.cpu().numpy()
    inside = np.zeros(got.shape[:3], bool)
    for i in range(len(imgs)):
        want = _want(i, percent, filter)
        ho, wo = want.shape[:2]
        assert out.sizes_host[i] == (ho, wo) and np.array_equal(got[i, :ho, :wo], want), (i, SIZES[i], (ho, wo))
        inside[i, :ho, :wo] = True
    assert not got[~inside].any()


@pytest.mark.parametrize("percent,filter", [(50, "bicubic"), (25, "lanczos"), (150, "bilinear")])
def test_guard_bands_and_untouched_slot_padding(percent, filter):
    """the kernel writes the pixels of the images and nothing else: sentinel bytes before, after and between the images stay"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    imgs = _images()
    batch = _batch(imgs, 3)
    new_sizes = [pipeline.scaled_size(h, w, percent) for h, w in batch.sizes_host]
    maxHo, maxWo = max(h for h, _ in new_sizes) + 1, max(w for _, w in new_sizes) + 1
    body = len(imgs) * maxHo * maxWo * 3
    for guard in (4096, 4099):                            # 4099: a destination that is not word-aligned
        buf = torch.full((body + 2 * guard,), 0xAB, dtype=torch.uint8, device="cuda")
        dst = buf[guard:guard + body].view(len(imgs), maxHo, maxWo, 3)
        pipeline._resample_into(batch, new_sizes, filter, dst)
        torch.cuda.synchronize()
        flat = buf.cpu().numpy()
        assert (flat[:guard] == 0xAB).all() and (flat[guard + body:] == 0xAB).all(), "written outside the buffer"
        got = flat[guard:guard + body].reshape(len(imgs), maxHo, maxWo, 3)
        inside = np.zeros(got.shape[:3], bool)
        for i, (ho, wo) in enumerate(new_sizes):
            assert np.array_equal(got[i, :ho, :wo], _want(i, percent, filter)), (i, guard)
            inside[i, :ho, :wo] = True
        assert (got[~inside] == 0xAB).all(), "written outside an image"


def _png(px) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, format="PNG")
    return buf.getvalue()


def test_rescale_then_recompress_decoded_sources():
    """a batch decoded from PNG and JPEG sources of different sizes: rescale, then recompress == Pillow resize -> save -> load"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    raws = [_png(content(21, 200, 200)), synth_jpeg(149), _png(content(22, 57, 31)), synth_jpeg(101), _png(content(23, 16, 16)[..., 0])]
    batch = pipeline.decode_images(raws)
    src = batch.rgb.cpu().numpy()
    for percent, filter in ((50, "bicubic"), (150, "lanczos"), (75, "bilinear")):
        got = pipeline.recompress(pipeline.rescale(batch, percent, filter), 70)
        px = got.rgb.cpu().numpy()
        for i, (h, w) in enumerate(batch.sizes_host):
            ho, wo = R.scaled_size(h, w, percent)
            small = R.pil_resize(np.ascontiguousarray(src[i, :h, :w]), ho, wo, filter)
            want = np.asarray(Image.open(io.BytesIO(pil_jpeg(small, 70, "4:2:0"))).convert("RGB"))
            assert got.sizes_host[i] == (ho, wo) and np.array_equal(px[i, :ho, :wo], want), (i, (h, w), percent, filter)
    assert np.array_equal(batch.rgb.cpu().numpy(), src)


def test_rescale_100_and_bad_arguments(monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    imgs = _images()
    batch = _batch(imgs, 3)
    before = batch.rgb.clone()
    out = pipeline.rescale(batch, 100, "lanczos")
    assert out.sizes_host == batch.sizes_host and out.rgb.data_ptr() != batch.rgb.data_ptr()
    got = out.rgb.cpu().numpy()
    for i, im in enumerate(imgs):
        assert np.array_equal(got[i, :im.shape[0], :im.shape[1]], im), i
    launches = []
    monkeypatch.setattr(pipeline, "_launch", lambda *a, **k: launches.append(a))
    for percent in (9, 401, 50.0, "50", None):
        with pytest.raises(ValueError, match="10..400"):
            pipeline.rescale(batch, percent)
    with pytest.raises(ValueError, match="bilinear, bicubic, lanczos"):
        pipeline.rescale(batch, 50, "nearest")
    monkeypatch.setattr(pipeline, "MAX_JPEG_PIXELS", 200 * 200)
    with pytest.raises(_abi.VipError, match="VIP_MAX_JPEG_PIXELS"):
        pipeline.rescale(batch, 150)
    assert not launches and torch.equal(batch.rgb, before)


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------
def _write_set(d, n):
    names = []
    for i in P.e2e_image_ids(n):
        name = f"img_{i:05d}.jpg"
        (d / name).write_bytes(synth_jpeg(i))
        names.append(name)
    (d / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
    return names


def _two_members(tmp_path, keys=("resnet_rs50", "convnext_tiny_in22k")):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import zoo
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS[k].ckpt_name, [zoo.MEMBERS[k].input_hw] * 2, 0] for k in keys]))
    return ["--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "4"]


def _variant_set(src, dst, names, percent, quality, filter):
    """the files a user would get by opening every image, resizing it to ``percent`` % (None: not at all) and saving it as PNG
    (``quality`` None: the pixels as they are) or as JPEG at ``quality`` - Pillow all the way; the rows keep the names of the sources"""
    dst.mkdir()
    for name in names:
        px = np.asarray(Image.open(io.BytesIO((src / name).read_bytes())).convert("RGB"))
        if percent is not None:
            ho, wo = R.scaled_size(px.shape[0], px.shape[1], percent)
            px = R.pil_resize(px, ho, wo, filter)
        (dst / name).write_bytes(_png(px) if quality is None else pil_jpeg(px, quality, "4:2:0"))
    (dst / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")


def _plain(scores_csv, out_csv):
    import pandas as pd
    from vipcup_amd import ensemble
    s = pd.read_csv(scores_csv)
    members = [c for c in s.columns if c not in ("filename", "ensemble_mean")]
    uniq, p, dec = ensemble.aggregate(s.filename.tolist(), np.stack([s[m].to_numpy(np.float32) for m in members]))
    o = pd.read_csv(out_csv)
    assert o.filename.tolist() == uniq and np.array_equal(o.logit.to_numpy(np.float32), dec)
    return uniq, p, dec


def _check_resize_run(tmp_path, names, percents, qs, extra, filter="bicubic", report=None):
    """plain run vs stress run (byte-identical CSVs), then one plain run per variant on the files Pillow makes against the columns"""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import main as cli
    csv = str(tmp_path / "test.csv")
    cli.main([csv, str(tmp_path / "o0.csv"), "--scores-out", str(tmp_path / "s0.csv"), *extra])
    args = ["--stress-resize", ",".join(str(v) for v in percents), "--stress-out", str(tmp_path / "stress.csv")]
    if qs:
        args += ["--stress-jpeg", ",".join(str(q) for q in qs)]
    if filter != "bicubic":
        args += ["--stress-resize-filter", filter]
    cli.main([csv, str(tmp_path / "o1.csv"), "--scores-out", str(tmp_path / "s1.csv"), *extra, *args])
    assert (tmp_path / "o0.csv").read_bytes() == (tmp_path / "o1.csv").read_bytes()
    assert (tmp_path / "s0.csv").read_bytes() == (tmp_path / "s1.csv").read_bytes()
    table = pd.read_csv(tmp_path / "stress.csv", dtype={"flips_at": str, "flips": str}, keep_default_na=False)
    qorder = sorted(set(qs), reverse=True)
    porder = sorted({v for v in percents if v != 100}, reverse=True)
    variants = [(f"q{q}", None, q) for q in qorder]
    for pc in porder:
        variants += [(f"r{pc}", pc, None)] + [(f"r{pc}_q{q}", pc, q) for q in qorder]
    labels = [v[0] for v in variants]
    assert list(table.columns) == ["filename", "p", "decision"] + [f"p_{v}" for v in labels] + [f"decision_{v}" for v in labels] + \
        ["stable", "flips_at", "flips"]
    assert table.filename.tolist() == sorted(names)
    uniq, p, dec = _plain(tmp_path / "s0.csv", tmp_path / "o0.csv")
    assert np.array_equal(table.p.to_numpy(np.float32), p) and np.array_equal(table.decision.to_numpy(np.float32), dec)
    for label, pc, q in variants:
        d = tmp_path / label
        _variant_set(tmp_path, d, names, pc, q, filter)
        cli.main([str(d / "test.csv"), str(d / "o.csv"), "--scores-out", str(d / "s.csv"), *extra])
        uq, pq, dq = _plain(d / "s.csv", d / "o.csv")
        got_p, got_d = table[f"p_{label}"].to_numpy(np.float32), table[f"decision_{label}"].to_numpy(np.float32)
        if report is not None:
            report(f"[resize cli] {label} {filter}: max|p - p(Pillow's files)| {float(np.abs(got_p - pq).max()):.3e}, "
                   f"mean|p - p0| {float(np.abs(got_p - p).mean()):.3e}, flips {int((got_d != dec).sum())}/{len(uniq)}")
        assert uq == uniq and np.array_equal(got_p, pq), (label, np.abs(got_p - pq).max())
        assert np.array_equal(got_d, dq), label
    # the table's own columns and the JSON next to it
    dv = np.stack([table[f"decision_{v}"].to_numpy(np.float32) for v in labels], axis=1)
    differs = dv != dec[:, None]
    assert table.stable.tolist() == [int(not r.any()) for r in differs]
    assert table.flips.tolist() == [";".join(v for v, f in zip(labels, r) if f) for r in differs]
    assert table.flips_at.tolist() == ["" if not r[:len(qorder)].any() else str(max(q for q, f in zip(qorder, r) if f)) for r in differs]
    info = json.loads((tmp_path / "stress.json").read_text())
    assert info["variants"] == labels and info["qualities"] == qorder
    assert info["n_files"] == len(uniq) and info["n_stable"] == int(table.stable.sum())
    assert list(info["flips"]) == labels and list(info["flip_rate"]) == labels and list(info["mean_abs_dp"]) == labels
    for k, v in enumerate(labels):
        assert info["flips"][v] == int(differs[:, k].sum())
        assert info["flip_rate"][v] == pytest.approx(differs[:, k].mean(), abs=1e-12)
        want = np.abs(table[f"p_{v}"].to_numpy(np.float32).astype(np.float64) - p.astype(np.float64)).mean()
        assert info["mean_abs_dp"][v] == pytest.approx(want, rel=1e-9, abs=1e-12)
    assert info["settings"]["scales"] == porder and info["settings"]["resize_filter"] == filter
    assert info["settings"]["qualities"] == qorder and info["settings"]["subsampling"] == "4:2:0"
    return table, info


def test_cli_resize_and_jpeg_grid_end_to_end(tmp_path, report):
    """--stress-resize 150,50 --stress-jpeg 70: the CSVs of a plain run unchanged, every column == a plain run on Pillow's files"""
    names = _write_set(tmp_path, 4)
    _, info = _check_resize_run(tmp_path, names, [50, 150], [70], _two_members(tmp_path), report=report)
    assert info["variants"] == ["q70", "r150", "r150_q70", "r50", "r50_q70"] and len(info["settings"]["members"]) == 2


def test_cli_resize_only(tmp_path, report):
    """without --stress-jpeg: no q columns, flips_at empty; duplicates and 100 dropped, another filter"""
    names = _write_set(tmp_path, 3)
    table, info = _check_resize_run(tmp_path, names, [50, 100, 50], [], _two_members(tmp_path, ("resnet_rs50",)), filter="lanczos",
                                    report=report)
    assert list(table.columns) == ["filename", "p", "decision", "p_r50", "decision_r50", "stable", "flips_at", "flips"]
    assert table.flips_at.tolist() == [""] * len(names) and info["qualities"] == [] and info["variants"] == ["r50"]


def test_cli_jpeg_only_output_is_unchanged(tmp_path):
    """--stress-jpeg alone: ``stress_batch`` with no scales is the earlier call, and the files keep the earlier layout, byte for byte"""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, main as cli, pipeline, zoo
    names = _write_set(tmp_path, 3)
    extra = _two_members(tmp_path, ("resnet_rs50",))
    for k in (0, 1):
        cli.main([str(tmp_path / "test.csv"), str(tmp_path / f"o{k}.csv"), *extra, "--stress-jpeg", "60,80", "--stress-out",
                  str(tmp_path / f"st{k}.csv")])
    assert (tmp_path / "st0.csv").read_bytes() == (tmp_path / "st1.csv").read_bytes()
    assert (tmp_path / "st0.json").read_bytes() == (tmp_path / "st1.json").read_bytes()
    table = pd.read_csv(tmp_path / "st0.csv", dtype={"flips_at": str}, keep_default_na=False)
    assert list(table.columns) == ["filename", "p", "decision", "p_q80", "p_q60", "decision_q80", "decision_q60", "stable", "flips_at"]
    info = json.loads((tmp_path / "st0.json").read_text())
    assert list(info) == ["n_files", "threshold", "qualities", "n_stable", "flips", "flip_rate", "mean_abs_dp", "settings"]
    assert list(info["flips"]) == ["80", "60"] and info["qualities"] == [80, 60]
    assert list(info["settings"]) == ["qualities", "subsampling", "threshold", "precision", "batch_size", "n_images", "members"]
    # the files are what the earlier code path writes from the same rows: the table of the quality list, column by column
    members = [(zoo.MEMBERS["resnet_rs50"], zoo.FoldMean([P.gpu_member("resnet_rs50")[1]]))]
    raws = [(tmp_path / n).read_bytes() for n in names]
    rows = ensemble.stress_batch(raws, members, [80, 60], "4:2:0", scales=())
    assert isinstance(rows, torch.Tensor) and rows.shape == (3, 1, 3)
    batch = pipeline.decode_images(raws)
    assert torch.equal(rows[0], ensemble._score_batch(raws, members))
    assert torch.equal(rows[1], ensemble._score_batch(pipeline.recompress(batch, 80), members))
    assert torch.equal(rows[2], ensemble._score_batch(pipeline.recompress(batch, 60), members))
    both, labels = ensemble.stress_batch(raws, members, [80, 60], "4:2:0", scales=[50])
    assert labels == ["q80", "q60", "r50", "r50_q80", "r50_q60"] and torch.equal(both[:3], rows)
    assert torch.equal(both[3], ensemble._score_batch(pipeline.rescale(batch, 50), members))
    assert torch.equal(both[5], ensemble._score_batch(pipeline.recompress(pipeline.rescale(batch, 50), 60), members))


REFUSALS = [
    (["--stress-resize", "50", "--stress-out", "S", "--tta", "2"], "--stress-resize works with --shard images and --tta 1 only"),
    (["--stress-resize", "50", "--stress-out", "S", "--shard", "members"], "--stress-resize works with --shard images and --tta 1 only"),
    (["--stress-resize", "50", "--stress-out", "S", "--heatmaps", "H"], "--stress-resize and --heatmaps cannot be combined"),
    (["--stress-resize", "50"], "--stress-resize needs --stress-out"),
    (["--stress-resize", "50,5", "--stress-out", "S"], "integer percents in 10..400"),
]


@pytest.mark.parametrize("extra,message", REFUSALS, ids=lambda v: "".join(v) if isinstance(v, list) else None)
def test_cli_refuses_before_scoring(tmp_path, extra, message):
    _write_set(tmp_path, 2)
    extra = [str(tmp_path / "stress.csv") if t == "S" else str(tmp_path / "hm") if t == "H" else t for t in extra]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "vip-cup-2022_amd", "main.py"), str(tmp_path / "test.csv"), str(tmp_path / "o.csv"),
                        "--synthetic", *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and message in (r.stderr + r.stdout), r.stderr[-400:]
    assert not (tmp_path / "o.csv").exists() and not (tmp_path / "stress.csv").exists() and "MODEL(" not in r.stdout
