"""GPU: the sharpening stress test - ``vip_sharpen_rgb_u8`` of csrc/blur.hip (``pipeline.sharpen``) against the integer restatement of
tests/_sharpen_ref.py pixel by pixel, ``stress_batch`` rows against the ``pipeline`` calls they stand for, and ``main.py --stress-sharpen``
against plain runs on the files a user would make from the restatement's pixels.  Every comparison is exact: the unsharp mask is integer
arithmetic on the bit-exact Gaussian, and the member passes see the same pixels in the same batch positions."""
import functools
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
from tests import _blur_ref as B  # noqa: E402
from tests import _parity as P  # noqa: E402
from tests import _sharpen_ref as S  # noqa: E402
from tests._jpeg_enc_ref import content, pil_jpeg  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402

SIZES = [(1, 1), (2, 3), (7, 5), (17, 31), (65, 129), (33, 200), (200, 200), (256, 192)]      # (height, width)
# (percent, sigma, radius; None = three sigma, threshold); sigma 5.0 gives R = 15; threshold 255 returns the input
PARAMS = [(50, 1.0, None, 0), (150, 1.0, None, 0), (500, 2.5, None, 0), (100, 5.0, None, 0), (150, 1.0, 1, 3), (1, 0.3, None, 0),
          (200, 1.0, None, 255)]
_WANT = {}


@functools.lru_cache(maxsize=None)
def _images():
    out = [content(31 + k, w, h) for k, (h, w) in enumerate(SIZES)]
    out[4] = B.two_level(4, *SIZES[4])                                                  # 0 / 255: the largest steps, both clamps
    out[5] = np.ascontiguousarray(out[5][..., :1].repeat(3, axis=2))                    # R = G = B
    for px in out:
        px.setflags(write=False)
    return tuple(out)


def _want(i, arg):
    """the restatement's pixels of image i, computed once"""
    key = (i, arg)
    if key not in _WANT:
        want = S.sharpen(_images()[i], *arg)
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


def test_sharpen_equals_the_restatement():
    """sides shorter than the radius (1 x 1 ... 7 x 5 at R = 15), several tiles per row and per column, the row tail, rows at an odd pitch;
    bit-repeatable; the input, the sizes and the pixels outside the images untouched / 0; threshold 255 returns the input"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    imgs = _images()
    for pad in (0, 3):                                    # pad 3: slot rows at an odd pitch
        batch = _batch(imgs, pad)
        before = batch.rgb.clone()
        for arg in PARAMS:
            out, again = pipeline.sharpen(batch, *arg), pipeline.sharpen(batch, *arg)
            torch.cuda.synchronize()
            assert out.rgb.data_ptr() != batch.rgb.data_ptr() and torch.equal(out.rgb, again.rgb), "sharpen is not bit-repeatable"
            got = out.rgb.cpu().numpy()
            assert got.shape == tuple(batch.rgb.shape)
            inside = np.zeros(got.shape[:3], bool)
            for i, im in enumerate(imgs):
                want = _want(i, arg)
                h, w = im.shape[:2]
                bad = int((got[i, :h, :w] != want).any(axis=2).sum())
                assert bad == 0, f"sharpen {arg}: image {i} {SIZES[i]} pad {pad}: {bad} pixels differ from the restatement"
                if arg[3] == 255:
                    assert np.array_equal(got[i, :h, :w], im), (arg, i)
                inside[i, :h, :w] = True
            assert not got[~inside].any(), f"sharpen {arg} pad {pad}: pixels outside an image are not 0"
            assert out.sizes_host == batch.sizes_host and out.sizes.cpu().tolist() == [list(s) for s in batch.sizes_host]
        assert torch.equal(batch.rgb, before), "sharpen changed its input"
    # the cases do what they are there for: both clamps on the 0 / 255 image, a threshold that holds some samples and not others
    assert (_want(4, PARAMS[2]) == 0).any() and (_want(4, PARAMS[2]) == 255).any()
    held = _want(6, PARAMS[4]) == _images()[6]
    assert held.any() and not held.all() and not np.array_equal(_want(6, PARAMS[1]), _images()[6])


def test_guard_bands_and_untouched_slot_padding():
    """the kernel writes the pixels of the images and nothing else: sentinel bytes before, after and between the images stay"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    imgs = _images()
    batch = _batch(imgs, 3)
    maxH, maxW = batch.rgb.shape[1] + 1, batch.rgb.shape[2] + 1                        # a slot pitch one larger than the source's
    body = len(imgs) * maxH * maxW * 3
    arg = (150, 2.5, 8, 2)
    for guard in (4096, 4099):                            # 4099: a destination that is not word-aligned
        buf = torch.full((body + 2 * guard,), 0xAB, dtype=torch.uint8, device="cuda")
        dst = buf[guard:guard + body].view(len(imgs), maxH, maxW, 3)
        pipeline._filter_into(batch, dst, "sharpen", (25, 8, pipeline.sharpen_amount(arg[0]), arg[3]))
        torch.cuda.synchronize()
        flat = buf.cpu().numpy()
        assert (flat[:guard] == 0xAB).all() and (flat[guard + body:] == 0xAB).all(), "written outside the buffer"
        got = flat[guard:guard + body].reshape(len(imgs), maxH, maxW, 3)
        inside = np.zeros(got.shape[:3], bool)
        for i, im in enumerate(imgs):
            h, w = im.shape[:2]
            assert np.array_equal(got[i, :h, :w], _want(i, arg)), (i, guard)
            inside[i, :h, :w] = True
        assert (got[~inside] == 0xAB).all(), "written outside an image"


def _png(px) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, format="PNG")
    return buf.getvalue()


def test_sharpen_then_recompress_decoded_sources():
    """a batch decoded from PNG and JPEG sources of different sizes: sharpen, then recompress == restatement -> Pillow save -> load"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    raws = [_png(content(21, 200, 200)), synth_jpeg(149), _png(content(22, 57, 31)), synth_jpeg(101), _png(content(23, 16, 16)[..., 0])]
    batch = pipeline.decode_images(raws)
    src = batch.rgb.cpu().numpy()
    got = pipeline.recompress(pipeline.sharpen(batch, 150), 70)
    px = got.rgb.cpu().numpy()
    for i, (h, w) in enumerate(batch.sizes_host):
        sharp = S.sharpen(np.ascontiguousarray(src[i, :h, :w]), 150)
        want = np.asarray(Image.open(io.BytesIO(pil_jpeg(sharp, 70, "4:2:0"))).convert("RGB"))
        assert got.sizes_host[i] == (h, w) and np.array_equal(px[i, :h, :w], want), (i, (h, w))
    assert np.array_equal(batch.rgb.cpu().numpy(), src)


# ---- stress_batch -----------------------------------------------------------------------------------------------------------------------
def _write_set(d, n):
    names = []
    for i in P.e2e_image_ids(n):
        name = f"img_{i:05d}.jpg"
        (d / name).write_bytes(synth_jpeg(i))
        names.append(name)
    (d / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
    return names


def test_stress_batch_rows(tmp_path):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, pipeline, zoo
    names = _write_set(tmp_path, 3)
    members = [(zoo.MEMBERS["resnet_rs50"], zoo.FoldMean([P.gpu_member("resnet_rs50")[1]]))]
    raws = [(tmp_path / n).read_bytes() for n in names]
    rows, labels = ensemble.stress_batch(raws, members, [80], sharpens=[150])
    assert labels == ["q80", "shp150", "shp150_q80"] and rows.shape == (4, 1, 3)
    old = ensemble.stress_batch(raws, members, [80])
    assert isinstance(old, torch.Tensor) and torch.equal(rows[:2], old)
    batch = pipeline.decode_images(raws)
    sharp = pipeline.sharpen(batch, 150)
    assert torch.equal(rows[2], ensemble._score_batch(sharp, members))
    assert torch.equal(rows[3], ensemble._score_batch(pipeline.recompress(sharp, 80), members))
    assert not torch.equal(rows[2], rows[0])
    # options of its own, sharpening alone: (rows, labels) as well, percents ascending
    rows, labels = ensemble.stress_batch(raws, members, [], sharpens=[200, 50], sharpen_sigma=2.5, sharpen_radius=2, sharpen_threshold=3)
    assert labels == ["shp050", "shp200"] and rows.shape == (3, 1, 3)
    assert torch.equal(rows[1], ensemble._score_batch(pipeline.sharpen(batch, 50, 2.5, 2, 3), members))
    assert torch.equal(rows[2], ensemble._score_batch(pipeline.sharpen(batch, 200, 2.5, 2, 3), members))
    assert isinstance(ensemble.stress_batch(raws, members, [80], sharpens=(), chains=()), torch.Tensor)


# ---- CLI --------------------------------------------------------------------------------------------------------------------------------
def _two_members(tmp_path, keys=("resnet_rs50", "convnext_tiny_in22k")):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import zoo
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS[k].ckpt_name, [zoo.MEMBERS[k].input_hw] * 2, 0] for k in keys]))
    return ["--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "4"]


def _variant_set(src, dst, names, smooth, quality):
    """the files a user would get by opening every image, sharpening it (``smooth``: pixels -> pixels, None: not at all) and saving it as
    PNG (``quality`` None) or as JPEG at ``quality`` with Pillow; the rows keep the names of the sources"""
    dst.mkdir()
    for name in names:
        px = np.asarray(Image.open(io.BytesIO((src / name).read_bytes())).convert("RGB"))
        if smooth is not None:
            px = smooth(px)
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


def _check_smooth_run(tmp_path, names, args, variants, qorder, extra, report):
    """plain run vs stress run (byte-identical CSVs), then one plain run per variant on the files made from the restatement's pixels
    against the columns; ``variants`` = [(label, smooth, quality)] in the specified order"""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import main as cli
    csv = str(tmp_path / "test.csv")
    cli.main([csv, str(tmp_path / "o0.csv"), "--scores-out", str(tmp_path / "s0.csv"), *extra])
    cli.main([csv, str(tmp_path / "o1.csv"), "--scores-out", str(tmp_path / "s1.csv"), *extra, *args, "--stress-out", str(tmp_path / "stress.csv")])
    assert (tmp_path / "o0.csv").read_bytes() == (tmp_path / "o1.csv").read_bytes()
    assert (tmp_path / "s0.csv").read_bytes() == (tmp_path / "s1.csv").read_bytes()
    table = pd.read_csv(tmp_path / "stress.csv", dtype={"flips_at": str, "flips": str}, keep_default_na=False)
    labels = [v[0] for v in variants]
    assert list(table.columns) == ["filename", "p", "decision"] + [f"p_{v}" for v in labels] + [f"decision_{v}" for v in labels] + \
        ["stable", "flips_at", "flips"]
    assert table.filename.tolist() == sorted(names)
    uniq, p, dec = _plain(tmp_path / "s0.csv", tmp_path / "o0.csv")
    assert np.array_equal(table.p.to_numpy(np.float32), p) and np.array_equal(table.decision.to_numpy(np.float32), dec)
    for label, smooth, q in variants:
        d = tmp_path / label
        _variant_set(tmp_path, d, names, smooth, q)
        cli.main([str(d / "test.csv"), str(d / "o.csv"), "--scores-out", str(d / "s.csv"), *extra])
        uq, pq, dq = _plain(d / "s.csv", d / "o.csv")
        got_p, got_d = table[f"p_{label}"].to_numpy(np.float32), table[f"decision_{label}"].to_numpy(np.float32)
        report(f"[sharpen cli] {label}: max|p - p(files)| {float(np.abs(got_p - pq).max()):.3e}, "
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
    assert info["settings"]["qualities"] == qorder and info["settings"]["subsampling"] == "4:2:0" and "scales" not in info["settings"]
    return table, info


def test_cli_sharpen_and_jpeg_end_to_end(tmp_path, report):
    """--stress-sharpen 150 --stress-jpeg 70: the CSVs of a plain run unchanged, every column == a plain run on the files"""
    names = _write_set(tmp_path, 4)
    sharp = lambda px: S.sharpen(px, 150)   # noqa: E731
    variants = [("q70", None, 70), ("shp150", sharp, None), ("shp150_q70", sharp, 70)]
    _, info = _check_smooth_run(tmp_path, names, ["--stress-sharpen", "150", "--stress-jpeg", "70"], variants, [70], _two_members(tmp_path),
                                report)
    assert info["variants"] == ["q70", "shp150", "shp150_q70"] and len(info["settings"]["members"]) == 2
    s = info["settings"]
    assert s["sharpen_percents"] == [150] and s["sharpen_sigma"] == 1.0 and s["sharpen_radius"] is None and s["sharpen_threshold"] == 0
    assert "chains" not in s and "blur_sigmas" not in s
