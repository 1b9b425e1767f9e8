"""GPU: lossy WebP input behind the ``lossy_webp`` switch - host token decode, device reconstruction (csrc/vp8_host.cpp,
csrc/vp8_pipeline.hip) - bit-exact against Pillow / libwebp over the whole corpus of tests/_vp8.py (Pillow's encoder, the
committed fixtures, hand-written key frames), in a mixed batch with JPEG, PNG and lossless WebP, in a batch of 256, and
against the lossless path on the same pixels through resize, two members and the CLI."""
import io

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from tests import _png  # noqa: E402
from tests import _vp8 as V  # noqa: E402
from tests import _webp as W  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402


def _check_batch(batch, expected, names):
    rgb = batch.rgb.cpu().numpy()
    for i, want in enumerate(expected):
        h, w = batch.sizes_host[i]
        assert (h, w) == want.shape[:2], names[i]
        got = rgb[i, :h, :w]
        assert np.array_equal(got, want), f"image {names[i]}: {int((got != want).any(-1).sum())} of {h * w} pixels differ"
        assert not rgb[i, h:].any() and not rgb[i, :, w:].any(), f"image {names[i]}: padding not zero"


def test_decode_corpus_bit_exact(report):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    corp = V.corpus(1)
    raws, names = [r for _, r in corp], [n for n, _ in corp]
    # 200 x 200 and below in one batch, the large files in one of their own (the batch's slots take the largest size)
    for part in ([i for i, r in enumerate(raws) if len(V.pillow_rgb(r)) <= 200], [i for i, r in enumerate(raws) if len(V.pillow_rgb(r)) > 200]):
        batch = pipeline.decode_images([raws[i] for i in part], lossy_webp=True)
        torch.cuda.synchronize()
        _check_batch(batch, [V.pillow_rgb(raws[i]) for i in part], [names[i] for i in part])
    report(f"[vp8] decode_images(lossy_webp=True): {len(raws)} lossy WebPs ({sum(n.startswith('fx_') for n in names)} fixtures, "
           f"{sum(n.startswith('hw_') for n in names)} hand-written, the rest Pillow's encoder over {len(V.KINDS)} kinds x 4 qualities x 3 "
           f"methods; 1x1 .. 304x400) bit-exact vs Pillow, padding zero")


def test_mixed_batch_of_four_formats():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    jpegs = [synth_jpeg(i) for i in (0, 1, 2)]
    pngs = _png.corpus(seed=2, sizes=[(17, 13), (65, 7)])[::11][:3]
    webps = W.corpus(2, [(17, 13), (200, 200), (65, 7)])[::13][:4]
    vp8s = V.corpus(1)[::7]
    raws, kinds = [], []
    for k in range(max(len(jpegs), len(pngs), len(webps), len(vp8s))):
        for kind, items in (("vp8", vp8s), ("webp", webps), ("png", pngs), ("jpeg", jpegs)):
            if k < len(items):
                raws.append(items[k] if kind == "jpeg" else items[k][1])
                kinds.append((kind, k))
    staged = pipeline.host_decode(raws, lossy_webp=True)
    assert isinstance(staged, pipeline.MixedStage) and len(staged.vp8_idx) == len(vp8s) and len(staged.webp_idx) == len(webps)
    batch = pipeline.decode_staged(staged)
    jb = pipeline.decode_jpegs(jpegs)
    rgb, jrgb = batch.rgb.cpu().numpy(), jb.rgb.cpu().numpy()
    for i, (kind, k) in enumerate(kinds):
        h, w = batch.sizes_host[i]
        if kind == "jpeg":
            assert (h, w) == jb.sizes_host[k]
            assert np.array_equal(rgb[i, :h, :w], jrgb[k, :h, :w]), i
        elif kind == "png":
            assert np.array_equal(rgb[i, :h, :w], pngs[k][2]), i
        elif kind == "webp":
            assert np.array_equal(rgb[i, :h, :w], W.pillow_rgb(webps[k][1])), (i, webps[k][0])
        else:
            assert np.array_equal(rgb[i, :h, :w], V.pillow_rgb(vp8s[k][1])), (i, vp8s[k][0])
        assert not rgb[i, h:].any() and not rgb[i, :, w:].any()
    # lossy and JPEG only: a MixedStage with neither a PNG nor a lossless part
    two = pipeline.decode_images([vp8s[0][1], jpegs[0], vp8s[1][1]], lossy_webp=True)
    assert np.array_equal(two.rgb.cpu().numpy()[2, :two.sizes_host[2][0], :two.sizes_host[2][1]], V.pillow_rgb(vp8s[1][1]))


def test_batch_of_256(report):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    rng = np.random.default_rng(7)
    distinct = []
    for k in range(32):                                      # 32 distinct files, eight times
        kind, make = V.KINDS[k % len(V.KINDS)]
        distinct.append(V.pillow_lossy(make(rng, 200, 200), quality=(0, 30, 75, 100)[(k // 5) % 4], method=(0, 4, 6)[k % 3],
                                       **({"exact": True} if kind == "rgba" else {})))
    raws = [distinct[(i * 5) % 32] for i in range(256)]
    staged = pipeline.host_decode(raws, lossy_webp=True)
    assert isinstance(staged, pipeline.Vp8Stage) and len(staged) == 256
    batch = pipeline.decode_staged(staged)
    rgb = batch.rgb.cpu().numpy()
    for i in (0, 1, 2, 3, 126, 127, 128, 129, 252, 253, 254, 255):
        assert np.array_equal(rgb[i], V.pillow_rgb(raws[i])), i
    report("[vp8] batch of 256 lossy WebPs (200x200, qualities 0-100, methods 0-6, photographs, flat, runs, gray, RGBA): "
           "images 0-3, 126-129, 252-255 bit-exact")


def _lossy_and_lossless(n, first=0):
    """n lossy files of the synthetic JPEGs' pixels, and lossless WebPs of the pixels libwebp decodes from them"""
    lossy = [V.pillow_lossy(np.asarray(Image.open(io.BytesIO(synth_jpeg(first + i))).convert("RGB")), quality=(75, 30, 100)[i % 3],
                            method=(4, 0, 6)[i % 3]) for i in range(n)]
    lossless = [W.pillow_webp(V.pillow_rgb(r), method=(0, 2, 4)[i % 3]) for i, r in enumerate(lossy)]
    return lossy, lossless


def test_same_pixels_resize_and_scores(report):
    """a lossy file's decoded pixels re-fed as a lossless WebP give the same resized inputs (fast, f32, packed) and member scores"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, ops, pipeline, zoo
    lossy, lossless = _lossy_and_lossless(6)
    bl, bw = pipeline.decode_images(lossy, lossy_webp=True), pipeline.decode_images(lossless)
    assert torch.equal(bl.rgb, bw.rgb) and bl.sizes_host == bw.sizes_host
    for hw in (200, 224):
        for dt in (torch.float16, torch.float32, ops.PACKED):
            assert torch.equal(bl.resized(hw, hw, dtype=dt), bw.resized(hw, hw, dtype=dt)), (hw, dt)
    members = [zoo.build_member(k) for k in ("resnet_rs50", "gcvit_tiny")]
    sl = ensemble.score_files(lambda lo, hi: lossy[lo:hi], len(lossy), members, batch_size=4, lossy_webp=True)
    sw = ensemble.score_files(lambda lo, hi: lossless[lo:hi], len(lossless), members, batch_size=4)
    assert np.array_equal(sl, sw)
    report(f"[vp8] same pixels as lossless WebP: rgb, resized (fast / f32 / packed) and 2 members' scores identical ({sl.shape})")


def test_cli_webp_lossy_flag(tmp_path):
    """--webp-lossy over lossy files == the run over lossless copies of the same pixels; without the flag the run is refused"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    from vipcup_amd import main as cli
    cfg = tmp_path / "ckpts2.json"
    cfg.write_text('[["ResNetRS50-200x200", [200, 200], 0], ["GCViTTiny-224x224", [224, 224], 1]]')
    lossy, lossless = _lossy_and_lossless(10, first=300)
    out = {}
    for kind, files in (("lossy", lossy), ("lossless", lossless)):
        d = tmp_path / kind
        d.mkdir()
        names = [f"img_{i:03d}.webp" for i in range(len(files))]
        for name, raw in zip(names, files):
            (d / name).write_bytes(raw)
        (d / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
        cli.main([str(d / "test.csv"), str(d / "out.csv"), "--synthetic", "--ckpt-cfg", str(cfg), "--scores-out", str(d / "scores.csv"),
                  "--batch-size", "4"] + (["--webp-lossy"] if kind == "lossy" else []))
        out[kind] = (pd.read_csv(d / "scores.csv"), pd.read_csv(d / "out.csv"))
    pd.testing.assert_frame_equal(out["lossy"][0], out["lossless"][0], check_exact=True)
    pd.testing.assert_frame_equal(out["lossy"][1], out["lossless"][1], check_exact=True)
    d = tmp_path / "lossy"
    with pytest.raises(_abi.VipError, match="webp image 0: .*lossy WebP"):
        cli.main([str(d / "test.csv"), str(d / "out2.csv"), "--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "4"])
