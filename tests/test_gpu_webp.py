"""GPU: lossless WebP input - host entropy decode, device inverse transforms (csrc/webp_host.cpp, csrc/webp_pipeline.hip) -
bit-exact against the pure-Python reference of tests/_webp.py and against Pillow / libwebp over the whole corpus, in mixed
batches with PNG and JPEG, in a batch of 256, and against the JPEG path on the same pixels through resize, the members and
the CLI.  Lossy and animated files are refused by the host stage."""
import io

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from tests import _png  # noqa: E402
from tests import _webp as W  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402


def _check_batch(batch, expected, names=None):
    rgb = batch.rgb.cpu().numpy()
    for i, want in enumerate(expected):
        h, w = batch.sizes_host[i]
        name = names[i] if names else i
        assert (h, w) == want.shape[:2], name
        got = rgb[i, :h, :w]
        assert np.array_equal(got, want), f"image {name}: {int((got != want).any(-1).sum())} pixels differ"
        assert not rgb[i, h:].any() and not rgb[i, :, w:].any(), f"image {name}: padding not zero"


def _webp_of(rgb: np.ndarray, k: int = 0) -> bytes:
    return W.pillow_webp(rgb, method=(0, 2, 4, 6)[k % 4], quality=(0, 75, 100)[k % 3])


def test_decode_corpus_bit_exact(report):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    corp = W.corpus(1, W.SIZES)
    raws, names = [r for _, r in corp], [n for n, _ in corp]
    batch = pipeline.decode_images(raws)
    torch.cuda.synchronize()
    ref = [W.reference_rgb(r) for r in raws]
    _check_batch(batch, ref, names)
    _check_batch(batch, [W.pillow_rgb(r) for r in raws], names)
    report(f"[webp] decode_images: {len(raws)} lossless WebPs (Pillow's encoder over {len(W.KINDS)} kinds x 4 methods x 3 qualities, "
           f"{sum(n.startswith('hw_') for n in names)} hand-written: every predictor mode, unusual transform orders, all plane codes; "
           f"1x1 .. 200x200) bit-exact vs the reference and vs Pillow")


def test_mixed_batch():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    jpegs = [synth_jpeg(i) for i in (0, 1, 2, 49)]
    pngs = _png.corpus(seed=2, sizes=[(17, 13), (65, 7)])[::11][:5]
    webps = W.corpus(2, [(17, 13), (200, 200), (65, 7)])[::9]
    raws, kinds = [], []
    for k in range(max(len(jpegs), len(pngs), len(webps))):
        for kind, items in (("webp", webps), ("png", pngs), ("jpeg", jpegs)):
            if k < len(items):
                raws.append(items[k] if kind == "jpeg" else items[k][1])
                kinds.append((kind, k))
    staged = pipeline.host_decode(raws)
    assert isinstance(staged, pipeline.MixedStage) and len(staged.webp_idx) == len(webps)
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
        else:
            assert np.array_equal(rgb[i, :h, :w], W.pillow_rgb(webps[k][1])), (i, webps[k][0])
        assert not rgb[i, h:].any() and not rgb[i, :, w:].any()
    # WebP and JPEG only: a MixedStage without a PNG part
    two = pipeline.decode_images([webps[0][1], jpegs[0], webps[1][1]])
    assert np.array_equal(two.rgb.cpu().numpy()[2, :two.sizes_host[2][0], :two.sizes_host[2][1]], W.pillow_rgb(webps[1][1]))


def test_batch_of_256(report):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    rng = np.random.default_rng(7)
    makers = [W._photo, W._runs, W._gray, W._green, W._rgba] + [(lambda n: lambda r, h, w: W._palette(r, h, w, n))(n)
                                                                for n in (2, 3, 4, 5, 16, 17, 200)]
    distinct = []
    for k in range(32):                                      # 32 distinct files (the encoder is the slow part), eight times
        arr = makers[k % len(makers)](rng, 200, 200)
        distinct.append(W.pillow_webp(arr, method=(0, 2, 4, 6)[(k // 3) % 4], quality=75, **({"exact": True} if arr.shape[-1] == 4 else {})))
    raws = [distinct[(i * 5) % 32] for i in range(256)]
    staged = pipeline.host_decode(raws)
    assert isinstance(staged, pipeline.WebpStage) and len(staged) == 256
    batch = pipeline.decode_staged(staged)
    rgb = batch.rgb.cpu().numpy()
    for i in (0, 1, 2, 3, 126, 127, 128, 129, 252, 253, 254, 255):
        assert np.array_equal(rgb[i], W.pillow_rgb(raws[i])), i
    report("[webp] batch of 256 WebPs (200x200, Pillow methods 0-6, photographs, runs, palettes of 2-200 colours, RGBA): "
           "images 0-3, 126-129, 252-255 bit-exact")


def test_same_pixels_resize_and_scores(report):
    """a lossless WebP of a JPEG's decoded pixels gives the same resized inputs (fast, f32, packed strict) and member scores"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, ops, pipeline, zoo
    jpegs = [synth_jpeg(i) for i in range(6)]
    pix = [np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs]
    webps = [_webp_of(p, k) for k, p in enumerate(pix)]
    bj, bw = pipeline.decode_jpegs(jpegs), pipeline.decode_images(webps)
    assert torch.equal(bj.rgb, bw.rgb) and bj.sizes_host == bw.sizes_host
    for hw in (200, 224):
        for dt in (torch.float16, torch.float32, ops.PACKED):
            assert torch.equal(bj.resized(hw, hw, dtype=dt), bw.resized(hw, hw, dtype=dt)), (hw, dt)
    members = [zoo.build_member(k) for k in ("resnet_rs50", "gcvit_tiny")]
    sj = ensemble.score_files(lambda lo, hi: jpegs[lo:hi], len(jpegs), members, batch_size=4)
    sw = ensemble.score_files(lambda lo, hi: webps[lo:hi], len(webps), members, batch_size=4)
    assert np.array_equal(sj, sw)
    report(f"[webp] same pixels as JPEG: rgb, resized (fast / f32 / packed) and 2 members' scores identical ({sj.shape})")


def test_cli_webp_csv_matches_jpeg_csv(tmp_path):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import main as cli
    cfg = tmp_path / "ckpts2.json"
    cfg.write_text('[["ResNetRS50-200x200", [200, 200], 0], ["GCViTTiny-224x224", [224, 224], 1]]')
    out = {}
    for ext in ("jpg", "webp"):
        d = tmp_path / ext
        d.mkdir()
        names = []
        for i in range(10):
            j = synth_jpeg(300 + i)
            raw = j if ext == "jpg" else _webp_of(np.asarray(Image.open(io.BytesIO(j)).convert("RGB")), i)
            names.append(f"img_{i:03d}.{ext}")
            (d / names[-1]).write_bytes(raw)
        (d / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
        cli.main([str(d / "test.csv"), str(d / "out.csv"), "--synthetic", "--ckpt-cfg", str(cfg), "--scores-out",
                  str(d / "scores.csv"), "--batch-size", "4"])
        sc, dec = pd.read_csv(d / "scores.csv"), pd.read_csv(d / "out.csv")
        sc["filename"] = sc["filename"].str.replace(f".{ext}", "", regex=False)
        dec["filename"] = dec["filename"].str.replace(f".{ext}", "", regex=False)
        out[ext] = (sc, dec)
    pd.testing.assert_frame_equal(out["jpg"][0], out["webp"][0], check_exact=True)
    pd.testing.assert_frame_equal(out["jpg"][1], out["webp"][1], check_exact=True)


def test_lossy_and_animated_are_refused_before_any_launch():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    rng = np.random.default_rng(0)
    good = W.pillow_webp(W._photo(rng, 16, 16))
    buf = io.BytesIO()
    Image.fromarray(W._photo(rng, 16, 16)).save(buf, "WEBP", quality=80)
    lossy = buf.getvalue()
    frames = [Image.fromarray(W._photo(rng, 16, 16)) for _ in range(2)]
    buf = io.BytesIO()
    frames[0].save(buf, "WEBP", save_all=True, append_images=frames[1:], lossless=True, duration=50)
    animated = buf.getvalue()
    with pytest.raises(_abi.VipError, match="webp image 2: .*lossy WebP"):
        pipeline.host_decode([synth_jpeg(0), good, lossy, synth_jpeg(1)])      # the host stage, before anything is launched
    with pytest.raises(_abi.VipError, match="webp image 1: .*animated"):
        pipeline.host_decode([good, animated])
    with pytest.raises(_abi.VipError, match="webp image 2"):
        pipeline.decode_images([synth_jpeg(0), good, lossy])
    with pytest.raises(_abi.VipError, match="image 1: neither"):
        pipeline.decode_images([good, b"GIF89a" + bytes(40)])
