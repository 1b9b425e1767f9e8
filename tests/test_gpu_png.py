"""GPU: PNG input (dataset/dataset.py:22-30, tf.image.decode_png(channels=3)) - host inflate, device unfilter + expansion
(csrc/png_host.cpp, csrc/png_pipeline.hip) - bit-exact against the pure-Python reference of tests/_png.py, against Pillow for
the 8-bit outputs, and against the JPEG path on the same pixels through resize, the members and the CLI."""
import io

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from tests import _png  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402


def _check_batch(batch, expected):
    rgb = batch.rgb.cpu().numpy()
    for i, want in enumerate(expected):
        h, w = batch.sizes_host[i]
        assert (h, w) == want.shape[:2], i
        got = rgb[i, :h, :w]
        assert np.array_equal(got, want), f"image {i}: {int((got != want).any(-1).sum())} pixels differ"
        assert not rgb[i, h:].any() and not rgb[i, :, w:].any(), f"image {i}: padding not zero"


def _png_of(rgb: np.ndarray, k: int = 0) -> bytes:
    return _png.write_png(rgb, 2, 8, filter_seed=k)


def test_decode_corpus_bit_exact(report):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    corp = _png.corpus(seed=1)
    pngs = [p for _, p, _ in corp]
    batch = pipeline.decode_images(pngs)
    torch.cuda.synchronize()
    ref = [_png.reference_rgb(p) for p in pngs]
    for (name, _, want), r in zip(corp, ref):
        assert np.array_equal(r, want), name                # the reference agrees with the pixels the writer was given
    _check_batch(batch, ref)
    n_pil = 0
    for name, png, want in corp:
        if "_d16" in name:
            continue                                          # Pillow keeps 16-bit gray as I;16 and truncates 16-bit RGB
        pil = np.asarray(Image.open(io.BytesIO(png)).convert("RGB"))
        assert np.array_equal(pil, want), name
        n_pil += 1
    report(f"[png] decode_images: {len(pngs)} PNGs (every colour type x depth, Adam7, 1x1 .. 7x1500) bit-exact vs the "
           f"reference; {n_pil} of them vs Pillow")


def test_palette_index_past_plte_is_black_and_16bit_rule():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 256, size=(37, 41, 1))
    pal = rng.integers(1, 256, size=(5, 3))
    p_pal = _png.write_png(idx, 3, 8, palette=pal)
    v = np.arange(65536, dtype=np.int64).reshape(256, 256, 1)
    p16 = _png.write_png(v, 0, 16, interlace=1)
    batch = pipeline.decode_images([p_pal, p16])
    rgb = batch.rgb.cpu().numpy()
    want = np.zeros((37, 41, 3), np.uint8)
    ok = idx[..., 0] < 5
    want[ok] = pal[idx[..., 0][ok]]
    assert np.array_equal(rgb[0, :37, :41], want)
    g = (2 * v[..., 0] + 257) // 514                          # round(v / 257) (png_set_scale_16), every 16-bit value
    assert np.array_equal(g, np.floor(v[..., 0] / 257 + 0.5))
    assert np.array_equal(rgb[1, :256, :256], np.repeat(g[..., None], 3, -1).astype(np.uint8))


def test_mixed_batch():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    jpegs = [synth_jpeg(i) for i in (0, 1, 2, 49)]
    corp = _png.corpus(seed=2, sizes=[(17, 13), (200, 200), (65, 7)])[::7]
    raws, kinds = [], []
    for k in range(max(len(jpegs), len(corp))):
        if k < len(corp):
            raws.append(corp[k][1])
            kinds.append(("png", k))
        if k < len(jpegs):
            raws.append(jpegs[k])
            kinds.append(("jpeg", k))
    batch = pipeline.decode_images(raws)
    jb = pipeline.decode_jpegs(jpegs)
    rgb, jrgb = batch.rgb.cpu().numpy(), jb.rgb.cpu().numpy()
    for i, (kind, k) in enumerate(kinds):
        h, w = batch.sizes_host[i]
        if kind == "jpeg":
            assert (h, w) == jb.sizes_host[k]
            assert np.array_equal(rgb[i, :h, :w], jrgb[k, :h, :w]), i
        else:
            assert np.array_equal(rgb[i, :h, :w], corp[k][2]), i
        assert not rgb[i, h:].any() and not rgb[i, :, w:].any()


def test_same_pixels_resize_and_scores(report):
    """a PNG of a JPEG's decoded pixels gives the same resized inputs (fast, f32, packed strict) and the same member scores"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, ops, pipeline, zoo
    jpegs = [synth_jpeg(i) for i in range(6)]
    pix = [np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs]
    pngs = [_png_of(p, k) for k, p in enumerate(pix)]
    bj, bp = pipeline.decode_jpegs(jpegs), pipeline.decode_images(pngs)
    assert torch.equal(bj.rgb, bp.rgb) and bj.sizes_host == bp.sizes_host
    for hw in (200, 224):
        for dt in (torch.float16, torch.float32, ops.PACKED):
            assert torch.equal(bj.resized(hw, hw, dtype=dt), bp.resized(hw, hw, dtype=dt)), (hw, dt)
    members = [zoo.build_member(k) for k in ("resnet_rs50", "gcvit_tiny")]
    sj = ensemble.score_files(lambda lo, hi: jpegs[lo:hi], len(jpegs), members, batch_size=4)
    sp = ensemble.score_files(lambda lo, hi: pngs[lo:hi], len(pngs), members, batch_size=4)
    assert np.array_equal(sj, sp)
    report(f"[png] same pixels as JPEG: rgb, resized (fast / f32 / packed) and 2 members' scores identical ({sj.shape})")


def test_batch_of_256(report):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    rng = np.random.default_rng(7)
    kinds = [(2, 8), (6, 8), (0, 8), (3, 8), (2, 16), (0, 4)]
    pngs, want = [], {}
    for i in range(256):
        ct, d = kinds[i % len(kinds)]
        png, rgb = _png.make_image(rng, 200, 200, ct, d, i % 2, i)
        pngs.append(png)
        if i in (0, 1, 2, 3, 126, 127, 128, 129, 252, 253, 254, 255):
            want[i] = rgb
    batch = pipeline.decode_images(pngs)
    rgb = batch.rgb.cpu().numpy()
    for i, w in want.items():
        assert np.array_equal(rgb[i], w), i
        assert np.array_equal(w, _png.reference_rgb(pngs[i])), i
    report("[png] batch of 256 PNGs (200x200): images 0-3, 126-129, 252-255 bit-exact")


def test_cli_png_csv_matches_jpeg_csv(tmp_path):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import main as cli
    cfg = tmp_path / "ckpts2.json"
    cfg.write_text('[["ResNetRS50-200x200", [200, 200], 0], ["GCViTTiny-224x224", [224, 224], 1]]')
    out = {}
    for ext in ("jpg", "png"):
        d = tmp_path / ext
        d.mkdir()
        names = []
        for i in range(10):
            j = synth_jpeg(300 + i)
            raw = j if ext == "jpg" else _png_of(np.asarray(Image.open(io.BytesIO(j)).convert("RGB")), i)
            names.append(f"img_{i:03d}.{ext}")
            (d / names[-1]).write_bytes(raw)
        (d / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
        cli.main([str(d / "test.csv"), str(d / "out.csv"), "--synthetic", "--ckpt-cfg", str(cfg), "--scores-out",
                  str(d / "scores.csv"), "--batch-size", "4"])
        sc, dec = pd.read_csv(d / "scores.csv"), pd.read_csv(d / "out.csv")
        sc["filename"] = sc["filename"].str.replace(f".{ext}", "", regex=False)
        dec["filename"] = dec["filename"].str.replace(f".{ext}", "", regex=False)
        out[ext] = (sc, dec)
    pd.testing.assert_frame_equal(out["jpg"][0], out["png"][0], check_exact=True)
    pd.testing.assert_frame_equal(out["jpg"][1], out["png"][1], check_exact=True)


@pytest.mark.parametrize("cache", [True, False])
def test_build_dataset_mixed_folder(tmp_path, cache):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    corp = _png.corpus(seed=3, sizes=[(129, 31), (200, 200)])[::5]
    raws = []
    for k in range(6):
        raws.append(corp[k][1])
        raws.append(synth_jpeg(400 + k))
    paths = []
    for i, raw in enumerate(raws):
        ext = "png" if raw[:8] == _png.SIG else "jpg"
        p = tmp_path / f"im{i:02d}.{ext}"
        p.write_bytes(raw)
        paths.append(str(p))
    ds = pipeline.build_dataset(paths, batch_size=5, cache=cache, augment=False, repeat=False, shuffle=0, dim=[200, 200])
    got = torch.cat([b for b in ds])
    for epoch in range(2 if cache else 1):                    # a cached dataset serves the second pass from HBM
        if epoch:
            got = torch.cat([b for b in ds])
        for i, raw in enumerate(raws):
            one = pipeline.decode_images([raw]).resized(200, 200)[0]
            assert torch.equal(got[i], one), i


def test_corrupt_png_names_its_index():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    good = _png.write_png(np.zeros((8, 8, 3), np.int64), 2, 8)
    bad = bytearray(good)
    bad[8 + 25 + 8 + 2] ^= 0x55                               # signature, IHDR chunk, IDAT header: a byte of IDAT data
    raws = [synth_jpeg(0), good, bytes(bad), synth_jpeg(1)]
    with pytest.raises(_abi.VipError, match="png image 2"):
        pipeline.host_decode(raws)                            # the host stage, before anything is launched
    with pytest.raises(_abi.VipError, match="png image 2"):
        pipeline.decode_images(raws)
    with pytest.raises(_abi.VipError, match="image 1"):
        pipeline.decode_images([synth_jpeg(0), b"GIF89a" + bytes(40)])
