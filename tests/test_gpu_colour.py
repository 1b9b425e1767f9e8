"""GPU: the colour stress tests - csrc/colour.hip (``pipeline.colour`` and ``gray`` / ``bgr`` / ``hue`` / ``saturation`` / ``contrast`` /
``brightness`` / ``gamma`` on top of it) against the integer restatement of tests/_colour_ref.py pixel by pixel, ``stress_batch`` rows
against the ``pipeline`` calls they stand for, and one ``main.py --stress-gray --stress-saturation`` run.  Every comparison is exact: the
kernel is integer arithmetic, and the member passes see the same pixels in the same batch positions.  The batch is test_gpu_warp.py's:
1- and 7-pixel rows (shorter than a dword group), sizes that are no multiple of the 128 x 8 tile, a 300-pixel row against a wider slot,
and slot pitches padded by 0 and by 3 pixels, so that rows start at every byte phase."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _colour_ref as R  # noqa: E402
from tests import _parity as P  # noqa: E402
from tests._jpeg_enc_ref import content  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402

SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (37, 53), (129, 64), (200, 200), (64, 300)]           # (height, width)
NAMED = [("gray", None), ("bgr", None), ("hue", 30), ("hue", -90), ("hue", 180), ("saturation", 0), ("saturation", 50), ("saturation", 200),
         ("contrast", 0), ("contrast", 50), ("contrast", 150), ("brightness", -50), ("brightness", 10), ("gamma", 0.8), ("gamma", 2.0)]


@functools.lru_cache(maxsize=None)
def _images():
    out = [content(61 + k, w, h) for k, (h, w) in enumerate(SIZES)]
    out[5] = np.random.default_rng(5).integers(0, 256, SIZES[5] + (3,), dtype=np.uint8)      # pure noise
    for px in out:
        px.setflags(write=False)
    return tuple(out)


def _batch(pad: int = 0, images=None):
    """a DecodedBatch holding the images in slots of the largest size (+ pad), the rest of every slot filled with noise"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    imgs = _images() if images is None else images
    sizes = [im.shape[:2] for im in imgs]
    maxH, maxW = max(h for h, _ in sizes) + pad, max(w for _, w in sizes) + pad
    rgb = np.random.default_rng(6).integers(0, 256, (len(imgs), maxH, maxW, 3), dtype=np.uint8)
    for i, im in enumerate(imgs):
        rgb[i, :im.shape[0], :im.shape[1]] = im
    return pipeline.DecodedBatch(torch.from_numpy(rgb).cuda(), torch.tensor(sizes, dtype=torch.int32, device="cuda"), list(sizes))


@functools.lru_cache(maxsize=None)
def _want(kind, arg):
    """the restatement's pixels of every image under a named variant (the mean: each image's own integer mean), computed once"""
    out = [R.apply(im, *R.variant(kind, arg)) for im in _images()]
    for px in out:
        px.setflags(write=False)
    return tuple(out)


def _check(out, want, what, pad_value=0, sizes=SIZES):
    """``out`` (a DecodedBatch, or a numpy slot array) == ``want`` on every image's pixels, ``pad_value`` everywhere else"""
    if not isinstance(out, np.ndarray):
        assert out.sizes_host == list(sizes) and out.sizes.cpu().tolist() == [list(s) for s in sizes], what
        out = out.rgb.cpu().numpy()
    inside = np.zeros(out.shape[:3], bool)
    for i, (px, (h, w)) in enumerate(zip(want, sizes)):
        bad = int((out[i, :h, :w] != px).any(axis=2).sum())
        assert bad == 0, f"{what}: image {i} {(h, w)}: {bad} pixels differ from the restatement"
        inside[i, :h, :w] = True
    assert (out[~inside] == pad_value).all(), f"{what}: written outside an image"


def _call(pipeline, batch, kind, arg):
    fn = getattr(pipeline, kind)
    return fn(batch) if arg is None else fn(batch, arg)


def test_named_variants_equal_the_restatement():
    """every named variant through ``pipeline``, slots at an even and an odd pitch; the source stays, the result is new and repeatable"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    for pad in (0, 3):
        batch = _batch(pad)
        before = batch.rgb.clone()
        for kind, arg in NAMED:
            out = _call(pipeline, batch, kind, arg)
            _check(out, _want(kind, arg), (kind, arg, pad))
            assert out.rgb.data_ptr() != batch.rgb.data_ptr() and out.rgb.shape == batch.rgb.shape
            assert torch.equal(_call(pipeline, batch, kind, arg).rgb, out.rgb), (kind, arg)
        assert torch.equal(batch.rgb, before), "a colour call changed its input"
    px = pipeline.bgr(batch).rgb.cpu().numpy()
    for i, (im, (h, w)) in enumerate(zip(_images(), SIZES)):
        assert np.array_equal(px[i, :h, :w], im[..., ::-1])
    assert torch.equal(pipeline.saturation(batch, 0).rgb, pipeline.gray(batch).rgb)


def _abi_call(lib, batch, dst, coef, mean=None, lut=None):
    n, maxH, maxW, _ = batch.rgb.shape
    coef = np.ascontiguousarray(coef, np.int32)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())              # noqa: E731
    st = lib.vip_colour_rgb_u8(ptr(batch.rgb), ptr(batch.sizes), maxH, maxW, ptr(dst), int(dst.shape[1]), int(dst.shape[2]),
                               coef.ctypes.data_as(C.c_void_p), ptr(mean), ptr(lut), n, None)
    torch.cuda.synchronize()
    return st


def _coef(M, K=None, O=None):
    return np.concatenate([np.asarray(M, np.int64).ravel(), np.zeros(3, np.int64) if K is None else np.asarray(K, np.int64),
                           np.zeros(3, np.int64) if O is None else np.asarray(O, np.int64)]).astype(np.int32)


@pytest.mark.parametrize("kind,arg", [("hue", 30), ("contrast", 150), ("gamma", 0.8)])
def test_c_abi_into_a_larger_destination_keeps_every_other_byte(kind, arg):
    """a destination whose slots are larger than the source's, at another pitch and not word-aligned, prefilled with a marker: the pixels
    equal the restatement and every byte outside the images - guard bands before and after included - still holds the marker"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    lib = _abi.lib()
    batch = _batch(3)
    n = len(SIZES)
    maxH, maxW = batch.rgb.shape[1] + 2, batch.rgb.shape[2] + 5
    body = n * maxH * maxW * 3
    M, K, O, lut = R.variant(kind, arg)
    mean = batch.mean_colour() if K is not None else None
    lut_d = None if lut is None else torch.from_numpy(lut.astype(np.uint8)).cuda()
    for guard in (4096, 4099):
        buf = torch.full((body + 2 * guard,), 0xAB, dtype=torch.uint8, device="cuda")
        dst = buf[guard:guard + body].view(n, maxH, maxW, 3)
        assert _abi_call(lib, batch, dst, _coef(M, K, O), mean, lut_d) == 0, lib.vip_last_error()
        flat = buf.cpu().numpy()
        assert (flat[:guard] == 0xAB).all() and (flat[guard + body:] == 0xAB).all(), "written outside the buffer"
        _check(flat[guard:guard + body].reshape(n, maxH, maxW, 3), _want(kind, arg), (kind, arg, guard), pad_value=0xAB)


def test_extreme_coefficients():
    """the largest admitted coefficients: a 32-bit overflow, a logical shift of a negative sum or a missing clamp shows here only"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    lib = _abi.lib()
    top, off = 1 << 18, 1 << 25
    white = tuple(np.full(s + (3,), 255, np.uint8) for s in [(3, 5), (9, 130)])
    batch = _batch(1, white)
    sizes = [im.shape[:2] for im in white]
    mean = batch.mean_colour()
    assert mean.cpu().numpy()[:, :3].tolist() == [[255] * 3] * 2
    for sign, value in ((1, 255), (-1, 0)):
        M, K, O = np.full((3, 3), sign * top), np.full(3, sign * top), np.full(3, sign * off)
        want = [R.apply(im, M, K, O) for im in white]
        assert all((px == value).all() for px in want)
        dst = torch.full_like(batch.rgb, 0x5A)
        assert _abi_call(lib, batch, dst, _coef(M, K, O), mean) == 0, lib.vip_last_error()
        _check(dst.cpu().numpy(), want, ("extreme", sign), pad_value=0x5A, sizes=sizes)
        _check(pipeline.colour(batch, M, K, O), want, ("extreme through pipeline", sign), sizes=sizes)
    # negative products against a positive offset: sums of both signs, the shift has to floor
    batch = _batch(3)
    M, O = np.full((3, 3), -top), np.full(3, off)
    want = [R.apply(im, M, None, O) for im in _images()]
    flat = np.concatenate([px.ravel() for px in want])
    assert (flat == 0).any() and ((flat > 0) & (flat < 255)).any() and (flat == 255).any(), "the case should reach both clamps and the middle"
    _check(pipeline.colour(batch, M, O=O), want, "negative matrix")
    M = np.array([[top, -top, 3], [-70000, 65536, -1], [-1, -1, -1]])
    O = np.array([-65536 * 40, 12345, 65536 * 3 - 32768 + 300])
    _check(pipeline.colour(batch, M, O=O), [R.apply(im, M, None, O) for im in _images()], "mixed signs")


def test_lookup_table_alone_and_after_a_matrix():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    perm = np.random.default_rng(9).permutation(256).astype(np.int64)
    ident = R.bgr()[0][::-1]
    batch = _batch(3)
    _check(pipeline.colour(batch, ident, lut=perm), [perm[im].astype(np.uint8) for im in _images()], "table alone")
    M = R.hue(-30)[0]
    _check(pipeline.colour(batch, M, lut=perm), [R.apply(im, M, lut=perm) for im in _images()], "table after a matrix")
    _check(pipeline.colour(batch, ident, lut=np.arange(256)), list(_images()), "identity")


def test_contrast_uses_each_images_own_integer_mean():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    batch = _batch(3)
    means = [R.int_mean(im) for im in _images()]
    assert batch.mean_colour().cpu().numpy()[:, :3].tolist() == [m.tolist() for m in means]
    assert len({tuple(m.tolist()) for m in means}) > 4, "the images' means should differ"
    M, K, _, _ = R.contrast(50)
    want = [R.apply(im, M, K, mean=m) for im, m in zip(_images(), means)]
    _check(pipeline.contrast(batch, 50), want, "contrast 50")
    _check(pipeline.contrast(batch, 50, batch.mean_colour()), want, "contrast 50, the mean handed in")
    # another image's mean gives other pixels: the term is per image
    assert not np.array_equal(R.apply(_images()[6], M, K, mean=means[5]), want[6])
    calls = []
    orig = pipeline.DecodedBatch.mean_colour
    pipeline.DecodedBatch.mean_colour = lambda self: calls.append(1) or orig(self)
    try:
        pipeline.gray(batch), pipeline.hue(batch, 30), pipeline.gamma(batch, 0.8)
        assert not calls, "mean_colour ran for a variant without a K"
        pipeline.contrast(batch, 150)
        assert len(calls) == 1
    finally:
        pipeline.DecodedBatch.mean_colour = orig


def test_entry_point_refuses_bad_arguments_without_a_launch():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    lib = _abi.lib()
    batch = _batch()
    n, maxH, maxW, _ = batch.rgb.shape
    dst = torch.full_like(batch.rgb, 0xAB)
    mean = batch.mean_colour()
    ptr = lambda t: C.c_void_p(t.data_ptr())              # noqa: E731
    ident = _coef(R.bgr()[0][::-1])
    cp = lambda v: v.ctypes.data_as(C.c_void_p)           # noqa: E731
    big_m, big_o, with_k = ident.copy(), ident.copy(), ident.copy()
    big_m[1], big_o[14], with_k[10] = (1 << 18) + 1, -(1 << 25) - 1, 5
    good = [ptr(batch.rgb), ptr(batch.sizes), maxH, maxW, ptr(dst), maxH, maxW, cp(ident), ptr(mean), None, n, None]
    for k, v, code, word in [(0, None, -1, b"null"), (1, None, -1, b"null"), (4, None, -1, b"null"), (7, None, -1, b"null"),
                             (10, 0, -1, b"bad size"), (2, 0, -1, b"bad size"), (6, -1, -1, b"bad size"),
                             (4, ptr(batch.rgb), -1, b"overlap"), (7, cp(big_m), -1, b"coefficient"), (7, cp(big_o), -1, b"coefficient"),
                             (1, C.c_void_p(batch.sizes.data_ptr() + 2), -2, b"4-byte"), (8, C.c_void_p(mean.data_ptr() + 1), -2, b"4-byte")]:
        args = list(good)
        args[k] = v
        assert lib.vip_colour_rgb_u8(*args) == code and word in lib.vip_last_error(), (k, v)
    args = list(good)
    args[7], args[8] = cp(with_k), None
    assert lib.vip_colour_rgb_u8(*args) == -1 and b"mean_u8" in lib.vip_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 0xAB).all()), "a refused call wrote pixels"
    assert lib.vip_colour_rgb_u8(*good) == 0                                                  # and the same arguments, valid: the identity
    torch.cuda.synchronize()
    for i, (h, w) in enumerate(SIZES):
        assert torch.equal(dst[i, :h, :w], batch.rgb[i, :h, :w])


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
    batch = pipeline.decode_images(raws)
    calls = []
    orig = pipeline.DecodedBatch.mean_colour
    pipeline.DecodedBatch.mean_colour = lambda self: calls.append(1) or orig(self)
    try:
        rows, labels = ensemble.stress_batch(raws, members, [75], gray=True, hues=[30], contrasts=[150, 50])
    finally:
        pipeline.DecodedBatch.mean_colour = orig
    assert len(calls) == 1, "mean_colour runs once per batch"
    assert labels == ensemble.stress_labels([75], gray=True, hues=[30], contrasts=[150, 50]) == \
        ["q75", "gray", "gray_q75", "hue030", "hue030_q75", "con050", "con050_q75", "con150", "con150_q75"] and rows.shape == (10, 1, 3)
    assert torch.equal(rows[0], ensemble._score_batch(batch, members))
    assert torch.equal(rows[:2], ensemble.stress_batch(raws, members, [75]))
    coloured = [pipeline.gray(batch), pipeline.hue(batch, 30), pipeline.contrast(batch, 50), pipeline.contrast(batch, 150)]
    for k, c in zip(range(2, 10, 2), coloured):
        assert torch.equal(rows[k], ensemble._score_batch(c, members)), labels[k - 1]
        assert torch.equal(rows[k + 1], ensemble._score_batch(pipeline.recompress(c, 75), members)), labels[k]
        assert not torch.equal(rows[k], rows[0]), labels[k - 1]
    # colour alone gives (rows, labels) as well; the other variants in their order
    rows, labels = ensemble.stress_batch(raws, members, [], bgr=True, saturations=[50], brightnesses=[-10], gammas=[0.8], flips=["h"])
    assert labels == ["fliph", "bgr", "sat050", "brim10", "gam080"] and rows.shape == (6, 1, 3)
    for k, c in enumerate([pipeline.flip(batch, "h"), pipeline.bgr(batch), pipeline.saturation(batch, 50), pipeline.brightness(batch, -10),
                           pipeline.gamma(batch, 0.8)]):
        assert torch.equal(rows[k + 1], ensemble._score_batch(c, members)), labels[k]
    assert isinstance(ensemble.stress_batch(raws, members, [75], gray=False, bgr=False, hues=(), gammas=()), torch.Tensor)


# ---- CLI --------------------------------------------------------------------------------------------------------------------------------
def test_cli_gray_saturation_and_jpeg_end_to_end(tmp_path):
    """--stress-gray --stress-saturation 50 --stress-jpeg 75: the CSVs of a plain run unchanged, the table's columns, the settings"""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import zoo
    from vipcup_amd import main as cli
    names = _write_set(tmp_path, 4)
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS["resnet_rs50"].ckpt_name, [zoo.MEMBERS["resnet_rs50"].input_hw] * 2, 0]]))
    extra = ["--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "4"]
    csv = str(tmp_path / "test.csv")
    cli.main([csv, str(tmp_path / "o0.csv"), "--scores-out", str(tmp_path / "s0.csv"), *extra])
    cli.main([csv, str(tmp_path / "o1.csv"), "--scores-out", str(tmp_path / "s1.csv"), *extra, "--stress-gray", "--stress-saturation", "50",
              "--stress-jpeg", "75", "--stress-out", str(tmp_path / "stress.csv")])
    assert (tmp_path / "o0.csv").read_bytes() == (tmp_path / "o1.csv").read_bytes()
    assert (tmp_path / "s0.csv").read_bytes() == (tmp_path / "s1.csv").read_bytes()
    labels = ["q75", "gray", "gray_q75", "sat050", "sat050_q75"]
    table = pd.read_csv(tmp_path / "stress.csv", dtype={"flips_at": str, "flips": str}, keep_default_na=False)
    assert list(table.columns) == ["filename", "p", "decision"] + [f"p_{v}" for v in labels] + [f"decision_{v}" for v in labels] + \
        ["stable", "flips_at", "flips"]
    assert table.filename.tolist() == sorted(names)
    p_all = np.stack([table[f"p_{v}"].to_numpy(np.float32) for v in labels], axis=1)
    assert np.isfinite(p_all).all() and (p_all != table.p.to_numpy(np.float32)[:, None]).any(axis=0).all(), "a variant scored the plain pixels"
    info = json.loads((tmp_path / "stress.json").read_text())
    assert info["variants"] == labels and info["qualities"] == [75] and info["n_files"] == len(names)
    st = info["settings"]
    assert st["gray"] is True and st["bgr"] is False and st["saturations"] == [50] and st["hues"] == [] and st["contrasts"] == []
    assert st["brightnesses"] == [] and st["gammas"] == [] and st["qualities"] == [75] and "flips" not in st and len(st["members"]) == 1
