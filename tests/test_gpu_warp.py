"""GPU: the geometric stress tests - csrc/warp.hip (``pipeline.warp`` and ``flip`` / ``crop`` / ``rotate`` on top of it) against the
integer restatement of tests/_warp_ref.py pixel by pixel, ``stress_batch`` rows against the ``pipeline`` calls they stand for, and one
``main.py --stress-flip / --stress-crop / --stress-rotate`` run.  Every comparison is exact: the warp is integer arithmetic, and the
member passes see the same pixels in the same batch positions.  The 129-pixel and larger sides are there because 32-bit coordinate
products overflow from 64-pixel sides on (2^24 * 2 * 64 = 2^31)."""
import ctypes as C
import functools
import io
import json
import math
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
from tests import _warp_ref as W  # noqa: E402
from tests._jpeg_enc_ref import content, pil_jpeg  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402

SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (37, 53), (129, 64), (200, 200), (64, 300)]           # (height, width)
ANGLES = [0.1, -0.1, 7.5, -12.3, 45, -45]


@functools.lru_cache(maxsize=None)
def _images():
    out = [content(51 + k, w, h) for k, (h, w) in enumerate(SIZES)]
    out[5] = np.random.default_rng(5).integers(0, 256, SIZES[5] + (3,), dtype=np.uint8)      # noise: the largest steps between taps
    for px in out:
        px.setflags(write=False)
    return tuple(out)


def _batch(pad: int = 0):
    """a DecodedBatch holding the images in slots of the largest size (+ pad), the rest of every slot filled with noise"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    imgs = _images()
    maxH, maxW = max(h for h, _ in SIZES) + pad, max(w for _, w in SIZES) + pad
    rgb = np.random.default_rng(6).integers(0, 256, (len(imgs), maxH, maxW, 3), dtype=np.uint8)
    for i, im in enumerate(imgs):
        rgb[i, :im.shape[0], :im.shape[1]] = im
    return pipeline.DecodedBatch(torch.from_numpy(rgb).cuda(), torch.tensor(SIZES, dtype=torch.int32, device="cuda"), list(SIZES))


def _general(h, w, out_h, out_w):
    """a ShiftScaleShearRotate-shaped inverse map: rotation by 10 degrees, shear, anisotropic zoom, a shift off the centre"""
    t = math.radians(10.0)
    a, b = 1.15 * math.cos(t), -0.9 * math.sin(t) + 0.2
    c, d = 1.15 * math.sin(t) - 0.1, 0.9 * math.cos(t)
    return (a, b, w / 2 + 1.3 - a * out_w / 2 - b * out_h / 2, c, d, h / 2 - 0.7 - c * out_w / 2 - d * out_h / 2)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(transforms [(a, b, tx, c, d, ty)] per image, output sizes, fill of the restatement) of a named case, from the restatement alone"""
    kind, *arg = name
    if kind == "flip":
        return [W.flip_xf(h, w, arg[0]) for h, w in SIZES], list(SIZES), "black"
    if kind == "crop":
        boxes = [W.crop_box(h, w, arg[0], arg[1]) for h, w in SIZES]
        return [W.crop_xf(y0, x0) for y0, x0, _, _ in boxes], [(hh, ww) for _, _, hh, ww in boxes], "black"
    if kind == "rotate":
        sizes = [W.rotated_rect(h, w, arg[0]) if arg[1] == "crop" else (h, w) for h, w in SIZES]
        return [W.rotate_xf(h, w, arg[0], hh, ww) for (h, w), (hh, ww) in zip(SIZES, sizes)], sizes, "black" if arg[1] == "black" else "mirror"
    sizes = [(h + 5, max(1, w - 3)) for h, w in SIZES]                                    # general: an output size of its own
    return [_general(h, w, hh, ww) for (h, w), (hh, ww) in zip(SIZES, sizes)], sizes, arg[0]


@functools.lru_cache(maxsize=None)
def _want(name):
    """the restatement's pixels of every image of a case, computed once"""
    xfs, sizes, fill = _case(name)
    out = [W.warp(im, W.quantise(*f), hh, ww, fill) for im, f, (hh, ww) in zip(_images(), xfs, sizes)]
    for px in out:
        px.setflags(write=False)
    return tuple(out)


def _check(out, name, pad_value=0):
    """``out`` (a DecodedBatch, or a numpy slot array) == the restatement on every image's pixels, ``pad_value`` everywhere else"""
    _, sizes, _ = _case(name)
    if not isinstance(out, np.ndarray):
        assert out.sizes_host == sizes and out.sizes.cpu().tolist() == [list(s) for s in sizes], name
        assert tuple(out.rgb.shape) == (len(SIZES), max(h for h, _ in sizes), max(w for _, w in sizes), 3), name
        out = out.rgb.cpu().numpy()
    inside = np.zeros(out.shape[:3], bool)
    for i, (want, (hh, ww)) in enumerate(zip(_want(name), sizes)):
        bad = int((out[i, :hh, :ww] != want).any(axis=2).sum())
        assert bad == 0, f"{name}: image {i} {SIZES[i]} -> {(hh, ww)}: {bad} pixels differ from the restatement"
        inside[i, :hh, :ww] = True
    assert (out[~inside] == pad_value).all(), f"{name}: written outside an image"


def test_flip_crop_rotate_equal_the_restatement():
    """the three perturbations through ``pipeline.warp`` and the C ABI, slots at an even and an odd pitch; the source stays as it was"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    for pad in (0, 3):
        batch = _batch(pad)
        before = batch.rgb.clone()
        for axis in ("h", "v"):
            _check(pipeline.flip(batch, axis), ("flip", axis))
        for pc in (50, 99):
            for origin in ("centre", "topleft"):
                _check(pipeline.crop(batch, pc, origin), ("crop", pc, origin))
        for deg in ANGLES:
            for fill in ("crop", "mirror", "black"):
                out = pipeline.rotate(batch, deg, fill)
                _check(out, ("rotate", deg, fill))
                assert out.rgb.data_ptr() != batch.rgb.data_ptr()
        assert torch.equal(batch.rgb, before), "a warp changed its input"
    assert torch.equal(pipeline.rotate(batch, 7.5).rgb, pipeline.rotate(batch, 7.5, "crop").rgb)           # the default; repeatable
    # flips and crops are copies
    px = pipeline.flip(batch, "h").rgb.cpu().numpy()
    for i, (im, (h, w)) in enumerate(zip(_images(), SIZES)):
        assert np.array_equal(px[i, :h, :w], im[:, ::-1])


@pytest.mark.parametrize("fill", ["black", "mirror"])
def test_general_matrix_equals_the_restatement(fill):
    """shear, zoom and a shift, output sizes of their own: ``pipeline.warp`` directly"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    xfs, sizes, _ = _case(("general", fill))
    xf = np.array([W.quantise(*f) for f in xfs], np.int64)
    assert xf.tolist() == [pipeline.warp_matrix(*f) for f in xfs]
    batch = _batch(3)
    before = batch.rgb.clone()
    _check(pipeline.warp(batch, xf, sizes, fill), ("general", fill))
    assert torch.equal(batch.rgb, before)


@pytest.mark.parametrize("name", [("rotate", -12.3, "black"), ("general", "mirror"), ("crop", 50, "centre")])
def test_guard_bands_and_untouched_slot_padding(name):
    """the kernel writes the pixels of the output images and nothing else: sentinel bytes before, after and between the images stay, in
    a destination whose slots are larger than needed"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    xfs, sizes, fill = _case(name)
    xf = np.array([W.quantise(*f) for f in xfs], np.int64)
    batch = _batch(3)
    n, maxH, maxW = len(SIZES), max(h for h, _ in sizes) + 2, max(w for _, w in sizes) + 1
    body = n * maxH * maxW * 3
    for guard in (4096, 4099):                            # 4099: a destination that is not word-aligned
        buf = torch.full((body + 2 * guard,), 0xAB, dtype=torch.uint8, device="cuda")
        dst = buf[guard:guard + body].view(n, maxH, maxW, 3)
        pipeline._warp_into(batch, xf, sizes, pipeline.WARP_FILLS[fill], dst)
        torch.cuda.synchronize()
        flat = buf.cpu().numpy()
        assert (flat[:guard] == 0xAB).all() and (flat[guard + body:] == 0xAB).all(), "written outside the buffer"
        _check(flat[guard:guard + body].reshape(n, maxH, maxW, 3), name, pad_value=0xAB)


def test_entry_point_refuses_bad_arguments_without_a_launch():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    lib = _abi.lib()
    batch = _batch()
    n, maxH, maxW, _ = batch.rgb.shape
    dst = torch.full_like(batch.rgb, 0xAB)
    xf = torch.tensor([pipeline.warp_matrix(1, 0, 0, 0, 1, 0)] * n, dtype=torch.int64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())              # noqa: E731
    good = [ptr(batch.rgb), ptr(batch.sizes), maxH, maxW, ptr(dst), ptr(batch.sizes), maxH, maxW, ptr(xf), 0, n, None]
    for k, v, code, word in [(0, None, -1, b"null"), (1, None, -1, b"null"), (4, None, -1, b"null"), (5, None, -1, b"null"),
                             (8, None, -1, b"null"), (10, 0, -1, b"bad size"), (2, 0, -1, b"bad size"), (7, -1, -1, b"bad size"),
                             (9, 2, -1, b"fill"), (9, -1, -1, b"fill"), (4, ptr(batch.rgb), -1, b"overlap"),
                             (8, C.c_void_p(xf.data_ptr() + 4), -2, b"8-byte"), (5, C.c_void_p(batch.sizes.data_ptr() + 2), -2, b"4-byte")]:
        args = list(good)
        args[k] = v
        assert lib.vip_warp_affine_rgb_u8(*args) == code and word in lib.vip_last_error(), (k, v)
    torch.cuda.synchronize()
    assert bool((dst == 0xAB).all()), "a refused call wrote pixels"
    assert lib.vip_warp_affine_rgb_u8(*good) == 0                                             # and the same arguments, valid: the identity
    torch.cuda.synchronize()
    for i, (h, w) in enumerate(SIZES):
        assert torch.equal(dst[i, :h, :w], batch.rgb[i, :h, :w])


def _png(px) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, format="PNG")
    return buf.getvalue()


def test_rotate_then_recompress_decoded_sources():
    """a batch decoded from PNG and JPEG sources of different sizes: rotate, then recompress == restatement -> Pillow save -> load"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    raws = [_png(content(21, 200, 200)), synth_jpeg(149), _png(content(22, 57, 31)), synth_jpeg(101), _png(content(23, 16, 16)[..., 0])]
    batch = pipeline.decode_images(raws)
    src = batch.rgb.cpu().numpy()
    for deg, fill in ((7.5, "crop"), (-12.3, "black")):
        got = pipeline.recompress(pipeline.rotate(batch, deg, fill), 70)
        px = got.rgb.cpu().numpy()
        for i, (h, w) in enumerate(batch.sizes_host):
            hh, ww = W.rotated_rect(h, w, deg) if fill == "crop" else (h, w)
            rotated = W.warp(np.ascontiguousarray(src[i, :h, :w]), W.quantise(*W.rotate_xf(h, w, deg, hh, ww)), hh, ww,
                             "mirror" if fill == "crop" else fill)
            want = np.asarray(Image.open(io.BytesIO(pil_jpeg(rotated, 70, "4:2:0"))).convert("RGB"))
            assert got.sizes_host[i] == (hh, ww) and np.array_equal(px[i, :hh, :ww], want), (deg, fill, i, (h, w))
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
    rows, labels = ensemble.stress_batch(raws, members, [80], blurs=[1.0], flips=["v", "h"], crops=[80], rotations=[7.5, -3])
    assert labels == ["q80", "b10", "b10_q80", "fliph", "fliph_q80", "flipv", "flipv_q80", "crop80", "crop80_q80",
                      "rotm030", "rotm030_q80", "rot075", "rot075_q80"] and rows.shape == (14, 1, 3)
    old, old_labels = ensemble.stress_batch(raws, members, [80], blurs=[1.0])
    assert old_labels == labels[:3] and torch.equal(rows[:4], old)
    assert torch.equal(ensemble.stress_batch(raws, members, [80], blurs=[1.0], flips=(), crops=(), rotations=())[0], old)
    batch = pipeline.decode_images(raws)
    warped = [pipeline.flip(batch, "h"), pipeline.flip(batch, "v"), pipeline.crop(batch, 80), pipeline.rotate(batch, -3), pipeline.rotate(batch, 7.5)]
    for k, w in zip(range(4, 14, 2), warped):
        assert torch.equal(rows[k], ensemble._score_batch(w, members)), labels[k - 1]
        assert torch.equal(rows[k + 1], ensemble._score_batch(pipeline.recompress(w, 80), members)), labels[k]
        assert not torch.equal(rows[k], rows[0]), labels[k - 1]
    # the origin and the fill reach the calls; geometry alone gives (rows, labels) as well
    rows, labels = ensemble.stress_batch(raws, members, [], crops=[90], rotations=[7.5], crop_origin="topleft", rotate_fill="black")
    assert labels == ["crop90", "rot075"] and rows.shape == (3, 1, 3)
    assert torch.equal(rows[1], ensemble._score_batch(pipeline.crop(batch, 90, "topleft"), members))
    assert torch.equal(rows[2], ensemble._score_batch(pipeline.rotate(batch, 7.5, "black"), members))
    assert isinstance(ensemble.stress_batch(raws, members, [80], flips=(), crops=(), rotations=()), torch.Tensor)


# ---- CLI --------------------------------------------------------------------------------------------------------------------------------
def test_cli_flip_crop_rotate_and_jpeg_end_to_end(tmp_path):
    """--stress-flip h --stress-crop 80 --stress-rotate 7.5 --stress-jpeg 75: the CSVs of a plain run unchanged, the table's columns, the
    settings of stress.json"""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, zoo
    from vipcup_amd import main as cli
    names = _write_set(tmp_path, 4)
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS["resnet_rs50"].ckpt_name, [zoo.MEMBERS["resnet_rs50"].input_hw] * 2, 0]]))
    extra = ["--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "4"]
    csv = str(tmp_path / "test.csv")
    cli.main([csv, str(tmp_path / "o0.csv"), "--scores-out", str(tmp_path / "s0.csv"), *extra])
    cli.main([csv, str(tmp_path / "o1.csv"), "--scores-out", str(tmp_path / "s1.csv"), *extra, "--stress-flip", "h", "--stress-crop", "80",
              "--stress-rotate", "7.5", "--stress-jpeg", "75", "--stress-out", str(tmp_path / "stress.csv")])
    assert (tmp_path / "o0.csv").read_bytes() == (tmp_path / "o1.csv").read_bytes()
    assert (tmp_path / "s0.csv").read_bytes() == (tmp_path / "s1.csv").read_bytes()
    labels = ["q75", "fliph", "fliph_q75", "crop80", "crop80_q75", "rot075", "rot075_q75"]
    table = pd.read_csv(tmp_path / "stress.csv", dtype={"flips_at": str, "flips": str}, keep_default_na=False)
    assert list(table.columns) == ["filename", "p", "decision"] + [f"p_{v}" for v in labels] + [f"decision_{v}" for v in labels] + \
        ["stable", "flips_at", "flips"]
    assert table.filename.tolist() == sorted(names)
    plain = pd.read_csv(tmp_path / "s0.csv")
    cols = [c for c in plain.columns if c not in ("filename", "ensemble_mean")]
    uniq, p, dec = ensemble.aggregate(plain.filename.tolist(), np.stack([plain[c].to_numpy(np.float32) for c in cols]))
    assert uniq == table.filename.tolist() and np.array_equal(table.p.to_numpy(np.float32), p)
    assert np.array_equal(table.decision.to_numpy(np.float32), dec)
    p_all = np.stack([table[f"p_{v}"].to_numpy(np.float32) for v in labels], axis=1)
    assert np.isfinite(p_all).all() and (p_all != table.p.to_numpy(np.float32)[:, None]).any(axis=0).all(), "a variant scored the plain pixels"
    dv = np.stack([table[f"decision_{v}"].to_numpy(np.float32) for v in labels], axis=1)
    differs = dv != table.decision.to_numpy(np.float32)[:, None]
    assert table.stable.tolist() == [int(not r.any()) for r in differs]
    assert table.flips.tolist() == [";".join(v for v, f in zip(labels, r) if f) for r in differs]
    info = json.loads((tmp_path / "stress.json").read_text())
    assert info["variants"] == labels and info["qualities"] == [75] and info["n_files"] == len(names)
    st = info["settings"]
    assert st["flips"] == ["h"] and st["crops"] == [80] and st["crop_origin"] == "centre" and st["rotations"] == [7.5] and st["rotate_fill"] == "crop"
    assert st["qualities"] == [75] and "scales" not in st and "blur_sigmas" not in st and len(st["members"]) == 1
