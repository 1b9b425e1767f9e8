"""GPU: the noise stress tests - csrc/noise.hip (``pipeline.noise`` and ``gaussian_noise`` / ``mono_noise`` / ``speckle`` / ``impulse`` on
top of it) against the integer restatement of tests/_noise_ref.py pixel by pixel, ``stress_batch`` rows against the ``pipeline`` calls they
stand for, and one ``main.py --stress-noise --stress-impulse`` run.  Every comparison is exact: the kernel is integer arithmetic from a
counter-based generator, and the member passes see the same pixels in the same batch positions.  The batch is test_gpu_colour.py's: 1- and
7-pixel rows (shorter than a dword group), sizes that are no multiple of the 128 x 8 tile, a 300-pixel row against a wider slot, and slot
pitches padded by 0 and by 3 pixels, so that rows start at every byte phase.  Its 75 (78 when padded) tiles per slot are no multiple of
the 8 consecutive tiles a workgroup takes when the table sits in LDS, so groups straddle images; the flat-image batch's 90 tiles leave
a last group of 2."""
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
from tests import _noise_ref as R  # noqa: E402
from tests import _parity as P  # noqa: E402
from tests._jpeg_enc_ref import content  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402

SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (37, 53), (129, 64), (200, 200), (64, 300)]           # (height, width)
CASES = [("gaussian", 3), ("gaussian", 50), ("mono", 0.5), ("mono", 50), ("speckle", 20), ("speckle", 50), ("impulse", 0.1), ("impulse", 50)]
SEED = 20221
KEYS = [7, 0, 0xFFFFFFFF, 0x80000000, 12345, 99, 0xCBF43926, 3]


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
def _want(kind, value):
    """the restatement's pixels of every image under (kind, value) with SEED and the image's KEYS entry, computed once"""
    out = [R.apply(im, kind, value, SEED, key) for im, key in zip(_images(), KEYS)]
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


def test_every_mode_equals_the_restatement():
    """the four modes at two amounts each, the largest included, through ``pipeline``, slots at an even and an odd pitch; the source
    stays, the result is new and repeatable; both table placements write the same bytes"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    named = {"gaussian": pipeline.gaussian_noise, "mono": pipeline.mono_noise, "speckle": pipeline.speckle, "impulse": pipeline.impulse}
    for pad in (0, 3):
        batch = _batch(pad)
        before = batch.rgb.clone()
        keys_d = pipeline.noise_keys_device(batch, KEYS)
        for kind, value in CASES:
            out = pipeline.noise(batch, kind, value, SEED, KEYS)
            _check(out, _want(kind, value), (kind, value, pad))
            assert out.rgb.data_ptr() != batch.rgb.data_ptr() and out.rgb.shape == batch.rgb.shape
            assert torch.equal(named[kind](batch, value, SEED, keys_d).rgb, out.rgb), (kind, value)
            for placement in (0, 1):
                dst = torch.zeros_like(batch.rgb)
                pipeline._noise_into(batch, pipeline.NOISE_KINDS[kind], pipeline.noise_amount(kind, value), SEED, keys_d, dst, placement)
                assert torch.equal(dst, out.rgb), (kind, value, placement)
        assert torch.equal(batch.rgb, before), "a noise call changed its input"
    # the default keys are the batch positions, the default seed is 0
    out = pipeline.gaussian_noise(batch, 3)
    _check(out, [R.apply(im, "gaussian", 3, 0, i) for i, im in enumerate(_images())], "default seed and keys")


def test_an_image_keeps_its_noise_at_another_batch_index_and_pitch():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    a = pipeline.noise(_batch(0), "gaussian", 10, SEED, KEYS)
    order = [6, 4, 7, 5]                                                              # a smaller batch: another slot pitch, other indices
    b = pipeline.noise(_batch(1, tuple(_images()[i] for i in order)), "gaussian", 10, SEED, [KEYS[i] for i in order])
    for j, i in enumerate(order):
        h, w = SIZES[i]
        assert torch.equal(b.rgb[j, :h, :w], a.rgb[i, :h, :w]), i
    other = pipeline.noise(_batch(0), "gaussian", 10, SEED, [k ^ 1 for k in KEYS])
    reseeded = pipeline.noise(_batch(0), "gaussian", 10, SEED + 1, KEYS)
    for i, (h, w) in enumerate(SIZES):
        if h * w >= 4:                                                                # a 1 x 1 image may meet the same three samples
            assert not torch.equal(other.rgb[i, :h, :w], a.rgb[i, :h, :w]), i
            assert not torch.equal(reseeded.rgb[i, :h, :w], a.rgb[i, :h, :w]), i


def _abi_call(lib, batch, dst, mode, amount, keys_d, table_d, seed=SEED):
    n, maxH, maxW, _ = batch.rgb.shape
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())              # noqa: E731
    st = lib.vip_noise_rgb_u8(ptr(batch.rgb), ptr(batch.sizes), maxH, maxW, ptr(dst), int(dst.shape[1]), int(dst.shape[2]), mode, amount,
                              seed, ptr(keys_d), ptr(table_d), n, None)
    torch.cuda.synchronize()
    return st


def _table_d():
    from vipcup_amd import pipeline
    return torch.from_numpy(pipeline.noise_table().copy()).cuda()


@pytest.mark.parametrize("kind,value", [("gaussian", 3), ("speckle", 50), ("impulse", 50)])
def test_c_abi_into_a_larger_destination_keeps_every_other_byte(kind, value):
    """a destination whose slots are larger than the source's, at another pitch and not word-aligned, prefilled with a marker: the pixels
    equal the restatement and every byte outside the images - guard bands before and after included - still holds the marker"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    lib = _abi.lib()
    batch = _batch(3)
    n = len(SIZES)
    maxH, maxW = batch.rgb.shape[1] + 2, batch.rgb.shape[2] + 5
    body = n * maxH * maxW * 3
    keys_d = pipeline.noise_keys_device(batch, KEYS)
    table_d = None if kind == "impulse" else _table_d()                               # the impulses take no table
    for guard in (4096, 4099):
        buf = torch.full((body + 2 * guard,), 0xAB, dtype=torch.uint8, device="cuda")
        dst = buf[guard:guard + body].view(n, maxH, maxW, 3)
        assert _abi_call(lib, batch, dst, pipeline.NOISE_KINDS[kind], R.amount(kind, value), keys_d, table_d) == 0, lib.vip_last_error()
        flat = buf.cpu().numpy()
        assert (flat[:guard] == 0xAB).all() and (flat[guard + body:] == 0xAB).all(), "written outside the buffer"
        _check(flat[guard:guard + body].reshape(n, maxH, maxW, 3), _want(kind, value), (kind, value, guard), pad_value=0xAB)


def test_flat_images_reach_both_clamps():
    """all-white and all-black images at sigma 50 and speckle 50: a 32-bit overflow, a logical shift of a negative sum or a missing clamp
    shows here only"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    flat = tuple(np.full(s + (3,), v, np.uint8) for s, v in [((3, 5), 255), ((9, 130), 255), ((9, 130), 0), ((70, 33), 0), ((2, 2), 255)])
    sizes = [im.shape[:2] for im in flat]
    batch = _batch(1, flat)
    for kind, value in (("gaussian", 50), ("mono", 50), ("speckle", 50)):
        want = [R.apply(im, kind, value, SEED, 40 + i) for i, im in enumerate(flat)]
        assert want[1].max() == 255 and want[1].min() < 255 and want[2].min() == 0
        assert (want[2] == 0).all() if kind == "speckle" else want[2].max() > 0
        _check(pipeline.noise(batch, kind, value, SEED, [40, 41, 42, 43, 44]), want, (kind, value), sizes=sizes)
    assert R.apply(flat[1], "speckle", 50, SEED, 41).min() == 0, "the case should take white to the lower clamp"


def test_entry_point_refuses_bad_arguments_without_a_launch():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    lib = _abi.lib()
    batch = _batch()
    n, maxH, maxW, _ = batch.rgb.shape
    dst = torch.full_like(batch.rgb, 0xAB)
    keys_d, table_d = pipeline.noise_keys_device(batch, KEYS), _table_d()
    ptr = lambda t: C.c_void_p(t.data_ptr())              # noqa: E731
    good = [ptr(batch.rgb), ptr(batch.sizes), maxH, maxW, ptr(dst), maxH, maxW, 0, 768, SEED, ptr(keys_d), ptr(table_d), n, None]
    cases = [(0, None, -1, b"null"), (1, None, -1, b"null"), (4, None, -1, b"null"), (10, None, -1, b"null"), (11, None, -1, b"null"),
             (12, 0, -1, b"bad size"), (2, 0, -1, b"bad size"), (6, -1, -1, b"bad size"), (4, ptr(batch.rgb), -1, b"overlap"),
             (8, 127, -1, b"amount"), (8, 12801, -1, b"amount"), (8, -768, -1, b"amount"), (7, 4, -1, b"amount"), (7, -1, -1, b"amount"),
             (1, C.c_void_p(batch.sizes.data_ptr() + 2), -2, b"4-byte"), (10, C.c_void_p(keys_d.data_ptr() + 1), -2, b"4-byte"),
             (11, C.c_void_p(table_d.data_ptr() + 2), -2, b"4-byte")]
    for k, v, code, word in cases:
        args = list(good)
        args[k] = v
        assert lib.vip_noise_rgb_u8(*args) == code and word in lib.vip_last_error(), (k, v)
    for mode, amount in ((2, 2), (2, 129), (3, 4294966), (3, (1 << 31) + 1), (1, 0)):          # every mode's own range
        args = list(good)
        args[7], args[8] = mode, amount
        assert lib.vip_noise_rgb_u8(*args) == -1 and b"amount" in lib.vip_last_error(), (mode, amount)
    torch.cuda.synchronize()
    assert bool((dst == 0xAB).all()), "a refused call wrote pixels"
    assert lib.vip_noise_rgb_u8(*good) == 0, lib.vip_last_error()                              # and the same arguments, valid
    torch.cuda.synchronize()
    _check(dst.cpu().numpy(), _want("gaussian", 3), "after the refusals", pad_value=0xAB)


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
    """one ResNet-RS-50 member, three images"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, pipeline, zoo
    names = _write_set(tmp_path, 3)
    members = [(zoo.MEMBERS["resnet_rs50"], zoo.FoldMean([P.gpu_member("resnet_rs50")[1]]))]
    raws = [(tmp_path / n).read_bytes() for n in names]
    batch = pipeline.decode_images(raws)
    keys = pipeline.noise_keys(names)
    kw = dict(noise_seed=5, noise_keys=keys)
    rows, labels = ensemble.stress_batch(raws, members, [75], noises=[10, 3], impulses=[1], **kw)
    assert labels == ensemble.stress_labels([75], noises=[10, 3], impulses=[1]) == \
        ["q75", "n030", "n030_q75", "n100", "n100_q75", "imp010", "imp010_q75"] and rows.shape == (8, 1, 3)
    assert torch.equal(rows[0], ensemble._score_batch(batch, members))
    assert torch.equal(rows[:2], ensemble.stress_batch(raws, members, [75]))
    noisy = [pipeline.gaussian_noise(batch, 3, 5, keys), pipeline.gaussian_noise(batch, 10, 5, keys), pipeline.impulse(batch, 1, 5, keys)]
    for k, c in zip(range(2, 8, 2), noisy):
        assert torch.equal(rows[k], ensemble._score_batch(c, members)), labels[k - 1]
        assert torch.equal(rows[k + 1], ensemble._score_batch(pipeline.recompress(c, 75), members)), labels[k]
        assert not torch.equal(rows[k], rows[0]), labels[k - 1]
    # noise alone gives (rows, labels) as well; the other variants in their order; the default seed and keys
    rows, labels = ensemble.stress_batch(raws, members, [], mono_noises=[3], speckles=[20], gray=True, flips=["h"])
    assert labels == ["fliph", "gray", "nm030", "spk20"] and rows.shape == (5, 1, 3)
    for k, c in enumerate([pipeline.flip(batch, "h"), pipeline.gray(batch), pipeline.mono_noise(batch, 3), pipeline.speckle(batch, 20)]):
        assert torch.equal(rows[k + 1], ensemble._score_batch(c, members)), labels[k]
    assert isinstance(ensemble.stress_batch(raws, members, [75], noises=(), mono_noises=(), speckles=(), impulses=(), noise_seed=9), torch.Tensor)


# ---- CLI --------------------------------------------------------------------------------------------------------------------------------
def test_cli_noise_impulse_and_jpeg_end_to_end(tmp_path):
    """--stress-noise 3 --stress-impulse 1 --stress-jpeg 75: the CSVs of a plain run unchanged, the table's columns, the settings; then
    the CSV rows reversed at --batch-size 2, so that every file changes its batch index and its place in the batch: every file keeps its p_n030.
    All runs use --batch-size 2: the members' convolutions are dispatched by B * Ho * Wo (csrc/conv_igemm.hip), so a score - the plain
    ``p`` as much as ``p_n030`` - is comparable bit for bit only between runs of one batch shape (measured: p of the first file 0.8234582
    at 4 per batch, 0.8234454 at 2, in either row order).  That the noisy PIXELS do not depend on the batch's size, index or pitch is
    ``test_an_image_keeps_its_noise_at_another_batch_index_and_pitch``."""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import zoo
    from vipcup_amd import main as cli
    names = _write_set(tmp_path, 4)
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS["resnet_rs50"].ckpt_name, [zoo.MEMBERS["resnet_rs50"].input_hw] * 2, 0]]))
    extra = ["--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "2"]
    flags = ["--stress-noise", "3", "--stress-impulse", "1", "--stress-jpeg", "75"]
    csv = str(tmp_path / "test.csv")
    cli.main([csv, str(tmp_path / "o0.csv"), "--scores-out", str(tmp_path / "s0.csv"), *extra])
    cli.main([csv, str(tmp_path / "o1.csv"), "--scores-out", str(tmp_path / "s1.csv"), *extra, *flags,
              "--stress-out", str(tmp_path / "stress.csv")])
    assert (tmp_path / "o0.csv").read_bytes() == (tmp_path / "o1.csv").read_bytes()
    assert (tmp_path / "s0.csv").read_bytes() == (tmp_path / "s1.csv").read_bytes()
    labels = ["q75", "n030", "n030_q75", "imp010", "imp010_q75"]
    table = pd.read_csv(tmp_path / "stress.csv", dtype={"flips_at": str, "flips": str}, keep_default_na=False)
    assert list(table.columns) == ["filename", "p", "decision"] + [f"p_{v}" for v in labels] + [f"decision_{v}" for v in labels] + \
        ["stable", "flips_at", "flips"]
    assert table.filename.tolist() == sorted(names)
    p_all = np.stack([table[f"p_{v}"].to_numpy(np.float32) for v in labels], axis=1)
    assert np.isfinite(p_all).all() and (p_all != table.p.to_numpy(np.float32)[:, None]).any(axis=0).all(), "a variant scored the plain pixels"
    info = json.loads((tmp_path / "stress.json").read_text())
    assert info["variants"] == labels and info["qualities"] == [75] and info["n_files"] == len(names)
    st = info["settings"]
    assert st["noise_sigmas"] == [3.0] and st["noise_mono_sigmas"] == [] and st["speckles"] == [] and st["impulses"] == [1.0]
    assert st["noise_seed"] == 0 and st["qualities"] == [75] and "gray" not in st and "noises" not in st and len(st["members"]) == 1
    # the rows reversed, two per batch: a file is keyed by its name, so its noise - and with it the score - is the same
    (tmp_path / "reversed.csv").write_text("filename\n" + "\n".join(reversed(names)) + "\n")
    cli.main([str(tmp_path / "reversed.csv"), str(tmp_path / "o2.csv"), *extra, *flags, "--stress-out", str(tmp_path / "stress2.csv")])
    again = pd.read_csv(tmp_path / "stress2.csv", dtype={"flips_at": str, "flips": str}, keep_default_na=False)
    assert again.filename.tolist() == table.filename.tolist()
    assert again.p_n030.tolist() == table.p_n030.tolist() and again.p_imp010_q75.tolist() == table.p_imp010_q75.tolist()
    assert info["settings"]["batch_size"] == 2
