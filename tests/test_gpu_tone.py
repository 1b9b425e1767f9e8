"""GPU: the tone stress tests - csrc/tone.hip (``pipeline.tone`` and ``autocontrast`` / ``equalize`` / ``clahe`` on top of it, and the three
entry points one by one) against the numpy restatement of tests/_tone_ref.py, which tests/test_tone_cpu.py holds against Pillow; the
``stress_batch`` rows and chains against the ``pipeline`` calls they stand for; one ``main.py --stress-equalize --stress-clahe`` run.
Every comparison is exact.  One mixed-size batch: grids of 2 x 3, 8 x 8, 1 x 8, 8 x 4, 1 x 1 (twice), 1 x 8 and 4 x 8 tiles at grid 8, image
tiles of 16..38 pixels that straddle the kernel's 128 x 8 pixel workgroups, a one-pixel image, and slots padded by 0 and by 1 pixel,
so that rows start at every byte phase."""
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
from tests import _parity as P  # noqa: E402
from tests import _tone_ref as R  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402

SIZES = [(37, 53), (200, 200), (15, 300), (129, 64), (16, 16), (1, 1), (8, 131), (64, 257)]           # (height, width)
# (mode, the argument of pipeline.tone, the restatement's parameter)
VARIANTS = [("autocontrast", 0, 0), ("autocontrast", 2, 2), ("autocontrast", 49, 49), ("autocontrast_luma", 2, 2), ("equalize", None, None),
            ("clahe", 1.0, 10), ("clahe", 2.0, 20), ("clahe", 9.9, 99)]
CAP = 1 << 26                                                                                    # the per-image pixel cap


@functools.lru_cache(maxsize=None)
def _images():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    rng = np.random.default_rng(20222)
    out = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in SIZES]
    decoded = pipeline.decode_images([synth_jpeg(103)])                                          # a JPEG-decoded synthetic image
    assert decoded.sizes_host == [(200, 200)]
    out[1] = decoded.rgb[0].cpu().numpy().copy()
    out[2] = (out[2] // 3 + 40).astype(np.uint8)                                                 # low range
    out[3] = np.clip(rng.normal(110, 12, SIZES[3] + (3,)), 0, 255).astype(np.uint8)              # narrow
    out[6] = np.full(SIZES[6] + (3,), 91, np.uint8)                                              # flat
    out[7] = (out[7] // 3 + 40).astype(np.uint8)
    for px in out:
        px.setflags(write=False)
    return tuple(out)


def _batch(pad: int = 0, fill=None):
    """a DecodedBatch holding the images in slots of the largest size (+ pad), the rest of every slot noise (or ``fill``)"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    imgs = _images()
    maxH, maxW = max(h for h, _ in SIZES) + pad, max(w for _, w in SIZES) + pad
    rgb = np.random.default_rng(6).integers(0, 256, (len(imgs), maxH, maxW, 3), dtype=np.uint8)
    if fill is not None:
        rgb[:] = fill
    for i, im in enumerate(imgs):
        rgb[i, :im.shape[0], :im.shape[1]] = im
    return pipeline.DecodedBatch(torch.from_numpy(rgb).cuda(), torch.tensor(SIZES, dtype=torch.int32, device="cuda"), list(SIZES))


@functools.lru_cache(maxsize=None)
def _want(mode, param, grid):
    """the restatement's pixels of every image, computed once"""
    out = [R.tone(im, mode, param, grid) for im in _images()]
    for px in out:
        px.setflags(write=False)
    return tuple(out)


def _check(out, want, what, pad_value=0):
    """``out`` (a DecodedBatch, or a numpy slot array) == ``want`` on every image's pixels, ``pad_value`` everywhere else"""
    if not isinstance(out, np.ndarray):
        assert out.sizes_host == list(SIZES) and out.sizes.cpu().tolist() == [list(s) for s in SIZES], what
        out = out.rgb.cpu().numpy()
    inside = np.zeros(out.shape[:3], bool)
    for i, (px, (h, w)) in enumerate(zip(want, SIZES)):
        bad = int((out[i, :h, :w] != px).any(axis=2).sum())
        assert bad == 0, f"{what}: image {i} {(h, w)}: {bad} pixels differ from the restatement"
        inside[i, :h, :w] = True
    assert (out[~inside] == pad_value).all(), f"{what}: written outside an image"


# ---- histograms -------------------------------------------------------------------------------------------------------------------------
def test_histograms_equal_bincount_per_tile():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    assert [pipeline.tone_grid(h, w, 8) for h, w in SIZES] == [(2, 3), (8, 8), (1, 8), (8, 4), (1, 1), (1, 1), (1, 8), (4, 8)]
    batch, padded = _batch(1), _batch(1, fill=255)
    for grid in (8, 3, 1):
        for channels in (3, 1):
            got = pipeline.tone_histograms(batch, grid, channels)
            slots = max(gy * gx for gy, gx in (pipeline.tone_grid(h, w, grid) for h, w in SIZES))
            assert got.dtype == torch.int32 and tuple(got.shape) == (len(SIZES), slots, channels, 256)
            assert torch.equal(got, pipeline.tone_histograms(padded, grid, channels)), "the slots' padding was read"
            assert torch.equal(got, pipeline.tone_histograms(batch, grid, channels)), "not reproducible"
            got = got.cpu().numpy()
            for i, im in enumerate(_images()):
                want = R.tile_histograms(im, grid, channels)
                assert np.array_equal(got[i, :len(want)], want), (grid, channels, i)
                assert not got[i, len(want):].any(), "a slot without a tile is not zero"
                whole = [R.hist256(im[..., c]) for c in range(3)] if channels == 3 else [R.hist256(R.luma(im))]
                assert np.array_equal(got[i].sum(0), np.stack(whole)), (grid, channels, i)


# ---- tables from synthetic histograms ---------------------------------------------------------------------------------------------------
def _tables(pipeline, hist, mode, arg=None):
    """``vip_tone_lut_u8`` on host histograms ``[n, slots, C, 256]``"""
    return pipeline.tone_tables(torch.from_numpy(np.ascontiguousarray(hist, np.int32)).cuda(), mode, arg).cpu().numpy()


def test_autocontrast_tables_for_every_pair_of_levels():
    """all 32 640 (lo, hi) as two-bin histograms, three to an 'image': the only check of the float64 path on the device, no exemptions"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    pairs, want = R.autocontrast_tables_all_pairs()
    assert len(pairs) == 32640 == 3 * 10880
    hist = np.zeros((len(pairs), 256), np.int32)
    hist[np.arange(len(pairs)), pairs[:, 0]] = 3
    hist[np.arange(len(pairs)), pairs[:, 1]] = 5
    got = _tables(pipeline, hist.reshape(10880, 1, 3, 256), "autocontrast", 0).reshape(-1, 256)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} of 32640 tables differ, first (lo, hi) = {pairs[bad[0]].tolist()}"
    got = _tables(pipeline, hist.reshape(-1, 1, 1, 256)[::7], "autocontrast_luma", 0).reshape(-1, 256)
    assert np.array_equal(got, want[::7])


def test_tables_at_the_pixel_cap_and_at_the_edges():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    rng = np.random.default_rng(8)
    big = np.zeros((4, 256), np.int64)
    big[0, [10, 100, 200, 255]] = [CAP // 2, CAP // 4, CAP // 4 - 1, 1]
    big[1] = rng.multinomial(CAP, rng.dirichlet(np.ones(256)))
    big[2, 7] = CAP                                                                   # one bin: the identity
    edge = CAP * 49 // 100 - 5                                                        # cut off whole at cutoff 49 only: lo and hi move
    big[3, [0, 100, 180, 255]] = [edge, (CAP - 2 * edge) // 2, CAP - 2 * edge - (CAP - 2 * edge) // 2, edge]
    assert (big.sum(1) == CAP).all() and CAP * 49 > 1 << 31
    for cutoff in (0, 2, 49):
        want = np.array([R.autocontrast_table(h, cutoff) for h in big], np.uint8)
        got = _tables(pipeline, np.repeat(big, 3, 0).reshape(4, 1, 3, 256), "autocontrast", cutoff)
        assert np.array_equal(got, np.repeat(want, 3, 0).reshape(4, 3, 256)), cutoff
        assert np.array_equal(_tables(pipeline, big.reshape(4, 1, 1, 256), "autocontrast_luma", cutoff)[:, 0], want), cutoff
        # the same counts spread over four slots: the table comes from their sum
        parts = np.stack([big // 4, big // 4, big // 4, big - 3 * (big // 4)], axis=1)
        assert np.array_equal(_tables(pipeline, parts.reshape(4, 4, 1, 256), "autocontrast_luma", cutoff)[:, 0], want), cutoff
    assert len({tuple(R.autocontrast_table(big[3], c)) for c in (0, 2, 49)}) > 1 and R.autocontrast_table(big[2], 2) == list(range(256))
    # equalisation: step 0, step 1, a single bin, nothing at all, a 200 x 200 image, the cap
    eq = np.zeros((6, 256), np.int64)
    eq[0, [3, 9, 200]] = [100, 154, 7]                                                # (261 - 7) // 255 = 0
    eq[1] = np.bincount(rng.integers(0, 256, 400), minlength=256)                     # 20 x 20: step 1, entries above 255 are cut
    eq[2, 77] = 40000
    eq[4] = np.bincount(np.clip(rng.normal(110, 20, 40000), 0, 255).astype(int), minlength=256)
    eq[5] = big[1]
    nz = eq[1][eq[1] > 0]
    assert (eq[0].sum() - 7) // 255 == 0 and (eq[1].sum() - nz[-1]) // 255 == 1
    want = np.array([R.equalize_table(h) for h in eq], np.uint8)
    assert want[0].tolist() == want[2].tolist() == want[3].tolist() == list(range(256)) and want[1].max() == 255
    got = _tables(pipeline, np.repeat(eq, 3, 0).reshape(6, 1, 3, 256), "equalize")
    assert np.array_equal(got, np.repeat(want, 3, 0).reshape(6, 3, 256))


def _clahe_case(A, clip, E, rng):
    """a histogram of area A whose part above ``clip`` is exactly E"""
    rest = A - clip - E
    h = np.full(256, rest // 255, np.int64)
    h[:rest % 255] += 1
    assert h.max() <= clip
    h[255] = clip + E
    assert h.sum() == A
    return rng.permutation(h)


def test_clahe_tables():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    rng = np.random.default_rng(9)
    for tt in (10, 20, 99):
        clip = max(1, tt * 40000 // 2560)
        cases = [np.ones(256, np.int64),                                              # A = 256
                 np.bincount(rng.integers(100, 120, 256), minlength=256),             # A = 256, narrow
                 np.bincount(np.clip(rng.normal(110, 9, 40000), 0, 255).astype(int), minlength=256),      # a whole 200 x 200 image
                 _clahe_case(40000, clip, 512, rng), _clahe_case(40000, clip, 511, rng),                   # E % 256 = 0 and 255
                 np.zeros(256, np.int64),                                             # a slot without a tile
                 np.eye(256, dtype=np.int64)[200] * CAP, rng.multinomial(CAP, rng.dirichlet(np.ones(256)))]
        for h, e in zip(cases[3:5], (0, 255)):
            assert (h.sum() - np.minimum(h, clip).sum()) % 256 == e
        want = np.array([R.clahe_table(h, tt) for h in cases], np.uint8)
        got = _tables(pipeline, np.stack(cases).reshape(1, len(cases), 1, 256), "clahe", tt / 10)
        assert tuple(got.shape) == (1, len(cases), 256) and np.array_equal(got[0], want), tt
        assert want[5].tolist() == list(range(256))


# ---- the variants end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 1])
def test_variants_equal_the_restatement(pad):
    """every variant through ``pipeline`` at grid 8 and grid 3; the source stays, the result is new and repeatable, and both placements
    of the CLAHE tables write the same bytes"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    batch = _batch(pad)
    before = batch.rgb.clone()
    for mode, arg, param in VARIANTS:
        for grid in (8, 3):
            out = pipeline.tone(batch, mode, arg, grid)
            _check(out, _want(mode, param, grid if mode == "clahe" else 8), (mode, arg, grid, pad))
            assert out.rgb.data_ptr() != batch.rgb.data_ptr() and out.rgb.shape == batch.rgb.shape
            assert torch.equal(pipeline.tone(batch, mode, arg, grid).rgb, out.rgb), (mode, arg, grid)
            if mode == "clahe":
                for placement in (0, 1):
                    placed = pipeline._tone_into(batch, mode, arg, grid, torch.zeros_like(batch.rgb), placement)
                    assert torch.equal(placed.rgb, out.rgb), (arg, grid, placement)
    assert torch.equal(batch.rgb, before), "a tone call changed its input"
    assert torch.equal(pipeline.autocontrast(batch, 2).rgb, pipeline.tone(batch, "autocontrast", 2).rgb)
    assert torch.equal(pipeline.autocontrast(batch, 2, luma=True).rgb, pipeline.tone(batch, "autocontrast_luma", 2).rgb)
    assert torch.equal(pipeline.equalize(batch).rgb, pipeline.tone(batch, "equalize").rgb)
    assert torch.equal(pipeline.clahe(batch, 2.0, 3).rgb, pipeline.tone(batch, "clahe", 2.0, 3).rgb)
    flat = pipeline.equalize(batch).rgb[6, :8, :131]
    assert bool((flat == 91).all()), "a flat image has nothing to stretch"


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("mode,arg,param,placement", [("autocontrast", 2, 2, None), ("autocontrast_luma", 2, 2, None), ("clahe", 2.0, 20, 0),
                                                      ("clahe", 2.0, 20, 1)])
def test_c_abi_into_a_larger_destination_keeps_every_other_byte(mode, arg, param, placement):
    """a destination whose slots are larger than the source's, at another pitch and not word-aligned, prefilled with a marker: the pixels
    equal the restatement and every byte outside the images - guard bands before and after included - still holds the marker"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    lib = _abi.lib()
    batch = _batch(1)
    n, srcH, srcW, _ = batch.rgb.shape
    maxH, maxW = srcH + 2, srcW + 5
    body = n * maxH * maxW * 3
    m = pipeline.TONE_MODES[mode]
    grid = 8
    hist = pipeline.tone_histograms(batch, grid, 3 if m in (0, 2) else 1)
    lut = pipeline.tone_tables(hist, mode, arg)
    for guard in (4096, 4099):
        buf = torch.full((body + 2 * guard,), 0xAB, dtype=torch.uint8, device="cuda")
        dst = buf[guard:guard + body].view(n, maxH, maxW, 3)
        args = [_ptr(batch.rgb), _ptr(batch.sizes), srcH, srcW, _ptr(dst), maxH, maxW, _ptr(lut), m, grid, int(hist.shape[1])]
        if placement is None:
            st = lib.vip_tone_apply_rgb_u8(*args, n, None)
        else:
            st = lib.vip_tone_apply_rgb_u8_placed(*args, placement, n, None)
        torch.cuda.synchronize()
        assert st == 0, lib.vip_last_error()
        flat = buf.cpu().numpy()
        assert (flat[:guard] == 0xAB).all() and (flat[guard + body:] == 0xAB).all(), "written outside the buffer"
        _check(flat[guard:guard + body].reshape(n, maxH, maxW, 3), _want(mode, param, grid), (mode, guard), pad_value=0xAB)


def test_entry_points_refuse_bad_arguments_without_a_launch():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    lib = _abi.lib()
    batch = _batch()
    n, maxH, maxW, _ = batch.rgb.shape
    dst = torch.full_like(batch.rgb, 0xAB)
    hist = torch.full((n, 64, 3, 256), 7, dtype=torch.int32, device="cuda")
    lut = torch.full((n, 64, 256), 0xCD, dtype=torch.uint8, device="cuda")
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)        # noqa: E731
    good = [_ptr(batch.rgb), _ptr(batch.sizes), n, maxH, maxW, 8, 3, _ptr(hist), 64, None]
    for k, v, code, word in [(0, None, -1, b"null"), (1, None, -1, b"null"), (7, None, -1, b"null"), (2, 0, -1, b"bad size"),
                             (3, 0, -1, b"bad size"), (4, (1 << 26) + 1, -1, b"bad size"), (5, 0, -1, b"grid"), (5, 17, -1, b"grid"),
                             (6, 2, -1, b"channels"), (8, 0, -1, b"slots"), (8, 257, -1, b"slots"), (1, off(batch.sizes, 2), -2, b"4-byte"),
                             (7, off(hist, 2), -2, b"4-byte")]:
        args = list(good)
        args[k] = v
        assert lib.vip_tone_hist_u8(*args) == code and word in lib.vip_last_error(), ("hist", k, v)
    good = [_ptr(hist), n, 64, 0, 2, _ptr(lut), None]
    for k, v, code, word in [(0, None, -1, b"null"), (5, None, -1, b"null"), (1, 0, -1, b"bad size"), (2, 0, -1, b"bad size"),
                             (2, 257, -1, b"bad size"), (3, 4, -1, b"mode"), (3, -1, -1, b"mode"), (4, 50, -1, b"cutoff"), (4, -1, -1, b"cutoff"),
                             (0, off(hist, 1), -2, b"4-byte"), (5, off(lut, 2), -2, b"4-byte")]:
        args = list(good)
        args[k] = v
        assert lib.vip_tone_lut_u8(*args) == code and word in lib.vip_last_error(), ("lut", k, v)
    for mode, param, word in [(1, 50, b"cutoff"), (2, 1, b"eq"), (3, 9, b"clip limit"), (3, 100, b"clip limit")]:
        assert lib.vip_tone_lut_u8(_ptr(hist), n, 64, mode, param, _ptr(lut), None) == -1 and word in lib.vip_last_error(), (mode, param)
    good = [_ptr(batch.rgb), _ptr(batch.sizes), maxH, maxW, _ptr(dst), maxH, maxW, _ptr(lut), 3, 8, 64, n, None]
    for k, v, code, word in [(0, None, -1, b"null"), (1, None, -1, b"null"), (4, None, -1, b"null"), (7, None, -1, b"null"),
                             (11, 0, -1, b"bad size"), (2, 0, -1, b"bad size"), (6, -1, -1, b"bad size"), (4, _ptr(batch.rgb), -1, b"overlap"),
                             (4, off(batch.rgb, 3 * maxW), -1, b"overlap"), (8, 4, -1, b"mode"), (9, 0, -1, b"grid"), (9, 17, -1, b"grid"),
                             (10, 0, -1, b"slots"), (1, off(batch.sizes, 2), -2, b"4-byte"), (7, off(lut, 1), -2, b"4-byte"),
                             (7, off(lut, 2), -2, b"4-byte")]:
        args = list(good)
        args[k] = v
        assert lib.vip_tone_apply_rgb_u8(*args) == code and word in lib.vip_last_error(), ("apply", k, v)
    assert lib.vip_tone_apply_rgb_u8_placed(*good[:11], 2, n, None) == -1 and b"placement" in lib.vip_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 0xAB).all()) and bool((hist == 7).all()) and bool((lut == 0xCD).all()), "a refused call wrote something"


# ---- stress_batch and chains --------------------------------------------------------------------------------------------------------
def _write_set(d, n):
    names = []
    for i in P.e2e_image_ids(n):
        name = f"img_{i:05d}.jpg"
        (d / name).write_bytes(synth_jpeg(i))
        names.append(name)
    (d / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
    return names


def test_stress_batch_rows_and_chains(tmp_path):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, pipeline, zoo
    names = _write_set(tmp_path, 3)
    members = [(zoo.MEMBERS["resnet_rs50"], zoo.FoldMean([P.gpu_member("resnet_rs50")[1]]))]
    raws = [(tmp_path / n).read_bytes() for n in names]
    batch = pipeline.decode_images(raws)
    chains = ["eq+q80", "ac02+q80", "acl02+q80", "clahe20+q80", "r50+clahe20+q75"]
    keywords = dict(autocontrasts=[2], autocontrast_lumas=[2], equalize=True, clahes=[2.0], clahe_grid=3)
    rows, labels = ensemble.stress_batch(raws, members, [80], sharpens=[80], chains=chains, **keywords)
    tone = ["ac02", "acl02", "eq", "clahe20"]
    assert labels == ensemble.stress_labels([80], sharpens=[80], chains=chains, **keywords) == \
        ["q80", "shp080", "shp080_q80"] + [x for v in tone for x in (v, f"{v}_q80")] + chains and rows.shape == (1 + len(labels), 1, 3)
    row = lambda label: rows[1 + labels.index(label)]      # noqa: E731
    assert torch.equal(rows[0], ensemble._score_batch(batch, members))
    toned = [pipeline.autocontrast(batch, 2), pipeline.autocontrast(batch, 2, luma=True), pipeline.equalize(batch), pipeline.clahe(batch, 2.0, 3)]
    for label, t in zip(tone, toned):
        assert torch.equal(row(label), ensemble._score_batch(t, members)), label
        assert torch.equal(row(f"{label}_q80"), ensemble._score_batch(pipeline.recompress(t, 80), members)), label
        assert torch.equal(row(f"{label}+q80"), row(f"{label}_q80")), label
        assert not torch.equal(row(label), rows[0]), label
    by_hand = pipeline.recompress(pipeline.clahe(pipeline.rescale(batch, 50), 2.0, 3), 75)
    assert torch.equal(pipeline.apply_chain(batch, "r50+clahe20+q75", clahe_grid=3).rgb, by_hand.rgb)
    assert torch.equal(row("r50+clahe20+q75"), ensemble._score_batch(by_hand, members))
    assert not torch.equal(pipeline.apply_chain(batch, "r50+clahe20+q75").rgb, by_hand.rgb), "clahe_grid did not reach the step"
    # a tone step measures the batch as it reaches that step
    assert torch.equal(pipeline.apply_chain(batch, "gray+eq").rgb, pipeline.equalize(pipeline.gray(batch)).rgb)
    # tone alone gives (rows, labels) as well; nothing of it leaves today's result as it is
    rows2, labels2 = ensemble.stress_batch(raws, members, [], equalize=True)
    assert labels2 == ["eq"] and torch.equal(rows2[1], row("eq"))
    plain = ensemble.stress_batch(raws, members, [80], autocontrasts=(), autocontrast_lumas=(), equalize=False, clahes=())
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, rows[:2])


# ---- CLI --------------------------------------------------------------------------------------------------------------------------------
def test_cli_equalize_clahe_and_jpeg_end_to_end(tmp_path):
    """--stress-equalize --stress-clahe 2 --stress-jpeg 80: the CSVs of a plain run unchanged, the table's columns, the settings"""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import zoo
    from vipcup_amd import main as cli
    names = _write_set(tmp_path, 8)
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS["resnet_rs50"].ckpt_name, [zoo.MEMBERS["resnet_rs50"].input_hw] * 2, 0]]))
    extra = ["--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "8"]
    csv = str(tmp_path / "test.csv")
    cli.main([csv, str(tmp_path / "o0.csv"), "--scores-out", str(tmp_path / "s0.csv"), *extra])
    cli.main([csv, str(tmp_path / "o1.csv"), "--scores-out", str(tmp_path / "s1.csv"), *extra, "--stress-equalize", "--stress-clahe", "2",
              "--stress-jpeg", "80", "--stress-out", str(tmp_path / "stress.csv")])
    assert (tmp_path / "o0.csv").read_bytes() == (tmp_path / "o1.csv").read_bytes()
    assert (tmp_path / "s0.csv").read_bytes() == (tmp_path / "s1.csv").read_bytes()
    labels = ["q80", "eq", "eq_q80", "clahe20", "clahe20_q80"]
    table = pd.read_csv(tmp_path / "stress.csv", dtype={"flips_at": str, "flips": str}, keep_default_na=False)
    assert list(table.columns) == ["filename", "p", "decision"] + [f"p_{v}" for v in labels] + [f"decision_{v}" for v in labels] + \
        ["stable", "flips_at", "flips"]
    assert table.filename.tolist() == sorted(names)
    p_all = np.stack([table[f"p_{v}"].to_numpy(np.float32) for v in labels], axis=1)
    assert np.isfinite(p_all).all() and (p_all != table.p.to_numpy(np.float32)[:, None]).any(axis=0).all(), "a variant scored the plain pixels"
    info = json.loads((tmp_path / "stress.json").read_text())
    assert info["variants"] == labels and info["qualities"] == [80] and info["n_files"] == len(names)
    st = info["settings"]
    assert st["autocontrast_cutoffs"] == [] and st["autocontrast_luma_cutoffs"] == [] and st["equalize"] is True
    assert st["clahe_limits"] == [2.0] and st["clahe_grid"] == 8 and st["qualities"] == [80] and len(st["members"]) == 1
