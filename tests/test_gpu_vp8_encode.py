"""GPU: the lossy WebP re-save (csrc/vp8_encode.hip, ``pipeline.webp_recompress``, ``--stress-webp``, chain step ``w<Q>``).
The yardstick is the CPU check program (tests/fuzz/vp8_enc_check.cpp: the same arithmetic run serially, which
tests/test_vp8_encode_cpu.py holds to libwebp through a written file): the kernel's records, levels, coefficients, planes and
pixels equal it bit for bit.  Then the decoder's own reconstruction of what the encoder wrote, libwebp's decode of the file made from
the GPU's levels, independence of the batch, and the wiring up to the CLI.  Every comparison is exact."""
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
from tests import _vp8 as V  # noqa: E402
from tests import _vp8_enc as E  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402


def _batch(images):
    """a DecodedBatch of uint8 [h, w, 3] arrays, each in the top-left corner of its slot"""
    from vipcup_amd import pipeline
    sizes = [(im.shape[0], im.shape[1]) for im in images]
    maxH, maxW = max(h for h, _ in sizes), max(w for _, w in sizes)
    rgb = np.zeros((len(images), maxH, maxW, 3), np.uint8)
    for i, im in enumerate(images):
        rgb[i, :im.shape[0], :im.shape[1]] = im
    return pipeline.DecodedBatch(torch.from_numpy(rgb).cuda(), torch.tensor(sizes, dtype=torch.int32, device="cuda"), sizes)


def _encode(images, quality):
    """[Encoded] of a batch as the GPU gives it: the encode launch's buffers and ``webp_recompress``'s pixels"""
    from vipcup_amd import pipeline
    batch = _batch(images)
    enc = pipeline.webp_encode(batch, quality)
    out = pipeline.webp_recompress(batch, quality)
    torch.cuda.synchronize()
    stream, levels, scratch, rgb = enc.stream.cpu().numpy(), enc.levels.cpu().numpy(), enc.scratch.cpu().numpy(), out.rgb.cpu().numpy()
    assert out.sizes_host == batch.sizes_host and torch.equal(out.sizes, batch.sizes)
    res = []
    for i, d in enumerate(enc.desc):
        nmb = d.mb_w * d.mb_h
        a = d.stream_off + d.mb_off
        mbs = np.frombuffer(stream[a:a + nmb * 40].tobytes(), dtype=E.MB_DTYPE)
        a = d.stream_off + d.coef_off
        coefs = stream[a:a + nmb * 800].view(np.int16).reshape(nmb, 25, 16)
        first = d.plane_off // 384
        h, w = batch.sizes_host[i]
        assert not rgb[i, h:].any() and not rgb[i, :, w:].any()               # nothing outside the image
        res.append(E.Encoded(w, h, quality, enc.params.base_q, enc.params.filter_level, mbs, levels[first:first + nmb], coefs,
                             scratch[d.plane_off:d.plane_off + nmb * 384], rgb[i, :h, :w]))
    return res


def _same(name, got, want):
    assert (got.w, got.h, got.base_q, got.filter_level) == (want.w, want.h, want.base_q, want.filter_level), name
    assert got.mbs.tobytes() == want.mbs.tobytes(), (name, "records", np.flatnonzero(got.mbs != want.mbs)[:4])
    assert np.array_equal(got.levels, want.levels), (name, "levels")
    assert np.array_equal(got.coefs, want.coefs), (name, "coefficients")
    assert np.array_equal(got.planes, want.planes), (name, "planes", np.flatnonzero(got.planes != want.planes)[:4])
    assert np.array_equal(got.rgb, want.rgb), (name, "rgb", int(np.abs(got.rgb.astype(int) - want.rgb).max()))


LARGE = ("photo_224x224_q75", 75, None)                          # 14 x 14 macroblocks: its planes do not fit LDS


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """{name: (quality, image, Encoded by the check program)} over the CPU test's corpus and the large image, computed once"""
    items = E.cases() + [(LARGE[0], LARGE[1], E.image("photo", 224, 224))]
    exe = E.build_check(tmp_path_factory.mktemp("vp8_enc_check"))
    encs = E.run_check(exe, items, tmp_path_factory.mktemp("vp8_enc_cases"))
    return {name: (q, img, e) for (name, q, img), e in zip(items, encs)}


@pytest.mark.parametrize("quality", E.QUALITIES)
def test_kernel_equals_the_check_program(reference, quality):
    """(a) every case of the corpus, the cases of one quality as ONE mixed-size batch"""
    import vipcup_amd  # noqa: F401
    names = [n for n, (q, _, _) in reference.items() if q == quality and n != LARGE[0]]
    assert len(names) >= 5 and len({reference[n][1].shape for n in names}) >= 4
    got = _encode([reference[n][1] for n in names], quality)
    for name, g in zip(names, got):
        _same(name, g, reference[name][2])


def test_mixed_batch_of_five_and_lds_next_to_scratch_planes(reference):
    """(a) five sizes in one batch; a 200 x 200 image (planes in LDS) next to a 224 x 224 one (planes in the scratch buffer)"""
    import vipcup_amd  # noqa: F401
    five = ["adramp_16x16_q75", "photo_17x33_q75", "flat_48x40_q75", "checker_200x200_q75", "adramp_224x16_q75"]
    for name, g in zip(five, _encode([reference[n][1] for n in five], 75)):
        _same(name, g, reference[name][2])
    pair = ["checker_200x200_q75", LARGE[0]]
    got = _encode([reference[n][1] for n in pair], 75)
    assert len(got[0].mbs) == 169 and len(got[1].mbs) == 196
    for name, g in zip(pair, got):
        _same(name, g, reference[name][2])
    for name, g in zip(reversed(pair), _encode([reference[n][1] for n in reversed(pair)], 75)):
        _same(name, g, reference[name][2])


def test_the_decoder_reconstructs_what_the_encoder_wrote(reference):
    """(b) records and coefficients through the unchanged ``vip_vp8_reconstruct_rgb_u8`` (prediction and inverse transforms anew, into a
    fresh scratch buffer) give the encoder's pixels"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    from vipcup_amd.ops import _launch, _p
    names = ["photo_17x33_q75", "adramp_224x16_q75", "checker_200x200_q75", LARGE[0], "flat_48x40_q75"]
    batch = _batch([reference[n][1] for n in names])
    enc = pipeline.webp_encode(batch, 75)
    want = pipeline.webp_recompress(batch, 75).rgb
    n, maxH, maxW, _ = batch.rgb.shape
    scratch = torch.full_like(enc.scratch, 0x5a)
    rgb = torch.zeros_like(batch.rgb)
    _launch("vip_vp8_reconstruct_rgb_u8", _p(enc.stream), enc.stream.numel(), _p(enc.desc_d), n, _p(scratch), scratch.numel(), _p(rgb), maxH, maxW)
    assert torch.equal(rgb, want)


def test_libwebp_decodes_the_file_of_the_gpus_levels(reference):
    """(c) three images: sub-block and 16 x 16 macroblocks, skipped ones, odd sizes"""
    import vipcup_amd  # noqa: F401
    names = ["photo_17x33_q75", "vramp_48x40_q75", "adramp_224x16_q75"]
    got = _encode([reference[n][1] for n in names], 75)
    assert any((g.mbs["ymode"] == V.B_PRED).any() for g in got) and any((g.mbs["ymode"] != V.B_PRED).any() for g in got)
    for name, g in zip(names, got):
        assert np.array_equal(V.pillow_rgb(E.keyframe(g)), g.rgb), name


def test_independent_of_the_batch_and_reproducible(reference):
    """(d) image 0 of a batch of 1 == the same image at slot 3 of a batch of 5; two runs are bit-identical"""
    import vipcup_amd  # noqa: F401
    img = reference["photo_17x33_q75"][1]
    others = [reference[n][1] for n in ("checker_200x200_q75", "adramp_16x16_q75", "photo_224x16_q30", "flat_48x40_q75")]
    alone = _encode([img], 30)[0]
    five = _encode(others[:3] + [img] + others[3:], 30)
    _same("slot 3 of 5", five[3], alone)
    again = _encode(others[:3] + [img] + others[3:], 30)
    for k, (a, b) in enumerate(zip(five, again)):
        _same(f"second run, image {k}", b, a)


def test_chain_step_and_stress_rows(tmp_path):
    """(e) ``apply_chain("r50+w75")`` is the two calls by hand; ``stress_batch(webps=...)`` rows are ``webp_recompress`` scored"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, pipeline, zoo
    raws = [synth_jpeg(i) for i in (100, 101)]
    batch = pipeline.decode_images(raws)
    a = pipeline.apply_chain(batch, "r50+w75")
    b = pipeline.webp_recompress(pipeline.rescale(batch, 50), 75)
    assert a.sizes_host == b.sizes_host == [(100, 100), (100, 100)] and torch.equal(a.rgb, b.rgb)
    assert not torch.equal(pipeline.webp_recompress(batch, 75).rgb, batch.rgb)
    assert torch.equal(pipeline.apply_step(batch, "webp_recompress", 75, {}).rgb, pipeline.webp_recompress(batch, 75).rgb)
    members = [(zoo.MEMBERS["resnet_rs50"], zoo.FoldMean([P.gpu_member("resnet_rs50")[1]]))]
    rows, labels = ensemble.stress_batch(raws, members, [80], webps=[75], chains=["r50+w75"])
    assert labels == ["q80", "w75", "w75_q80", "r50+w75"]
    made = pipeline.webp_recompress(batch, 75)
    assert torch.equal(rows[2], ensemble.stress_batch(made, members, [])[0])
    assert torch.equal(rows[3], ensemble.stress_batch(made, members, [80])[1])
    assert torch.equal(rows[4], ensemble.stress_batch(a, members, [])[0])
    assert not torch.equal(rows[2], rows[0])


def test_cli_stress_webp(tmp_path):
    """(e) ``--stress-webp 75 --stress-jpeg 80`` on four synthetic files and one member: the columns, the settings, the plain CSVs byte for
    byte those of a run without the flag, and every ``p_w75`` == ``stress_batch`` called directly"""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, pipeline, zoo
    from vipcup_amd import main as cli
    names = [f"img_{i:05d}.jpg" for i in range(100, 104)]
    for i, name in zip(range(100, 104), names):
        (tmp_path / name).write_bytes(synth_jpeg(i))
    (tmp_path / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS["resnet_rs50"].ckpt_name, [zoo.MEMBERS["resnet_rs50"].input_hw] * 2, 0]]))
    extra = ["--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "2", "--precision", "fast"]
    csv = str(tmp_path / "test.csv")
    cli.main([csv, str(tmp_path / "o0.csv"), "--scores-out", str(tmp_path / "s0.csv"), *extra])
    cli.main([csv, str(tmp_path / "o1.csv"), "--scores-out", str(tmp_path / "s1.csv"), *extra, "--stress-out", str(tmp_path / "stress.csv"),
              "--stress-webp", "75", "--stress-jpeg", "80"])
    assert (tmp_path / "o0.csv").read_bytes() == (tmp_path / "o1.csv").read_bytes()
    assert (tmp_path / "s0.csv").read_bytes() == (tmp_path / "s1.csv").read_bytes()
    labels = ["q80", "w75", "w75_q80"]
    table = pd.read_csv(tmp_path / "stress.csv", dtype={"flips_at": str, "flips": str}, keep_default_na=False)
    assert list(table.columns) == ["filename", "p", "decision"] + [f"p_{v}" for v in labels] + [f"decision_{v}" for v in labels] + \
        ["stable", "flips_at", "flips"]
    info = json.loads((tmp_path / "stress.json").read_text())
    assert info["variants"] == labels
    assert info["settings"] == {"qualities": [80], "subsampling": "4:2:0", "threshold": 0.487, "precision": "fast", "batch_size": 2, "n_images": 4,
                                "members": ["resnet_rs50"], "webp_qualities": [75]}
    members = [(zoo.MEMBERS["resnet_rs50"], zoo.FoldMean([P.gpu_member("resnet_rs50")[1]]))]
    for b0 in (0, 2):
        part = names[b0:b0 + 2]
        rows, got = ensemble.stress_batch([(tmp_path / n).read_bytes() for n in part], members, [80], webps=[75],
                                          noise_keys=pipeline.noise_keys(part))
        assert got == labels
        rows = rows.cpu().numpy()
        for k, v in enumerate(labels):
            want = ensemble.aggregate(part, rows[1 + k])[1]
            assert np.array_equal(table[f"p_{v}"].to_numpy(np.float32)[b0:b0 + 2], want), (v, b0)
    # a chain with a w step and no flag lists the (empty) setting too
    cli.main([csv, str(tmp_path / "o2.csv"), *extra, "--stress-out", str(tmp_path / "chain.csv"), "--stress-chain", "r50+w75"])
    s = json.loads((tmp_path / "chain.json").read_text())["settings"]
    assert s["webp_qualities"] == [] and s["chains"] == ["r50+w75"] and s["resize_filter"] == "bicubic"
