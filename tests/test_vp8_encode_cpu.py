"""CPU: the lossy WebP re-save without a GPU.  The encoder arithmetic (csrc/vp8_enc.hpp), the numbers of a quality
(csrc/vp8_enc_host.cpp) and the decoder arithmetic (csrc/vp8_recon.hpp) are compiled as plain C++ (tests/fuzz/vp8_enc_check.cpp) and
run serially; its modes and levels are written out as a key frame by ``_vp8.write_keyframe`` - a writer that shares no code with the
product's - and Pillow / libwebp must decode that file to the program's own RGB, bit for bit.  That holds everything downstream of
the encoder's decisions to libwebp: a wrong quantiser step, filter strength, skip rule, coefficient order or reconstruction shows
as a pixel.  The decisions themselves are the project's own; what is checked of them is that every kind occurs.  Also here: the
forward transforms' round trip, the quality curve as literals, the chain grammar and labels of the ``w<Q>`` step, and the C ABI's
argument checks."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import _vp8 as V
from tests import _vp8_enc as E


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return E.build_check(tmp_path_factory.mktemp("vp8_enc_check"))


@pytest.fixture(scope="module")
def encoded(exe, tmp_path_factory):
    items = E.cases()
    return items, E.run_check(exe, items, tmp_path_factory.mktemp("vp8_enc_cases"))


def test_the_corpus_covers_shapes_contents_and_qualities():
    items = E.cases()
    assert {(img.shape[1], img.shape[0]) for _, _, img in items} == {(16, 16), (17, 33), (48, 40), (200, 200), (224, 16)}
    assert {q for _, q, _ in items} == {1, 30, 75, 100}
    assert {name.split("_")[0] for name, _, _ in items} == set(E.KINDS)
    assert len({name for name, _, _ in items}) == len(items)


def test_libwebp_decodes_the_written_file_to_the_programs_pixels(encoded):
    items, encs = encoded
    for (name, q, img), e in zip(items, encs):
        assert (e.w, e.h) == (img.shape[1], img.shape[0]) and e.base_q == E.BASE_Q[q - 1], name
        raw = E.keyframe(e)
        got = V.pillow_rgb(raw)
        assert got.shape == e.rgb.shape and np.array_equal(got, e.rgb), (name, int(np.abs(got.astype(int) - e.rgb).max()))


def test_records_agree_with_the_levels(encoded):
    """what the device path reads - the records and the coefficient area - says what the levels say"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    items, encs = encoded
    steps = {q: [list(p.y1), list(p.uv), list(p.y2)] for q in E.QUALITIES for p in [pipeline.webp_encode_params(q)]}
    for (name, q, _), e in zip(items, encs):
        for i, (m, lv, cf) in enumerate(zip(e.mbs, e.levels, e.coefs)):
            i4 = int(m["ymode"]) == V.B_PRED
            coded = [b for b in range(25) if lv[b].any()]
            assert int(m["nz"]) == sum(1 << b for b in coded), (name, i)
            assert int(m["skip"]) == int(not coded) and int(m["coef_idx"]) == 25 * i
            assert not (i4 and lv[24].any())
            if not i4:
                assert not lv[:16, 0].any(), (name, i)          # the luma DCs travel in Y2
            assert int(m["flevel"]) == e.filter_level and (int(m["inner"]) == 1 if i4 else True)
            for slot, b in enumerate(coded):                  # back to back, dequantised with the block kind's steps
                dc, ac = steps[q][0 if b < 16 else 1 if b < 24 else 2]
                assert np.array_equal(cf[slot], lv[b] * np.array([dc] + [ac] * 15)), (name, i, b)
            assert not cf[len(coded):].any()


def test_every_kind_of_decision_occurs(encoded):
    """coverage is a condition: a corpus that never takes a path checks nothing on it"""
    y16, uv, sub, skipped, coded, top = E.coverage(encoded[1])
    assert y16 == {V.B_DC, V.B_TM, V.B_VE, V.B_HE}
    assert uv == {V.B_DC, V.B_TM, V.B_VE, V.B_HE}
    assert sub == set(range(10))
    assert skipped and coded
    assert top >= 67                                             # the token writer's largest category
    flat = [e for (name, _, _), e in zip(*encoded) if name.startswith("flat_")]
    assert len(flat) == len(E.SHAPES) and all(not e.levels.any() and e.mbs["skip"].all() for e in flat)      # every macroblock skipped
    assert any(e.filter_level == 0 for e in encoded[1]) and any(e.filter_level >= 40 for e in encoded[1])      # hev 0 and 2


def test_forward_transforms_round_trip(exe):
    """idct(fdct(x)) within 1 of x for residual blocks in -255..255; inverse WHT of the forward WHT within 1 of the DCs; the quantiser's
    reciprocal multiplication against a plain division, every step 2..1023 with every value 0..65535"""
    r = subprocess.run([exe, "--roundtrip", "200000", "7"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    worst_dct, worst_wht, bad_quotients = (int(v) for v in r.stdout.split())
    assert worst_dct <= 1 and worst_wht <= 1, (worst_dct, worst_wht)
    assert bad_quotients == 0                                    # the quantiser's multiplication is the division, for every step and value


def test_quality_curve_is_pinned():
    assert len(E.BASE_Q) == 100 and E.BASE_Q[74] == 26 and E.BASE_Q[49] == 38 and E.BASE_Q[99] == 0
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    got = [pipeline.webp_encode_params(q).base_q for q in range(1, 101)]
    assert tuple(got) == E.BASE_Q
    p = pipeline.webp_encode_params(75)
    assert (p.quality, p.base_q) == (75, 26) and list(p.y1) == [24, 30] and list(p.y2) == [48, 46] and list(p.uv) == [24, 30]
    assert p.i4_bias == (61 * 30 * 30) >> 4 and p.filter_level == max(0, (13 * 26 - 242) >> 4) == p.flevel
    p = pipeline.webp_encode_params(100)                         # the smallest steps; Y2's AC step has a floor of 8
    assert list(p.y1) == [4, 4] and list(p.y2) == [8, 8] and list(p.uv) == [4, 4] and p.filter_level == 0 and p.hev == 0
    for bad in (0, 101, -1, 7.5, "75", True, None):
        with pytest.raises(ValueError, match="quality"):
            pipeline.webp_encode_params(bad)
    assert C.sizeof(_abi.Vp8EncParams) == 80 and list(p.y1_inv) == [1 << 30, 1 << 30] and list(p.y2_inv) == [1 << 29, 1 << 29]


def test_chain_grammar_of_the_webp_step():
    from vipcup_amd import chain
    row = chain.STEPS["webp_recompress"]
    assert list(chain.STEPS)[-1] == "webp_recompress" and list(chain.STEPS)[-2] == "clahe"
    assert (row.prefix, row.digits, row.lo, row.hi, row.flag, row.keyword, row.order, row.family) == \
        ("w", 0, 1, 100, "--stress-webp", "webps", "desc", "recompression")
    for q in (1, 75, 100):
        assert chain.parse_step(f"w{q}") == ("webp_recompress", q) and chain.step_label("webp_recompress", q) == f"w{q}"
        assert chain.parse_chain(f"w{q}+q80") == [("webp_recompress", q), ("recompress", 80)]
        assert chain.parse_chain(f"r50+w{q}") == [("rescale", 50), ("webp_recompress", q)]
    assert chain.parse_chain("r50+shp080+w75") == [("rescale", 50), ("sharpen", 80), ("webp_recompress", 75)]
    for bad in ("w0", "w101", "w075", "W75", "w7.5"):
        for text in (f"{bad}+q80", f"q80+{bad}"):
            with pytest.raises(ValueError, match=repr(bad).replace(".", r"\.")):
                chain.parse_chain(text)
        with pytest.raises(ValueError, match="w<Q>"):
            chain.parse_step(bad)
    with pytest.raises(ValueError, match="--stress-webp"):
        chain.parse_chain("w75")
    assert chain.chain_kinds(["r50+w75"]) == {"rescale", "webp_recompress"}


def test_labels_of_the_webp_rows():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    assert ensemble.stress_labels([80], webps=[90, 60]) == ["q80", "w90", "w90_q80", "w60", "w60_q80"]
    assert ensemble.stress_labels([80], webps=[60, 90]) == ["q80", "w90", "w90_q80", "w60", "w60_q80"]            # largest first
    assert ensemble.stress_labels([], webps=[75]) == ["w75"]
    assert ensemble.stress_labels([80, 50], clahes=[2.0], webps=[75], chains=["r50+w75"]) == \
        ["q80", "q50", "clahe20", "clahe20_q80", "clahe20_q50", "w75", "w75_q80", "w75_q50", "r50+w75"]
    for kw in (dict(), dict(scales=[50]), dict(clahes=[2.0], gray=True, chains=["r50+q75"])):
        assert ensemble.stress_labels([80, 50], webps=[], **kw) == ensemble.stress_labels([80, 50], **kw)
        assert ensemble.stress_labels([80, 50], webps=(), **kw) == ensemble.stress_labels([80, 50], **kw)


def test_cli_refusals_of_the_webp_flag(tmp_path):
    from vipcup_amd import main as cli
    csv = str(tmp_path / "t.csv")
    out = ["--stress-out", str(tmp_path / "s.csv")]
    for argv, want in (
            ([csv, "o.csv", "--stress-webp", "75"], "--stress-webp needs --stress-out"),
            ([csv, "o.csv", "--stress-webp", "75,75", *out], "each listed once"),
            ([csv, "o.csv", "--stress-webp", "0", *out], "integer qualities in 1..100"),
            ([csv, "o.csv", "--stress-webp", "101", *out], "integer qualities in 1..100"),
            ([csv, "o.csv", "--stress-webp", "7.5", *out], "integer qualities in 1..100"),
            ([csv, "o.csv", "--stress-webp", "75", *out, "--tta", "2"], "--stress-webp works with --shard images and --tta 1 only"),
            ([csv, "o.csv", "--stress-webp", "75", *out, "--heatmaps", str(tmp_path / "h")], "--stress-webp and --heatmaps cannot be combined"),
            ([csv, "o.csv", "--stress-chain", "w75", *out], "--stress-webp"),
            ([csv, "o.csv", "--stress-chain", "q80+w0", *out], "'w0'")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert want in str(e.value), (argv, str(e.value))


def test_c_abi_argument_checks_without_a_gpu(monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    lib = _abi.lib()
    p = C.c_void_p(64)
    enc = lib.vip_vp8_encode_rgb_u8
    assert enc(None, None, 0, 0, 0, 0, None, 0, None, 0, None, 0, None) == -1 and b"null" in lib.vip_last_error()
    for ptrs in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        rgb, desc, stream, levels, scratch = ptrs
        assert enc(rgb, desc, 1, 16, 16, 75, stream, 64, levels, 400, scratch, 384, None) == -1 and b"null" in lib.vip_last_error()
    for q in (0, 101, -5):
        assert enc(p, p, 1, 16, 16, q, p, 64, p, 400, p, 384, None) == -1
        assert f"quality {q}: expected 1..100".encode() in lib.vip_last_error()
    assert enc(p, p, 0, 16, 16, 75, p, 64, p, 400, p, 384, None) == -1 and b"bad size" in lib.vip_last_error()
    assert enc(p, p, 1, 0, 16, 75, p, 64, p, 400, p, 384, None) == -1 and b"bad size" in lib.vip_last_error()
    assert enc(p, p, 1, 16, 16, 75, p, 0, p, 400, p, 384, None) == -1 and b"empty buffer" in lib.vip_last_error()
    assert enc(p, p, 1, 16, 16, 75, C.c_void_p(72), 64, p, 400, p, 384, None) == -2 and b"aligned" in lib.vip_last_error()
    monkeypatch.setenv("VIP_MAX_JPEG_PIXELS", "1000")
    assert enc(p, p, 1, 40, 36, 75, p, 64, p, 400, p, 384, None) == -1 and b"36x40 exceeds VIP_MAX_JPEG_PIXELS=1000" in lib.vip_last_error()
    hw = (C.c_int32 * 2)(40, 36)
    d, a, b = _abi.Vp8Desc(), C.c_size_t(0), C.c_size_t(0)
    assert lib.vip_vp8_encode_layout_h(hw, 1, 75, C.byref(d), C.byref(a), C.byref(b)) == -1
    assert b"36x40 exceeds VIP_MAX_JPEG_PIXELS=1000" in lib.vip_last_error()
    monkeypatch.delenv("VIP_MAX_JPEG_PIXELS")
    # the layout: the decoder's, every macroblock with room for all 25 blocks
    hw = (C.c_int32 * 4)(40, 36, 17, 33)
    ds = (_abi.Vp8Desc * 2)()
    assert lib.vip_vp8_encode_layout_h(hw, 2, 75, ds, C.byref(a), C.byref(b)) == 0
    assert [(x.width, x.height, x.mb_w, x.mb_h, x.filter_type) for x in ds] == [(36, 40, 3, 3, 2), (33, 17, 3, 2, 2)]
    assert ds[0].stream_off == 0 and ds[0].coef_off == 368 and ds[0].coef_blocks == 225 and ds[0].plane_off == 0
    assert ds[1].stream_off == 368 + 225 * 32 and ds[1].coef_off == 240 and ds[1].plane_off == 9 * 384
    assert a.value == ds[1].stream_off + 240 + 150 * 32 and b.value == 15 * 384
    assert lib.vip_vp8_encode_layout_h(hw, 2, 100, ds, C.byref(a), C.byref(b)) == 0 and ds[0].filter_type == 0
    assert lib.vip_vp8_encode_layout_h(None, 1, 75, ds, C.byref(a), C.byref(b)) == -1
    assert lib.vip_vp8_encode_layout_h(hw, 2, 0, ds, C.byref(a), C.byref(b)) == -1 and b"quality 0" in lib.vip_last_error()
    bad = (C.c_int32 * 2)(0, 16)
    assert lib.vip_vp8_encode_layout_h(bad, 1, 75, ds, C.byref(a), C.byref(b)) == -1 and b"image 0" in lib.vip_last_error()
    assert lib.vip_vp8_encode_params_h(75, None) == -1 and lib.vip_vp8_encode_params_h(0, C.byref(_abi.Vp8EncParams())) == -1


def test_pipeline_argument_checks_run_before_any_launch():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    for bad in (0, 101, 7.5, "75", None, True):
        with pytest.raises(ValueError, match="quality"):
            pipeline.webp_recompress(object(), bad)
    with pytest.raises(ValueError, match="DecodedBatch"):
        pipeline.webp_recompress(object(), 75)
