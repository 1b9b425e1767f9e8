"""CPU: the host half of the lossy WebP path (csrc/vp8_host.cpp) over the corpus of tests/_vp8.py - Pillow's encoder, the
committed fixtures, hand-written key frames: probe and token decode, the macroblock records and coefficients, the coverage
word, every refusal with its message, thread independence, and the ``lossy_webp`` switch of ``pipeline.host_decode``.  The
pixel arithmetic of the device half (csrc/vp8_recon.hpp) is compiled as plain C++ (tests/fuzz/vp8_recon_check.cpp), run
serially and compared with Pillow / libwebp, so the decoder is held to the yardstick without a GPU too."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import _vp8 as V
from tests import _webp as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def corp():
    return V.corpus(1)


@pytest.fixture(scope="module")
def staged(corp):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    return pipeline.entropy_decode_vp8s([r for _, r in corp], threads=4)


def _image(staged, i):
    """(desc, records as a structured array, coefficients [blocks][16]) of image i"""
    from vipcup_amd import _abi
    d = staged.desc[i]
    buf = np.asarray(staged.stream)
    n = d.mb_w * d.mb_h
    a = d.stream_off + d.mb_off
    recs = (_abi.Vp8Mb * n).from_buffer_copy(buf[a:a + n * C.sizeof(_abi.Vp8Mb)].tobytes())
    a = d.stream_off + d.coef_off
    coefs = buf[a:a + d.coef_blocks * 32].view(np.int16).reshape(-1, 16)
    return d, recs, coefs


def _probe(raw):
    from vipcup_amd import _abi
    lib = _abi.lib()
    d, need = _abi.Vp8Desc(), C.c_size_t(0)
    st = lib.vip_vp8_probe_h(raw, len(raw), C.byref(d), C.byref(need))
    return st, d, need.value, lib.vip_last_error().decode()


def test_probe_gives_the_size_and_a_bound(corp, staged):
    from vipcup_amd import _abi
    assert C.sizeof(_abi.Vp8Mb) == 40 and C.sizeof(_abi.Vp8Desc) == 72
    for i, (name, raw) in enumerate(corp):
        st, d, need, msg = _probe(raw)
        assert st == 0, (name, msg)
        h, w = V.pillow_rgb(raw).shape[:2]
        assert (d.width, d.height, d.mb_w, d.mb_h) == (w, h, (w + 15) // 16, (h + 15) // 16), name
        assert d.has_alpha == int(name.startswith("rgba")), name
        assert d.stats == 0 and d.coef_blocks == 0
        e = staged.desc[i]
        assert (e.width, e.height) == (w, h) and e.mb_off + e.mb_w * e.mb_h * 40 <= e.coef_off
        assert e.coef_off + e.coef_blocks * 32 <= need, name                # what an image uses stays inside its probe bound
    assert staged.scratch_bytes == sum(d.mb_w * d.mb_h * 384 for d in staged.desc)
    assert [d.plane_off for d in staged.desc] == list(np.cumsum([0] + [d.mb_w * d.mb_h * 384 for d in staged.desc])[:-1])


def test_records_and_coefficients_are_sane(corp, staged):
    end = 0
    for i, (name, _) in enumerate(corp):
        d, recs, coefs = _image(staged, i)
        assert d.stream_off == end and d.stream_off % 8 == 0, name          # packed back to back
        end = d.stream_off + (d.coef_off + d.coef_blocks * 32 + 7) // 8 * 8
        assert d.filter_type in (0, 1, 2)
        idx = 0
        for k, M in enumerate(recs):
            assert M.ymode <= V.B_PRED and M.uvmode <= 3 and all(m <= 9 for m in M.bmodes), (name, k)
            assert M.flevel <= 63 and M.hev <= 2 and M.inner <= 1 and M.segment <= 3 and M.skip <= 1
            assert (M.flevel == 0) == (M.ilevel == 0) or d.filter_type == 0
            assert M.hev == (2 if M.flevel >= 40 else 1 if M.flevel >= 15 else 0) or d.filter_type == 0
            assert M.nz < (1 << 25) and M.dc_only & ~M.nz == 0 and M.coef_idx == idx, (name, k)
            i16 = M.ymode != V.B_PRED
            if not i16:
                assert not M.nz >> 24 and M.inner == 1
            if M.skip:
                assert M.nz == 0
            if M.nz & 0xffffff == 0 and not M.nz >> 24:
                assert M.inner == int(not i16)
            for b in range(25):
                if M.nz >> b & 1:
                    blk = coefs[idx]
                    if i16 and b < 16:
                        assert blk[0] == 0 and blk[1:].any(), (name, k, b)  # its DC comes from Y2
                    if M.dc_only >> b & 1:
                        assert not blk[1:].any() and not (i16 and b < 16)
                    idx += 1
        assert idx == d.coef_blocks, name
    assert end <= len(staged.stream) < end + 8 or end == len(staged.stream)


def test_coverage_word_is_full_over_the_corpus(corp, staged):
    seen = 0
    for d in staged.desc:
        seen |= d.stats
    assert seen == V.STAT_ALL, f"never met: {V.stat_names(V.STAT_ALL & ~seen)}"
    # each source brings what only it can: the fixtures the partitions, the hand-written files the rest
    of = {name: staged.desc[i].stats for i, (name, _) in enumerate(corp)}
    assert of["fx_normal_p3_s4_sh0_f100"] & V.STAT["PARTS8"] and of["fx_simple_p2_s4_sh7_f20"] & V.STAT["PARTS4"]
    assert of["fx_simple_p1_s2_sh3_f100"] & V.STAT["PARTS2"] and of["fx_simple_p0_s1_sh0_f20"] & V.STAT["SIMPLE_FILTER"]
    assert of["hw_i16_r0"] & V.STAT["SEG_DELTA"] and of["hw_i16_r0"] & V.STAT["LEVEL0_MB"] and of["hw_bmodes_lfdelta"] & V.STAT["LF_DELTA"]
    assert of["hw_cat6_clamp"] & V.STAT["CAT6"] and not of["hw_i16_r1"] & V.STAT["SKIP"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpu_build_of_the_pixel_arithmetic_equals_pillow(corp, tmp_path):
    exe = tmp_path / "vp8_recon_check"
    cmd = ["g++", "-O2", "-std=c++17", f"-I{ROOT}/include", f"-I{ROOT}/vip-cup-2022_amd/csrc", os.path.join(ROOT, "tests", "fuzz", "vp8_recon_check.cpp"),
           os.path.join(ROOT, "vip-cup-2022_amd", "csrc", "vp8_host.cpp"), "-o", str(exe), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    files = []
    for name, raw in corp:
        (tmp_path / f"{name}.webp").write_bytes(raw)
        files.append(str(tmp_path / f"{name}.webp"))
    r = subprocess.run([str(exe), *files], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for (name, raw), f in zip(corp, files):
        want = V.pillow_rgb(raw)
        got = np.fromfile(f + ".rgb", dtype=np.uint8).reshape(want.shape)
        assert np.array_equal(got, want), f"{name}: {int((got != want).any(-1).sum())} pixels differ"


def _frame(raw):
    return bytearray(V.vp8_payload(raw))


def _refiled(frame, extra=()):
    return V.riff(list(extra) + [(b"VP8 ", bytes(frame))])


def test_every_refusal_has_its_message(corp, monkeypatch):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    good = dict(corp)["hw_i16_r3"]                           # two partitions, behind VP8X
    f = _frame(good)
    cases = []
    g = bytearray(f); g[0] |= 1
    cases.append(("inter frame", _refiled(g)))
    g = bytearray(f); g[0] = (g[0] & ~0x0e) | (4 << 1)
    cases.append(("profile 4", _refiled(g)))
    g = bytearray(f); g[0] &= ~0x10
    cases.append(("not shown", _refiled(g)))
    g = bytearray(f); g[3] = 0
    cases.append(("start code", _refiled(g)))
    g = bytearray(f); g[6] = g[7] = 0
    cases.append(("0x36 pixels", _refiled(g)))
    g = bytearray(f); g[8] = 0; g[9] &= 0xc0                # the scale bits alone do not make a height
    cases.append(("40x0 pixels", _refiled(g)))
    g = bytearray(f); tag = int.from_bytes(g[:3], "little"); g[:3] = ((tag & 31) | ((len(f) + 5) << 5)).to_bytes(3, "little")
    cases.append(("first partition .* runs past the chunk", _refiled(g)))
    p0 = int.from_bytes(f[:3], "little") >> 5
    g = bytearray(f); g[10 + p0:13 + p0] = (len(f)).to_bytes(3, "little")
    cases.append(("token partition 0 .* runs past the chunk", _refiled(g)))
    cases.append(("partition sizes run past the chunk", _refiled(f[:10 + p0 + 2])))
    g = bytearray(f[:10 + p0 + 3 + 4]); g[10 + p0:13 + p0] = (2).to_bytes(3, "little")
    cases.append(("token partition [01] ends at macroblock", _refiled(g)))
    g = bytearray(f[:10 + 6]); tag = int.from_bytes(g[:3], "little"); g[:3] = ((tag & 31) | (6 << 5)).to_bytes(3, "little")
    cases.append(("first partition ends", _refiled(g)))
    cases.append(("VP8X canvas 41x36 differs from the VP8 size 40x36", _refiled(f, [W.vp8x_chunk(41, 36)])))
    cases.append(("animated", _refiled(f, [W.vp8x_chunk(40, 36, flags=2)])))
    cases.append(("animated", _refiled(f, [W.vp8x_chunk(40, 36), (b"ANIM", bytes(6))])))
    cases.append(("lossless .VP8L. file on the lossy path", W.pillow_webp(V._photo(np.random.default_rng(0), 8, 8))))
    cases.append(("no image chunk", V.riff([W.vp8x_chunk(40, 36), (b"EXIF", b"abcd")])))
    cases.append(("first chunk is EXIF", V.riff([(b"EXIF", b"abcd"), (b"VP8 ", bytes(f))])))
    g = bytearray(_refiled(f)); g[16:20] = struct.pack("<I", len(f) + 100)
    cases.append(("truncated VP8  chunk", bytes(g)))
    cases.append(("RIFF size 582 runs past the buffer", good[:-7]))
    cases.append(("VP8 chunk too short", V.riff([(b"VP8 ", bytes(f[:9]))])))
    for want, raw in cases:
        st, _, _, msg = _probe(raw)
        if st == 0:                                          # the header is fine: the damage is met by the token decode
            with pytest.raises(_abi.VipError, match="webp image 5: webp: .*" + want):
                pipeline.entropy_decode_vp8s([raw], index=[5])
        else:
            assert st == -7 and __import__("re").search(want, msg), (want, msg)
            with pytest.raises(_abi.VipError, match="webp image 5: .*" + want):
                pipeline.entropy_decode_vp8s([raw], index=[5])
    # the size cap, read by the host code per call
    monkeypatch.setenv("VIP_MAX_JPEG_PIXELS", "1000")
    st, _, _, msg = _probe(good)
    assert st == -7 and "40x36 exceeds VIP_MAX_JPEG_PIXELS=1000" in msg
    monkeypatch.delenv("VIP_MAX_JPEG_PIXELS")
    # argument checks, without a GPU
    lib = _abi.lib()
    assert lib.vip_vp8_probe_h(None, 0, None, None) == -1 and b"null" in lib.vip_last_error()
    assert lib.vip_vp8_entropy_h(None, None, 0, None, None, 0, None, 1) == -1
    assert lib.vip_vp8_scratch_bytes(None, 0, None) == -1
    assert lib.vip_vp8_reconstruct_rgb_u8(None, 0, None, 0, None, 0, None, 0, 0, None) == -1 and b"null" in lib.vip_last_error()
    p = C.c_void_p(64)
    assert lib.vip_vp8_reconstruct_rgb_u8(p, 8, p, 0, p, 16, p, 8, 8, None) == -1 and b"bad size" in lib.vip_last_error()
    assert lib.vip_vp8_reconstruct_rgb_u8(C.c_void_p(68), 8, p, 1, p, 16, p, 8, 8, None) == -2
    # a buffer smaller than the probe bound is refused before any work
    d, used = (_abi.Vp8Desc * 1)(), C.c_size_t(0)
    buf = np.zeros(64, dtype=np.uint64)
    ptrs, lens = (C.c_void_p * 1)(C.cast(C.c_char_p(good), C.c_void_p)), (C.c_size_t * 1)(len(good))
    assert lib.vip_vp8_entropy_h(ptrs, lens, 1, d, buf.ctypes.data_as(C.c_void_p), 512, C.byref(used), 1) == -1
    assert b"too small" in lib.vip_last_error() and used.value > 512


def test_ignored_header_bits_and_skipped_chunks(corp):
    """the scale, colour-space and clamp bits change nothing; ALPH / ICCP / unknown chunks are walked over"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    name, raw = next((n, r) for n, r in corp if n == "hw_i16_r1")
    f = _frame(raw)
    assert f[7] >> 6 == 2 and f[9] >> 6 == 1
    g = bytearray(f); g[7] &= 0x3f; g[9] &= 0x3f
    wrapped = V.riff([W.vp8x_chunk(40, 36, flags=0x10), (b"ICCP", b"xyz"), (b"ALPH", bytes(9)), (b"VP8 ", bytes(g)), (b"XMP ", b"<x/>")])
    a = pipeline.entropy_decode_vp8s([raw, wrapped, _refiled(g)], threads=1)
    assert a.desc[1].has_alpha == 1 and a.desc[0].has_alpha == 0
    streams = [bytes(np.asarray(a.stream)[d.stream_off + d.mb_off:d.stream_off + d.coef_off + d.coef_blocks * 32]) for d in a.desc]
    assert streams[0] == streams[1] == streams[2]


def test_the_lossless_entry_points_still_refuse(corp):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    lib = _abi.lib()
    raw = corp[0][1]
    d, need = _abi.WebpDesc(), C.c_size_t(0)
    assert lib.vip_webp_probe_h(raw, len(raw), C.byref(d), C.byref(need)) == -7
    assert lib.vip_last_error() == b"webp: lossy WebP (VP8) is not supported"
    with pytest.raises(_abi.VipError, match=r"webp image 0: vip_webp_probe_h failed with vip_status -7: webp: lossy WebP \(VP8\) is not supported"):
        pipeline.entropy_decode_webps([raw])


def test_threads_give_identical_buffers(corp, staged):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    raws = [r for _, r in corp]
    want = bytes(np.asarray(staged.stream))
    for threads in (1, 2, 3, 7, 16):
        s = pipeline.entropy_decode_vp8s(raws, threads=threads)
        assert bytes(np.asarray(s.stream)) == want and bytes(s.desc) == bytes(staged.desc), threads


def test_the_switch(corp, monkeypatch):
    import vipcup_amd  # noqa: F401
    from tools.make_synth import synth_jpeg
    from vipcup_amd import _abi, pipeline
    monkeypatch.delenv("VIP_WEBP_LOSSY", raising=False)
    lossy, other = corp[3][1], corp[5][1]
    lossless = W.pillow_webp(V._photo(np.random.default_rng(0), 16, 16))
    jpeg = synth_jpeg(0)
    # off (the default): today's refusal, with today's text, from today's calls
    for raws, k in (([lossy, other], 0), ([jpeg, lossless, lossy], 2), ([lossless, lossy], 1)):
        with pytest.raises(_abi.VipError, match=f"webp image {k}: vip_webp_probe_h failed with vip_status -7: webp: lossy WebP"):
            pipeline.host_decode(raws)
        with pytest.raises(_abi.VipError, match=f"webp image {k}: .*lossy WebP"):
            pipeline.host_decode(raws, lossy_webp=False)
    assert isinstance(pipeline.host_decode([lossless, lossless]), pipeline.WebpStage)
    assert not pipeline.lossy_webp_enabled() and pipeline.lossy_webp_enabled(True)
    # on: by keyword, or by the knob (read per call)
    st = pipeline.host_decode([lossy, other], lossy_webp=True)
    assert isinstance(st, pipeline.Vp8Stage) and len(st) == 2
    monkeypatch.setenv("VIP_WEBP_LOSSY", "1")
    assert pipeline.lossy_webp_enabled() and not pipeline.lossy_webp_enabled(False)
    assert isinstance(pipeline.host_decode([lossy, other]), pipeline.Vp8Stage)
    mixed = pipeline.host_decode([jpeg, lossless, lossy, lossless, other])
    assert isinstance(mixed, pipeline.MixedStage) and mixed.vp8_idx == [2, 4] and mixed.webp_idx == [1, 3] and mixed.jpeg_idx == [0]
    assert isinstance(mixed.vp8, pipeline.Vp8Stage) and isinstance(mixed.webp, pipeline.WebpStage)
    assert isinstance(pipeline.host_decode([lossless, lossless]), pipeline.WebpStage)           # nothing lossy: as before
    assert isinstance(pipeline.host_decode([jpeg, jpeg]), tuple)
    with pytest.raises(_abi.VipError, match="webp image 2: .*VP8 inter frame"):                 # errors name the batch position
        bad = bytearray(lossy)
        bad[20] |= 1
        pipeline.host_decode([jpeg, lossless, bytes(bad)])
    monkeypatch.setenv("VIP_WEBP_LOSSY", "0")
    with pytest.raises(_abi.VipError, match="lossy WebP"):
        pipeline.host_decode([lossy])


def test_fixture_manifest_matches_the_files():
    import json
    with open(os.path.join(V.GOLDEN, "MANIFEST.json")) as f:
        man = json.load(f)
    names = sorted(x["name"] for x in man["files"])
    assert names == sorted(n for n in os.listdir(V.GOLDEN) if n.endswith(".webp")) and len(names) >= 8
    for x in man["files"]:
        raw = open(os.path.join(V.GOLDEN, x["name"]), "rb").read()
        assert len(raw) == x["bytes"] <= 8192 and x["width"] <= 64 and x["height"] <= 64
        w, h = struct.unpack("<HH", V.vp8_payload(raw)[6:10])
        assert (w & 0x3fff, h & 0x3fff) == (x["width"], x["height"])
    for key, values in (("filter_type", {0, 1}), ("partitions", {0, 1, 2, 3}), ("segments", {1, 2, 3, 4}), ("filter_sharpness", {0, 3, 7}),
                        ("filter_strength", {0, 20, 100})):
        assert values <= {x[key] for x in man["files"]}, key
