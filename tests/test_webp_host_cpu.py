"""CPU: the host half of the lossless WebP path (csrc/webp_host.cpp) through ctypes on the built library - no GPU needed.
Over the whole corpus (Pillow's encoder over kinds x methods x qualities, and hand-written files): the pure Python reference
decoder equals Pillow / libwebp; the host decoder's still-transformed ARGB words and transform data equal the reference
decoder's intermediate state; the numpy restatement of the device half, fed by the host output, equals Pillow.  Coverage is
asserted, so a thinner corpus fails.  Containers and streams the decoder must refuse give VIP_ERR_WEBP and their message."""
import ctypes as C
import io
import struct

import numpy as np
import pytest

from tests import _webp as W

VIP_ERR_WEBP = -7
SEED = 5
ENCODER_ORDERS = {(), (0,), (2,), (3,), (0, 1), (2, 0)}


@pytest.fixture(scope="module")
def lib():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, build
    build.build_lib()
    return _abi.lib()


@pytest.fixture(scope="module")
def corp():
    return W.corpus(SEED, W.SIZES)


@pytest.fixture(scope="module")
def reference(corp):
    """reference_state of every corpus file, computed once"""
    return [W.reference_state(raw) for _, raw in corp]


@pytest.fixture(scope="module")
def pillow(corp):
    return [W.pillow_rgba(raw) for _, raw in corp]


@pytest.fixture(scope="module")
def staged(lib, corp):
    from vipcup_amd import pipeline
    return pipeline.entropy_decode_webps([raw for _, raw in corp], threads=16)


def _pixels(mode, argb):
    return W.argb_to_rgba(argb) if mode == "RGBA" else W.argb_to_rgb(argb)


def _probe(lib, raw):
    from vipcup_amd import _abi
    d = _abi.WebpDesc()
    need = C.c_size_t(0)
    buf = (C.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
    st = lib.vip_webp_probe_h(buf, len(raw), C.byref(d), C.byref(need))
    return st, d, need.value


def _decode(lib, raws, threads=4, cap=None):
    from vipcup_amd import _abi
    n = len(raws)
    bufs = [(C.c_uint8 * len(r)).from_buffer_copy(r) for r in raws]
    ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_size_t * n)(*[len(r) for r in raws])
    desc = (_abi.WebpDesc * n)()
    if cap is None:
        cap = sum(_probe(lib, r)[2] for r in raws) if all(_probe(lib, r)[0] == 0 for r in raws) else 1 << 20
    out = np.zeros(max(cap, 4) // 4, np.uint32).view(np.uint8)
    used = C.c_size_t(0)
    st = lib.vip_webp_entropy_h(ptrs, lens, n, desc, out.ctypes.data_as(C.c_void_p), cap, C.byref(used), threads)
    return st, desc, out, used.value


def _refused(lib, raw, text):
    st, _, _, _ = _decode(lib, [raw], threads=1)
    msg = lib.vip_last_error().decode()
    assert st == VIP_ERR_WEBP, (st, msg)
    assert msg.startswith("webp image 0: ") and text in msg, (text, msg)


def test_reference_decoder_equals_pillow(corp, reference, pillow):
    assert len(pillow) == len(corp)                          # no case is left out of the comparison
    modes = set()
    for (name, _), s, (mode, px) in zip(corp, reference, pillow):
        assert np.array_equal(_pixels(mode, W.apply_inverse(s["coded"], s["transforms"])), px), name
        modes.add(mode)
    assert modes == {"RGB", "RGBA"}


def test_host_decoder_equals_reference_state(corp, reference, staged):
    stream = np.asarray(staged.stream)
    for i, ((name, _), s) in enumerate(zip(corp, reference)):
        d = staged.desc[i]
        assert d.stream_off % 4 == 0 and d.argb_off % 4 == 0 and all(d.data_off[k] % 4 == 0 for k in range(4)), name
        assert d.coded_width == s["coded"].shape[1], name
        assert W.same_state(W.host_state(d, stream), s), name
        assert d.stats == s["stats"], (name, d.stats, s["stats"])


def test_inverse_transforms_of_host_output_equal_pillow(corp, pillow, staged):
    stream = np.asarray(staged.stream)
    for i, ((name, _), (mode, px)) in enumerate(zip(corp, pillow)):
        assert np.array_equal(_pixels(mode, W.inverse_transforms(staged.desc[i], stream)), px), name


def test_corpus_coverage(corp, reference, staged):
    """every stats bit, the encoder's six transform orders and at least three hand-written ones, all 120 plane codes"""
    stats, planes = 0, set()
    orders = {"pillow": set(), "hw": set()}
    for i, ((name, _), s) in enumerate(zip(corp, reference)):
        stats |= staged.desc[i].stats
        planes |= s["plane_codes"]
        orders["hw" if name.startswith("hw_") else "pillow"].add(tuple(t[0] for t in s["transforms"]))
    assert stats == W.STAT_ALL, bin(stats)
    assert ENCODER_ORDERS <= orders["pillow"], orders["pillow"]
    assert len(orders["hw"] - orders["pillow"]) >= 3, orders["hw"]
    assert planes == set(range(1, 121)), sorted(set(range(1, 121)) - planes)
    sizes = {(s["height"], s["width"]) for s in reference}
    assert set(W.SIZES) <= sizes


def test_probe_sizes_and_pixel_cap(lib, corp, monkeypatch):
    for name, raw in corp[::7]:
        st, d, need = _probe(lib, raw)
        assert st == 0 and need % 4 == 0, name
        w, h = d.width, d.height
        assert need == 4 * (w * h + 2 * W.sub_size(w, 2) * W.sub_size(h, 2) + 256), name
        assert (d.n_transforms, d.coded_width, d.stats, d.stream_off) == (0, 0, 0, 0), name
    raw = W.pillow_webp(np.zeros((40, 50, 3), np.uint8))
    monkeypatch.setenv("VIP_MAX_JPEG_PIXELS", "1999")
    st, _, _ = _probe(lib, raw)
    assert st == VIP_ERR_WEBP and b"VIP_MAX_JPEG_PIXELS" in lib.vip_last_error()
    monkeypatch.setenv("VIP_MAX_JPEG_PIXELS", "2000")
    assert _probe(lib, raw)[0] == 0


def test_threads_give_identical_streams(lib, corp):
    raws = [raw for _, raw in corp[::3]]
    st1, d1, s1, u1 = _decode(lib, raws, threads=1)
    st16, d16, s16, u16 = _decode(lib, raws, threads=16)
    assert st1 == 0 and st16 == 0 and u1 == u16
    assert np.array_equal(s1, s16) and bytes(d1) == bytes(d16)


def _lossy():
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(W._photo(np.random.default_rng(0), 16, 16)).save(buf, "WEBP", quality=80)
    return buf.getvalue()


def _animated():
    from PIL import Image
    frames = [Image.fromarray(W._photo(np.random.default_rng(k), 16, 16)) for k in range(2)]
    buf = io.BytesIO()
    frames[0].save(buf, "WEBP", save_all=True, append_images=frames[1:], lossless=True, duration=50)
    return buf.getvalue()


def _good(**kw):
    rng = np.random.default_rng(3)
    return W.write_vp8l(6, 5, W._rand_argb(rng, 5, 6), **kw)


def _payload(raw):
    return bytearray(W.vp8l_payload(raw))


def test_container_refusals(lib):
    good = _good()
    assert _decode(lib, [good])[0] == 0
    _refused(lib, _lossy(), "lossy WebP (VP8) is not supported")
    _refused(lib, W.riff([(b"VP8 ", b"\0" * 12)]), "lossy WebP (VP8) is not supported")
    _refused(lib, _animated(), "animated WebP is not supported")
    p = bytes(_payload(good))
    _refused(lib, W.riff([W.vp8x_chunk(6, 5, 0x02), (b"VP8L", p)]), "animated")
    _refused(lib, W.riff([W.vp8x_chunk(6, 5), (b"ANMF", b"\0" * 16), (b"VP8L", p)]), "animated")
    _refused(lib, W.riff([W.vp8x_chunk(6, 5), (b"ANIM", b"\0" * 6), (b"VP8L", p)]), "animated")
    big = bytearray(good)
    big[4:8] = struct.pack("<I", len(good) - 8 + 1)
    _refused(lib, bytes(big), "runs past the buffer")
    _refused(lib, W.riff([W.vp8x_chunk(6, 5), (b"EXIF", b"abc")]), "no image chunk")
    _refused(lib, W.riff([(b"ABCD", b"abcd"), (b"VP8L", p)]), "no image chunk")
    _refused(lib, W.riff([W.vp8x_chunk(7, 5), (b"VP8L", p)]), "canvas")
    q = bytearray(p)
    q[0] = 0x2E
    _refused(lib, W.riff([(b"VP8L", bytes(q))]), "signature byte")
    q = bytearray(p)
    q[4] |= 0x20                                             # version bits 29..31 of the header word
    _refused(lib, W.riff([(b"VP8L", bytes(q))]), "version")
    _refused(lib, b"RIFF\x04\0\0\0WEBQ", "bad RIFF / WEBP signature")
    # accepted: VP8X with ICCP, EXIF, XMP and an unknown chunk of odd length before and after the image
    ok = W.riff([W.vp8x_chunk(6, 5, 0x2C), (b"ICCP", b"x" * 7), (b"zzzz", b"12345"), (b"VP8L", p), (b"EXIF", b"e" * 3), (b"XMP ", b"<x/>")])
    st, d, out, _ = _decode(lib, [ok])
    assert st == 0 and np.array_equal(W.inverse_transforms(d[0], out), W.reference_argb(good))


def _header(bw, w=4, h=4):
    bw.put(0x2F, 8)
    bw.put(w - 1, 14)
    bw.put(h - 1, 14)
    bw.put(1, 1)
    bw.put(0, 3)


def _file(bw):
    return W.riff([(b"VP8L", bw.bytes() + b"\0" * 8)])       # padding: the refusal is not one for running out of data


def _normal_code_start(bw, clens):
    """a normal prefix code's start: the code length code lengths for the first symbols of CLEN_ORDER; no max_symbol"""
    bw.put(0, 1)
    bw.put(len(clens) - 4, 4)
    for v in clens:
        bw.put(v, 3)
    bw.put(0, 1)


def test_malformed_streams_are_refused(lib):
    # colour cache bits outside 1..11
    for bits in (0, 12):
        bw = W.BitWriter()
        _header(bw)
        bw.put(0, 1)
        bw.put(1, 1)
        bw.put(bits, 4)
        _refused(lib, _file(bw), "colour cache bits")
    # a transform type twice
    bw = W.BitWriter()
    _header(bw)
    for _ in range(2):
        bw.put(1, 1)
        bw.put(W.SUBTRACT_GREEN, 2)
    _refused(lib, _file(bw), "occurs twice")
    # green code, lengths written with the code length code {0: '0', 1: '10', 2: '11'} (order 17, 18, 0, 1, 2)
    for lens, text in (([1, 1, 1], "over-subscribed prefix code"), ([1, 2], "incomplete prefix code"), ([], "empty prefix code")):
        bw = W.BitWriter()
        _header(bw)
        bw.put(0, 3)                                         # no transform, no cache, no meta image
        _normal_code_start(bw, [0, 0, 1, 2, 2])
        for v in lens + [0] * (280 - len(lens)):
            for b in ("0", "10", "11")[v]:
                bw.put(int(b), 1)
        _refused(lib, _file(bw), text)
    # an over-subscribed code length code
    bw = W.BitWriter()
    _header(bw)
    bw.put(0, 3)
    _normal_code_start(bw, [1, 1, 1, 0])
    _refused(lib, _file(bw), "over-subscribed code length code")
    # a repeat past the alphabet: code length code {0: '0', 18: '1'}, three times 138 zeros in an alphabet of 280
    bw = W.BitWriter()
    _header(bw)
    bw.put(0, 3)
    _normal_code_start(bw, [0, 1, 1, 0])
    for _ in range(3):
        bw.put(1, 1)
        bw.put(127, 7)
    _refused(lib, _file(bw), "repeat runs past the alphabet")
    # backward references out of the image
    lits = [("lit", 0xFF000000 + k) for k in range(4)]
    _refused(lib, W.write_vp8l(4, 4, script=lits + [("ref", 12, 120 + 5)], strict=False), "before the first pixel")
    _refused(lib, W.write_vp8l(4, 4, script=lits + [("ref", 13, 120 + 2)], strict=False), "past the last pixel")
    # reading past the end of the chunk is an error, not zeros
    good = W.pillow_webp(W._photo(np.random.default_rng(1), 20, 20))
    p = W.vp8l_payload(good)
    for cut in (6, len(p) // 2, len(p) - 2):
        _refused(lib, W.riff([(b"VP8L", p[:cut])]), "truncated")
    # a meta prefix image that names group 65 535 in a file that ends there: refused without allocating 65 536 groups
    bw = W.BitWriter()
    _header(bw, 8, 8)
    bw.put(0, 2)
    bw.put(1, 1)
    bw.put(0, 3)
    W.encode_stream(bw, [("lit", 0xFFFF << 8)] * 4, 2, 2)
    _refused(lib, W.riff([(b"VP8L", bw.bytes())]), "truncated")


def test_batch_errors_name_the_image(lib):
    from vipcup_amd import _abi, pipeline
    good, bad = _good(), _lossy()
    st, _, _, _ = _decode(lib, [good, good, bad, good])
    assert st == VIP_ERR_WEBP and lib.vip_last_error().decode().startswith("webp image 2: ")
    cut = good[:len(good) - 6]
    cut = cut[:4] + struct.pack("<I", len(cut) - 8) + cut[8:16] + struct.pack("<I", len(cut) - 20) + cut[20:]
    st, _, _, _ = _decode(lib, [good, cut, good], threads=3)
    assert st == VIP_ERR_WEBP and lib.vip_last_error().decode().startswith("webp image 1: ")
    with pytest.raises(_abi.VipError, match="webp image 7: .*lossy"):
        pipeline.entropy_decode_webps([good, bad, good], index=[4, 7, 9])
    with pytest.raises(_abi.VipError, match="webp image 7: .*truncated"):
        pipeline.entropy_decode_webps([good, cut, good], index=[4, 7, 9])
    with pytest.raises(_abi.VipError, match="webp image 1: .*animated"):
        pipeline.host_decode([good, _animated()])
    assert pipeline.image_format(good) == "webp"
    with pytest.raises(_abi.VipError, match=r"image 3: neither a JPEG .* PNG .* WebP"):
        pipeline.image_format(b"GIF89a", 3)
    assert isinstance(pipeline.host_decode([good, good]), pipeline.WebpStage)


def test_argument_checks_do_not_need_a_gpu(lib):
    from vipcup_amd import _abi
    good = _good()
    d = _abi.WebpDesc()
    need = C.c_size_t(0)
    assert lib.vip_webp_probe_h(None, 10, C.byref(d), C.byref(need)) == -1 and b"null" in lib.vip_last_error()
    buf = (C.c_uint8 * len(good)).from_buffer_copy(good)
    assert lib.vip_webp_probe_h(buf, len(good), None, C.byref(need)) == -1
    ptrs, lens = (C.c_void_p * 1)(C.addressof(buf)), (C.c_size_t * 1)(len(good))
    out = np.zeros(4096, np.uint32)
    used = C.c_size_t(0)
    o = out.ctypes.data_as(C.c_void_p)
    assert lib.vip_webp_entropy_h(None, lens, 1, C.byref(d), o, out.nbytes, C.byref(used), 1) == -1
    assert lib.vip_webp_entropy_h(ptrs, lens, 0, C.byref(d), o, out.nbytes, C.byref(used), 1) == -1 and b"n <= 0" in lib.vip_last_error()
    assert lib.vip_webp_entropy_h(ptrs, lens, 1, C.byref(d), None, out.nbytes, C.byref(used), 1) == -1
    assert lib.vip_webp_entropy_h(ptrs, lens, 1, C.byref(d), o, 64, C.byref(used), 1) == -1 and b"too small" in lib.vip_last_error()
    assert used.value == _probe(lib, good)[2]
    p = C.c_void_p(64)
    assert lib.vip_webp_inverse_rgb_u8(None, p, 1, p, 8, 8, None) == -1 and b"null" in lib.vip_last_error()
    assert lib.vip_webp_inverse_rgb_u8(p, p, 0, p, 8, 8, None) == -1 and b"bad size" in lib.vip_last_error()
    assert lib.vip_webp_inverse_rgb_u8(p, p, 1, p, 0, 8, None) == -1
