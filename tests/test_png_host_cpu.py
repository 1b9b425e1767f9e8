"""CPU: the host half of the PNG path (csrc/png_host.cpp) through ctypes on the built library - no GPU needed.  The inflated,
still-filtered scanlines equal Python's zlib.decompress of the concatenated IDAT data over the whole test corpus (every
colour type x bit depth, Adam7, stored / fixed / dynamic / RLE / Huffman-only blocks, 1-byte IDAT chunks) and over random
payloads at every window size; descriptors match IHDR / PLTE; malformed files are refused with VIP_ERR_PNG and a message."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from tests import _png

VIP_ERR_PNG = -6


@pytest.fixture(scope="module")
def lib():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, build
    build.build_lib()
    return _abi.lib()


def _probe(lib, raw):
    from vipcup_amd import _abi
    d = _abi.PngDesc()
    need = C.c_size_t(0)
    buf = (C.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
    st = lib.vip_png_probe_h(buf, len(raw), C.byref(d), C.byref(need))
    return st, d, need.value


def _inflate(lib, raws, threads=4):
    from vipcup_amd import _abi
    n = len(raws)
    bufs = [(C.c_uint8 * len(r)).from_buffer_copy(r) for r in raws]
    ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_size_t * n)(*[len(r) for r in raws])
    desc = (_abi.PngDesc * n)()
    cap = sum(_probe(lib, r)[2] for r in raws) if all(_probe(lib, r)[0] == 0 for r in raws) else 1 << 16
    out = np.zeros(max(cap, 1), np.uint8)
    used = C.c_size_t(0)
    st = lib.vip_png_inflate_h(ptrs, lens, n, desc, out.ctypes.data_as(C.c_void_p), out.size, C.byref(used), threads)
    return st, desc, out[:used.value]


def test_corpus_inflates_like_zlib(lib):
    from vipcup_amd import pipeline
    corp = _png.corpus(seed=0)
    st = pipeline.inflate_pngs([p for _, p, _ in corp], threads=16)
    stream = np.asarray(st.stream)
    for i, (name, png, _) in enumerate(corp):
        z = zlib.decompress(_png.idat_stream(png))
        d = st.desc[i]
        end = st.desc[i + 1].stream_off if i + 1 < len(corp) else d.stream_off + len(z)
        assert end - d.stream_off == len(z), name
        assert bytes(stream[d.stream_off:end]) == z, name


def test_descriptors_match_ihdr_and_plte(lib):
    for name, png, _ in _png.corpus(seed=4, sizes=[(9, 1), (17, 13)]):
        st, d, need = _probe(lib, png)
        assert st == 0, name
        chunks = dict(_png.read_chunks(png))
        w, h, depth, ct, _, _, il = struct.unpack(">IIBBBBB", chunks[b"IHDR"])
        assert (d.width, d.height, d.bit_depth, d.color_type, d.interlace) == (w, h, depth, ct, il), name
        ch = _png.CHANNELS[ct]
        assert d.channels == ch and d.bpp == max(1, ch * depth // 8), name
        total = 0
        for p, x0, y0, dx, dy, pw, ph in _png.passes(h, w, il):
            assert (d.pass_w[p], d.pass_h[p], d.pass_off[p]) == (pw, ph, total), (name, p)
            total += ph * (1 + (pw * ch * depth + 7) // 8)
        assert need == total, name
        pal = np.frombuffer(bytes(d.palette), np.uint8).reshape(256, 3)
        if ct == 3:
            plte = np.frombuffer(chunks[b"PLTE"], np.uint8).reshape(-1, 3)
            assert d.palette_size == len(plte) and np.array_equal(pal[:len(plte)], plte) and not pal[len(plte):].any(), name
        else:
            assert d.palette_size == 0 and not pal.any(), name


@pytest.mark.parametrize("wbits", range(9, 16))
def test_random_payloads_every_window(lib, wbits):
    rng = np.random.default_rng(wbits)
    raws, payloads = [], []
    for k, (h, w) in enumerate([(50, 700), (300, 257), (3, 40000)]):
        rows = []
        pool = rng.integers(0, 256, size=w, dtype=np.uint8)
        for r in range(h):                                   # noise, long repeats far back, runs: every kind of match
            kind = (r + k) % 3
            body = rng.integers(0, 256, size=w, dtype=np.uint8) if kind == 0 else (
                np.roll(pool, r) if kind == 1 else np.full(w, r % 256, np.uint8))
            rows.append(bytes([r % 5]) + body.tobytes())
        payload = b"".join(rows)
        png = _png.write_png(np.zeros((h, w, 1), np.int64), 0, 8, level=(1, 6, 9)[k], wbits=wbits, raw_stream=payload)
        raws.append(png)
        payloads.append(payload)
    st, desc, out = _inflate(lib, raws)
    assert st == 0, lib.vip_last_error()
    for i, p in enumerate(payloads):
        assert zlib.decompress(_png.idat_stream(raws[i])) == p
        assert bytes(out[desc[i].stream_off:desc[i].stream_off + len(p)]) == p


def _good():
    rng = np.random.default_rng(11)
    return _png.write_png(rng.integers(0, 256, size=(20, 30, 3)), 2, 8)


def _with_ihdr(w, h, depth, ct, il=0):
    png = _good()
    ihdr = struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, il)
    return png[:8] + _png.chunk(b"IHDR", ihdr) + png[8 + 25:]


def _bad_cases():
    good = _good()
    chunks = _png.read_chunks(good)
    z = _png.idat_stream(good)
    idat_at = 8 + 25 + 8
    crc = bytearray(good)
    crc[idat_at + 5] ^= 0x01
    short = zlib.compress(zlib.decompress(z)[:-7])
    adler = bytearray(z)
    adler[-1] ^= 0xFF
    filt = bytearray(zlib.decompress(z))
    filt[91 * 3] = 7                                          # filter byte of row 3
    rebuild = lambda zz: good[:8] + _png.chunk(b"IHDR", chunks[0][1]) + _png.chunk(b"IDAT", zz) + _png.chunk(b"IEND", b"")
    return {
        "signature": b"\x89PNG\r\n\x1a\x0b" + good[8:],
        "crc": bytes(crc),
        "ihdr_rgb_depth4": _with_ihdr(30, 20, 4, 2),
        "ihdr_palette_depth16": _with_ihdr(30, 20, 16, 3),
        "ihdr_colour_type5": _with_ihdr(30, 20, 8, 5),
        "ihdr_zero_width": _with_ihdr(0, 20, 8, 2),
        "ihdr_interlace2": _with_ihdr(30, 20, 8, 2, 2),
        "truncated_mid_idat": good[:idat_at + 20],
        "truncated_no_iend": good[:-12],
        "short_inflate": rebuild(short),
        "adler": rebuild(bytes(adler)),
        "truncated_zlib": rebuild(z[:len(z) // 2]),
        "bad_filter_type": rebuild(zlib.compress(bytes(filt))),
        "over_cap": _with_ihdr(100000, 100000, 8, 2),
        "palette_without_plte": _png.write_png(np.zeros((4, 4, 1), np.int64), 3, 8, palette=None),
        "unknown_critical_chunk": good[:8 + 25] + _png.chunk(b"ABCD", b"xyz") + good[8 + 25:],
    }


@pytest.mark.parametrize("case", sorted(_bad_cases()))
def test_malformed_files_are_refused(lib, case):
    raw = _bad_cases()[case]
    st, _, _ = _probe(lib, raw)
    if st == 0:                                               # header-valid: the inflate pass must find it
        st, _, _ = _inflate(lib, [_good(), raw], threads=2)
        msg = lib.vip_last_error().decode()
        assert "png image 1" in msg, msg
    assert st == VIP_ERR_PNG, (case, st)
    assert lib.vip_last_error().startswith(b"png"), lib.vip_last_error()


def test_pipeline_names_the_image(lib):
    from vipcup_amd import _abi, pipeline
    bad = _bad_cases()
    with pytest.raises(_abi.VipError, match="png image 4.*exceeds VIP_MAX_JPEG_PIXELS"):
        pipeline.inflate_pngs([_good(), bad["over_cap"]], index=[0, 4])
    with pytest.raises(_abi.VipError, match="png image 7.*CRC mismatch"):
        pipeline.inflate_pngs([_good(), bad["crc"]], index=[3, 7])
    with pytest.raises(_abi.VipError, match="image 1: neither"):
        pipeline.host_decode([_good(), b"BM" + bytes(60)])


def test_ancillary_chunks_are_ignored(lib):
    rng = np.random.default_rng(3)
    s = rng.integers(0, 256, size=(9, 11, 4))
    plain = _png.write_png(s, 6, 8)
    extra = [(b"gAMA", struct.pack(">I", 45455)), (b"sRGB", b"\0"), (b"tEXt", b"Comment\0hi"), (b"iCCP", b"x\0\0" + zlib.compress(b"p")),
             (b"acTL", struct.pack(">II", 1, 0)), (b"fcTL", bytes(26))]
    decorated = _png.write_png(s, 6, 8, extra_chunks=extra)
    decorated = decorated[:-12] + _png.chunk(b"fdAT", bytes(8)) + decorated[-12:]
    st, d1, o1 = _inflate(lib, [plain])
    st2, d2, o2 = _inflate(lib, [decorated])
    assert st == 0 and st2 == 0 and np.array_equal(o1, o2)
