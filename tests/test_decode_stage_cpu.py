"""CPU: the staged decode path of pipeline.py as one thing - the four host stages give the same bytes whatever the thread count,
their streams have the size the probes ask for, every refusal keeps its exact text (tests/golden/stage_messages.json, recorded
from the code before the stages were folded onto one format table) with one worker and with four, ``as_batch`` and
``host_decode`` dispatch as they always did - and csrc/host_batch.hpp, the worker loop the host files share, as a stand-alone
C++ program under the sanitizers (tests/fuzz/host_batch_check.cpp)."""
import ctypes as C
import functools
import io
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import _png as P
from tests import _vp8 as V
from tests import _webp as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "stage_messages.json")) as _f:
    MESSAGES = json.load(_f)

# format -> (host stage, descriptor, probe, stream word in bytes)
FORMATS = {"jpeg": ("entropy_decode", "JpegDesc", "vip_jpeg_probe_h", 2), "png": ("inflate_pngs", "PngDesc", "vip_png_probe_h", 4),
           "webp": ("entropy_decode_webps", "WebpDesc", "vip_webp_probe_h", 4), "vp8": ("entropy_decode_vp8s", "Vp8Desc", "vip_vp8_probe_h", 8)}


def _jpeg(i, h, w):
    """image i of tools/make_synth.py cut to h x w, saved with the quality and subsampling ``synth_jpeg`` gives it"""
    from PIL import Image
    from tools.make_synth import QUALITIES, synth_pixels
    buf = io.BytesIO()
    Image.fromarray(synth_pixels(i)[:h, :w]).save(buf, format="JPEG", quality=QUALITIES[i % 6], subsampling=0 if i % 4 == 0 else 2)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def corpora():
    """format -> 4 or 5 files of at most 65 px on a side.  The PNGs and lossless WebPs come from the tests' own writers and the lossy
    WebPs are committed fixtures, so the byte positions in the recorded messages do not hang on an encoder's version."""
    rng = np.random.default_rng(5)
    sizes = [(33, 65), (17, 15), (65, 7), (40, 48)]
    argb = [rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32) for h, w in sizes]
    green = [(W.SUBTRACT_GREEN, 0, None)]
    return {"jpeg": [_jpeg(i, h, w) for i, (h, w) in enumerate(sizes)],
            "png": [png for _, png, _ in P.corpus(seed=9, sizes=[(3, 5), (17, 13), (65, 7)])[5::23][:5]],
            "webp": [W.write_vp8l(a.shape[1], a.shape[0], a, transforms=t, cache_bits=c, rle=r, vp8x=x)
                     for a, (t, c, r, x) in zip(argb, (((), 0, False, False), (green, 4, True, False), ((), 0, True, False), (green, 0, False, True)))],
            "vp8": [raw for _, raw in V.fixture_corpus()[:4]]}


def _stage(pipeline, fmt, raws, threads, **kw):
    return getattr(pipeline, FORMATS[fmt][0])(raws, threads=threads, **kw)


def _probe_total(fmt, raws):
    from vipcup_amd import _abi
    lib = _abi.lib()
    d, need, total = getattr(_abi, FORMATS[fmt][1])(), C.c_size_t(0), 0
    for raw in raws:
        assert getattr(lib, FORMATS[fmt][2])(raw, len(raw), C.byref(d), C.byref(need)) == 0
        total += need.value
    return total


def _written(fmt, desc, stream, total):
    """The bytes of ``stream`` that the host stage wrote.  The JPEG coefficients are zeroed first and the lossy WebP stream is packed,
    so that is all of them; a PNG's scanlines fill what its probe asked for and leave the stream's last, spare word as it was
    allocated; a lossless WebP's probe is an upper bound, and what lies between an image's parts is never written or read."""
    if fmt == "png":
        return stream[:total].tobytes()
    if fmt == "webp":
        states = [W.host_state(d, stream) for d in desc]
        return b"".join(s["coded"].tobytes() + b"".join(t[3].tobytes() for t in s["transforms"] if t[3] is not None) for s in states)
    return stream.tobytes()


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_stage_bytes_do_not_depend_on_the_thread_count(fmt):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    raws = corpora()[fmt]
    assert 3 <= len(raws) <= 6
    total, word = _probe_total(fmt, raws), FORMATS[fmt][3]
    seen = []
    for threads in (1, 2, 5):
        st = _stage(pipeline, fmt, raws, threads)
        desc, stream = st if fmt == "jpeg" else (st.desc, st.stream)
        assert max(max(d.width, d.height) for d in desc) <= 65
        seen.append((bytes(desc), _written(fmt, desc, np.asarray(stream), total)))
        if fmt == "jpeg":
            assert stream.dtype == np.int16 and len(stream) == total                 # the probe counts coefficients, and all are used
        elif fmt == "vp8":                                                              # trimmed to what the images used, never empty
            last = desc[len(desc) - 1]
            used = last.stream_off + (last.coef_off + last.coef_blocks * 32 + 7) // 8 * 8
            assert len(stream) == max(used, 8) <= total
            assert stream.base.nbytes == (total + 7) // 8 * 8 + 8                       # what the C call was handed
        else:
            assert len(stream) == (total + word - 1) // word * word + word
        if fmt != "jpeg":
            assert stream.dtype == np.uint8 and stream.ctypes.data % word == 0
    assert seen[0] == seen[1] == seen[2]
    if fmt == "vp8":
        assert st.scratch_bytes == sum(d.mb_w * d.mb_h * 384 for d in st.desc)


# ---- refusals, text for text --------------------------------------------------------------------------------------------------

def _cut(fmt, raw):
    """``raw`` with the second half of its coded data missing and every container size made right again: the probe passes,
    the decode on the worker meets the end"""
    if fmt == "png":
        chunks = P.read_chunks(raw)
        idat = P.idat_stream(raw)
        head = [P.chunk(k, b) for k, b in chunks if k not in (b"IDAT", b"IEND")]
        return P.SIG + b"".join(head) + P.chunk(b"IDAT", idat[:len(idat) // 2]) + P.chunk(b"IEND", b"")
    riff = W.riff if fmt == "webp" else V.riff
    tag = b"VP8L" if fmt == "webp" else b"VP8 "
    return riff([(t, b[:len(b) // 2] if t == tag else b) for t, b in V.chunks_of(raw)])


def _huge(fmt, raw):
    """``raw`` with a header that claims more pixels than the default VIP_MAX_JPEG_PIXELS"""
    if fmt == "jpeg":
        at = next(i for i in range(2, len(raw)) if raw[i] == 0xFF and raw[i + 1] in (0xC0, 0xC1, 0xC2))
        return raw[:at + 5] + struct.pack(">HH", 65535, 65535) + raw[at + 9:]
    if fmt == "png":
        chunks = P.read_chunks(raw)
        ihdr = struct.pack(">II", 16384, 8192) + chunks[0][1][8:]
        return P.SIG + P.chunk(b"IHDR", ihdr) + b"".join(P.chunk(k, b) for k, b in chunks[1:])
    if fmt == "webp":
        return W.riff([(t, b[:1] + struct.pack("<I", (struct.unpack("<I", b[1:5])[0] | 0x0FFFFFFF)) + b[5:] if t == b"VP8L" else b)
                       for t, b in V.chunks_of(raw)])
    return V.riff([(t, b[:6] + struct.pack("<HH", 16383, 16383) + b[10:] if t == b"VP8 " else b) for t, b in V.chunks_of(raw)])


def _scan_of_fe(raw):
    """a baseline JPEG with every byte of its entropy-coded data overwritten with 0xFE"""
    at = raw.index(b"\xff\xda")
    start = at + 2 + struct.unpack(">H", raw[at + 2:at + 4])[0]
    return raw[:start] + b"\xfe" * (len(raw) - 2 - start) + raw[-2:]


def _with_cap(pipeline, cap, fn):
    old, pipeline.MAX_JPEG_PIXELS = pipeline.MAX_JPEG_PIXELS, cap
    try:
        return fn()
    finally:
        pipeline.MAX_JPEG_PIXELS = old


def _cases():
    """name -> f(pipeline, threads), each of which raises VipError"""
    c = corpora()
    cases = {}
    for fmt in ("png", "webp", "vp8"):
        a, b, bad = c[fmt][0], c[fmt][1], c[fmt][2]
        kw = {"index": [4, 7, 9]}
        cases[f"{fmt}_truncated"] = lambda p, t, fmt=fmt, r=[a, bad[:len(bad) // 2], b], kw=kw: _stage(p, fmt, r, t, **kw)
        cases[f"{fmt}_cut_data"] = lambda p, t, fmt=fmt, r=[a, _cut(fmt, bad), b], kw=kw: _stage(p, fmt, r, t, **kw)
        cases[f"{fmt}_pixel_cap"] = lambda p, t, fmt=fmt, r=[a, _huge(fmt, bad), b], kw=kw: _stage(p, fmt, r, t, **kw)
        cases[f"{fmt}_pixel_cap_of_the_caller"] = lambda p, t, fmt=fmt, r=[a, bad, b], kw=kw: _with_cap(p, 100, lambda: _stage(p, fmt, r, t, **kw))
    a, b, bad = c["jpeg"][0], c["jpeg"][1], c["jpeg"][2]
    cases["jpeg_truncated"] = lambda p, t: _stage(p, "jpeg", [a, bad[:len(bad) // 6], b], t)
    cases["jpeg_pixel_cap"] = lambda p, t: _stage(p, "jpeg", [a, _huge("jpeg", bad), b], t)
    cases["jpeg_pixel_cap_of_the_caller"] = lambda p, t: _with_cap(p, 100, lambda: _stage(p, "jpeg", [a, bad, b], t))
    cases["jpeg_scan_of_fe"] = lambda p, t: _stage(p, "jpeg", [a, _scan_of_fe(b)], t)
    mixed = [c["jpeg"][0], c["webp"][0], c["png"][0], _cut("png", c["png"][2]), c["vp8"][0], c["png"][1]]
    cases["mixed_cut_png_at_3"] = lambda p, t: p.host_decode(mixed, threads=t, lossy_webp=True)
    return cases


def record_messages():
    """name -> text, with one worker: what tests/golden/stage_messages.json holds"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    out = {}
    for name, fn in _cases().items():
        with pytest.raises(_abi.VipError) as e:
            fn(pipeline, 1)
        out[name] = str(e.value)
    return out


def test_the_golden_file_lists_every_case():
    assert sorted(MESSAGES) == sorted(_cases())


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("name", sorted(MESSAGES))
def test_refusals_keep_their_text(name, threads):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    lib = _abi.lib()
    assert lib.vip_jpeg_probe_h(None, 0, None, None) == -1          # leaves a text of its own with the calling thread: a failure on a
    assert b"null pointer" in lib.vip_last_error()                  # worker that never reaches this thread cannot pass for a stale one
    with pytest.raises(_abi.VipError) as e:
        _cases()[name](pipeline, threads)
    assert str(e.value) == MESSAGES[name]


# ---- dispatch -------------------------------------------------------------------------------------------------------------------

def test_as_batch_decodes_only_what_is_not_decoded(monkeypatch):
    import torch
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    done = pipeline.DecodedBatch(torch.zeros((1, 2, 2, 3), dtype=torch.uint8), torch.tensor([[2, 2]], dtype=torch.int32), [(2, 2)])
    calls = []
    monkeypatch.setattr(pipeline, "decode_images", lambda raws, *a, **k: calls.append(("images", raws)) or done)
    monkeypatch.setattr(pipeline, "decode_staged", lambda staged, *a, **k: calls.append(("staged", staged)) or done)
    assert pipeline.as_batch(done) is done and calls == []
    raws = corpora()["png"][:2]
    for given in (raws, tuple(raws), [bytearray(r) for r in raws]):
        assert pipeline.as_batch(given) is done and calls.pop() == ("images", given) and calls == []
    for staged in (pipeline.inflate_pngs(raws), pipeline.entropy_decode(corpora()["jpeg"][:2]), pipeline.host_decode(raws),
                   pipeline.entropy_decode_webps(corpora()["webp"][:2]), pipeline.entropy_decode_vp8s(corpora()["vp8"][:2])):
        assert pipeline.as_batch(staged) is done and calls.pop() == ("staged", staged) and calls == []


@pytest.mark.parametrize("lossy", [False, True])
def test_host_decode_returns_the_stage_types_it_always_did(lossy):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    c = corpora()
    st = pipeline.host_decode(c["jpeg"][:2], lossy_webp=lossy)
    assert isinstance(st, tuple) and len(st) == 2 and isinstance(st[0], _abi.JpegDesc * 2)
    st = pipeline.host_decode(c["png"][:3], lossy_webp=lossy)                             # all PNG: a mixed stage with one part
    assert isinstance(st, pipeline.MixedStage) and len(st) == 3 and isinstance(st.png, pipeline.PngStage) and st.png_idx == [0, 1, 2]
    assert st.jpeg is None and st.webp is None and st.vp8 is None and not st.jpeg_idx and not st.webp_idx and not st.vp8_idx
    st = pipeline.host_decode(c["webp"][:2], lossy_webp=lossy)
    assert type(st) is pipeline.WebpStage and len(st) == 2
    if lossy:
        st = pipeline.host_decode(c["vp8"][:2], lossy_webp=True)
        assert type(st) is pipeline.Vp8Stage and len(st) == 2 and st.scratch_bytes > 0
    else:
        with pytest.raises(_abi.VipError, match=r"webp image 0: .*lossy WebP \(VP8\) is not supported"):
            pipeline.host_decode(c["vp8"][:2], lossy_webp=False)
    raws = [c["webp"][0], c["jpeg"][0], c["png"][0], c["webp"][1], c["jpeg"][1]] + ([c["vp8"][0], c["vp8"][1]] if lossy else [])
    st = pipeline.host_decode(raws, lossy_webp=lossy)
    assert type(st) is pipeline.MixedStage and len(st) == st.n == len(raws)
    assert (st.png_idx, st.jpeg_idx, st.webp_idx, list(st.vp8_idx)) == ([2], [1, 4], [0, 3], [5, 6] if lossy else [])
    assert type(st.png) is pipeline.PngStage and isinstance(st.jpeg, tuple) and type(st.webp) is pipeline.WebpStage
    assert type(st.vp8) is pipeline.Vp8Stage if lossy else st.vp8 is None
    for sub, n in ((st.png, 1), (st.webp, 2), (st.jpeg[0], 2)):
        assert len(sub) == n
    assert issubclass(pipeline.PngStage, pipeline.HostStage) and not issubclass(pipeline.WebpStage, pipeline.PngStage)


# ---- csrc/host_batch.hpp ----------------------------------------------------------------------------------------------------------

def _build(tmp_path, name, sanitize):
    exe = tmp_path / name
    cmd = ["g++", "-O1", "-g", "-std=c++17", f"-fsanitize={sanitize}", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "fuzz", "host_batch_check.cpp"), "-o", str(exe), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@functools.lru_cache(maxsize=None)
def _links_with_tsan():
    """whether a trivial program links with -fsanitize=thread here (the runtime is a separate package on some systems)"""
    import tempfile
    if shutil.which("g++") is None:
        return False
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "trivial.cpp"), "w") as f:
            f.write("int main() { return 0; }\n")
        return subprocess.run(["g++", "-fsanitize=thread", os.path.join(d, "trivial.cpp"), "-o", os.path.join(d, "trivial")],
                              capture_output=True).returncode == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shared_worker_loop_reports_the_lowest_failing_item(tmp_path):
    r = subprocess.run([str(_build(tmp_path, "host_batch_asan", "address,undefined"))], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"})
    assert r.returncode == 0 and "host_batch ok" in r.stdout, (r.stdout[-500:], r.stderr[-4000:])


@pytest.mark.skipif(not _links_with_tsan(), reason="needs g++ and a ThreadSanitizer runtime to link against")
def test_shared_worker_loop_is_free_of_data_races(tmp_path):
    r = subprocess.run([str(_build(tmp_path, "host_batch_tsan", "thread"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "host_batch ok" in r.stdout, (r.stdout[-500:], r.stderr[-4000:])
