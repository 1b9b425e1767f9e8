"""Test helpers for the PNG path: a tiny PNG writer (struct + zlib) that picks the filter type per row, cycling all five,
and a pure-Python reference decoder (chunk walk, zlib.decompress, unfilter, expansion to 8-bit RGB by the rules of
tf.image.decode_png(channels=3) / libpng: gray 1/2/4 by bit replication, palette via PLTE (index past it = black),
alpha dropped, tRNS ignored, 16-bit samples -> round(v / 257)).  Independent of csrc/png_host.cpp and png_pipeline.hip."""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
LEGAL = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
# Adam7: (x0, y0, dx, dy) of each pass
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]


def chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def _pack_row(samples: np.ndarray, depth: int) -> bytes:
    """one row of samples [w, ch] -> scanline bytes (big-endian 16-bit, sub-byte depths MSB first, row padded)"""
    flat = samples.reshape(-1).astype(np.int64)
    if depth == 16:
        return flat.astype(">u2").tobytes()
    if depth == 8:
        return flat.astype(np.uint8).tobytes()
    per = 8 // depth
    n = (len(flat) + per - 1) // per
    out = bytearray(n)
    for i, v in enumerate(flat):
        out[i // per] |= int(v) << (8 - depth * (i % per + 1))
    return bytes(out)


def _filter_row(ft: int, raw: bytes, prev: bytes, bpp: int) -> bytes:
    """encode one row (every predictor input is known here, so this is vectorised; decoding is the serial direction)"""
    x = np.frombuffer(raw, dtype=np.uint8).astype(np.int64)
    b = np.frombuffer(prev, dtype=np.uint8).astype(np.int64)
    a = np.concatenate([np.zeros(min(bpp, len(x)), np.int64), x[:-bpp] if len(x) > bpp else x[:0]])
    c = np.concatenate([np.zeros(min(bpp, len(b)), np.int64), b[:-bpp] if len(b) > bpp else b[:0]])
    if ft == 4:
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    else:
        pred = (np.zeros_like(x), a, b, (a + b) >> 1)[ft]
    return ((x - pred) & 255).astype(np.uint8).tobytes()


def passes(h: int, w: int, interlace: int):
    """(pass index, x0, y0, dx, dy, pass width, pass height) of every non-empty pass"""
    if not interlace:
        return [(0, 0, 0, 1, 1, w, h)]
    out = []
    for p, (x0, y0, dx, dy) in enumerate(ADAM7):
        pw = (w - x0 + dx - 1) // dx if w > x0 else 0
        ph = (h - y0 + dy - 1) // dy if h > y0 else 0
        if pw and ph:
            out.append((p, x0, y0, dx, dy, pw, ph))
    return out


def scanlines(samples: np.ndarray, depth: int, interlace: int, filter_seed: int = 0) -> bytes:
    """the filtered scanline stream of an image: samples [h, w, ch] (or palette indices [h, w, 1])"""
    h, w, ch = samples.shape
    bpp = max(1, ch * depth // 8)
    out = bytearray()
    for p, x0, y0, dx, dy, pw, ph in passes(h, w, interlace):
        sub = samples[y0::dy, x0::dx][:ph, :pw]
        prev = None
        for r in range(ph):
            raw = _pack_row(sub[r], depth)
            if prev is None:
                prev = bytes(len(raw))
            ft = (r + p + filter_seed) % 5                      # every filter type, on every row position
            out.append(ft)
            out += _filter_row(ft, raw, prev, bpp)
            prev = raw
    return bytes(out)


def write_png(samples: np.ndarray, color_type: int, depth: int, interlace: int = 0, palette=None, trns=None,
              level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, wbits: int = 15, idat_chunk=None,
              filter_seed: int = 0, extra_chunks=(), raw_stream=None) -> bytes:
    """PNG bytes.  samples uint [h, w, CHANNELS[color_type]] within the bit depth; ``idat_chunk`` splits the zlib stream
    into IDAT chunks of that many bytes; ``raw_stream`` replaces the filtered scanlines (random payload tests)."""
    h, w = samples.shape[:2]
    ihdr = struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, interlace)
    data = raw_stream if raw_stream is not None else scanlines(samples, depth, interlace, filter_seed)
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    z = co.compress(data) + co.flush()
    out = SIG + chunk(b"IHDR", ihdr)
    for kind, body in extra_chunks:
        out += chunk(kind, body)
    if palette is not None:
        out += chunk(b"PLTE", bytes(np.asarray(palette, dtype=np.uint8).reshape(-1)))
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    step = idat_chunk or max(len(z), 1)
    for i in range(0, max(len(z), 1), step):
        out += chunk(b"IDAT", z[i:i + step])
    return out + chunk(b"IEND", b"")


# ---- reference decoder ----------------------------------------------------------------------------------------------

def read_chunks(png: bytes):
    assert png[:8] == SIG
    pos, out = 8, []
    while pos < len(png):
        n = struct.unpack(">I", png[pos:pos + 4])[0]
        out.append((png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]))
        pos += 12 + n
        if out[-1][0] == b"IEND":
            break
    return out


def idat_stream(png: bytes) -> bytes:
    return b"".join(body for kind, body in read_chunks(png) if kind == b"IDAT")


def _unfilter(stream: bytes, pos: int, ph: int, rowbytes: int, bpp: int):
    rows, prev = [], bytearray(rowbytes)
    for _ in range(ph):
        ft = stream[pos]
        line = bytearray(stream[pos + 1:pos + 1 + rowbytes])
        pos += 1 + rowbytes
        if ft == 1:
            for x in range(bpp, rowbytes):
                line[x] = (line[x] + line[x - bpp]) & 255
        elif ft == 2:
            line = bytearray(((np.frombuffer(bytes(line), np.uint8).astype(np.int32) +
                               np.frombuffer(bytes(prev), np.uint8)) & 255).astype(np.uint8).tobytes())
        elif ft == 3:
            for x in range(rowbytes):
                a = line[x - bpp] if x >= bpp else 0
                line[x] = (line[x] + ((a + prev[x]) >> 1)) & 255
        elif ft == 4:
            for x in range(rowbytes):
                a = line[x - bpp] if x >= bpp else 0
                c = prev[x - bpp] if x >= bpp else 0
                line[x] = (line[x] + _paeth(a, prev[x], c)) & 255
        else:
            assert ft == 0, ft
        rows.append(bytes(line))
        prev = line
    return rows, pos


def _samples(row: bytes, pw: int, ch: int, depth: int) -> np.ndarray:
    b = np.frombuffer(row, dtype=np.uint8)
    if depth == 16:
        return b.view(">u2").astype(np.int64).reshape(pw, ch)
    if depth == 8:
        return b.astype(np.int64).reshape(pw, ch)
    bits = np.unpackbits(b).reshape(-1, depth)
    vals = np.zeros(len(bits), dtype=np.int64)
    for k in range(depth):
        vals = (vals << 1) | bits[:, k]
    return vals[:pw].reshape(pw, 1)


def expand(samples: np.ndarray, color_type: int, depth: int, palette=None) -> np.ndarray:
    """samples [h, w, ch] -> uint8 RGB [h, w, 3] (the rules of the module docstring)"""
    s = samples.astype(np.int64)
    if color_type == 3:
        pal = np.zeros((256, 3), dtype=np.uint8)                # an index past PLTE is black
        p = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
        pal[:len(p)] = p
        return pal[s[..., 0]]
    if depth == 16:
        s = np.floor(s / 257.0 + 0.5).astype(np.int64)          # round(v / 257)
    elif depth < 8:
        s = s * (255 // ((1 << depth) - 1))                     # bit replication: x255, x85, x17
    if CHANNELS[color_type] >= 3:
        return s[..., :3].astype(np.uint8)
    return np.repeat(s[..., :1], 3, axis=-1).astype(np.uint8)


def reference_rgb(png: bytes) -> np.ndarray:
    """pure-Python decode of a PNG to uint8 RGB [h, w, 3]"""
    chunks = read_chunks(png)
    w, h, depth, ct, _, _, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    palette = next((body for kind, body in chunks if kind == b"PLTE"), None)
    ch = CHANNELS[ct]
    bpp = max(1, ch * depth // 8)
    stream = zlib.decompress(idat_stream(png))
    samples = np.zeros((h, w, ch), dtype=np.int64)
    pos = 0
    for p, x0, y0, dx, dy, pw, ph in passes(h, w, interlace):
        rowbytes = (pw * ch * depth + 7) // 8
        rows, pos = _unfilter(stream, pos, ph, rowbytes, bpp)
        for r, row in enumerate(rows):
            samples[y0 + r * dy, x0::dx][:pw] = _samples(row, pw, ch, depth)
    pal = None if palette is None else np.frombuffer(palette, dtype=np.uint8).reshape(-1, 3)
    return expand(samples, ct, depth, pal)


# ---- corpus ---------------------------------------------------------------------------------------------------------

SIZES = [(1, 1), (1, 9), (9, 1), (3, 5), (17, 13), (64, 7), (65, 7), (129, 31), (200, 200), (7, 1500)]   # (h, w)
KINDS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16),
         (6, 8), (6, 16)]
COMPRESSION = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY),
               (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_RLE), (6, zlib.Z_HUFFMAN_ONLY)]


def random_samples(rng, h, w, ch, depth, flat: bool):
    """noise, or (``flat``) values from a narrow range with repeated rows and columns: many Paeth ties"""
    top = (1 << depth) - 1
    if not flat:
        return rng.integers(0, top + 1, size=(h, w, ch))
    base = rng.integers(0, top + 1, size=(1, 1, ch))
    s = (base + rng.integers(0, 3, size=(h, w, ch))) % (top + 1)
    for r in range(1, h, 3):                                       # repeated rows (Up / Paeth with b == c)
        s[r] = s[r - 1]
    for c in range(2, w, 4):                                       # repeated columns (Sub / Paeth with a == c)
        s[:, c] = s[:, c - 1]
    return s


def make_image(rng, h, w, ct, depth, interlace, k, trns=False):
    """(png bytes, expected rgb) of one corpus entry; k picks the compression setting and the IDAT split"""
    ch = CHANNELS[ct]
    palette = None
    if ct == 3:
        n_pal = min(1 << depth, 1 + int(rng.integers(0, 1 << depth)))
        palette = rng.integers(0, 256, size=(n_pal, 3))
        samples = rng.integers(0, n_pal, size=(h, w, 1))
    else:
        samples = random_samples(rng, h, w, ch, depth, flat=bool(k % 2))
    level, strategy = COMPRESSION[k % len(COMPRESSION)]
    split = (None, 1, 97)[k % 3]
    raw_size = sum(ph * (1 + (pw * ch * depth + 7) // 8) for *_, pw, ph in passes(h, w, interlace))
    if split == 1 and raw_size > 4096:
        split = 61
    t = None
    if trns and ct == 3:
        t = rng.integers(0, 256, size=len(palette)).astype(np.uint8).tobytes()
    png = write_png(samples, ct, depth, interlace, palette=palette, trns=t, level=level, strategy=strategy,
                    idat_chunk=split, filter_seed=k)
    return png, expand(samples, ct, depth, palette)


def corpus(seed: int = 0, sizes=SIZES):
    """every legal colour type x bit depth (palette with and without tRNS), non-interlaced and Adam7, at every size:
    list of (name, png bytes, expected rgb)"""
    rng = np.random.default_rng(seed)
    out, k = [], 0
    for ct, depth in KINDS:
        for trns in ((False, True) if ct == 3 else (False,)):
            for interlace in (0, 1):
                for h, w in sizes:
                    png, rgb = make_image(rng, h, w, ct, depth, interlace, k, trns)
                    out.append((f"ct{ct}_d{depth}{'_trns' if trns else ''}_i{interlace}_{h}x{w}", png, rgb))
                    k += 1
    return out
