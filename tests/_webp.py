"""Test helpers for the lossless WebP path, independent of csrc/webp_host.cpp and webp_pipeline.hip:
(a) a VP8L writer (bit writer, normal and simple prefix codes, optional colour cache, meta prefix image, backward
    references by distance code, any list of transforms in any order, optional VP8X wrapping),
(b) ``reference_state`` / ``reference_argb`` / ``reference_rgb``: a pure Python + numpy decoder,
(c) ``inverse_transforms(desc, stream)``: the numpy restatement of the device half alone, fed by the host decoder's output,
(d) ``corpus(seed, sizes)``: Pillow-encoded and hand-written files."""
import heapq
import io
import struct

import numpy as np

PREDICTOR, CROSS_COLOR, SUBTRACT_GREEN, COLOR_INDEXING = 0, 1, 2, 3
STAT_CACHE, STAT_META, STAT_SIMPLE, STAT_MAX_SYMBOL, STAT_REP16, STAT_REP17, STAT_REP18, STAT_PLANE, STAT_LINEAR = (
    1, 2, 4, 8, 16, 32, 64, 128, 256)
STAT_ALL = 511
CLEN_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
PLANE = bytes.fromhex(
    "1807171928062729161a262a38053739151b363a252b4804"
    "4749141c353b464a242c58454b343c035759131d565a232d"
    "444c555b333d68026769121e666a222e545c434d656b323e"
    "78017779535d111f646c424e767a212f757b313f636d525e"
    "00747c414f1020626e30737d515f40727e616f50717f6070")
BLACK = 0xFF000000


def sub_size(n, bits):
    return (n + (1 << bits) - 1) >> bits


def index_bits(n):
    return 3 if n <= 2 else 2 if n <= 4 else 1 if n <= 16 else 0


def plane_distance(dcode, xs):
    """(distance, is_plane_code) of a distance code value >= 1 in an image xs pixels wide"""
    if dcode > 120:
        return dcode - 120, False
    c = PLANE[dcode - 1]
    return max(1, (c >> 4) * xs + 8 - (c & 15)), True


def cache_key(argb, bits):
    return ((0x1E35A7BD * argb) & 0xFFFFFFFF) >> (32 - bits)


# ---- (a) writer ------------------------------------------------------------------------------------------------

class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0, (value, nbits)
        self.acc |= value << self.n
        self.n += nbits
        if self.n >= 64:
            k = self.n // 8
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def bytes(self):
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) // 8, "little")


def huffman_lengths(freq, limit=15):
    """code lengths (0 = unused) of a complete prefix code for the symbols with freq > 0; one symbol gets length 1"""
    freq = list(freq)
    used = [s for s, f in enumerate(freq) if f > 0]
    lens = [0] * len(freq)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    while True:
        heap = [(freq[s], s, (s,)) for s in used]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        while len(heap) > 1:
            fa, ka, a = heapq.heappop(heap)
            fb, kb, b = heapq.heappop(heap)
            for s in a + b:
                depth[s] += 1
            heapq.heappush(heap, (fa + fb, min(ka, kb), a + b))
        if max(depth.values()) <= limit:
            break
        freq = [(f + 1) // 2 + 1 if f > 0 else 0 for f in freq]       # flatten and try again
    for s in used:
        lens[s] = depth[s]
    return lens


def canonical_codes(lens):
    """{symbol: (code, length)}: by length, then by symbol"""
    codes, code, prev = {}, 0, 0
    for l, s in sorted((l, s) for s, l in enumerate(lens) if l):
        code <<= l - prev
        codes[s] = (code, l)
        code += 1
        prev = l
    return codes


def prefix_encode(v):
    """value >= 1 -> (prefix symbol, extra bits, extra value)"""
    d = v - 1
    if d < 4:
        return d, 0, 0
    hb = d.bit_length() - 1
    e = hb - 1
    return 2 * hb + ((d >> e) & 1), e, d & ((1 << e) - 1)


# code length code of the normal form: literal lengths 0..12 in 4 bits, 13..15 and the repeat codes 16..18 in 5 (complete)
_CL_LENS = [4] * 13 + [5] * 6


class PrefixCode:
    """a prefix code over an alphabet, from symbol frequencies; ``write`` emits its description, ``put`` one symbol"""

    def __init__(self, freq, simple=True, rle=False, max_symbol=False):
        freq = list(freq)
        if not any(freq):
            freq[0] = 1                                      # an unused alphabet still needs a code: the one symbol 0
        self.lens = huffman_lengths(freq)
        self.used = [s for s, l in enumerate(self.lens) if l]
        self.codes = canonical_codes(self.lens)
        self.simple = simple and len(self.used) <= 2 and all(s < 256 for s in self.used)
        self.rle, self.max_symbol = rle, max_symbol

    def write(self, bw):
        if self.simple:
            bw.put(1, 1)
            bw.put(len(self.used) - 1, 1)
            s0 = self.used[0]
            bw.put(int(s0 > 1), 1)
            bw.put(s0, 8 if s0 > 1 else 1)
            if len(self.used) == 2:
                bw.put(self.used[1], 8)
            return
        bw.put(0, 1)
        bw.put(19 - 4, 4)
        for s in CLEN_ORDER:
            bw.put(_CL_LENS[s], 3)
        cl = canonical_codes(_CL_LENS)
        toks = self._tokens()
        if self.max_symbol and len(toks) >= 2:
            bw.put(1, 1)
            nb = 2
            while (len(toks) - 2) >> nb:
                nb += 2
            bw.put((nb - 2) // 2, 3)
            bw.put(len(toks) - 2, nb)
        else:
            bw.put(0, 1)
        for sym, eb, ev in toks:
            code, l = cl[sym]
            for i in reversed(range(l)):
                bw.put((code >> i) & 1, 1)
            bw.put(ev, eb)

    def _tokens(self):
        lens = list(self.lens)
        if self.max_symbol:
            while len(lens) > 2 and lens[-1] == 0:
                lens.pop()                                   # max_symbol ends the list: trailing zeros are implied
        if not self.rle:
            return [(l, 0, 0) for l in lens]
        toks, prev, i = [], 8, 0
        while i < len(lens):
            v, n = lens[i], 1
            while i + n < len(lens) and lens[i + n] == v:
                n += 1
            i += n
            if v == 0:
                while n >= 11:
                    k = min(n, 138)
                    toks.append((18, 7, k - 11))
                    n -= k
                while n >= 3:
                    k = min(n, 10)
                    toks.append((17, 3, k - 3))
                    n -= k
            else:
                if v != prev:
                    toks.append((v, 0, 0))
                    prev = v
                    n -= 1
                while n >= 3:
                    k = min(n, 6)
                    toks.append((16, 2, k - 3))
                    n -= k
            toks += [(v, 0, 0)] * n
        return toks

    def put(self, bw, sym):
        if len(self.used) == 1:
            assert sym == self.used[0]
            return                                           # a one-symbol code costs no bits
        code, l = self.codes[sym]
        for i in reversed(range(l)):
            bw.put((code >> i) & 1, 1)


def simulate(script, xs, cache_bits=0, strict=True):
    """script: ("lit", argb) | ("ref", length, dcode) -> (tokens with colour-cache hits put in, the pixels it decodes to).
    strict=False lets a reference reach before the first pixel (for files that must be refused)."""
    px, toks = [], []
    cache = [None] * (1 << cache_bits) if cache_bits else None
    for t in script:
        if t[0] == "lit":
            v = t[1] & 0xFFFFFFFF
            if cache is not None and cache[cache_key(v, cache_bits)] == v:
                toks.append(("cache", cache_key(v, cache_bits), v))
            else:
                toks.append(("lit", v))
            px.append(v)
            if cache is not None:
                cache[cache_key(v, cache_bits)] = v
        else:
            _, length, dcode = t
            dist, _ = plane_distance(dcode, xs)
            assert dist <= len(px) or not strict, (dist, len(px))
            toks.append(("ref", length, dcode))
            for _ in range(length):
                v = px[len(px) - dist] if dist <= len(px) else 0
                px.append(v)
                if cache is not None:
                    cache[cache_key(v, cache_bits)] = v
    return toks, px


def encode_stream(bw, script, xs, ys, level0=False, cache_bits=0, meta=None, simple=True, rle=False, max_symbol=False, strict=True):
    """one entropy-coded image.  meta = (prefix_bits, group map [sub(ys)][sub(xs)]) for a level-0 stream"""
    toks, px = simulate(script, xs, cache_bits, strict)
    assert len(px) == xs * ys or not strict, (len(px), xs, ys)
    bw.put(int(cache_bits > 0), 1)
    if cache_bits:
        bw.put(cache_bits, 4)
    ngroups = 1
    if level0:
        bw.put(int(meta is not None), 1)
        if meta is not None:
            pb, gmap = meta
            gmap = np.asarray(gmap)
            assert gmap.shape == (sub_size(ys, pb), sub_size(xs, pb))
            bw.put(pb - 2, 3)
            encode_stream(bw, [("lit", int(g) << 8) for g in gmap.reshape(-1)], gmap.shape[1], gmap.shape[0], simple=simple)
            ngroups = int(gmap.max()) + 1
    else:
        assert meta is None
    sizes = (256 + 24 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)
    freq = [[[0] * n for n in sizes] for _ in range(ngroups)]
    where, pos = [], 0
    for t in toks:                                           # the group of every token, from the position it starts at
        g = int(meta[1][min(pos // xs, ys - 1) >> meta[0]][(pos % xs) >> meta[0]]) if meta is not None else 0
        where.append(g)
        f = freq[g]
        if t[0] == "lit":
            v = t[1]
            f[0][(v >> 8) & 255] += 1
            f[1][(v >> 16) & 255] += 1
            f[2][v & 255] += 1
            f[3][v >> 24] += 1
            pos += 1
        elif t[0] == "cache":
            f[0][280 + t[1]] += 1
            pos += 1
        else:
            f[0][256 + prefix_encode(t[1])[0]] += 1
            f[4][prefix_encode(t[2])[0]] += 1
            pos += t[1]
    codes = [[PrefixCode(fr, simple, rle, max_symbol) for fr in f] for f in freq]
    for group in codes:
        for c in group:
            c.write(bw)
    for t, g in zip(toks, where):
        c = codes[g]
        if t[0] == "lit":
            v = t[1]
            c[0].put(bw, (v >> 8) & 255)
            c[1].put(bw, (v >> 16) & 255)
            c[2].put(bw, v & 255)
            c[3].put(bw, v >> 24)
        elif t[0] == "cache":
            c[0].put(bw, 280 + t[1])
        else:
            p, eb, ev = prefix_encode(t[1])
            c[0].put(bw, 256 + p)
            bw.put(ev, eb)
            p, eb, ev = prefix_encode(t[2])
            c[4].put(bw, p)
            bw.put(ev, eb)


def riff(chunks):
    body = b"WEBP"
    for tag, data in chunks:
        body += tag + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")
    return b"RIFF" + struct.pack("<I", len(body)) + body


def vp8x_chunk(width, height, flags=0):
    return (b"VP8X", bytes([flags, 0, 0, 0]) + (width - 1).to_bytes(3, "little") + (height - 1).to_bytes(3, "little"))


def write_vp8l(width, height, coded=None, script=None, transforms=(), alpha=1, cache_bits=0, meta=None, simple=True, rle=False,
               max_symbol=False, vp8x=False, extra_chunks=(), strict=True):
    """A lossless WebP file.  transforms: (type, bits, data) in the order written - data is the sub-image (2-D uint32) of a
    predictor / cross-colour transform, the final colours (list of ARGB) of a colour-indexing one (bits is then derived).
    The main image is ``coded`` ([height][coded width] uint32, the values as entropy-coded: still transformed) or a
    ``script`` of ("lit", argb) / ("ref", length, distance code) items."""
    bw = BitWriter()
    bw.put(0x2F, 8)
    bw.put(width - 1, 14)
    bw.put(height - 1, 14)
    bw.put(alpha, 1)
    bw.put(0, 3)
    xs = width
    for ttype, bits, data in transforms:
        bw.put(1, 1)
        bw.put(ttype, 2)
        if ttype in (PREDICTOR, CROSS_COLOR):
            data = np.asarray(data, dtype=np.uint32)
            assert data.shape == (sub_size(height, bits), sub_size(xs, bits)), data.shape
            bw.put(bits - 2, 3)
            encode_stream(bw, [("lit", int(v)) for v in data.reshape(-1)], data.shape[1], data.shape[0], simple=simple)
        elif ttype == COLOR_INDEXING:
            pal = [int(v) & 0xFFFFFFFF for v in data]
            bw.put(len(pal) - 1, 8)
            delta = [pal[0]] + [sum((((pal[i] >> s) - (pal[i - 1] >> s)) & 255) << s for s in (0, 8, 16, 24)) for i in range(1, len(pal))]
            encode_stream(bw, [("lit", v) for v in delta], len(pal), 1, simple=simple)
            xs = sub_size(xs, index_bits(len(pal)))
    bw.put(0, 1)
    if script is None:
        coded = np.asarray(coded, dtype=np.uint32)
        assert coded.shape == (height, xs), (coded.shape, height, xs)
        script = [("lit", int(v)) for v in coded.reshape(-1)]
    encode_stream(bw, script, xs, height, level0=True, cache_bits=cache_bits, meta=meta, simple=simple, rle=rle, max_symbol=max_symbol,
                  strict=strict)
    chunks = [(b"VP8L", bw.bytes())]
    if vp8x:
        chunks = [vp8x_chunk(width, height, 0x10 if alpha else 0)] + list(extra_chunks) + chunks
    return riff(chunks)


# ---- (b) reference decoder -------------------------------------------------------------------------------------

class WebpError(ValueError):
    pass


class _Bits:
    def __init__(self, data):
        self.data, self.pos, self.acc, self.n = data, 0, 0, 0

    def _fill(self):
        chunk = self.data[self.pos:self.pos + 8]
        self.acc |= int.from_bytes(chunk, "little") << self.n
        self.n += 64                                         # past the end: zeros, found out by ``check``
        self.pos += 8

    def get(self, k):
        if self.n < k:
            self._fill()
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def check(self):
        if self.pos * 8 - self.n > len(self.data) * 8:
            raise WebpError("read past the end of the VP8L chunk")


class _Code:
    def __init__(self, lens):
        used = [s for s, l in enumerate(lens) if l]
        if not used:
            raise WebpError("empty prefix code")
        self.single = used[0] if len(used) == 1 else None
        if self.single is not None:
            return
        if sum(1 << (15 - l) for l in lens if l) != 1 << 15:
            raise WebpError("prefix code not complete")
        self.bits = max(lens)
        table = np.zeros(1 << self.bits, dtype=np.int32)
        for s, (code, l) in canonical_codes(lens).items():
            rev = int(format(code, f"0{l}b")[::-1], 2)
            table[rev::1 << l] = (l << 16) | s
        self.table = table.tolist()
        self.mask = (1 << self.bits) - 1

    def read(self, B):
        if self.single is not None:
            return self.single
        if B.n < 15:
            B._fill()
        e = self.table[B.acc & self.mask]
        l = e >> 16
        B.acc >>= l
        B.n -= l
        return e & 0xFFFF


def _read_code(B, alphabet, info):
    lens = [0] * alphabet
    if B.get(1):
        info["stats"] |= STAT_SIMPLE
        count = B.get(1) + 1
        s0 = B.get(8 if B.get(1) else 1)
        syms = [s0] + ([B.get(8)] if count == 2 else [])
        for s in syms:
            if s >= alphabet:
                raise WebpError("simple code symbol outside the alphabet")
            lens[s] = 1
    else:
        num = B.get(4) + 4
        cl = [0] * 19
        for i in range(num):
            cl[CLEN_ORDER[i]] = B.get(3)
        L = _Code(cl)
        max_symbol = alphabet
        if B.get(1):
            info["stats"] |= STAT_MAX_SYMBOL
            max_symbol = 2 + B.get(2 + 2 * B.get(3))
            if max_symbol > alphabet:
                raise WebpError("max_symbol beyond the alphabet")
        k, prev = 0, 8
        while k < alphabet and max_symbol > 0:
            max_symbol -= 1
            s = L.read(B)
            B.check()
            if s < 16:
                lens[k] = s
                k += 1
                if s:
                    prev = s
                continue
            if s == 16:
                info["stats"] |= STAT_REP16
                rep, v = 3 + B.get(2), prev
            elif s == 17:
                info["stats"] |= STAT_REP17
                rep, v = 3 + B.get(3), 0
            else:
                info["stats"] |= STAT_REP18
                rep, v = 11 + B.get(7), 0
            if k + rep > alphabet:
                raise WebpError("repeat past the alphabet")
            lens[k:k + rep] = [v] * rep
            k += rep
    B.check()
    return _Code(lens)


def _prefix_value(B, p):
    if p < 4:
        return p + 1
    e = (p - 2) >> 1
    return ((2 + (p & 1)) << e) + B.get(e) + 1


def _decode_stream(B, xs, ys, level0, info):
    cache_bits = 0
    if B.get(1):
        cache_bits = B.get(4)
        if not 1 <= cache_bits <= 11:
            raise WebpError("colour cache bits outside 1..11")
        info["stats"] |= STAT_CACHE
    meta, pb, mw = None, 0, 0
    ngroups = 1
    if level0 and B.get(1):
        info["stats"] |= STAT_META
        pb = B.get(3) + 2
        mw = sub_size(xs, pb)
        meta = [(v >> 8) & 0xFFFF for v in _decode_stream(B, mw, sub_size(ys, pb), False, info)]
        ngroups = max(meta) + 1
    sizes = (256 + 24 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)
    groups = [[_read_code(B, n, info) for n in sizes] for _ in range(ngroups)]
    cache = [0] * (1 << cache_bits) if cache_bits else None
    shift = 32 - cache_bits
    total = xs * ys
    out = []
    x = y = 0
    while len(out) < total:
        G = groups[meta[(y >> pb) * mw + (x >> pb)]] if meta is not None else groups[0]
        s = G[0].read(B)
        if s < 256:
            r = G[1].read(B)
            b = G[2].read(B)
            a = G[3].read(B)
            v = (a << 24) | (r << 16) | (s << 8) | b
            out.append(v)
            if cache is not None:
                cache[((0x1E35A7BD * v) & 0xFFFFFFFF) >> shift] = v
            adv = 1
        elif s < 280:
            length = _prefix_value(B, s - 256)
            dcode = _prefix_value(B, G[4].read(B))
            dist, plane = plane_distance(dcode, xs)
            if plane:
                info["stats"] |= STAT_PLANE
                info["plane_codes"].add(dcode)
            else:
                info["stats"] |= STAT_LINEAR
            if dist > len(out) or length > total - len(out):
                raise WebpError("backward reference out of the image")
            for _ in range(length):
                v = out[len(out) - dist]
                out.append(v)
                if cache is not None:
                    cache[((0x1E35A7BD * v) & 0xFFFFFFFF) >> shift] = v
            adv = length
        else:
            if s - 280 >= (1 << cache_bits if cache_bits else 0):
                raise WebpError("green symbol outside the alphabet")
            out.append(cache[s - 280])
            adv = 1
        x += adv
        while x >= xs:
            x -= xs
            y += 1
        B.check()
    return out


def vp8l_payload(raw):
    """the VP8L chunk's payload (container rules of the product: VP8L, or VP8X then VP8L; VP8 / animation refused)"""
    if raw[:4] != b"RIFF" or raw[8:12] != b"WEBP":
        raise WebpError("not a RIFF / WEBP file")
    end = 8 + struct.unpack("<I", raw[4:8])[0]
    if end > len(raw):
        raise WebpError("RIFF size beyond the buffer")
    pos, first = 12, True
    while pos + 8 <= end:
        tag, n = raw[pos:pos + 4], struct.unpack("<I", raw[pos + 4:pos + 8])[0]
        if tag == b"VP8 ":
            raise WebpError("lossy")
        if tag in (b"ANIM", b"ANMF") or (first and tag == b"VP8X" and raw[pos + 8] & 2):
            raise WebpError("animated")
        if tag == b"VP8L":
            return raw[pos + 8:pos + 8 + n]
        if first and tag != b"VP8X":
            raise WebpError("no image chunk")
        first = False
        pos += 8 + n + (n & 1)
    raise WebpError("no image chunk")


def reference_state(raw):
    """Decode everything serial: dict with width, height, has_alpha, coded ([h][coded width] uint32), transforms
    [(type, bits, xsize, data)] in the order read (data: 2-D sub-image, or the 256-entry palette), stats, plane_codes."""
    p = vp8l_payload(raw)
    if len(p) < 5 or p[0] != 0x2F:
        raise WebpError("bad VP8L signature")
    B = _Bits(p[1:])
    w, h = B.get(14) + 1, B.get(14) + 1
    alpha = B.get(1)
    if B.get(3) != 0:
        raise WebpError("bad version")
    info = {"stats": 0, "plane_codes": set()}
    transforms, xs, seen = [], w, set()
    while B.get(1):
        t = B.get(2)
        if t in seen:
            raise WebpError("transform twice")
        seen.add(t)
        if t in (PREDICTOR, CROSS_COLOR):
            bits = B.get(3) + 2
            sw, sh = sub_size(xs, bits), sub_size(h, bits)
            data = np.array(_decode_stream(B, sw, sh, False, info), dtype=np.uint32).reshape(sh, sw)
            transforms.append((t, bits, xs, data))
        elif t == COLOR_INDEXING:
            n = B.get(8) + 1
            bits = index_bits(n)
            pal = np.array(_decode_stream(B, n, 1, False, info), dtype=np.uint32).view(np.uint8).reshape(n, 4)
            pal = np.cumsum(pal, axis=0, dtype=np.uint8).view(np.uint32).reshape(n)
            transforms.append((t, bits, xs, np.concatenate([pal, np.zeros(256 - n, np.uint32)])))
            xs = sub_size(xs, bits)
        else:
            transforms.append((t, 0, xs, None))
    coded = np.array(_decode_stream(B, xs, h, True, info), dtype=np.uint32).reshape(h, xs)
    return {"width": w, "height": h, "has_alpha": alpha, "coded": coded, "transforms": transforms, **info}


# ---- inverse transforms (shared by (b) and (c)) ----------------------------------------------------------------

def _add(a, b):
    return (((a & 0xFF00FF00) + (b & 0xFF00FF00)) & 0xFF00FF00) | (((a & 0x00FF00FF) + (b & 0x00FF00FF)) & 0x00FF00FF)


def _avg(a, b):
    return (((a ^ b) & 0xFEFEFEFE) >> 1) + (a & b)


def _ch(v):
    return (v >> 24, (v >> 16) & 255, (v >> 8) & 255, v & 255)


def _pack(c):
    return (c[0] << 24) | (c[1] << 16) | (c[2] << 8) | c[3]


def _clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _predict(mode, L, T, TL, TR):
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _avg(_avg(L, TR), T)
    if mode == 6:
        return _avg(L, TL)
    if mode == 7:
        return _avg(L, T)
    if mode == 8:
        return _avg(TL, T)
    if mode == 9:
        return _avg(T, TR)
    if mode == 10:
        return _avg(_avg(L, TL), _avg(T, TR))
    if mode == 11:
        l, t, tl = _ch(L), _ch(T), _ch(TL)
        d = sum(abs(l[i] - tl[i]) - abs(t[i] - tl[i]) for i in range(4))
        return T if d <= 0 else L
    if mode == 12:
        l, t, tl = _ch(L), _ch(T), _ch(TL)
        return _pack([_clip(l[i] + t[i] - tl[i]) for i in range(4)])
    if mode == 13:
        a, tl = _ch(_avg(L, T)), _ch(TL)
        return _pack([_clip(a[i] + int((a[i] - tl[i]) / 2)) for i in range(4)])       # division towards zero
    return BLACK                                             # 0, 14, 15


def inverse_predictor(argb, sub, bits):
    h, w = argb.shape
    rows = argb.tolist()
    modes = ((sub >> 8) & 15).tolist()
    for y in range(h):
        row = rows[y]
        if y == 0:
            row[0] = _add(row[0], BLACK)
            for x in range(1, w):
                row[x] = _add(row[x], row[x - 1])
            continue
        top = rows[y - 1]
        m = modes[y >> bits]
        row[0] = _add(row[0], top[0])
        for x in range(1, w):
            TR = top[x + 1] if x + 1 < w else row[0]         # libwebp reads on into the current row
            row[x] = _add(row[x], _predict(m[x >> bits], row[x - 1], top[x], top[x - 1], TR))
    return np.array(rows, dtype=np.uint32)


def inverse_cross_colour(argb, sub, bits):
    h, w = argb.shape
    m = np.repeat(np.repeat(sub, 1 << bits, axis=0), 1 << bits, axis=1)[:h, :w]
    s8 = lambda v: (v & 255).astype(np.uint8).view(np.int8).astype(np.int32)     # noqa: E731
    g2r, g2b, r2b = s8(m), s8(m >> 8), s8(m >> 16)
    g = s8(argb >> 8)
    r = (((argb >> 16) & 255).astype(np.int32) + ((g2r * g) >> 5)) & 255
    b = ((argb & 255).astype(np.int32) + ((g2b * g) >> 5)) & 255
    b = (b + ((r2b * s8(r.astype(np.uint32))) >> 5)) & 255
    return (argb & np.uint32(0xFF00FF00)) | (r.astype(np.uint32) << 16) | b.astype(np.uint32)


def inverse_add_green(argb):
    g = (argb >> 8) & 255
    return (argb & np.uint32(0xFF00FF00)) | (((argb & 0x00FF00FF) + ((g << 16) | g)) & np.uint32(0x00FF00FF))


def inverse_indexing(argb, pal256, bits, width):
    h = argb.shape[0]
    x = np.arange(width)
    per = 8 >> bits
    g = (argb[:, x >> bits] >> 8) & 255
    idx = (g >> ((x & ((1 << bits) - 1)) * per).astype(np.uint32)) & ((1 << per) - 1)
    return pal256[idx].reshape(h, width)


def apply_inverse(coded, transforms):
    argb = np.asarray(coded, dtype=np.uint32)
    for t, bits, xs, data in reversed(transforms):
        if t == PREDICTOR:
            assert argb.shape[1] == xs
            argb = inverse_predictor(argb, data, bits)
        elif t == CROSS_COLOR:
            argb = inverse_cross_colour(argb, data, bits)
        elif t == SUBTRACT_GREEN:
            argb = inverse_add_green(argb)
        else:
            argb = inverse_indexing(argb, data, bits, xs)
    return argb


def argb_to_rgb(argb):
    return np.stack([(argb >> 16) & 255, (argb >> 8) & 255, argb & 255], axis=-1).astype(np.uint8)


def argb_to_rgba(argb):
    return np.stack([(argb >> 16) & 255, (argb >> 8) & 255, argb & 255, argb >> 24], axis=-1).astype(np.uint8)


def reference_argb(raw):
    s = reference_state(raw)
    return apply_inverse(s["coded"], s["transforms"])


def reference_rgb(raw):
    return argb_to_rgb(reference_argb(raw))


# ---- (c) the device half alone ---------------------------------------------------------------------------------

def host_state(desc, stream):
    """the host decoder's output (one WebpDesc, the batch's uint8 stream) in the shape of ``reference_state``"""
    stream = np.asarray(stream, dtype=np.uint8)
    words = stream[desc.stream_off:desc.stream_off + (len(stream) - desc.stream_off) // 4 * 4].view(np.uint32)
    h, cw = desc.height, desc.coded_width
    a0 = desc.argb_off // 4
    coded = words[a0:a0 + h * cw].reshape(h, cw).copy()
    transforms = []
    for k in range(desc.n_transforms):
        t, bits, xs, off = desc.type[k], desc.bits[k], desc.xsize[k], desc.data_off[k] // 4
        if t in (PREDICTOR, CROSS_COLOR):
            sh, sw = sub_size(h, bits), sub_size(xs, bits)
            transforms.append((t, bits, xs, words[off:off + sh * sw].reshape(sh, sw).copy()))
        elif t == COLOR_INDEXING:
            transforms.append((t, bits, xs, words[off:off + 256].copy()))
        else:
            transforms.append((t, 0, xs, None))
    return {"width": desc.width, "height": h, "has_alpha": desc.has_alpha, "coded": coded, "transforms": transforms,
            "stats": desc.stats}


def inverse_transforms(desc, stream):
    s = host_state(desc, stream)
    return apply_inverse(s["coded"], s["transforms"])


def same_state(a, b):
    if (a["width"], a["height"], a["has_alpha"]) != (b["width"], b["height"], b["has_alpha"]):
        return False
    if not np.array_equal(a["coded"], b["coded"]) or len(a["transforms"]) != len(b["transforms"]):
        return False
    for (t, bits, xs, d), (t2, bits2, xs2, d2) in zip(a["transforms"], b["transforms"]):
        if (t, bits, xs) != (t2, bits2, xs2) or (d is None) != (d2 is None) or (d is not None and not np.array_equal(d, d2)):
            return False
    return True


# ---- (d) corpus ------------------------------------------------------------------------------------------------

def pillow_rgba(raw):
    """(mode, pixels) as Pillow / libwebp decode the file: RGBA files keep all four channels"""
    from PIL import Image
    im = Image.open(io.BytesIO(raw))
    im.load()
    if im.mode == "RGBA":
        return "RGBA", np.array(im)
    return "RGB", np.array(im.convert("RGB"))


def pillow_rgb(raw):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(raw)).convert("RGB"))


def pillow_webp(arr, method=4, quality=75, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "WEBP", lossless=True, method=method, quality=quality, **kw)
    return buf.getvalue()


def _photo(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 9.0 + c) * np.cos(yy / 7.0 - c) for c in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def _runs(rng, h, w):
    """noise with copied runs at offsets dx -7..8, dy 0..7 (what the encoder codes with plane codes)"""
    img = rng.integers(0, 256, (h * w, 3), dtype=np.uint8)
    pos = 8 * w + 8
    while pos < h * w:
        dy, dx = int(rng.integers(0, 8)), int(rng.integers(-7, 9))
        dist = dy * w + dx
        n = int(rng.integers(4, 40))
        if dist >= 1 and dist <= pos:
            for i in range(pos, min(pos + n, h * w)):
                img[i] = img[i - dist]
        pos += n + int(rng.integers(0, 6))
    return img.reshape(h, w, 3)


def _palette(rng, h, w, n):
    colours = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    idx = rng.integers(0, n, (h, w))
    idx[:, : w // 2] = np.minimum(idx[:, : w // 2], n - 1) // 2 * 2 % n          # some structure, every colour still likely
    if h * w >= n:
        idx.reshape(-1)[:n] = np.arange(n)                  # every colour occurs
    return colours[idx]


def _gray(rng, h, w):
    g = _photo(rng, h, w)[..., 0]
    return np.stack([g, g, g], axis=-1)


def _green(rng, h, w):
    """only the green channel varies: the one kind for which the encoder writes the predictor transform alone"""
    return _photo(rng, h, w) * np.array([0, 1, 0], np.uint8)


def _flat(rng, h, w):
    return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)).copy()


def _rgba(rng, h, w):
    a = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    a[rng.random((h, w, 1)) < 0.3] = 0                      # exact=True keeps the colour under alpha 0
    return np.concatenate([_photo(rng, h, w), a], axis=-1)


KINDS = [("photo", _photo), ("runs", _runs)] + [(f"pal{n}", (lambda n: lambda r, h, w: _palette(r, h, w, n))(n))
                                                for n in (2, 3, 4, 5, 16, 17, 200)] + [("gray", _gray), ("green", _green), ("flat", _flat), ("rgba", _rgba)]
METHODS, QUALITIES = (0, 2, 4, 6), (0, 75, 100)
LARGE = 20000                                               # pixels: larger sizes are used once per kind


def pillow_corpus(seed, sizes):
    """(name, bytes) from Pillow's encoder: every kind x method x quality; the sizes go round, a size of more than
    LARGE pixels is met once per kind (the reference decoder is Python)"""
    rng = np.random.default_rng(seed)
    small = [s for s in sizes if s[0] * s[1] <= LARGE] or list(sizes)
    large = [s for s in sizes if s[0] * s[1] > LARGE]
    out = []
    for ki, (kind, make) in enumerate(KINDS):
        k = 0
        for method in METHODS:
            for quality in QUALITIES:
                if large and (method, quality) == (4, 75):
                    h, w = large[ki % len(large)]
                else:
                    h, w = small[(ki + k) % len(small)]
                k += 1
                kw = {"exact": True} if kind == "rgba" else {}
                out.append((f"{kind}_{h}x{w}_m{method}_q{quality}", pillow_webp(make(rng, h, w), method, quality, **kw)))
    h, w = small[-1]
    exif = b"Exif\0\0II*\0\x08\0\0\0\0\0\0\0\0\0"
    out.append((f"exif_{h}x{w}", pillow_webp(_photo(rng, h, w), exif=exif)))
    out.append((f"icc_{h}x{w}", pillow_webp(_photo(rng, h, w), icc_profile=bytes(range(128)) * 3 + b"\0")))
    return out


def _rand_argb(rng, h, w):
    return rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)


def _modes_image(rng, h, w, bits, mode=None):
    sh, sw = sub_size(h, bits), sub_size(w, bits)
    m = np.full((sh, sw), mode, dtype=np.uint32) if mode is not None else rng.integers(0, 16, (sh, sw)).astype(np.uint32)
    return (rng.integers(0, 1 << 32, (sh, sw), dtype=np.uint64).astype(np.uint32) & np.uint32(0xFFFFF0FF)) | (m << 8)   # mode: bits 8..11


def _plane_script(rng, xs, copy_len):
    """literals, then one backward reference for each of the 120 plane codes, a literal after each"""
    lead = 8 * xs + 9
    script = [("lit", int(v)) for v in rng.integers(0, 1 << 32, lead, dtype=np.uint64)]
    for c in range(1, 121):
        script += [("ref", copy_len, c), ("lit", int(rng.integers(0, 1 << 32, dtype=np.uint64)))]
    n = lead + 120 * (copy_len + 1)
    pad = (-n) % xs
    script += [("lit", int(v)) for v in rng.integers(0, 1 << 32, pad, dtype=np.uint64)]
    return script, (n + pad) // xs


def handwritten_corpus(seed):
    """(name, bytes, transform order) of files no encoder emits"""
    rng = np.random.default_rng(seed + 1000)
    out = []
    # every predictor mode alone, at block bits 2 and 5; the image crosses a band boundary and a block boundary
    for bits in (2, 5):
        h, w = (67, 37) if bits == 2 else (66, 35)
        for mode in range(16):
            out.append((f"hw_pred_b{bits}_m{mode}", write_vp8l(w, h, _rand_argb(rng, h, w), transforms=[(PREDICTOR, bits, _modes_image(rng, h, w, bits, mode))])))
        h, w = (130, 67)
        out.append((f"hw_pred_b{bits}_mixed", write_vp8l(w, h, _rand_argb(rng, h, w), transforms=[(PREDICTOR, bits, _modes_image(rng, h, w, bits))],
                                                         cache_bits=3 + bits, rle=True, max_symbol=(bits == 2))))
    out.append(("hw_pred_wide", write_vp8l(301, 3, _rand_argb(rng, 3, 301), transforms=[(PREDICTOR, 3, _modes_image(rng, 3, 301, 3))])))
    # transform orders the encoder never emits
    pal16 = [int(v) for v in rng.integers(0, 1 << 32, 16, dtype=np.uint64)]
    pal3 = [int(v) for v in rng.integers(0, 1 << 32, 3, dtype=np.uint64)]
    pal2 = [int(v) for v in rng.integers(0, 1 << 32, 2, dtype=np.uint64)]
    pal200 = [int(v) for v in rng.integers(0, 1 << 32, 200, dtype=np.uint64)]

    def packed(h, cw):                                       # coded pixels of an indexed image: the indices sit in green
        return (rng.integers(0, 256, (h, cw)).astype(np.uint32) << 8) | np.uint32(0xFF000000)

    h, w = 70, 45
    cw = sub_size(w, 1)
    out.append(("hw_order_30", write_vp8l(w, h, packed(h, cw), transforms=[
        (COLOR_INDEXING, 0, pal16), (PREDICTOR, 2, _modes_image(rng, h, cw, 2))])))
    out.append(("hw_order_03", write_vp8l(w, h, packed(h, cw), transforms=[(PREDICTOR, 3, _modes_image(rng, h, w, 3)), (COLOR_INDEXING, 0, pal16)])))
    out.append(("hw_order_10", write_vp8l(w, h, _rand_argb(rng, h, w), transforms=[
        (CROSS_COLOR, 2, _rand_argb(rng, sub_size(h, 2), sub_size(w, 2))), (PREDICTOR, 4, _modes_image(rng, h, w, 4))])))
    out.append(("hw_order_1", write_vp8l(w, h, _rand_argb(rng, h, w), transforms=[(CROSS_COLOR, 3, _rand_argb(rng, sub_size(h, 3), sub_size(w, 3)))])))
    out.append(("hw_order_012", write_vp8l(w, h, _rand_argb(rng, h, w), transforms=[
        (PREDICTOR, 2, _modes_image(rng, h, w, 2)), (CROSS_COLOR, 2, _rand_argb(rng, sub_size(h, 2), sub_size(w, 2))), (SUBTRACT_GREEN, 0, None)])))
    cw = sub_size(w, 2)
    out.append(("hw_order_3012", write_vp8l(w, h, packed(h, cw), transforms=[
        (COLOR_INDEXING, 0, pal3), (PREDICTOR, 2, _modes_image(rng, h, cw, 2)),
        (CROSS_COLOR, 2, _rand_argb(rng, sub_size(h, 2), sub_size(cw, 2))), (SUBTRACT_GREEN, 0, None)])))
    cw = sub_size(w, 3)
    out.append(("hw_order_1203", write_vp8l(w, h, packed(h, cw), transforms=[
        (CROSS_COLOR, 2, _rand_argb(rng, sub_size(h, 2), sub_size(w, 2))), (SUBTRACT_GREEN, 0, None),
        (PREDICTOR, 2, _modes_image(rng, h, w, 2)), (COLOR_INDEXING, 0, pal2)])))
    out.append(("hw_order_23", write_vp8l(w, h, packed(h, w), transforms=[(SUBTRACT_GREEN, 0, None), (COLOR_INDEXING, 0, pal200)], vp8x=True)))
    # a palette index past the table: 5 colours in 4-bit indices, 200 colours in 8-bit indices
    pal5 = [int(v) | 0xFF000000 for v in rng.integers(0, 1 << 24, 5, dtype=np.uint64)]
    out.append(("hw_index_past_5", write_vp8l(21, 9, packed(9, 11), transforms=[(COLOR_INDEXING, 0, pal5)])))
    out.append(("hw_index_past_200", write_vp8l(21, 9, packed(9, 21), transforms=[(COLOR_INDEXING, 0, pal200)])))
    # backward references: each of the 120 plane codes on a 40-wide and on a 3-wide image (distances clamp to 1 there),
    # an overlapping copy, a linear distance; with a meta prefix image and a colour cache
    for xs, n in ((40, 3), (3, 2)):
        script, ys = _plane_script(rng, xs, n)
        out.append((f"hw_plane_w{xs}", write_vp8l(xs, ys, script=script)))
    script = [("lit", 0xFF112233), ("ref", 50, 121)] + [("lit", int(v)) for v in rng.integers(0, 1 << 32, 9, dtype=np.uint64)] + \
             [("ref", 30, 120 + 7), ("ref", 30, 120 + 45)]
    out.append(("hw_overlap", write_vp8l(12, 10, script=script)))
    h, w = 40, 50
    px = (rng.integers(0, 4, h * w) * 0x00404040 + 0xFF000000).tolist()
    gmap = rng.integers(0, 5, (sub_size(h, 3), sub_size(w, 3)))
    gmap[0, 0] = 4
    out.append(("hw_meta_cache", write_vp8l(w, h, script=[("lit", v) for v in px], cache_bits=4, meta=(3, gmap), rle=True, max_symbol=True, alpha=0)))
    return out


_CORPUS = {}


def corpus(seed, sizes):
    """list of (name, bytes): Pillow's encoder over kinds x methods x qualities, then the hand-written files (cached)"""
    key = (seed, tuple(sizes))
    if key not in _CORPUS:
        _CORPUS[key] = pillow_corpus(seed, list(sizes)) + handwritten_corpus(seed)
    return _CORPUS[key]


SIZES = [(1, 1), (1, 9), (13, 1), (64, 5), (65, 7), (130, 67), (200, 200)]
