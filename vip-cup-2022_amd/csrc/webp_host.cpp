// Host half of the lossless WebP path: the RIFF container walk (VP8L, or VP8X + VP8L; ICCP / EXIF / XMP and unknown
// chunks are skipped) and everything in a VP8L stream that is serial - the transform headers with their sub-images, the
// colour cache, the meta prefix image, the prefix codes and the LZ77 backward references.  The result is, per image,
// the still-transformed 32-bit ARGB words of the main image followed by the transforms' data (predictor / cross-colour
// sub-images, the delta-decoded palette padded to 256 entries); the inverse transforms are pixel-parallel and run on the
// GPU (webp_pipeline.hip).
//
// Lossy WebP (a `VP8 ` chunk) and animation (the VP8X animation flag, ANIM / ANMF chunks) are refused.  Every read is
// bounded by the VP8L chunk: running past its end is an error.  Recursion is two levels deep at most (the main image,
// then one sub-image), and prefix-code groups are allocated one by one as they are read.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "host_batch.hpp"
#include "vipcup_hip.h"

void vip_set_error(const char* fmt, ...);

namespace {

using Err = host_batch::Err<VIP_ERR_WEBP>;

uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint32_t le24(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }

uint64_t max_pixels() {
    const char* s = getenv("VIP_MAX_JPEG_PIXELS");      // the per-image cap of the JPEG path covers WebP too
    if (s && *s) {
        const long long v = atoll(s);
        if (v > 0) return (uint64_t)v;
    }
    return (uint64_t)64 << 20;
}

int sub_size(int n, int bits) { return (n + (1 << bits) - 1) >> bits; }

// ---- container ---------------------------------------------------------------------------------------------

// Find the VP8L chunk's payload.
int find_vp8l(const uint8_t* d, size_t n, const uint8_t** payload, size_t* payload_len, Err& e) {
    if (n < 12 || memcmp(d, "RIFF", 4) != 0 || memcmp(d + 8, "WEBP", 4) != 0) return fail(e, "webp: bad RIFF / WEBP signature");
    const uint64_t riff = le32(d + 4);
    if (riff + 8 > n) return fail(e, "webp: RIFF size %llu runs past the buffer (%zu bytes)", (unsigned long long)riff, n);
    if (riff < 4) return fail(e, "webp: RIFF size %llu too small", (unsigned long long)riff);
    const size_t end = (size_t)riff + 8;
    size_t pos = 12;
    bool first = true, extended = false;
    uint32_t canvas_w = 0, canvas_h = 0;
    while (pos + 8 <= end) {
        const uint8_t* tag = d + pos;
        const uint64_t len = le32(d + pos + 4);
        if (len > end - pos - 8) return fail(e, "webp: truncated %.4s chunk at byte %zu", (const char*)tag, pos);
        const uint8_t* body = d + pos + 8;
        if (memcmp(tag, "VP8 ", 4) == 0) return fail(e, "webp: lossy WebP (VP8) is not supported");
        if (memcmp(tag, "ANIM", 4) == 0 || memcmp(tag, "ANMF", 4) == 0) return fail(e, "webp: animated WebP is not supported");
        if (memcmp(tag, "VP8L", 4) == 0) {
            if (len < 5) return fail(e, "webp: VP8L chunk too short");
            if (body[0] != 0x2f) return fail(e, "webp: VP8L signature byte 0x%02x, expected 0x2f", body[0]);
            if (extended) {
                const uint32_t hdr = le32(body + 1);
                const uint32_t w = (hdr & 0x3fff) + 1, h = ((hdr >> 14) & 0x3fff) + 1;
                if (w != canvas_w || h != canvas_h)
                    return fail(e, "webp: VP8X canvas %ux%u differs from the VP8L size %ux%u", canvas_w, canvas_h, w, h);
            }
            *payload = body;
            *payload_len = (size_t)len;
            return VIP_OK;
        }
        if (first) {
            if (memcmp(tag, "VP8X", 4) != 0) return fail(e, "webp: first chunk is %.4s, not VP8L or VP8X: no image chunk", (const char*)tag);
            if (len < 10) return fail(e, "webp: VP8X chunk too short");
            if (body[0] & 0x02) return fail(e, "webp: animated WebP is not supported");
            canvas_w = le24(body + 4) + 1;
            canvas_h = le24(body + 7) + 1;
            extended = true;
        }
        first = false;
        pos += 8 + (size_t)len + (size_t)(len & 1);           // chunks are padded to even length
    }
    return fail(e, "webp: no image chunk (VP8L) in the file");
}

// Container + VP8L header: width, height, alpha hint; the rest of the descriptor is zero.
int parse_header(const uint8_t* d, size_t n, vip_webp_desc* D, size_t* stream_bytes, const uint8_t** payload,
                 size_t* payload_len, Err& e) {
    const uint8_t* p = nullptr;
    size_t pl = 0;
    const int st = find_vp8l(d, n, &p, &pl, e);
    if (st != VIP_OK) return st;
    const uint32_t hdr = le32(p + 1);
    const uint32_t w = (hdr & 0x3fff) + 1, h = ((hdr >> 14) & 0x3fff) + 1;
    const int version = (int)(hdr >> 29);
    if (version != 0) return fail(e, "webp: VP8L version %d, expected 0", version);
    const uint64_t cap = max_pixels();
    if ((uint64_t)w * h > cap) return fail(e, "webp: %ux%u exceeds VIP_MAX_JPEG_PIXELS=%llu", w, h, (unsigned long long)cap);
    memset(D, 0, sizeof(*D));
    D->width = (int32_t)w;
    D->height = (int32_t)h;
    D->has_alpha = (int32_t)((hdr >> 28) & 1);
    // upper bound in words: the main image, a predictor and a cross-colour sub-image (block bits >= 2), the palette
    const uint64_t words = (uint64_t)w * h + 2 * (uint64_t)sub_size((int)w, 2) * sub_size((int)h, 2) + 256;
    *stream_bytes = (size_t)(words * 4);
    if (payload) *payload = p;
    if (payload_len) *payload_len = pl;
    return VIP_OK;
}

// ---- bit reader, prefix codes ------------------------------------------------------------------------------

struct Bits {
    const uint8_t* in;
    size_t len, pos = 0;          // pos: next byte to load (may run past len: zero bytes, counted as overrun)
    uint64_t acc = 0;
    int n = 0;

    void refill() {
        while (n <= 56) {
            const uint64_t b = pos < len ? in[pos] : 0;
            ++pos;
            acc |= b << n;
            n += 8;
        }
    }
    bool overrun() const { return pos > len && (pos - len) * 8 > (size_t)n; }   // consumed bits past the end
    uint32_t get(int k) {          // k <= 32
        if (k == 0) return 0;
        if (n < k) refill();
        const uint32_t v = (uint32_t)(acc & ((1ull << k) - 1));
        acc >>= k;
        n -= k;
        return v;
    }
};

constexpr int FAST_BITS = 10;
constexpr int MAX_ALPHABET = 256 + 24 + (1 << 11);

uint32_t bit_reverse(uint32_t v, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

// canonical prefix code (by length, then by symbol; packed like deflate's).  Tables are sized by the code itself, so
// what a stream can make the decoder allocate is proportional to what it spends on describing codes.
struct Table {
    int fast_bits = 0;
    std::vector<uint16_t> fast;          // (length << 12) | symbol for codes of <= fast_bits bits, 0 = longer code
    uint16_t first_code[17], first_sym[17];
    int32_t max_code[18];                // (last code of each length + 1) << (16 - length)
    std::vector<uint16_t> value;         // symbols in code order
};

struct Code {
    int single = -1;                     // the only symbol of a one-symbol code: reading it consumes no bits
    std::unique_ptr<Table> t;
};

// 0 = ok, 1 = no symbol, 2 = over-subscribed, 3 = incomplete
int build_code(Code& C, const uint8_t* lens, int n) {
    int count[16] = {0};
    int used = 0, last = -1;
    for (int i = 0; i < n; ++i) {
        ++count[lens[i]];
        if (lens[i]) {
            ++used;
            last = i;
        }
    }
    if (used == 0) return 1;
    if (used == 1) {
        C.single = last;
        C.t.reset();
        return 0;
    }
    count[0] = 0;
    int left = 1, maxlen = 0;
    for (int l = 1; l <= 15; ++l) {
        left <<= 1;
        left -= count[l];
        if (left < 0) return 2;
        if (count[l]) maxlen = l;
    }
    if (left > 0) return 3;
    C.single = -1;
    C.t.reset(new Table);
    Table& H = *C.t;
    H.fast_bits = maxlen < FAST_BITS ? maxlen : FAST_BITS;
    H.fast.assign((size_t)1 << H.fast_bits, 0);
    H.value.assign((size_t)used, 0);
    int next_code[16];
    int code = 0, k = 0;
    for (int l = 1; l <= 15; ++l) {
        next_code[l] = code;
        H.first_code[l] = (uint16_t)code;
        H.first_sym[l] = (uint16_t)k;
        code += count[l];
        H.max_code[l] = code << (16 - l);
        code <<= 1;
        k += count[l];
    }
    H.first_code[16] = H.first_sym[16] = 0;
    H.max_code[16] = 0x10000;
    H.max_code[17] = 0x7FFFFFFF;
    for (int i = 0; i < n; ++i) {
        const int l = lens[i];
        if (!l) continue;
        const int c = next_code[l] - H.first_code[l] + H.first_sym[l];
        H.value[(size_t)c] = (uint16_t)i;
        if (l <= H.fast_bits) {
            for (uint32_t j = bit_reverse((uint32_t)next_code[l], l); j < (1u << H.fast_bits); j += 1u << l)
                H.fast[j] = (uint16_t)((l << 12) | i);
        }
        ++next_code[l];
    }
    return 0;
}

inline int read_symbol(Bits& B, const Code& C) {
    if (C.single >= 0) return C.single;
    if (B.n < 16) B.refill();
    const Table& H = *C.t;
    const uint16_t f = H.fast[B.acc & ((1u << H.fast_bits) - 1)];
    if (f) {
        const int l = f >> 12;
        B.acc >>= l;
        B.n -= l;
        return f & 0xfff;
    }
    const int32_t k = (int32_t)bit_reverse((uint32_t)(B.acc & 0xFFFF), 16);
    int l = H.fast_bits + 1;
    while (k >= H.max_code[l]) ++l;
    if (l > 15) return -1;                                   // cannot happen with a complete code
    const int c = (k >> (16 - l)) - H.first_code[l] + H.first_sym[l];
    if (c < 0 || (size_t)c >= H.value.size()) return -1;
    B.acc >>= l;
    B.n -= l;
    return H.value[(size_t)c];
}

const uint8_t CLEN_ORDER[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

int read_code(Bits& B, Code& C, int alphabet, uint8_t* lens, int* stats, Err& e) {
    memset(lens, 0, (size_t)alphabet);
    if (B.get(1)) {                                          // simple: one or two symbols
        *stats |= VIP_WEBP_STAT_SIMPLE;
        const int count = (int)B.get(1) + 1;
        const int first8 = (int)B.get(1);
        const int s0 = (int)B.get(first8 ? 8 : 1);
        if (s0 >= alphabet) return fail(e, "webp: simple code symbol %d outside its alphabet of %d", s0, alphabet);
        lens[s0] = 1;
        if (count == 2) {
            const int s1 = (int)B.get(8);
            if (s1 >= alphabet) return fail(e, "webp: simple code symbol %d outside its alphabet of %d", s1, alphabet);
            lens[s1] = 1;
        }
    } else {
        uint8_t clen[19] = {0};
        const int num = (int)B.get(4) + 4;
        for (int i = 0; i < num; ++i) clen[CLEN_ORDER[i]] = (uint8_t)B.get(3);
        if (B.overrun()) return fail(e, "webp: VP8L data truncated (in a prefix code)");
        Code L;
        const int bad = build_code(L, clen, 19);
        if (bad) return fail(e, "webp: %s code length code", bad == 1 ? "empty" : bad == 2 ? "over-subscribed" : "incomplete");
        int max_symbol = alphabet;
        if (B.get(1)) {
            *stats |= VIP_WEBP_STAT_MAX_SYMBOL;
            const int nb = 2 + 2 * (int)B.get(3);
            max_symbol = 2 + (int)B.get(nb);
            if (max_symbol > alphabet) return fail(e, "webp: max_symbol %d beyond the alphabet of %d", max_symbol, alphabet);
        }
        int k = 0, prev = 8;
        while (k < alphabet) {
            if (max_symbol-- == 0) break;
            const int s = read_symbol(B, L);
            if (s < 0) return fail(e, "webp: bad code length symbol");
            if (B.overrun()) return fail(e, "webp: VP8L data truncated (in a prefix code)");
            if (s < 16) {
                lens[k++] = (uint8_t)s;
                if (s) prev = s;
                continue;
            }
            int rep;
            uint8_t v = 0;
            if (s == 16) {
                *stats |= VIP_WEBP_STAT_REP16;
                rep = 3 + (int)B.get(2);
                v = (uint8_t)prev;
            } else if (s == 17) {
                *stats |= VIP_WEBP_STAT_REP17;
                rep = 3 + (int)B.get(3);
            } else {
                *stats |= VIP_WEBP_STAT_REP18;
                rep = 11 + (int)B.get(7);
            }
            if (k + rep > alphabet) return fail(e, "webp: code length repeat runs past the alphabet of %d", alphabet);
            while (rep--) lens[k++] = v;
        }
    }
    if (B.overrun()) return fail(e, "webp: VP8L data truncated (in a prefix code)");
    const int bad = build_code(C, lens, alphabet);
    if (bad) return fail(e, "webp: %s prefix code", bad == 1 ? "empty" : bad == 2 ? "over-subscribed" : "incomplete");
    return VIP_OK;
}

// ---- image stream ------------------------------------------------------------------------------------------

const uint8_t PLANE[120] = {
    0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a,
    0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03,
    0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e,
    0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f,
    0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e, 0x00, 0x74, 0x7c, 0x41,
    0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};

struct Group {
    Code c[5];                           // green (+ lengths + cache), red, blue, alpha, distance
};

inline uint32_t prefix_value(Bits& B, int p) {          // length or distance code from its prefix symbol
    if (p < 4) return (uint32_t)p + 1;
    const int eb = (p - 2) >> 1;
    return ((uint32_t)(2 + (p & 1)) << eb) + B.get(eb) + 1;
}

// Decode one entropy-coded image of xs x ys pixels into out.  level0: the main image, which may carry a meta prefix
// image (decoded by one nested call with level0 = false; sub-images have neither a meta image nor transforms).
int decode_stream(Bits& B, int xs, int ys, bool level0, uint32_t* out, int* stats, Err& e) {
    int cache_bits = 0;
    if (B.get(1)) {
        cache_bits = (int)B.get(4);
        if (cache_bits < 1 || cache_bits > 11) return fail(e, "webp: colour cache bits %d outside 1..11", cache_bits);
        *stats |= VIP_WEBP_STAT_CACHE;
    }
    std::vector<uint32_t> meta;
    int prefix_bits = 0, meta_w = 0;
    size_t ngroups = 1;
    if (level0 && B.get(1)) {
        *stats |= VIP_WEBP_STAT_META;
        prefix_bits = (int)B.get(3) + 2;
        meta_w = sub_size(xs, prefix_bits);
        const int meta_h = sub_size(ys, prefix_bits);
        meta.resize((size_t)meta_w * meta_h);
        const int st = decode_stream(B, meta_w, meta_h, false, meta.data(), stats, e);
        if (st != VIP_OK) return st;
        uint32_t mx = 0;
        for (uint32_t& m : meta) {
            m = (m >> 8) & 0xffff;
            if (m > mx) mx = m;
        }
        ngroups = (size_t)mx + 1;                            // <= 65 536
    }
    if (B.overrun()) return fail(e, "webp: VP8L data truncated");
    // groups are read (and allocated) one at a time, so a short stream that names group 65 535 fails early and small
    const int alphabet[5] = {256 + 24 + (cache_bits ? 1 << cache_bits : 0), 256, 256, 256, 40};
    std::vector<Group> groups;
    groups.reserve(ngroups < 64 ? ngroups : 64);
    std::vector<uint8_t> lens(MAX_ALPHABET);
    for (size_t g = 0; g < ngroups; ++g) {
        groups.emplace_back();
        for (int k = 0; k < 5; ++k) {
            const int st = read_code(B, groups.back().c[k], alphabet[k], lens.data(), stats, e);
            if (st != VIP_OK) return st;
        }
    }
    std::vector<uint32_t> cache;
    if (cache_bits) cache.assign((size_t)1 << cache_bits, 0);
    const int cache_shift = 32 - cache_bits;
    const size_t total = (size_t)xs * ys;
    const int cache_limit = 280 + (cache_bits ? 1 << cache_bits : 0);
    size_t pos = 0;
    int x = 0, y = 0;
    while (pos < total) {
        const Group& G = meta.empty() ? groups[0] : groups[meta[(size_t)(y >> prefix_bits) * meta_w + (x >> prefix_bits)]];
        const int s = read_symbol(B, G.c[0]);
        if (s < 0) return fail(e, "webp: bad prefix code in the pixel data");
        if (s < 256) {
            const int r = read_symbol(B, G.c[1]), b = read_symbol(B, G.c[2]), a = read_symbol(B, G.c[3]);
            if (r < 0 || b < 0 || a < 0) return fail(e, "webp: bad prefix code in the pixel data");
            if (B.overrun()) return fail(e, "webp: VP8L data truncated (pixel %zu of %zu)", pos, total);
            const uint32_t px = ((uint32_t)a << 24) | ((uint32_t)r << 16) | ((uint32_t)s << 8) | (uint32_t)b;
            out[pos++] = px;
            if (cache_bits) cache[(0x1e35a7bdu * px) >> cache_shift] = px;
            if (++x == xs) {
                x = 0;
                ++y;
            }
        } else if (s < 280) {
            const size_t length = prefix_value(B, s - 256);
            const int ds = read_symbol(B, G.c[4]);
            if (ds < 0) return fail(e, "webp: bad prefix code in the pixel data");
            const uint32_t dcode = prefix_value(B, ds);
            if (B.overrun()) return fail(e, "webp: VP8L data truncated (pixel %zu of %zu)", pos, total);
            size_t dist;
            if (dcode > 120) {
                dist = dcode - 120;
                *stats |= VIP_WEBP_STAT_LINEAR;
            } else {
                const int c = PLANE[dcode - 1];
                const long long d = (long long)(c >> 4) * xs + 8 - (c & 15);
                dist = d >= 1 ? (size_t)d : 1;
                *stats |= VIP_WEBP_STAT_PLANE;
            }
            if (dist > pos) return fail(e, "webp: backward reference reaches before the first pixel (distance %zu at pixel %zu)", dist, pos);
            if (length > total - pos) return fail(e, "webp: backward reference runs past the last pixel (length %zu at pixel %zu of %zu)", length, pos, total);
            for (size_t i = 0; i < length; ++i) {              // one at a time: the copy may overlap itself
                const uint32_t px = out[pos - dist];
                out[pos++] = px;
                if (cache_bits) cache[(0x1e35a7bdu * px) >> cache_shift] = px;
            }
            x += (int)length;
            while (x >= xs) {
                x -= xs;
                ++y;
            }
        } else if (s < cache_limit) {
            if (B.overrun()) return fail(e, "webp: VP8L data truncated (pixel %zu of %zu)", pos, total);
            out[pos++] = cache[(size_t)(s - 280)];
            if (++x == xs) {
                x = 0;
                ++y;
            }
        } else {
            return fail(e, "webp: green symbol %d outside its alphabet", s);
        }
    }
    if (B.overrun()) return fail(e, "webp: VP8L data truncated");
    return VIP_OK;
}

// Decode one file into its share of the batch buffer (out, out_bytes = the probe bound) and complete the descriptor.
int decode_image(const uint8_t* d, size_t n, vip_webp_desc* D, uint8_t* out, size_t out_bytes, Err& e) {
    vip_webp_desc H;
    size_t bytes = 0, pl = 0;
    const uint8_t* p = nullptr;
    int st = parse_header(d, n, &H, &bytes, &p, &pl, e);
    if (st != VIP_OK) return st;
    if (bytes != out_bytes || H.width != D->width || H.height != D->height) return fail(e, "webp: stream changed since probe");
    Bits B{p + 5, pl - 5};
    const int w = H.width, h = H.height;
    uint32_t* words = (uint32_t*)out;
    size_t next = (size_t)w * h;                             // first free word after the main image's reservation
    int stats = 0, xsize = w, seen = 0;
    D->n_transforms = 0;
    D->argb_off = 0;
    while (B.get(1)) {
        const int type = (int)B.get(2);
        if (seen & (1 << type)) return fail(e, "webp: transform type %d occurs twice", type);
        seen |= 1 << type;
        const int k = D->n_transforms++;
        D->type[k] = type;
        D->xsize[k] = xsize;
        D->bits[k] = 0;
        D->data_off[k] = 0;
        if (type == VIP_WEBP_PREDICTOR || type == VIP_WEBP_CROSS_COLOR) {
            const int bits = (int)B.get(3) + 2;
            const int sw = sub_size(xsize, bits), sh = sub_size(h, bits);
            D->bits[k] = bits;
            D->data_off[k] = (int64_t)(next * 4);
            st = decode_stream(B, sw, sh, false, words + next, &stats, e);
            if (st != VIP_OK) return st;
            next += (size_t)sw * sh;
        } else if (type == VIP_WEBP_COLOR_INDEXING) {
            const int nc = (int)B.get(8) + 1;
            const int bits = nc <= 2 ? 3 : nc <= 4 ? 2 : nc <= 16 ? 1 : 0;
            D->bits[k] = bits;
            D->data_off[k] = (int64_t)(next * 4);
            uint32_t* pal = words + next;
            st = decode_stream(B, nc, 1, false, pal, &stats, e);
            if (st != VIP_OK) return st;
            for (int i = 1; i < nc; ++i) {                   // delta-coded per byte
                const uint32_t a = pal[i], b = pal[i - 1];
                pal[i] = (((a & 0xff00ff00u) + (b & 0xff00ff00u)) & 0xff00ff00u) | (((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu);
            }
            for (int i = nc; i < 256; ++i) pal[i] = 0;
            next += 256;
            xsize = sub_size(xsize, bits);
        }
        if (B.overrun()) return fail(e, "webp: VP8L data truncated (in a transform)");
    }
    D->coded_width = xsize;
    st = decode_stream(B, xsize, h, true, words, &stats, e);
    if (st != VIP_OK) return st;
    D->stats = stats;
    return VIP_OK;
}

}  // namespace

extern "C" int vip_webp_probe_h(const uint8_t* webp_h, size_t len, vip_webp_desc* desc_h, size_t* stream_bytes_h) {
    if (!webp_h || !desc_h || !stream_bytes_h) {
        vip_set_error("vip_webp_probe_h: null pointer");
        return VIP_ERR_BAD_ARG;
    }
    Err e;
    const int st = parse_header(webp_h, len, desc_h, stream_bytes_h, nullptr, nullptr, e);
    if (st != VIP_OK) vip_set_error("%s", e.msg);
    return st;
}

extern "C" int vip_webp_entropy_h(const uint8_t* const* webp_h, const size_t* len_h, int n, vip_webp_desc* desc_h,
                                  uint8_t* stream_h, size_t stream_cap, size_t* stream_used_h, int threads) {
    if (!webp_h || !len_h || !desc_h || !stream_h || n <= 0) {
        vip_set_error("vip_webp_entropy_h: bad argument (null pointer or n <= 0)");
        return VIP_ERR_BAD_ARG;
    }
    if (((uintptr_t)stream_h & 3) != 0) {
        vip_set_error("vip_webp_entropy_h: stream buffer is not 4-byte aligned");
        return VIP_ERR_BAD_ARG;
    }
    // pass 1 (serial, headers only): sizes and stream offsets
    std::vector<size_t> bytes((size_t)n);
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        Err e;
        if (!webp_h[i]) {
            vip_set_error("vip_webp_entropy_h: image %d: null pointer", i);
            return VIP_ERR_BAD_ARG;
        }
        const int st = parse_header(webp_h[i], len_h[i], &desc_h[i], &bytes[(size_t)i], nullptr, nullptr, e);
        if (st != VIP_OK) {
            vip_set_error("webp image %d: %s", i, e.msg);
            return st;
        }
        desc_h[i].stream_off = (int64_t)off;
        off += bytes[(size_t)i];
    }
    if (stream_used_h) *stream_used_h = off;
    if (off > stream_cap) {
        vip_set_error("vip_webp_entropy_h: stream buffer too small (%zu > %zu)", off, stream_cap);
        return VIP_ERR_BAD_ARG;
    }
    // pass 2: the entropy decode, one image at a time per worker
    if (threads < 1) threads = 1;
    if (threads > n) threads = n;
    const auto failed = host_batch::run<Err>(n, threads, [&](int i, Err& e) {
        return decode_image(webp_h[i], len_h[i], &desc_h[i], stream_h + desc_h[i].stream_off, bytes[(size_t)i], e);
    });
    if (failed.status != VIP_OK) vip_set_error("webp image %d: %s", failed.index, failed.err.msg);
    return failed.status;
}
