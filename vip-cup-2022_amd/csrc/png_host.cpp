// Host half of the PNG path: chunk walk (signature, IHDR / PLTE validation, CRC-32 of the critical chunks) and a
// self-contained inflate (RFC 1950 zlib wrapper + RFC 1951 stored / fixed / dynamic Huffman blocks, 32 KiB window,
// Adler-32) over the concatenated IDAT data - the bit-serial part of tf.image.decode_png (dataset/dataset.py:30).
// The result is the still-filtered scanline stream, (1 + rowbytes) bytes per row of every Adam7 pass in turn; the
// filters and the expansion to RGB are byte-parallel and run on the GPU (png_pipeline.hip).
//
// Ancillary chunks (gAMA, iCCP, sRGB, tRNS, tEXt, APNG acTL / fcTL / fdAT, ...) are skipped: only the default image
// is decoded, without colour management; tRNS does not matter for channels=3 (alpha is dropped).
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "host_batch.hpp"
#include "vipcup_hip.h"

void vip_set_error(const char* fmt, ...);

namespace {

using Err = host_batch::Err<VIP_ERR_PNG>;

const uint8_t SIGNATURE[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};

// Adam7: first column / row and step of each pass
const int A7_X0[7] = {0, 4, 0, 2, 0, 1, 0}, A7_Y0[7] = {0, 0, 4, 0, 2, 0, 1};
const int A7_DX[7] = {8, 8, 4, 4, 2, 2, 1}, A7_DY[7] = {8, 8, 8, 4, 4, 2, 2};

uint32_t CRC_TABLE[256];
std::once_flag crc_once;

void crc_init() {
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        CRC_TABLE[i] = c;
    }
}

uint32_t crc32(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = CRC_TABLE[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

uint64_t max_pixels() {
    const char* s = getenv("VIP_MAX_JPEG_PIXELS");      // the per-image cap of the JPEG path covers PNG too
    if (s && *s) {
        const long long v = atoll(s);
        if (v > 0) return (uint64_t)v;
    }
    return (uint64_t)64 << 20;
}

struct Chunks {
    std::vector<std::pair<size_t, size_t>> idat;   // (offset, length) of every IDAT payload, in file order
    size_t idat_bytes = 0;
};

// Walk the chunks, fill the descriptor (stream_off = 0) and the stream size.  check_crc: verify the CRC of every
// critical chunk (IHDR, PLTE, IDAT, IEND).
int parse(const uint8_t* d, size_t n, vip_png_desc* D, size_t* stream_bytes, Chunks* C, bool check_crc, Err& e) {
    if (n < 8 || memcmp(d, SIGNATURE, 8) != 0) return fail(e, "png: bad signature");
    memset(D, 0, sizeof(*D));
    bool have_ihdr = false, have_plte = false, have_iend = false, seen_idat = false;
    size_t pos = 8;
    while (pos < n) {
        if (n - pos < 12) return fail(e, "png: truncated chunk header at byte %zu", pos);
        const uint32_t len = be32(d + pos);
        const uint8_t* type = d + pos + 4;
        if (len > 0x7FFFFFFFu) return fail(e, "png: chunk length %u out of range", len);
        if ((uint64_t)len + 12 > n - pos) return fail(e, "png: truncated %.4s chunk at byte %zu", (const char*)type, pos);
        for (int k = 0; k < 4; ++k) {
            const uint8_t c = type[k];
            if (!((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'))) return fail(e, "png: bad chunk type at byte %zu", pos);
        }
        const uint8_t* body = d + pos + 8;
        const bool critical = !(type[0] & 0x20);
        if (critical && check_crc && crc32(type, (size_t)len + 4) != be32(body + len))
            return fail(e, "png: CRC mismatch in %.4s chunk", (const char*)type);
        if (!have_ihdr && memcmp(type, "IHDR", 4) != 0) return fail(e, "png: first chunk is not IHDR");
        if (memcmp(type, "IHDR", 4) == 0) {
            if (have_ihdr) return fail(e, "png: duplicate IHDR");
            if (len != 13) return fail(e, "png: IHDR length %u", len);
            const uint32_t w = be32(body), h = be32(body + 4);
            const int depth = body[8], ct = body[9];
            if (w == 0 || h == 0 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) return fail(e, "png: bad size %ux%u", w, h);
            int ch = 0;
            switch (ct) {      // PNG spec table 11.1: legal colour type / bit depth combinations
                case 0: ch = (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16) ? 1 : 0; break;
                case 2: ch = (depth == 8 || depth == 16) ? 3 : 0; break;
                case 3: ch = (depth == 1 || depth == 2 || depth == 4 || depth == 8) ? 1 : 0; break;
                case 4: ch = (depth == 8 || depth == 16) ? 2 : 0; break;
                case 6: ch = (depth == 8 || depth == 16) ? 4 : 0; break;
                default: break;
            }
            if (!ch) return fail(e, "png: illegal colour type %d / bit depth %d", ct, depth);
            if (body[10] != 0 || body[11] != 0) return fail(e, "png: unknown compression / filter method %d / %d", body[10], body[11]);
            if (body[12] > 1) return fail(e, "png: unknown interlace method %d", body[12]);
            const uint64_t cap = max_pixels();
            if ((uint64_t)w * h > cap)
                return fail(e, "png: %ux%u exceeds VIP_MAX_JPEG_PIXELS=%llu", w, h, (unsigned long long)cap);
            D->width = (int32_t)w;
            D->height = (int32_t)h;
            D->bit_depth = depth;
            D->color_type = ct;
            D->interlace = body[12];
            D->channels = ch;
            D->bpp = ch * depth >= 8 ? ch * depth / 8 : 1;
            have_ihdr = true;
        } else if (memcmp(type, "PLTE", 4) == 0) {
            if (have_plte) return fail(e, "png: duplicate PLTE");
            if (seen_idat) return fail(e, "png: PLTE after IDAT");
            if (len == 0 || len % 3 != 0 || len > 768) return fail(e, "png: PLTE length %u", len);
            have_plte = true;
            if (D->color_type == 3) {            // libpng ignores a suggested palette of a truecolour image
                D->palette_size = (int32_t)(len / 3);
                if (D->palette_size > (1 << D->bit_depth)) D->palette_size = 1 << D->bit_depth;
                memcpy(D->palette, body, (size_t)D->palette_size * 3);
            }
        } else if (memcmp(type, "IDAT", 4) == 0) {
            seen_idat = true;
            if (C) C->idat.emplace_back(pos + 8, (size_t)len);
            if (C) C->idat_bytes += len;
        } else if (memcmp(type, "IEND", 4) == 0) {
            have_iend = true;
            break;                               // trailing bytes after IEND are ignored
        } else if (critical) {
            return fail(e, "png: unknown critical chunk %.4s", (const char*)type);
        }
        pos += (size_t)len + 12;
    }
    if (!have_ihdr) return fail(e, "png: no IHDR");
    if (!seen_idat) return fail(e, "png: no IDAT");
    if (!have_iend) return fail(e, "png: truncated (no IEND)");
    if (D->color_type == 3 && D->palette_size == 0) return fail(e, "png: palette image without PLTE");
    // pass geometry and stream size (64-bit: width <= 2^31, <= 64 bits per pixel)
    uint64_t off = 0;
    const int npass = D->interlace ? 7 : 1;
    for (int p = 0; p < npass; ++p) {
        uint64_t pw = D->width, ph = D->height;
        if (D->interlace) {
            pw = D->width > A7_X0[p] ? (uint64_t)(D->width - A7_X0[p] + A7_DX[p] - 1) / A7_DX[p] : 0;
            ph = D->height > A7_Y0[p] ? (uint64_t)(D->height - A7_Y0[p] + A7_DY[p] - 1) / A7_DY[p] : 0;
            if (pw == 0) ph = 0;
            if (ph == 0) pw = 0;
        }
        D->pass_off[p] = (int64_t)off;
        D->pass_w[p] = (int32_t)pw;
        D->pass_h[p] = (int32_t)ph;
        const uint64_t rowbytes = (pw * (uint64_t)(D->channels * D->bit_depth) + 7) / 8;
        if (pw) off += ph * (1 + rowbytes);
    }
    for (int p = npass; p < 7; ++p) D->pass_off[p] = (int64_t)off;
    if (off > ((uint64_t)1 << 40)) return fail(e, "png: scanline stream too large");
    *stream_bytes = (size_t)off;
    return VIP_OK;
}

// ---- inflate (RFC 1951) ----------------------------------------------------------------------------------

constexpr int FAST_BITS = 10;

struct Huffman {
    uint16_t fast[1 << FAST_BITS];   // (length << 9) | symbol for codes of <= FAST_BITS bits, 0 = longer code
    uint16_t first_code[17], first_sym[17];
    int32_t max_code[18];            // (last code of each length + 1) << (16 - length): left-justified bound
    uint8_t size[288];
    uint16_t value[288];
};

uint32_t bit_reverse(uint32_t v, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

// canonical Huffman code from code lengths; over-subscribed sets are refused, incomplete ones too unless they are a
// single code of one bit (zlib's inflate_table rule: a distance tree with one code) - code length codes must be complete
bool build_huffman(Huffman& H, const uint8_t* lens, int n, bool lengths_code) {
    int count[17] = {0};
    for (int i = 0; i < n; ++i) ++count[lens[i]];
    count[0] = 0;
    int left = 1, maxlen = 0;
    for (int l = 1; l <= 15; ++l) {
        left <<= 1;
        left -= count[l];
        if (left < 0) return false;
        if (count[l]) maxlen = l;
    }
    if (left > 0 && (lengths_code || maxlen > 1)) return false;
    memset(H.fast, 0, sizeof(H.fast));
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
    H.max_code[16] = 0x10000;
    H.max_code[17] = 0x7FFFFFFF;
    for (int i = 0; i < n; ++i) {
        const int l = lens[i];
        if (!l) continue;
        const int c = next_code[l] - H.first_code[l] + H.first_sym[l];
        H.size[c] = (uint8_t)l;
        H.value[c] = (uint16_t)i;
        if (l <= FAST_BITS) {
            for (uint32_t j = bit_reverse((uint32_t)next_code[l], l); j < (1u << FAST_BITS); j += 1u << l)
                H.fast[j] = (uint16_t)((l << 9) | i);
        }
        ++next_code[l];
    }
    return true;
}

struct Inflater {
    const uint8_t* in;
    size_t in_len, pos = 0;       // pos: next byte to load (may run past in_len: zero bytes, counted as overrun)
    uint64_t bits = 0;
    int nbits = 0;
    uint8_t* out;
    size_t out_cap, out_pos = 0;

    void refill() {
        while (nbits <= 56) {
            const uint64_t b = pos < in_len ? in[pos] : 0;
            ++pos;
            bits |= b << nbits;
            nbits += 8;
        }
    }
    bool overrun() const { return pos > in_len && (pos - in_len) * 8 > (size_t)nbits; }   // consumed bits past the end
    uint32_t get(int n) {            // n <= 32
        if (nbits < n) refill();
        const uint32_t v = (uint32_t)(bits & ((1ull << n) - 1));
        bits >>= n;
        nbits -= n;
        return v;
    }
    int decode(const Huffman& H) {   // symbol, or -1 for a code that is not in the table
        if (nbits < 16) refill();
        const uint16_t f = H.fast[bits & ((1u << FAST_BITS) - 1)];
        if (f) {
            const int l = f >> 9;
            bits >>= l;
            nbits -= l;
            return f & 511;
        }
        const int32_t k = (int32_t)bit_reverse((uint32_t)(bits & 0xFFFF), 16);
        int l = FAST_BITS + 1;
        while (k >= H.max_code[l]) ++l;
        if (l > 15) return -1;
        const int c = (k >> (16 - l)) - H.first_code[l] + H.first_sym[l];
        if (c < 0 || c >= 288 || H.size[c] != l) return -1;
        bits >>= l;
        nbits -= l;
        return H.value[c];
    }
};

const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
                               131, 163, 195, 227, 258};
const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
                                2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
const uint8_t CLEN_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// Inflate a zlib stream into out[0, out_cap).  The output must fill out_cap exactly: a shorter stream is an error,
// compressed data beyond out_cap is ignored (libpng reads only the rows it needs).  The Adler-32 trailer is checked when
// the stream ends exactly at out_cap.
int inflate_zlib(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap, Err& e) {
    if (in_len < 2) return fail(e, "png: zlib header truncated");
    const int cmf = in[0], flg = in[1];
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0) return fail(e, "png: bad zlib header");
    if (flg & 0x20) return fail(e, "png: zlib preset dictionary");
    Inflater Z{in, in_len, 2, 0, 0, out, out_cap, 0};
    static Huffman fixed_lit, fixed_dist;
    static std::once_flag fixed_once;
    std::call_once(fixed_once, [] {
        uint8_t l[288];
        for (int i = 0; i < 288; ++i) l[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
        build_huffman(fixed_lit, l, 288, false);
        uint8_t d[32];                                       // 30 and 31 complete the code; decoding them is an error
        memset(d, 5, sizeof(d));
        build_huffman(fixed_dist, d, 32, false);
    });
    std::vector<Huffman> dyn(2);
    bool final_block = false, stream_end = false;    // stream_end: the final block was decoded to its end
    while (!final_block && Z.out_pos < out_cap) {
        final_block = Z.get(1) != 0;
        const int type = (int)Z.get(2);
        if (type == 0) {                                     // stored: byte-align, LEN, NLEN, raw bytes
            Z.get(Z.nbits & 7);
            const size_t byte_pos = Z.pos - (size_t)(Z.nbits / 8);
            Z.bits = 0;
            Z.nbits = 0;
            Z.pos = byte_pos;
            if (byte_pos + 4 > in_len) return fail(e, "png: truncated stored block");
            const uint32_t len = in[byte_pos] | (in[byte_pos + 1] << 8);
            const uint32_t nlen = in[byte_pos + 2] | (in[byte_pos + 3] << 8);
            if ((len ^ 0xFFFF) != nlen) return fail(e, "png: stored block length check failed");
            Z.pos += 4;
            if (len > in_len - Z.pos) return fail(e, "png: truncated stored block");
            const size_t take = len < out_cap - Z.out_pos ? len : out_cap - Z.out_pos;
            memcpy(out + Z.out_pos, in + Z.pos, take);
            Z.out_pos += take;
            Z.pos += len;
            stream_end = final_block && take == len;
            continue;
        }
        if (type == 3) return fail(e, "png: invalid deflate block type");
        const Huffman* lit = &fixed_lit;
        const Huffman* dist = &fixed_dist;
        if (type == 2) {
            const int hlit = (int)Z.get(5) + 257, hdist = (int)Z.get(5) + 1, hclen = (int)Z.get(4) + 4;
            if (hlit > 286 || hdist > 30) return fail(e, "png: bad dynamic block header");
            uint8_t clen[19] = {0};
            for (int i = 0; i < hclen; ++i) clen[CLEN_ORDER[i]] = (uint8_t)Z.get(3);
            Huffman hc;
            if (!build_huffman(hc, clen, 19, true)) return fail(e, "png: bad code length code");
            uint8_t lens[286 + 30];
            int k = 0;
            while (k < hlit + hdist) {
                const int sym = Z.decode(hc);
                if (sym < 0) return fail(e, "png: bad code length symbol");
                if (sym < 16) {
                    lens[k++] = (uint8_t)sym;
                    continue;
                }
                int rep = 0;
                uint8_t v = 0;
                if (sym == 16) {
                    if (k == 0) return fail(e, "png: repeat with no previous length");
                    v = lens[k - 1];
                    rep = 3 + (int)Z.get(2);
                } else if (sym == 17) {
                    rep = 3 + (int)Z.get(3);
                } else {
                    rep = 11 + (int)Z.get(7);
                }
                if (k + rep > hlit + hdist) return fail(e, "png: code lengths overflow");
                while (rep--) lens[k++] = v;
                if (Z.overrun()) return fail(e, "png: truncated deflate stream");
            }
            if (lens[256] == 0) return fail(e, "png: no end-of-block code");
            if (!build_huffman(dyn[0], lens, hlit, false)) return fail(e, "png: bad literal/length code");
            if (!build_huffman(dyn[1], lens + hlit, hdist, false)) return fail(e, "png: bad distance code");
            lit = &dyn[0];
            dist = &dyn[1];
        }
        for (;;) {                                            // Huffman-coded data
            const int sym = Z.decode(*lit);
            if (sym < 0) return fail(e, "png: bad literal/length code");
            if (sym < 256) {
                if (Z.out_pos == out_cap) break;             // more data than the image needs: ignored
                out[Z.out_pos++] = (uint8_t)sym;
                continue;
            }
            if (sym == 256) {
                stream_end = final_block;
                break;
            }
            if (sym > 285) return fail(e, "png: bad length symbol %d", sym);
            const int len = LEN_BASE[sym - 257] + (int)Z.get(LEN_EXTRA[sym - 257]);
            const int ds = Z.decode(*dist);
            if (ds < 0 || ds > 29) return fail(e, "png: bad distance code");
            const size_t d = DIST_BASE[ds] + Z.get(DIST_EXTRA[ds]);
            if (d > Z.out_pos) return fail(e, "png: distance too far back");
            if (Z.overrun()) return fail(e, "png: truncated deflate stream");
            const size_t take = (size_t)len < out_cap - Z.out_pos ? (size_t)len : out_cap - Z.out_pos;
            uint8_t* o = out + Z.out_pos;
            for (size_t i = 0; i < take; ++i) o[i] = o[(ptrdiff_t)i - (ptrdiff_t)d];
            Z.out_pos += take;
            if (Z.out_pos == out_cap && take < (size_t)len) break;
            if (Z.overrun()) return fail(e, "png: truncated deflate stream");
        }
        if (Z.overrun()) return fail(e, "png: truncated deflate stream");
    }
    if (Z.out_pos < out_cap) return fail(e, "png: inflated data too short (%zu of %zu bytes)", Z.out_pos, out_cap);
    if (stream_end) {                                         // the stream ends here: Adler-32 of the output
        Z.get(Z.nbits & 7);
        const size_t byte_pos = Z.pos - (size_t)(Z.nbits / 8);
        if (byte_pos + 4 > in_len) return fail(e, "png: zlib stream truncated before its Adler-32");
        uint32_t a = 1, b = 0;
        for (size_t i = 0; i < out_cap;) {
            const size_t end = i + 5552 < out_cap ? i + 5552 : out_cap;
            for (; i < end; ++i) {
                a += out[i];
                b += a;
            }
            a %= 65521;
            b %= 65521;
        }
        if (((b << 16) | a) != be32(in + byte_pos)) return fail(e, "png: Adler-32 mismatch");
    }
    return VIP_OK;
}

int inflate_image(const uint8_t* d, size_t n, const vip_png_desc& ref, uint8_t* out, size_t out_bytes, Err& e) {
    vip_png_desc D;
    size_t bytes = 0;
    Chunks C;
    int st = parse(d, n, &D, &bytes, &C, true, e);
    if (st != VIP_OK) return st;
    if (bytes != out_bytes || D.width != ref.width || D.height != ref.height) return fail(e, "png: stream changed since probe");
    std::vector<uint8_t> z;
    const uint8_t* zp = nullptr;
    if (C.idat.size() == 1) {
        zp = d + C.idat[0].first;
    } else {
        z.resize(C.idat_bytes);
        size_t o = 0;
        for (auto& c : C.idat) {
            memcpy(z.data() + o, d + c.first, c.second);
            o += c.second;
        }
        zp = z.data();
    }
    st = inflate_zlib(zp, C.idat_bytes, out, out_bytes, e);
    if (st != VIP_OK) return st;
    // filter types (the device trusts them)
    for (int p = 0; p < 7; ++p) {
        if (!D.pass_w[p]) continue;
        const size_t rowbytes = ((size_t)D.pass_w[p] * (size_t)(D.channels * D.bit_depth) + 7) / 8;
        for (int64_t r = 0; r < D.pass_h[p]; ++r) {
            const uint8_t f = out[D.pass_off[p] + r * (int64_t)(rowbytes + 1)];
            if (f > 4) return fail(e, "png: bad filter type %d in row %lld of pass %d", f, (long long)r, p);
        }
    }
    return VIP_OK;
}

}  // namespace

extern "C" int vip_png_probe_h(const uint8_t* png_h, size_t len, vip_png_desc* desc_h, size_t* stream_bytes_h) {
    if (!png_h || !desc_h || !stream_bytes_h) {
        vip_set_error("vip_png_probe_h: null pointer");
        return VIP_ERR_BAD_ARG;
    }
    std::call_once(crc_once, crc_init);
    Err e;
    const int st = parse(png_h, len, desc_h, stream_bytes_h, nullptr, false, e);
    if (st != VIP_OK) vip_set_error("%s", e.msg);
    return st;
}

extern "C" int vip_png_inflate_h(const uint8_t* const* png_h, const size_t* len_h, int n, vip_png_desc* desc_h,
                                 uint8_t* stream_h, size_t stream_cap, size_t* stream_used_h, int threads) {
    if (!png_h || !len_h || !desc_h || (!stream_h && stream_cap) || n < 0) {
        vip_set_error("vip_png_inflate_h: bad argument");
        return VIP_ERR_BAD_ARG;
    }
    std::call_once(crc_once, crc_init);
    // pass 1 (serial, headers only): descriptors and stream offsets
    std::vector<size_t> bytes(n);
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        Err e;
        if (!png_h[i]) {
            vip_set_error("vip_png_inflate_h: image %d: null pointer", i);
            return VIP_ERR_BAD_ARG;
        }
        const int st = parse(png_h[i], len_h[i], &desc_h[i], &bytes[i], nullptr, false, e);
        if (st != VIP_OK) {
            vip_set_error("png image %d: %s", i, e.msg);
            return st;
        }
        desc_h[i].stream_off = (int64_t)off;
        off += bytes[i];
    }
    if (stream_used_h) *stream_used_h = off;
    if (off > stream_cap) {
        vip_set_error("vip_png_inflate_h: stream buffer too small (%zu > %zu)", off, stream_cap);
        return VIP_ERR_BAD_ARG;
    }
    // pass 2: CRCs + inflate, one image at a time per worker
    if (threads < 1) threads = 1;
    if (threads > n) threads = n > 0 ? n : 1;
    const auto failed = host_batch::run<Err>(n, threads, [&](int i, Err& e) {
        return inflate_image(png_h[i], len_h[i], desc_h[i], stream_h + desc_h[i].stream_off, bytes[i], e);
    });
    if (failed.status != VIP_OK) vip_set_error("png image %d: %s", failed.index, failed.err.msg);
    return failed.status;
}
