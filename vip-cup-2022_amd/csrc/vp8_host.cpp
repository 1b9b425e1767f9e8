// Host half of the lossy WebP path: the RIFF container walk (a `VP8 ` chunk, alone or behind VP8X; ALPH / ICCP / EXIF / XMP
// and unknown chunks are skipped) and everything in a VP8 key frame (RFC 6386) that the boolean decoder carries - the frame
// header (segments, filter, partitions, quantisers, probability updates), per macroblock the segment, skip flag and
// prediction modes from the first partition and the residual tokens from the macroblock row's token partition.  The
// coefficients are dequantised here, as libwebp does it, and every macroblock gets a fixed-size record with all the
// device needs: modes, the filter parameters already resolved, which blocks are coded.  Prediction, the inverse
// transforms, the in-loop filter and the conversion to RGB are pixel work and run on the GPU (vp8_pipeline.hip).
//
// Reads past the end of a partition follow libwebp: the boolean decoder takes one zero byte past the end and then flags
// the partition as exhausted, which is an error once the macroblock is done.  Plain C++, no HIP: tests/fuzz/vp8_fuzz.cpp
// compiles this file alone.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "host_batch.hpp"
#include "vipcup_hip.h"
#include "vp8_params.hpp"
#include "vp8_tables.hpp"

void vip_set_error(const char* fmt, ...);

namespace {

using namespace vp8_tables;

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

const uint8_t ZIGZAG[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
const uint8_t BANDS[17] = {0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7, 0};      // [16]: read after the last coefficient, never used
const uint8_t CAT3[] = {173, 148, 140, 0};
const uint8_t CAT4[] = {176, 155, 140, 135, 0};
const uint8_t CAT5[] = {180, 157, 141, 134, 130, 0};
const uint8_t CAT6[] = {254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129, 0};
const uint8_t* const CAT3456[4] = {CAT3, CAT4, CAT5, CAT6};

// ---- container ---------------------------------------------------------------------------------------------

struct Frame {
    const uint8_t* part0 = nullptr;      // first partition
    size_t part0_len = 0;
    const uint8_t* rest = nullptr;       // what follows it in the chunk: partition sizes, token partitions
    size_t rest_len = 0;
    int width = 0, height = 0, has_alpha = 0;
};

int find_frame(const uint8_t* d, size_t n, Frame& F, Err& e) {
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
        if (memcmp(tag, "VP8L", 4) == 0) return fail(e, "webp: a lossless (VP8L) file on the lossy path");
        if (memcmp(tag, "ANIM", 4) == 0 || memcmp(tag, "ANMF", 4) == 0) return fail(e, "webp: animated WebP is not supported");
        if (memcmp(tag, "VP8 ", 4) == 0) {
            if (len < 10) return fail(e, "webp: VP8 chunk too short");
            const uint32_t bits = le24(body);
            if (bits & 1) return fail(e, "webp: VP8 inter frame (only key frames are images)");
            const int profile = (int)((bits >> 1) & 7);
            if (profile > 3) return fail(e, "webp: VP8 profile %d, expected 0..3", profile);
            if (!((bits >> 4) & 1)) return fail(e, "webp: VP8 frame is not shown");
            const size_t part0 = bits >> 5;
            if (body[3] != 0x9d || body[4] != 0x01 || body[5] != 0x2a) return fail(e, "webp: bad VP8 key frame start code");
            const uint32_t w = (uint32_t)(body[6] | (body[7] << 8)) & 0x3fff;       // the two scale bits above are ignored
            const uint32_t h = (uint32_t)(body[8] | (body[9] << 8)) & 0x3fff;
            if (w == 0 || h == 0) return fail(e, "webp: VP8 frame of %ux%u pixels", w, h);
            if (part0 > len - 10) return fail(e, "webp: VP8 first partition (%zu bytes) runs past the chunk", part0);
            if (extended && (w != canvas_w || h != canvas_h))
                return fail(e, "webp: VP8X canvas %ux%u differs from the VP8 size %ux%u", canvas_w, canvas_h, w, h);
            F.part0 = body + 10;
            F.part0_len = part0;
            F.rest = body + 10 + part0;
            F.rest_len = (size_t)len - 10 - part0;
            F.width = (int)w;
            F.height = (int)h;
            return VIP_OK;
        }
        if (first) {
            if (memcmp(tag, "VP8X", 4) != 0) return fail(e, "webp: first chunk is %.4s, not VP8 or VP8X: no image chunk", (const char*)tag);
            if (len < 10) return fail(e, "webp: VP8X chunk too short");
            if (body[0] & 0x02) return fail(e, "webp: animated WebP is not supported");
            F.has_alpha = (body[0] >> 4) & 1;
            canvas_w = le24(body + 4) + 1;
            canvas_h = le24(body + 7) + 1;
            extended = true;
        }
        first = false;
        pos += 8 + (size_t)len + (size_t)(len & 1);           // chunks are padded to even length
    }
    return fail(e, "webp: no image chunk (VP8) in the file");
}

constexpr size_t MB_BOUND = sizeof(vip_vp8_mb) + 25 * 32;      // a record and every block coded

int parse_header(const uint8_t* d, size_t n, vip_vp8_desc* D, size_t* stream_bytes, Frame& F, Err& e) {
    const int st = find_frame(d, n, F, e);
    if (st != VIP_OK) return st;
    const uint64_t cap = max_pixels();
    if ((uint64_t)F.width * F.height > cap)
        return fail(e, "webp: %dx%d exceeds VIP_MAX_JPEG_PIXELS=%llu", F.width, F.height, (unsigned long long)cap);
    memset(D, 0, sizeof(*D));
    D->width = F.width;
    D->height = F.height;
    D->mb_w = (F.width + 15) >> 4;
    D->mb_h = (F.height + 15) >> 4;
    D->has_alpha = F.has_alpha;
    *stream_bytes = (size_t)D->mb_w * D->mb_h * MB_BOUND + 8;
    return VIP_OK;
}

// ---- boolean decoder (libwebp's arithmetic: range - 1 is kept, bytes are taken when they are needed) --------------

struct Bool {
    const uint8_t* buf;
    const uint8_t* end;
    uint64_t value = 0;
    uint32_t range = 254;
    int bits = -8;
    bool eof = false;

    Bool(const uint8_t* p, size_t n) : buf(p), end(p + n) {}
    void load() {
        if (end - buf >= 4) {
            value = (value << 32) | ((uint64_t)buf[0] << 24) | ((uint64_t)buf[1] << 16) | ((uint64_t)buf[2] << 8) | buf[3];
            buf += 4;
            bits += 32;
        } else if (buf < end) {
            value = (value << 8) | *buf++;
            bits += 8;
        } else if (!eof) {
            value <<= 8;
            bits += 8;
            eof = true;
        } else {
            bits = 0;
        }
    }
    int bit(int prob) {
        if (bits < 0) load();
        const uint32_t split = (range * (uint32_t)prob) >> 8;
        const uint32_t v = (uint32_t)(value >> bits);
        int b;
        if (v > split) {
            range -= split;
            value -= (uint64_t)(split + 1) << bits;
            b = 1;
        } else {
            range = split + 1;
            b = 0;
        }
        const int shift = 7 ^ (31 - __builtin_clz(range));
        range <<= shift;
        bits -= shift;
        range -= 1;
        return b;
    }
    uint32_t get(int n) {
        uint32_t v = 0;
        while (n-- > 0) v |= (uint32_t)bit(128) << n;
        return v;
    }
    int get_signed(int n) {
        const int v = (int)get(n);
        return bit(128) ? -v : v;
    }
};

// ---- frame header ------------------------------------------------------------------------------------------

using vp8_params::clipi;
using vp8_params::Quant;

struct Header {
    int use_segment = 0, update_map = 0, absolute_delta = 1;
    int seg_quant[4] = {0, 0, 0, 0}, seg_filter[4] = {0, 0, 0, 0};
    uint8_t seg_proba[3] = {255, 255, 255};
    int simple = 0, level = 0, sharpness = 0, use_lf_delta = 0, ref_lf_delta[4] = {0, 0, 0, 0}, mode_lf_delta[4] = {0, 0, 0, 0};
    int filter_type = 0, nparts = 1;
    Quant q[4];
    uint8_t proba[4][8][3][11];
    int use_skip = 0, skip_p = 0;
    uint8_t flevel[4][2], ilevel[4][2], hev[4][2];
};

int read_frame_header(Bool& br, Header& H, int64_t* stats, Err& e) {
    br.get(1);                                               // colour space
    br.get(1);                                               // clamping type: both ignored, as libwebp ignores them
    H.use_segment = (int)br.get(1);
    if (H.use_segment) {
        *stats |= VIP_VP8_STAT_SEGMENTS;
        H.update_map = (int)br.get(1);
        if (br.get(1)) {
            H.absolute_delta = (int)br.get(1);
            if (!H.absolute_delta) *stats |= VIP_VP8_STAT_SEG_DELTA;
            for (int s = 0; s < 4; ++s) H.seg_quant[s] = br.get(1) ? br.get_signed(7) : 0;
            for (int s = 0; s < 4; ++s) H.seg_filter[s] = br.get(1) ? br.get_signed(6) : 0;
        }
        if (H.update_map) {
            *stats |= VIP_VP8_STAT_MAP_UPDATE;
            for (int s = 0; s < 3; ++s) H.seg_proba[s] = br.get(1) ? (uint8_t)br.get(8) : 255;
        }
    }
    if (br.eof) return fail(e, "webp: VP8 first partition ends in the segment header");
    H.simple = (int)br.get(1);
    H.level = (int)br.get(6);
    H.sharpness = (int)br.get(3);
    H.use_lf_delta = (int)br.get(1);
    if (H.use_lf_delta) {
        *stats |= VIP_VP8_STAT_LF_DELTA;
        if (br.get(1)) {
            for (int i = 0; i < 4; ++i)
                if (br.get(1)) H.ref_lf_delta[i] = br.get_signed(6);
            for (int i = 0; i < 4; ++i)
                if (br.get(1)) H.mode_lf_delta[i] = br.get_signed(6);
        }
    }
    H.filter_type = H.level == 0 ? 0 : H.simple ? 1 : 2;
    if (br.eof) return fail(e, "webp: VP8 first partition ends in the filter header");
    if (H.filter_type) {
        *stats |= H.simple ? VIP_VP8_STAT_SIMPLE_FILTER : VIP_VP8_STAT_NORMAL_FILTER;
        if (H.sharpness > 0) *stats |= VIP_VP8_STAT_SHARPNESS;
    }
    H.nparts = 1 << br.get(2);
    if (H.nparts == 2) *stats |= VIP_VP8_STAT_PARTS2;
    if (H.nparts == 4) *stats |= VIP_VP8_STAT_PARTS4;
    if (H.nparts == 8) *stats |= VIP_VP8_STAT_PARTS8;
    // quantisers
    const int base_q = (int)br.get(7);
    int dq[5];                                               // y1 dc, y2 dc, y2 ac, uv dc, uv ac
    for (int i = 0; i < 5; ++i) dq[i] = br.get(1) ? br.get_signed(4) : 0;
    for (int s = 0; s < 4; ++s) {
        int q = base_q;
        if (H.use_segment) q = H.seg_quant[s] + (H.absolute_delta ? 0 : base_q);
        vp8_params::quant_steps(q, dq, H.q[s]);
    }
    br.get(1);                                               // refresh_entropy_probs: meaningless in a single frame
    for (int t = 0; t < 4; ++t)
        for (int b = 0; b < 8; ++b)
            for (int c = 0; c < 3; ++c)
                for (int p = 0; p < 11; ++p) {
                    const int k = ((t * 8 + b) * 3 + c) * 11 + p;
                    if (br.bit(COEF_UPDATE[k])) {
                        H.proba[t][b][c][p] = (uint8_t)br.get(8);
                        *stats |= VIP_VP8_STAT_PROBA_UPDATE;
                    } else {
                        H.proba[t][b][c][p] = COEF_PROBA0[k];
                    }
                }
    H.use_skip = (int)br.get(1);
    if (H.use_skip) H.skip_p = (int)br.get(8);
    if (br.eof) return fail(e, "webp: VP8 first partition ends in the frame header");
    // filter strengths per segment and prediction kind (libwebp's PrecomputeFilterStrengths)
    for (int s = 0; s < 4; ++s) {
        int base = H.level;
        if (H.use_segment) base = H.seg_filter[s] + (H.absolute_delta ? 0 : H.level);
        for (int i4 = 0; i4 < 2; ++i4) {
            int level = base;
            if (H.use_lf_delta) {
                level += H.ref_lf_delta[0];
                if (i4) level += H.mode_lf_delta[0];
            }
            vp8_params::filter_strength(level, H.sharpness, H.filter_type, H.flevel[s][i4], H.ilevel[s][i4], H.hev[s][i4]);
        }
    }
    return VIP_OK;
}

// ---- tokens ------------------------------------------------------------------------------------------------

int large_value(Bool& br, const uint8_t* p, int64_t* stats) {
    int v;
    if (!br.bit(p[3])) {
        v = !br.bit(p[4]) ? 2 : 3 + br.bit(p[5]);
    } else if (!br.bit(p[6])) {
        if (!br.bit(p[7])) {
            v = 5 + br.bit(159);
        } else {
            v = 7 + 2 * br.bit(165);
            v += br.bit(145);
        }
    } else {
        const int bit1 = br.bit(p[8]);
        const int bit0 = br.bit(p[9 + bit1]);
        const int cat = 2 * bit1 + bit0;
        if (cat == 3) *stats |= VIP_VP8_STAT_CAT6;
        v = 0;
        for (const uint8_t* tab = CAT3456[cat]; *tab; ++tab) v += v + br.bit(*tab);
        v += 3 + (8 << cat);
    }
    return v;
}

// one block: coefficients n.. into out (raster order, dequantised, wrapped to int16 as libwebp stores them); returns the
// position after the last token read
int get_coeffs(Bool& br, const uint8_t (*prob)[3][11], int ctx, const int* dq, int n, int16_t* out, int64_t* stats) {
    const uint8_t* p = prob[BANDS[n]][ctx];
    for (; n < 16; ++n) {
        if (!br.bit(p[0])) return n;
        while (!br.bit(p[1])) {
            p = prob[BANDS[++n]][0];
            if (n == 16) return 16;
        }
        const uint8_t(*next)[11] = prob[BANDS[n + 1]];
        int v;
        if (!br.bit(p[2])) {
            v = 1;
            p = next[1];
        } else {
            v = large_value(br, p, stats);
            p = next[2];
        }
        const int s = br.bit(128) ? -v : v;
        out[ZIGZAG[n]] = (int16_t)(s * dq[n > 0]);
    }
    return 16;
}

// does the inverse WHT of Y2 give any luma block a DC?  (libwebp's in-loop "inner edges" rule looks at the blocks' data)
bool wht_any_nonzero(const int16_t* in) {
    int tmp[16];
    for (int i = 0; i < 4; ++i) {
        const int a0 = in[0 + i] + in[12 + i], a1 = in[4 + i] + in[8 + i], a2 = in[4 + i] - in[8 + i], a3 = in[0 + i] - in[12 + i];
        tmp[0 + i] = a0 + a1;
        tmp[8 + i] = a0 - a1;
        tmp[4 + i] = a3 + a2;
        tmp[12 + i] = a3 - a2;
    }
    for (int i = 0; i < 4; ++i) {
        const int dc = tmp[0 + i * 4] + 3;
        const int a0 = dc + tmp[3 + i * 4], a1 = tmp[1 + i * 4] + tmp[2 + i * 4], a2 = tmp[1 + i * 4] - tmp[2 + i * 4], a3 = dc - tmp[3 + i * 4];
        if ((int16_t)((a0 + a1) >> 3) || (int16_t)((a3 + a2) >> 3) || (int16_t)((a0 - a1) >> 3) || (int16_t)((a3 - a2) >> 3)) return true;
    }
    return false;
}

// ---- one image ---------------------------------------------------------------------------------------------

struct Image {
    std::vector<vip_vp8_mb> mbs;
    std::vector<int16_t> coefs;
};

int decode_image(const uint8_t* d, size_t n, vip_vp8_desc* D, Image& out, Err& e) {
    vip_vp8_desc P;
    Frame F;
    size_t bound = 0;
    int st = parse_header(d, n, &P, &bound, F, e);
    if (st != VIP_OK) return st;
    if (P.width != D->width || P.height != D->height) return fail(e, "webp: stream changed since probe");
    int64_t stats = 0;
    Bool br(F.part0, F.part0_len);
    Header H;
    st = read_frame_header(br, H, &stats, e);
    if (st != VIP_OK) return st;
    // token partitions: nparts - 1 sizes of 3 bytes, then the partitions back to back; the last takes what is left
    const int np = H.nparts;
    if (F.rest_len < (size_t)3 * (np - 1)) return fail(e, "webp: VP8 partition sizes run past the chunk");
    std::vector<Bool> parts;
    parts.reserve((size_t)np);
    {
        const uint8_t* start = F.rest + 3 * (np - 1);
        size_t left = F.rest_len - (size_t)3 * (np - 1);
        for (int p = 0; p + 1 < np; ++p) {
            const size_t psize = le24(F.rest + 3 * p);
            if (psize > left) return fail(e, "webp: VP8 token partition %d (%zu bytes) runs past the chunk", p, psize);
            parts.emplace_back(start, psize);
            start += psize;
            left -= psize;
        }
        parts.emplace_back(start, left);
    }
    const int mb_w = P.mb_w, mb_h = P.mb_h;
    out.mbs.assign((size_t)mb_w * mb_h, vip_vp8_mb{});
    out.coefs.clear();
    // contexts: the sub-block modes above / left, and the "had coefficients" flags above / left (4 Y, 2 U, 2 V, Y2)
    std::vector<uint8_t> top_modes((size_t)mb_w * 4, VIP_VP8_B_DC), top_nz((size_t)mb_w * 9, 0);
    uint8_t left_modes[4], left_nz[9];
    int16_t blocks[25][16];
    for (int my = 0; my < mb_h; ++my) {
        Bool& tk = parts[(size_t)(my & (np - 1))];
        memset(left_modes, VIP_VP8_B_DC, sizeof left_modes);
        memset(left_nz, 0, sizeof left_nz);
        for (int mx = 0; mx < mb_w; ++mx) {
            vip_vp8_mb& M = out.mbs[(size_t)my * mb_w + mx];
            // --- modes (first partition)
            int seg = 0;
            if (H.update_map) seg = !br.bit(H.seg_proba[0]) ? br.bit(H.seg_proba[1]) : br.bit(H.seg_proba[2]) + 2;
            const int skip_flag = H.use_skip ? br.bit(H.skip_p) : 0;
            if (skip_flag) stats |= VIP_VP8_STAT_SKIP;
            const bool i4 = !br.bit(145);
            uint8_t* tm = &top_modes[(size_t)mx * 4];
            if (!i4) {
                const int ymode = br.bit(156) ? (br.bit(128) ? VIP_VP8_B_TM : VIP_VP8_B_HE) : (br.bit(163) ? VIP_VP8_B_VE : VIP_VP8_B_DC);
                M.ymode = (uint8_t)ymode;
                memset(tm, ymode, 4);
                memset(left_modes, ymode, 4);
                stats |= VIP_VP8_STAT_YMODE0 << ymode;
            } else {
                M.ymode = VIP_VP8_B_PRED;
                stats |= VIP_VP8_STAT_BPRED;
                for (int y = 0; y < 4; ++y) {
                    int ymode = left_modes[y];
                    for (int x = 0; x < 4; ++x) {
                        const uint8_t* prob = &BMODE_PROBA[((size_t)tm[x] * 10 + ymode) * 9];
                        ymode = !br.bit(prob[0]) ? VIP_VP8_B_DC
                              : !br.bit(prob[1]) ? VIP_VP8_B_TM
                              : !br.bit(prob[2]) ? VIP_VP8_B_VE
                              : !br.bit(prob[3]) ? (!br.bit(prob[4]) ? VIP_VP8_B_HE : (!br.bit(prob[5]) ? VIP_VP8_B_RD : VIP_VP8_B_VR))
                                                 : (!br.bit(prob[6]) ? VIP_VP8_B_LD
                                                                     : (!br.bit(prob[7]) ? VIP_VP8_B_VL : (!br.bit(prob[8]) ? VIP_VP8_B_HD : VIP_VP8_B_HU)));
                        tm[x] = (uint8_t)ymode;
                        M.bmodes[y * 4 + x] = (uint8_t)ymode;
                        stats |= VIP_VP8_STAT_BMODE0 << ymode;
                    }
                    left_modes[y] = (uint8_t)ymode;
                }
            }
            const int uvmode = !br.bit(142) ? VIP_VP8_B_DC : !br.bit(114) ? VIP_VP8_B_VE : br.bit(183) ? VIP_VP8_B_TM : VIP_VP8_B_HE;
            M.uvmode = (uint8_t)uvmode;
            stats |= VIP_VP8_STAT_UVMODE0 << uvmode;
            M.segment = (uint8_t)seg;
            M.skip = (uint8_t)skip_flag;
            if (br.eof) return fail(e, "webp: VP8 first partition ends at macroblock (%d, %d)", mx, my);
            // --- residuals (the row's token partition)
            uint8_t* tnz = &top_nz[(size_t)mx * 9];
            uint32_t nzmask = 0, dconly = 0;
            bool any = false;                                // libwebp's non_zero_y | non_zero_uv
            if (!skip_flag) {
                memset(blocks, 0, sizeof blocks);
                const Quant& Q = H.q[seg];
                int first = 0;
                const uint8_t(*ac)[3][11] = H.proba[3];
                if (!i4) {
                    const int ctx = tnz[8] + left_nz[8];
                    const int nz = get_coeffs(tk, H.proba[1], ctx, Q.y2, 0, blocks[24], &stats);
                    tnz[8] = left_nz[8] = nz > 0;
                    if (nz > 0) {
                        nzmask |= 1u << 24;
                        if (nz > 1) stats |= VIP_VP8_STAT_Y2_AC;
                        any |= wht_any_nonzero(blocks[24]);
                    }
                    first = 1;
                    ac = H.proba[0];
                }
                for (int y = 0; y < 4; ++y)
                    for (int x = 0; x < 4; ++x) {
                        const int b = y * 4 + x;
                        const int nz = get_coeffs(tk, ac, tnz[x] + left_nz[y], Q.y1, first, blocks[b], &stats);
                        tnz[x] = left_nz[y] = nz > first;
                        if (nz > first) nzmask |= 1u << b;
                        if (nz > 1 || blocks[b][0]) any = true;
                        if (!first && nz == 1) dconly |= 1u << b;
                    }
                for (int ch = 0; ch < 2; ++ch)
                    for (int y = 0; y < 2; ++y)
                        for (int x = 0; x < 2; ++x) {
                            const int b = 16 + ch * 4 + y * 2 + x;
                            uint8_t &t = tnz[4 + ch * 2 + x], &l = left_nz[4 + ch * 2 + y];
                            const int nz = get_coeffs(tk, H.proba[2], t + l, Q.uv, 0, blocks[b], &stats);
                            t = l = nz > 0;
                            if (nz > 0) nzmask |= 1u << b;
                            if (nz > 1 || blocks[b][0]) any = true;
                            if (nz == 1) dconly |= 1u << b;
                        }
                if (tk.eof) return fail(e, "webp: VP8 token partition %d ends at macroblock (%d, %d)", my & (np - 1), mx, my);
            } else {
                memset(tnz, 0, 8);
                memset(left_nz, 0, 8);
                if (!i4) tnz[8] = left_nz[8] = 0;
            }
            if (nzmask & ~dconly & 0xffffff) stats |= VIP_VP8_STAT_FULL_BLOCK;
            if (dconly) stats |= VIP_VP8_STAT_DC_ONLY;
            M.nz = nzmask;
            M.dc_only = dconly;
            M.coef_idx = (uint32_t)(out.coefs.size() / 16);
            for (int b = 0; b < 25; ++b)
                if (nzmask & (1u << b)) out.coefs.insert(out.coefs.end(), blocks[b], blocks[b] + 16);
            M.flevel = H.flevel[seg][i4];
            M.ilevel = H.ilevel[seg][i4];
            M.hev = H.hev[seg][i4];
            M.inner = (uint8_t)(i4 || any);
            if (H.filter_type && M.flevel == 0) stats |= VIP_VP8_STAT_LEVEL0_MB;
        }
    }
    D->filter_type = H.filter_type;
    D->stats = stats;
    return VIP_OK;
}

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

extern "C" int vip_vp8_probe_h(const uint8_t* webp_h, size_t len, vip_vp8_desc* desc_h, size_t* stream_bytes_h) {
    if (!webp_h || !desc_h || !stream_bytes_h) {
        vip_set_error("vip_vp8_probe_h: null pointer");
        return VIP_ERR_BAD_ARG;
    }
    Err e;
    Frame F;
    const int st = parse_header(webp_h, len, desc_h, stream_bytes_h, F, e);
    if (st != VIP_OK) vip_set_error("%s", e.msg);
    return st;
}

extern "C" int vip_vp8_entropy_h(const uint8_t* const* webp_h, const size_t* len_h, int n, vip_vp8_desc* desc_h,
                                 uint8_t* stream_h, size_t stream_cap, size_t* stream_used_h, int threads) {
    if (!webp_h || !len_h || !desc_h || !stream_h || n <= 0) {
        vip_set_error("vip_vp8_entropy_h: bad argument (null pointer or n <= 0)");
        return VIP_ERR_BAD_ARG;
    }
    if (((uintptr_t)stream_h & 7) != 0) {
        vip_set_error("vip_vp8_entropy_h: stream buffer is not 8-byte aligned");
        return VIP_ERR_BAD_ARG;
    }
    // pass 1 (serial, headers only): sizes, so that a buffer too small is refused before any work
    size_t bound = 0;
    for (int i = 0; i < n; ++i) {
        Err e;
        Frame F;
        size_t bytes = 0;
        if (!webp_h[i]) {
            vip_set_error("vip_vp8_entropy_h: image %d: null pointer", i);
            return VIP_ERR_BAD_ARG;
        }
        const int st = parse_header(webp_h[i], len_h[i], &desc_h[i], &bytes, F, e);
        if (st != VIP_OK) {
            vip_set_error("webp image %d: %s", i, e.msg);
            return st;
        }
        bound += bytes;
    }
    if (bound > stream_cap) {
        if (stream_used_h) *stream_used_h = bound;
        vip_set_error("vip_vp8_entropy_h: stream buffer too small (%zu > %zu)", bound, stream_cap);
        return VIP_ERR_BAD_ARG;
    }
    // pass 2: the decode, one image at a time per worker, each into memory of its own
    std::vector<Image> images((size_t)n);
    if (threads < 1) threads = 1;
    if (threads > 16) threads = 16;
    if (threads > n) threads = n;
    const auto failed = host_batch::run<Err>(n, threads, [&](int i, Err& e) {
        return decode_image(webp_h[i], len_h[i], &desc_h[i], images[(size_t)i], e);
    });
    if (failed.status != VIP_OK) {
        vip_set_error("webp image %d: %s", failed.index, failed.err.msg);
        return failed.status;
    }
    // pass 3: pack what was used, in image order - the offsets serially, the copies on the workers again (a fresh buffer's
    // pages are first touched here, and one thread touching them all costs more than the decode)
    size_t off = 0, plane = 0;
    for (int i = 0; i < n; ++i) {
        const Image& I = images[(size_t)i];
        vip_vp8_desc& D = desc_h[i];
        const size_t mb_bytes = I.mbs.size() * sizeof(vip_vp8_mb), coef_bytes = I.coefs.size() * sizeof(int16_t);
        D.stream_off = (int64_t)off;
        D.mb_off = 0;
        D.coef_off = (int64_t)align8(mb_bytes);
        D.coef_blocks = (int64_t)(I.coefs.size() / 16);
        D.plane_off = (int64_t)plane;
        off += align8((size_t)D.coef_off + coef_bytes);
        plane += (size_t)D.mb_w * D.mb_h * 384;
    }
    host_batch::run<Err>(n, threads, [&](int i, Err&) {
        const Image& I = images[(size_t)i];
        const vip_vp8_desc& D = desc_h[i];
        uint8_t* out = stream_h + D.stream_off;
        const size_t mb_bytes = I.mbs.size() * sizeof(vip_vp8_mb), coef_bytes = I.coefs.size() * sizeof(int16_t);
        memcpy(out, I.mbs.data(), mb_bytes);
        memset(out + mb_bytes, 0, (size_t)D.coef_off - mb_bytes);
        if (coef_bytes) memcpy(out + D.coef_off, I.coefs.data(), coef_bytes);
        const size_t end = (size_t)D.coef_off + coef_bytes;
        memset(out + end, 0, align8(end) - end);
        return VIP_OK;
    });
    if (stream_used_h) *stream_used_h = off;
    return VIP_OK;
}

extern "C" int vip_vp8_scratch_bytes(const vip_vp8_desc* desc_h, int n, size_t* bytes_h) {
    if (!desc_h || !bytes_h || n <= 0) {
        vip_set_error("vip_vp8_scratch_bytes: bad argument (null pointer or n <= 0)");
        return VIP_ERR_BAD_ARG;
    }
    size_t need = 16;
    for (int i = 0; i < n; ++i) {
        const vip_vp8_desc& D = desc_h[i];
        if (D.mb_w < 0 || D.mb_h < 0 || D.plane_off < 0) {
            vip_set_error("vip_vp8_scratch_bytes: descriptor %d is damaged", i);
            return VIP_ERR_BAD_ARG;
        }
        const size_t end = (size_t)D.plane_off + (size_t)D.mb_w * D.mb_h * 384;
        if (end > need) need = end;
    }
    *bytes_h = need;
    return VIP_OK;
}
