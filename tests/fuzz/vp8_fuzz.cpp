// Test infrastructure (CPU only): mutation fuzzing of the host half of the lossy WebP path (container walk, VP8 frame
// header, modes and tokens: csrc/vp8_host.cpp) under AddressSanitizer + UBSan.  Built by tests/test_vp8_fuzz.py as
//   g++ -fsanitize=address,undefined vp8_fuzz.cpp ../../vip-cup-2022_amd/csrc/vp8_host.cpp
// The decoder takes untrusted files: whatever the bytes are, it must return a status - never read or write outside its
// buffers, never allocate without bound - and what it hands to the device must index inside what it wrote.
// usage: vp8_fuzz <iterations per file> <file.webp>...
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vipcup_hip.h"

void vip_set_error(const char*, ...) {}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

// make the RIFF size, the size of a leading `VP8 ` chunk and the first partition's size fit the mutated length again, so
// that a cut stream reaches the boolean decoder instead of stopping at the container or partition checks
static void fix_sizes(std::vector<uint8_t>& m) {
    if (m.size() < 20) return;
    const uint32_t riff = (uint32_t)m.size() - 8;
    for (int k = 0; k < 4; ++k) m[4 + k] = (uint8_t)(riff >> (8 * k));
    if (memcmp(&m[12], "VP8 ", 4) != 0) return;
    const uint32_t len = (uint32_t)m.size() - 20;
    for (int k = 0; k < 4; ++k) m[16 + k] = (uint8_t)(len >> (8 * k));
    if (len < 10) return;
    uint32_t tag = (uint32_t)m[20] | ((uint32_t)m[21] << 8) | ((uint32_t)m[22] << 16);
    if ((tag >> 5) > len - 10) {
        tag = (tag & 31u) | ((len - 10) << 5);
        for (int k = 0; k < 3; ++k) m[20 + k] = (uint8_t)(tag >> (8 * k));
    }
}

static void run_one(const std::vector<uint8_t>& buf, long* decoded) {
    vip_vp8_desc d;
    size_t bytes = 0;
    // exact-size heap copy: ASan sees a read one byte past the end of the stream
    std::vector<uint8_t> copy(buf);
    const uint8_t* p = copy.data();
    size_t len = copy.size();
    if (vip_vp8_probe_h(p, len, &d, &bytes) != VIP_OK) return;
    if (bytes > (size_t)64 << 20) return;                       // a mutated header may ask for a large image: not a decoder bug
    std::vector<uint64_t> out(bytes / 8 + 1);                   // the probe bound, 8-byte aligned: a write past it is caught
    size_t used = 0;
    if (vip_vp8_entropy_h(&p, &len, 1, &d, (uint8_t*)out.data(), bytes, &used, 1) != VIP_OK) return;
    ++*decoded;
    // what the device will index with: records and coefficients inside what was written, modes inside their tables
    if (used > bytes || d.stream_off != 0 || d.mb_off < 0 || d.coef_off < 0) abort();
    const size_t nmb = (size_t)d.mb_w * d.mb_h;
    if ((size_t)d.mb_off + nmb * sizeof(vip_vp8_mb) > used || (size_t)d.coef_off + (size_t)d.coef_blocks * 32 > used) abort();
    const vip_vp8_mb* M = (const vip_vp8_mb*)((const uint8_t*)out.data() + d.mb_off);
    uint64_t next = 0;
    for (size_t k = 0; k < nmb; ++k) {
        if (M[k].ymode > VIP_VP8_B_PRED || M[k].uvmode > 3 || M[k].flevel > 63 || M[k].nz >> 25 || (M[k].dc_only & ~M[k].nz)) abort();
        for (int b = 0; b < 16; ++b)
            if (M[k].bmodes[b] > 9) abort();
        if (M[k].coef_idx != next) abort();
        next += (uint64_t)__builtin_popcount(M[k].nz);
    }
    if (next != (uint64_t)d.coef_blocks) abort();
    size_t scratch = 0;
    if (vip_vp8_scratch_bytes(&d, 1, &scratch) != VIP_OK || scratch < nmb * 384) abort();
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const int iters = atoi(argv[1]);
    long total = 0, decoded = 0;
    for (int f = 2; f < argc; ++f) {
        FILE* fp = fopen(argv[f], "rb");
        if (!fp) return 3;
        std::vector<uint8_t> orig;
        uint8_t tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, fp)) > 0) orig.insert(orig.end(), tmp, tmp + n);
        fclose(fp);
        run_one(orig, &decoded);
        ++total;
        for (int it = 0; it < iters; ++it) {
            std::vector<uint8_t> m(orig);
            switch (rnd() % 5) {
                case 0: m.resize(rnd() % (m.size() + 1)); fix_sizes(m); break;             // truncate anywhere
                case 1: for (int k = 1 + rnd() % 8; k > 0; --k) m[rnd() % m.size()] ^= (uint8_t)(1u << (rnd() % 8)); break;
                case 2: {                                                                  // the boolean-coded data behind the headers
                    const size_t lo = m.size() > 31 ? 30 : 0;
                    for (int k = 1 + rnd() % 4; k > 0; --k) m[lo + rnd() % (m.size() - lo)] ^= (uint8_t)(1u << (rnd() % 8));
                    break;
                }
                case 3: {                                                                  // header bytes only
                    const size_t hdr = m.size() < 48 ? m.size() : 48;
                    for (int k = 1 + rnd() % 6; k > 0; --k) m[rnd() % hdr] = (uint8_t)rnd();
                    break;
                }
                default: {                                                                 // cut a span out of the middle
                    const size_t a = rnd() % m.size(), b = a + rnd() % (m.size() - a + 1);
                    m.erase(m.begin() + a, m.begin() + b);
                    fix_sizes(m);
                    break;
                }
            }
            if (m.empty()) continue;
            run_one(m, &decoded);
            ++total;
        }
    }
    printf("fuzzed %ld streams, %ld decoded to the end\n", total, decoded);
    return 0;
}
