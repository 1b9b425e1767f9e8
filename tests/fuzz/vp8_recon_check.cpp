// Test infrastructure (CPU only): the lossy WebP path without a GPU.  The host stage (csrc/vp8_host.cpp) and the pixel
// arithmetic the kernels are made of (csrc/vp8_recon.hpp) are compiled as plain C++ and run serially, macroblocks in
// raster order - any order that respects the dependencies gives the same pixels, and raster order is the simplest one.
// tests/test_vp8_host_cpu.py compares the result with Pillow's decode.  Built as
//   g++ -I include -I vip-cup-2022_amd/csrc vp8_recon_check.cpp ../../vip-cup-2022_amd/csrc/vp8_host.cpp
// usage: vp8_recon_check <file.webp>...   writes <file.webp>.rgb (height x width x 3 bytes) and prints "width height stats"
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vipcup_hip.h"
#include "vp8_recon.hpp"

static char last_error[512];
void vip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
}

static int edge_sum(const uint8_t* plane, int stride, int size, int mx, int my, bool top) {
    int s = 0;
    for (int i = 0; i < size; ++i) {
        if (top) s += my > 0 ? plane[(int64_t)(my * size - 1) * stride + mx * size + i] : 0;
        else s += mx > 0 ? plane[(int64_t)(my * size + i) * stride + mx * size - 1] : 0;
    }
    return s;
}

int main(int argc, char** argv) {
    for (int f = 1; f < argc; ++f) {
        FILE* fp = fopen(argv[f], "rb");
        if (!fp) return 3;
        std::vector<uint8_t> raw;
        uint8_t tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, fp)) > 0) raw.insert(raw.end(), tmp, tmp + n);
        fclose(fp);
        vip_vp8_desc D;
        size_t bytes = 0, used = 0;
        const uint8_t* p = raw.data();
        size_t len = raw.size();
        if (vip_vp8_probe_h(p, len, &D, &bytes) != VIP_OK) {
            fprintf(stderr, "%s: %s\n", argv[f], last_error);
            return 4;
        }
        std::vector<uint64_t> stream(bytes / 8 + 1);
        if (vip_vp8_entropy_h(&p, &len, 1, &D, (uint8_t*)stream.data(), bytes, &used, 1) != VIP_OK) {
            fprintf(stderr, "%s: %s\n", argv[f], last_error);
            return 4;
        }
        const uint8_t* base = (const uint8_t*)stream.data() + D.stream_off;
        const vip_vp8_mb* mbs = (const vip_vp8_mb*)(base + D.mb_off);
        const int16_t* coefs = (const int16_t*)(base + D.coef_off);
        std::vector<uint8_t> planes((size_t)D.mb_w * D.mb_h * 384);
        const Vp8Planes P = vp8_planes(planes.data(), D.mb_w, D.mb_h);
        for (int my = 0; my < D.mb_h; ++my)
            for (int mx = 0; mx < D.mb_w; ++mx) {
                const vip_vp8_mb& M = mbs[(size_t)my * D.mb_w + mx];
                const int dc_y = vp8_dc_value(edge_sum(P.y, P.ys, 16, mx, my, true), edge_sum(P.y, P.ys, 16, mx, my, false), 16, mx, my);
                const int dc_u = vp8_dc_value(edge_sum(P.u, P.cs, 8, mx, my, true), edge_sum(P.u, P.cs, 8, mx, my, false), 8, mx, my);
                const int dc_v = vp8_dc_value(edge_sum(P.v, P.cs, 8, mx, my, true), edge_sum(P.v, P.cs, 8, mx, my, false), 8, mx, my);
                const bool subs = M.ymode == VIP_VP8_B_PRED;
                for (int item = subs ? 64 : 0; item < 96; ++item) vp8_recon_item(P, M, coefs, mx, my, item, dc_y, dc_u, dc_v);
                if (subs)
                    for (int b = 0; b < 16; ++b)
                        for (int k = 0; k < 4; ++k) vp8_recon_sub_item(P, M, coefs, mx, my, b & 3, b >> 2, k);
            }
        if (D.filter_type)
            for (int my = 0; my < D.mb_h; ++my)
                for (int mx = 0; mx < D.mb_w; ++mx) {
                    const vip_vp8_mb& M = mbs[(size_t)my * D.mb_w + mx];
                    for (int item = 0; item < 32; ++item) vp8_filter_item(P, M, D.filter_type, mx, my, item, false);
                    for (int item = 0; item < 32; ++item) vp8_filter_item(P, M, D.filter_type, mx, my, item, true);
                }
        std::vector<uint8_t> rgb((size_t)D.width * D.height * 3);
        for (int y = 0; y < D.height; ++y)
            for (int x = 0; x < D.width; ++x) vp8_rgb_px(P, D.width, D.height, x, y, &rgb[((size_t)y * D.width + x) * 3]);
        char name[4096];
        snprintf(name, sizeof name, "%s.rgb", argv[f]);
        fp = fopen(name, "wb");
        if (!fp) return 5;
        fwrite(rgb.data(), 1, rgb.size(), fp);
        fclose(fp);
        printf("%d %d %lld\n", D.width, D.height, (long long)D.stats);
    }
    return 0;
}
