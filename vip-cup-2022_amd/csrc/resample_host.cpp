// Host half of the antialiased u8 resampler (resample.hip): the integer coefficient tables of one axis.
//
// The tables restate the published behaviour of Pillow's 8-bit Image.resize (precompute_coeffs + normalize_coeffs_8bpc): a filter whose
// support widens with the shrink factor, weights normalised in double precision and rounded to 22 fractional bits.  They are built on
// the host on purpose: a device sin or a contracted multiply-add would move a coefficient by one unit, and the resampler is held to
// Pillow bit for bit.  This file is compiled with -ffp-contract=off (build.py) for the same reason.
#include "common.hpp"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int MAX_SIDE = 1 << 20;
constexpr double PI = 3.14159265358979323846;

double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

double bicubic_filter(double x) {      // Keys, a = -0.5
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

double sinc_filter(double x) {
    if (x == 0.0) return 1.0;
    x = x * PI;
    return sin(x) / x;
}

double lanczos_filter(double x) {      // truncated sinc, 3 lobes
    if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
    return 0.0;
}

}  // namespace

extern "C" int vip_resample_coeffs_h(int in_size, int out_size, int filter, int32_t* bounds_h, size_t bounds_cap, int32_t* k_h,
                                     size_t k_cap, int* ksize_h) {
    VIP_REQUIRE(ksize_h, VIP_ERR_BAD_ARG, "vip_resample_coeffs_h: null ksize pointer");
    VIP_REQUIRE(in_size >= 1 && out_size >= 1 && in_size <= MAX_SIDE && out_size <= MAX_SIDE, VIP_ERR_BAD_ARG,
                "vip_resample_coeffs_h: size %d -> %d outside 1..%d", in_size, out_size, MAX_SIDE);
    double (*f)(double) = nullptr;
    double filter_support = 0.0;
    switch (filter) {
        case VIP_RESAMPLE_BILINEAR: f = bilinear_filter, filter_support = 1.0; break;
        case VIP_RESAMPLE_BICUBIC: f = bicubic_filter, filter_support = 2.0; break;
        case VIP_RESAMPLE_LANCZOS: f = lanczos_filter, filter_support = 3.0; break;
        default: break;
    }
    VIP_REQUIRE(f, VIP_ERR_BAD_ARG, "vip_resample_coeffs_h: unknown filter %d (0 bilinear, 1 bicubic, 2 lanczos)", filter);
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    *ksize_h = ksize;
    if (!bounds_h && !k_h) return VIP_OK;                   // size query
    VIP_REQUIRE(bounds_h && k_h, VIP_ERR_BAD_ARG, "vip_resample_coeffs_h: null pointer (pass both buffers, or neither to query ksize)");
    VIP_REQUIRE(bounds_cap >= (size_t)out_size * 2 && k_cap >= (size_t)out_size * ksize, VIP_ERR_BAD_ARG,
                "vip_resample_coeffs_h: buffers too short (bounds %zu < %zu or k %zu < %zu int32)", bounds_cap, (size_t)out_size * 2,
                k_cap, (size_t)out_size * ksize);
    const double ss = 1.0 / filterscale;
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = f((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t* k = k_h + (size_t)xx * ksize;
        for (int x = 0; x < xmax; ++x) {
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << PRECISION_BITS)) : (int32_t)(0.5 + v * (1 << PRECISION_BITS));
        }
        for (int x = xmax; x < ksize; ++x) k[x] = 0;
        bounds_h[xx * 2] = xmin;
        bounds_h[xx * 2 + 1] = xmax;
    }
    return VIP_OK;
}
