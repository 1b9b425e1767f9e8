// Host half of the Gaussian blur (blur.hip): the integer weights of one axis.
//
// The weights are built on the host in double precision on purpose: the blur is held to its integer restatement bit for bit, and a device
// exp or a contracted multiply-add could move a weight by one unit.  This file is compiled with -ffp-contract=off (build.py) for the same
// reason.
#include "common.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int MAX_RADIUS = 15;
constexpr int WEIGHT_ONE = 1 << 16;

}  // namespace

extern "C" int vip_blur_weights_h(double sigma, int radius, int32_t* w_h, size_t cap) {
    VIP_REQUIRE(w_h, VIP_ERR_BAD_ARG, "vip_blur_weights_h: null pointer");
    VIP_REQUIRE(sigma >= 0.3 && sigma <= 5.0, VIP_ERR_BAD_ARG, "vip_blur_weights_h: sigma %g outside 0.3..5.0", sigma);
    VIP_REQUIRE(radius >= 1 && radius <= MAX_RADIUS, VIP_ERR_BAD_ARG, "vip_blur_weights_h: radius %d outside 1..%d", radius, MAX_RADIUS);
    VIP_REQUIRE(cap >= (size_t)(2 * radius + 1), VIP_ERR_BAD_ARG, "vip_blur_weights_h: buffer too short (%zu < %d int32)", cap,
                2 * radius + 1);
    double g[2 * MAX_RADIUS + 1];
    const double denom = 2.0 * sigma * sigma;
    double total = 0.0;
    for (int j = -radius; j <= radius; ++j) {               // summed left to right
        g[j + radius] = exp(-(double)(j * j) / denom);
        total += g[j + radius];
    }
    int32_t sum = 0;
    for (int k = 0; k <= 2 * radius; ++k) {
        w_h[k] = (int32_t)floor(g[k] / total * WEIGHT_ONE + 0.5);
        sum += w_h[k];
    }
    w_h[radius] += WEIGHT_ONE - sum;                        // the centre takes the rounding: the weights sum to exactly 2^16
    return VIP_OK;
}
