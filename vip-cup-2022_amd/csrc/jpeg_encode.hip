// Forward half of a JPEG re-save, the counterpart of jpeg_pipeline.hip's decode half (dataset/augment.py:110-113, JpegCompress =
// tf.image.random_jpeg_quality: an encode -> decode round trip):
//   RGB u8 -> YCbCr -> chroma downsample (4:2:0) or not (4:4:4) -> component planes (u8)
//   -> level shift + 8x8 ISLOW forward DCT -> quantise -> int16 coefficients, natural order, block-major per component
// which is exactly what vip_jpeg_idct_rgb_u8 reads.  Entropy coding is lossless, so the pixels that kernel then produces are the pixels a
// real re-saved file decodes to.
//
// The integer stages restate libjpeg's baseline compressor with its defaults bit for bit: jccolor.c (rgb_ycc_convert), jcprepct.c /
// jcsample.c (edge replication, h2v2_downsample), jfdctint.c (jpeg_fdct_islow), jcdctmgr.c (quantisation), jccoefct.c (the dummy
// blocks that pad the last MCU column / row) and jcparam.c (jpeg_set_quality).  HBM-bound byte work, no MFMA, no atomics.
#include "common.hpp"

#include <cstdlib>
#include <cstring>

namespace {

// ---- jfdctint.c constants (CONST_BITS = 13, PASS1_BITS = 2) ----
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270,
              F_0_899976223 = 7373, F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137,
              F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995, F_3_072711026 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 1-D pass of jpeg_fdct_islow; FIRST: the row pass (even part scaled up by PASS1_BITS), else the column pass
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(const int (&in)[8], int (&out)[8]) {
    constexpr int SH = FIRST ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    const int tmp0 = in[0] + in[7], tmp7 = in[0] - in[7];
    const int tmp1 = in[1] + in[6], tmp6 = in[1] - in[6];
    const int tmp2 = in[2] + in[5], tmp5 = in[2] - in[5];
    const int tmp3 = in[3] + in[4], tmp4 = in[3] - in[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (FIRST) {
        out[0] = (tmp10 + tmp11) << PASS1_BITS;
        out[4] = (tmp10 - tmp11) << PASS1_BITS;
    } else {
        out[0] = descale(tmp10 + tmp11, PASS1_BITS);
        out[4] = descale(tmp10 - tmp11, PASS1_BITS);
    }
    int z1 = (tmp12 + tmp13) * F_0_541196100;
    out[2] = descale(z1 + tmp13 * F_0_765366865, SH);
    out[6] = descale(z1 + tmp12 * (-F_1_847759065), SH);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * F_1_175875602;
    const int t4 = tmp4 * F_0_298631336, t5 = tmp5 * F_2_053119869, t6 = tmp6 * F_3_072711026, t7 = tmp7 * F_1_501321110;
    z1 *= -F_0_899976223;
    z2 *= -F_2_562915447;
    z3 *= -F_1_961570560;
    z4 *= -F_0_390180644;
    z3 += z5;
    z4 += z5;
    out[7] = descale(t4 + z1 + z3, SH);
    out[5] = descale(t5 + z2 + z4, SH);
    out[3] = descale(t6 + z2 + z3, SH);
    out[1] = descale(t7 + z1 + z4, SH);
}

// jccolor.c rgb_ycc_start: SCALEBITS = 16, FIX(x) = (int)(x * 65536 + 0.5); ONE_HALF on luma, CBCR_OFFSET + ONE_HALF - 1 on chroma
constexpr int ONE_HALF = 1 << 15, CBCR_ROUND = (128 << 16) + ONE_HALF - 1;
__device__ __forceinline__ int ycc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + ONE_HALF) >> 16; }
__device__ __forceinline__ int ycc_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + CBCR_ROUND) >> 16; }
__device__ __forceinline__ int ycc_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + CBCR_ROUND) >> 16; }

struct Strip {      // 8 pixels of one image row
    uint8_t r[8], g[8], b[8];
};

// pixels x0 .. x0+7 of row `row`, columns past the image replicating its last one (jcsample.c expand_right_edge)
__device__ __forceinline__ void load_strip(const uint8_t* __restrict__ row, int x0, int w, Strip& s) {
    const uint8_t* p = row + (long)x0 * 3;
    if (x0 + 8 <= w && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        uint32_t v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = reinterpret_cast<const uint32_t*>(p)[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            s.r[k] = (uint8_t)(v[(3 * k) >> 2] >> (8 * ((3 * k) & 3)));
            s.g[k] = (uint8_t)(v[(3 * k + 1) >> 2] >> (8 * ((3 * k + 1) & 3)));
            s.b[k] = (uint8_t)(v[(3 * k + 2) >> 2] >> (8 * ((3 * k + 2) & 3)));
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int x = x0 + k < w ? x0 + k : w - 1;
        s.r[k] = row[(long)x * 3];
        s.g[k] = row[(long)x * 3 + 1];
        s.b[k] = row[(long)x * 3 + 2];
    }
}

// Colour conversion + chroma downsampling into the component planes.  One thread = 8 luma columns x S luma rows (S = the luma sampling
// factor, 2 for 4:2:0 and 1 for 4:4:4): S 8-byte luma stores and one store of 8 / S bytes per chroma plane.
// Plane c sits at planes + coef_off[c] with a row pitch of blocks_w[c] * 8 bytes (the layout jpeg_idct_kernel writes on the decode side).
// Edges as libjpeg pads them: the last column is replicated to the right before the 2x2 sums, the rows are replicated down to an even
// count before them, and below that the last DOWNSAMPLED row is repeated (jcprepct.c pre_process_data).
template <int S>
__device__ __forceinline__ void ycc_planes(const uint8_t* __restrict__ rgb, const vip_jpeg_desc& d, uint8_t* __restrict__ planes,
                                           int maxH, int maxW) {
    const int w = d.width < maxW ? d.width : maxW, h = d.height < maxH ? d.height : maxH;   // never read outside the image's slot
    const int strip = blockIdx.x * 32 + (threadIdx.x & 31);         // 8 luma columns
    const int group = blockIdx.y * 8 + (threadIdx.x >> 5);          // S luma rows = one chroma row
    const int ystride = d.blocks_w[0] * 8, cstride = d.blocks_w[1] * 8;
    if (w <= 0 || h <= 0 || strip * 8 >= ystride || group * S >= d.blocks_h[0] * 8) return;
    const uint8_t* img = rgb + (long)blockIdx.z * maxH * maxW * 3;
    uint8_t* py = planes + d.coef_off[0];
    const int dh = (h + S - 1) / S;                                 // downsampled height
    const int cgroup = group < dh ? group : dh - 1;                 // chroma: rows below the image repeat the last downsampled row
    int cb[8 / S], cr[8 / S];
#pragma unroll
    for (int k = 0; k < 8 / S; ++k) cb[k] = cr[k] = 0;
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const int y = group * S + j < h ? group * S + j : h - 1;
        const int yc = cgroup * S + j < h ? cgroup * S + j : h - 1;
        Strip s;
        load_strip(img + (long)y * maxW * 3, strip * 8, w, s);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (uint32_t)ycc_y(s.r[k], s.g[k], s.b[k]) << (8 * k);
            hi |= (uint32_t)ycc_y(s.r[k + 4], s.g[k + 4], s.b[k + 4]) << (8 * k);
        }
        *reinterpret_cast<uint2*>(py + (long)(group * S + j) * ystride + strip * 8) = make_uint2(lo, hi);
        if (yc != y) load_strip(img + (long)yc * maxW * 3, strip * 8, w, s);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            cb[k / S] += ycc_cb(s.r[k], s.g[k], s.b[k]);
            cr[k / S] += ycc_cr(s.r[k], s.g[k], s.b[k]);
        }
    }
    if (group >= d.blocks_h[1] * 8) return;
    uint8_t* pcb = planes + d.coef_off[1] + (long)group * cstride + strip * (8 / S);
    uint8_t* pcr = planes + d.coef_off[2] + (long)group * cstride + strip * (8 / S);
    if (S == 2) {                                                   // h2v2_downsample: bias 1, 2, 1, 2 along the row
        uint32_t vb = 0, vr = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            vb |= (uint32_t)((cb[k] + 1 + (k & 1)) >> 2) << (8 * k);
            vr |= (uint32_t)((cr[k] + 1 + (k & 1)) >> 2) << (8 * k);
        }
        *reinterpret_cast<uint32_t*>(pcb) = vb;
        *reinterpret_cast<uint32_t*>(pcr) = vr;
    } else {
        uint32_t vb[2] = {0, 0}, vr[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 8 / S; ++k) {
            vb[k >> 2] |= (uint32_t)cb[k] << (8 * (k & 3));
            vr[k >> 2] |= (uint32_t)cr[k] << (8 * (k & 3));
        }
        *reinterpret_cast<uint2*>(pcb) = make_uint2(vb[0], vb[1]);
        *reinterpret_cast<uint2*>(pcr) = make_uint2(vr[0], vr[1]);
    }
}

// grid.z = image, grid.y covers the rows of a 4:4:4 image (the workgroups past a 4:2:0 image's half as many row pairs leave at once)
__global__ __launch_bounds__(256) void jpeg_ycc_planes_kernel(const uint8_t* __restrict__ rgb,
                                                              const vip_jpeg_desc* __restrict__ desc,
                                                              uint8_t* __restrict__ planes, int maxH, int maxW) {
    const vip_jpeg_desc& d = desc[blockIdx.z];
    if (d.ncomp != 3) return;
    if (d.hsamp[0] == 2) ycc_planes<2>(rgb, d, planes, maxH, maxW);
    else ycc_planes<1>(rgb, d, planes, maxH, maxW);
}

// one thread = one 8x8 block; grid.y = image, grid.x covers the image's blocks (all components), as jpeg_idct_kernel does
__global__ __launch_bounds__(64) void jpeg_fdct_quant_kernel(const uint8_t* __restrict__ planes,
                                                             const vip_jpeg_desc* __restrict__ desc,
                                                             int16_t* __restrict__ coef) {
    const vip_jpeg_desc& d = desc[blockIdx.y];
    int blk = blockIdx.x * 64 + threadIdx.x;
    int c = 0;
    for (; c < d.ncomp; ++c) {
        const int nb = d.blocks_w[c] * d.blocks_h[c];
        if (blk < nb) break;
        blk -= nb;
    }
    if (c >= d.ncomp || d.ncomp != 3) return;
    const int bw = d.blocks_w[c];
    const int brow = blk / bw, bcol = blk - brow * bw;
    // Blocks that only fill the last MCU column / row hold no samples: jccoefct.c compress_data writes DUMMY blocks there, all AC zero and
    // the DC of the block before them in the MCU - to the right of the image the block on their left, below it the LAST block of the MCU's
    // row above (for every block of the dummy row).  Such a thread transforms that source block and keeps its DC alone.
    const int rw = (((d.width * d.hsamp[c] + d.hsamp[0] - 1) / d.hsamp[0]) + 7) >> 3;       // blocks that hold samples
    const int rh = (((d.height * d.vsamp[c] + d.vsamp[0] - 1) / d.vsamp[0]) + 7) >> 3;
    int srow = brow, scol = bcol;
    if (srow >= rh) {
        srow = rh - 1;
        scol = bcol - bcol % d.hsamp[c] + d.hsamp[c] - 1;
    }
    if (scol >= rw) scol = rw - 1;
    const bool dummy = srow != brow || scol != bcol;
    const uint8_t* src = planes + d.coef_off[c] + ((long)srow * 8) * (bw * 8) + scol * 8;
    int ws[8][8];  // [row][col]
    // pass 1: rows (level shift, jcdctmgr.c convsamp)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint2 v = *reinterpret_cast<const uint2*>(src + (long)r * (bw * 8));
        int in[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            in[k] = (int)((v.x >> (8 * k)) & 255) - 128;
            in[k + 4] = (int)((v.y >> (8 * k)) & 255) - 128;
        }
        fdct_1d<true>(in, ws[r]);
    }
    // pass 2: columns
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        int in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = ws[r][col];
        fdct_1d<false>(in, out);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r][col] = out[r];
    }
    // quantise (jcdctmgr.c forward_DCT): divisor = 8 * table entry, magnitude rounded to nearest, sign restored; 16-byte stores
    int16_t* dst = coef + d.coef_off[c] + (long)blk * 64;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        uint32_t pk[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int div = (int)d.qt[c][r * 8 + k] << 3;
            const int v = ws[r][k];
            const int mag = ((v < 0 ? -v : v) + (div >> 1)) / div;
            int q = v < 0 ? -mag : mag;
            if (dummy && (r | k) != 0) q = 0;
            pk[k >> 1] |= (uint32_t)(q & 0xffff) << (16 * (k & 1));
        }
        *reinterpret_cast<uint4*>(dst + r * 8) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    }
}

// T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural order
const uint8_t BASE_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                               14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                               18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t BASE_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

uint64_t max_pixels() {      // the per-image cap of the decode paths (pipeline.py, png_host.cpp) covers what is re-encoded too
    const char* s = getenv("VIP_MAX_JPEG_PIXELS");
    if (s && *s) {
        const long long v = atoll(s);
        if (v > 0) return (uint64_t)v;
    }
    return (uint64_t)64 << 20;
}

}  // namespace

extern "C" int vip_jpeg_quality_tables_h(int quality, uint16_t* luma_h, uint16_t* chroma_h) {
    VIP_REQUIRE(luma_h && chroma_h, VIP_ERR_BAD_ARG, "vip_jpeg_quality_tables_h: null pointer");
    VIP_REQUIRE(quality >= 1 && quality <= 100, VIP_ERR_BAD_ARG, "vip_jpeg_quality_tables_h: quality %d outside 1..100", quality);
    // jcparam.c jpeg_quality_scaling + jpeg_add_quant_table(force_baseline = TRUE)
    const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
    for (int i = 0; i < 64; ++i) {
        const int l = (BASE_LUMA[i] * scale + 50) / 100, c = (BASE_CHROMA[i] * scale + 50) / 100;
        luma_h[i] = (uint16_t)(l < 1 ? 1 : (l > 255 ? 255 : l));
        chroma_h[i] = (uint16_t)(c < 1 ? 1 : (c > 255 ? 255 : c));
    }
    return VIP_OK;
}

extern "C" int vip_jpeg_encode_layout_h(int width, int height, int subsampling, int quality, vip_jpeg_desc* desc_h,
                                        size_t* coef_elems_h) {
    VIP_REQUIRE(desc_h && coef_elems_h, VIP_ERR_BAD_ARG, "vip_jpeg_encode_layout_h: null pointer");
    VIP_REQUIRE(width >= 1 && height >= 1 && width <= 65535 && height <= 65535, VIP_ERR_BAD_ARG,
                "vip_jpeg_encode_layout_h: size %dx%d outside 1..65535", width, height);
    VIP_REQUIRE(subsampling == 420 || subsampling == 444, VIP_ERR_BAD_ARG,
                "vip_jpeg_encode_layout_h: subsampling %d (420 or 444)", subsampling);
    const uint64_t cap = max_pixels();
    VIP_REQUIRE((uint64_t)width * (uint64_t)height <= cap, VIP_ERR_BAD_ARG,
                "vip_jpeg_encode_layout_h: %dx%d exceeds VIP_MAX_JPEG_PIXELS=%llu", width, height, (unsigned long long)cap);
    vip_jpeg_desc d;
    memset(&d, 0, sizeof(d));
    const int st = vip_jpeg_quality_tables_h(quality, d.qt[0], d.qt[1]);
    if (st != VIP_OK) return st;
    memcpy(d.qt[2], d.qt[1], sizeof(d.qt[1]));
    d.width = width;
    d.height = height;
    d.ncomp = 3;
    const int s = subsampling == 420 ? 2 : 1;
    const int mcus_x = (width + 8 * s - 1) / (8 * s), mcus_y = (height + 8 * s - 1) / (8 * s);
    size_t off = 0;
    for (int c = 0; c < 3; ++c) {
        d.hsamp[c] = d.vsamp[c] = c == 0 ? s : 1;
        d.blocks_w[c] = mcus_x * d.hsamp[c];
        d.blocks_h[c] = mcus_y * d.vsamp[c];
        d.coef_off[c] = (int64_t)off;
        off += (size_t)d.blocks_w[c] * d.blocks_h[c] * 64;
    }
    *desc_h = d;
    *coef_elems_h = off;
    return VIP_OK;
}

extern "C" int vip_jpeg_fdct_quant_u8(const uint8_t* rgb_u8, const vip_jpeg_desc* desc, int n, int max_blocks,
                                      uint8_t* planes_ws, int16_t* coef, int maxH, int maxW, void* stream) {
    VIP_REQUIRE(rgb_u8 && desc && planes_ws && coef, VIP_ERR_BAD_ARG, "vip_jpeg_fdct_quant_u8: null pointer");
    VIP_REQUIRE(n > 0 && max_blocks > 0 && maxH > 0 && maxW > 0, VIP_ERR_BAD_ARG, "vip_jpeg_fdct_quant_u8: bad size");
    VIP_REQUIRE((reinterpret_cast<uintptr_t>(planes_ws) & 15) == 0 && (reinterpret_cast<uintptr_t>(coef) & 15) == 0,
                VIP_ERR_ALIGNMENT, "vip_jpeg_fdct_quant_u8: planes_ws and coef must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // the padded luma plane of an image is at most maxW, maxH rounded up to whole 16-pixel MCUs
    const int strips = ((maxW + 15) / 16) * 2, rows = ((maxH + 15) / 16) * 16;
    hipLaunchKernelGGL(jpeg_ycc_planes_kernel, dim3((strips + 31) / 32, (rows + 7) / 8, n), dim3(256), 0, s, rgb_u8, desc, planes_ws,
                       maxH, maxW);
    const int st = vip_launch_status("vip_jpeg_fdct_quant_u8(planes)");
    if (st != VIP_OK) return st;
    hipLaunchKernelGGL(jpeg_fdct_quant_kernel, dim3((max_blocks + 63) / 64, n), dim3(64), 0, s, (const uint8_t*)planes_ws, desc,
                       coef);
    return vip_launch_status("vip_jpeg_fdct_quant_u8(fdct)");
}
