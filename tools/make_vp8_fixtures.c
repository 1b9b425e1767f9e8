/* Driver of libwebp's advanced encoding API for tools/make_vp8_fixtures.py: one lossy WebP file with the settings that
 * Pillow's encoder cannot be asked for.
 *   make_vp8_fixtures out.webp width height seed quality method filter_type partitions segments sharpness strength
 * The picture is synthetic (smooth waves, a block of noise, a flat corner), so nothing but the settings is needed to
 * make the file again. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <webp/encode.h>

int main(int argc, char** argv) {
    if (argc != 12) return 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]);
    uint32_t s = (uint32_t)atoi(argv[4]) * 2654435761u + 1u;
    WebPConfig cfg;
    if (!WebPConfigPreset(&cfg, WEBP_PRESET_DEFAULT, (float)atof(argv[5]))) return 3;
    cfg.method = atoi(argv[6]);
    cfg.filter_type = atoi(argv[7]);
    cfg.partitions = atoi(argv[8]);
    cfg.segments = atoi(argv[9]);
    cfg.filter_sharpness = atoi(argv[10]);
    cfg.filter_strength = atoi(argv[11]);
    cfg.autofilter = 0;
    if (!WebPValidateConfig(&cfg)) return 4;
    uint8_t* rgb = (uint8_t*)malloc((size_t)w * h * 3);
    if (!rgb) return 5;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c) {
                s = s * 1664525u + 1013904223u;
                double v = 128 + 100 * sin(x / 5.0 + c) * cos(y / 4.0 - c);
                if (x >= w / 2 && y < h / 2) v += (double)((s >> 24) & 63) - 32;       /* noise: busy segments */
                if (x < w / 3 && y >= 2 * h / 3) v = 40 + 60 * c;                      /* flat: skipped macroblocks */
                rgb[((size_t)y * w + x) * 3 + c] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
            }
    WebPPicture pic;
    WebPMemoryWriter wr;
    if (!WebPPictureInit(&pic)) return 6;
    pic.width = w;
    pic.height = h;
    if (!WebPPictureImportRGB(&pic, rgb, w * 3)) return 7;
    WebPMemoryWriterInit(&wr);
    pic.writer = WebPMemoryWrite;
    pic.custom_ptr = &wr;
    if (!WebPEncode(&cfg, &pic)) return 8;
    FILE* f = fopen(argv[1], "wb");
    if (!f) return 9;
    fwrite(wr.mem, 1, wr.size, f);
    fclose(f);
    WebPPictureFree(&pic);
    WebPMemoryWriterClear(&wr);
    free(rgb);
    return 0;
}
