// The host build of csrc/denoise_rule.h behind C entry points: tests/test_denoise_host.py compiles this with g++ -ffp-contract=off and
// holds the numpy restatement of the rule (tests/denoise_sets.py) to it.
#include <vector>

#include "../course-assignment-danielhalachev_amd/csrc/denoise_rule.h"

// from the fold's state, n pixels: sum and mean 3 floats a pixel
extern "C" void shim_denoise_variance(const float *sum, const float *sq, const uint32_t *count, uint64_t n, float *mean, float *var) {
    for (uint64_t i = 0; i < n; i++) {
        const crt_denoise_pixel p = crt_denoise_variance(sum + 3 * i, sq[i], count[i]);
        mean[3 * i] = p.c[0]; mean[3 * i + 1] = p.c[1]; mean[3 * i + 2] = p.c[2];
        var[i] = p.v;
    }
}

// `iterations` iterations on a width x height image; the guides' fields as crt_hit has them, one array each
extern "C" void shim_denoise(uint32_t iterations, uint32_t normal_squarings, float sigma_colour, float sigma_plane, float floor, int32_t width,
                             int32_t height, const float *rgb, const float *var, const float *t, const float *point, const float *normal,
                             const uint32_t *mesh, const uint32_t *hit, float *out_rgb, float *out_var) {
    const crt_denoise_rule rule{normal_squarings, sigma_colour, sigma_plane, floor};
    const int64_t n = (int64_t)width * height;
    std::vector<crt_denoise_pixel> a(n), b(n);
    std::vector<crt_guide> g(n);
    for (int64_t i = 0; i < n; i++) {
        a[i].c[0] = rgb[3 * i]; a[i].c[1] = rgb[3 * i + 1]; a[i].c[2] = rgb[3 * i + 2];
        a[i].v = var[i];
        g[i] = crt_guide_of(t[i], point + 3 * i, normal + 3 * i, mesh[i], hit[i]);
    }
    for (uint32_t k = 0; k < iterations; k++) {
        for (int32_t y = 0; y < height; y++)
            for (int32_t x = 0; x < width; x++) b[(int64_t)y * width + x] = crt_denoise_atrous(rule, width, height, (int32_t)(1u << k), y, x, a.data(), g.data());
        a.swap(b);
    }
    for (int64_t i = 0; i < n; i++) {
        out_rgb[3 * i] = a[i].c[0]; out_rgb[3 * i + 1] = a[i].c[1]; out_rgb[3 * i + 2] = a[i].c[2];
        out_var[i] = a[i].v;
    }
}
