// The host build of csrc/variance_rule.h behind a C entry point: tests/test_variance_host.py compiles this with g++ -ffp-contract=off and
// holds the numpy restatement of the rule (tests/variance_sets.py) to it.
#include <vector>

#include "../course-assignment-danielhalachev_amd/csrc/variance_rule.h"

static_assert(sizeof(crt_history_record) == 64, "crt_history_pixel's 64 bytes");

// one image of width x height pixels; the guides' fields as crt_hit has them, one array each; records: 64-byte records aligned to 16
extern "C" void shim_variance(float min_history, uint32_t normal_squarings, float sigma_plane, int32_t width, int32_t height,
                              const crt_history_record *records, const float *t, const float *point, const float *normal, const uint32_t *mesh,
                              const uint32_t *hit, const float *var, float *out_var) {
    const crt_variance_rule rule{min_history, normal_squarings, sigma_plane};
    const int64_t n = (int64_t)width * height;
    std::vector<crt_guide> guides((size_t)n);
    for (int64_t i = 0; i < n; i++) guides[(size_t)i] = crt_guide_of(t[i], point + 3 * i, normal + 3 * i, mesh[i], hit[i]);
    for (int32_t y = 0; y < height; y++)
        for (int32_t x = 0; x < width; x++) {
            const int64_t i = (int64_t)y * width + x;
            out_var[i] = crt_variance_pixel(rule, width, height, y, x, records, guides.data(), var[i]);
        }
}
