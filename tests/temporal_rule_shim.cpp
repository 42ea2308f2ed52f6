// The host build of csrc/temporal_rule.h behind a C entry point: tests/test_temporal_host.py compiles this with g++ -ffp-contract=off and
// holds the numpy restatement of the rule (tests/temporal_sets.py) to it.
#include "../course-assignment-danielhalachev_amd/csrc/temporal_rule.h"

static_assert(sizeof(crt_history_record) == 64, "crt_history_pixel's 64 bytes");

// one frame of width x height pixels; the guides' fields as crt_hit has them, one array each; prev: 64-byte records or null (pose: 12 floats)
extern "C" void shim_temporal(float max_history, float normal_min, float sigma_plane, int32_t width, int32_t height, const float *pose,
                              const crt_history_record *prev, const float *sum, const float *sq, const uint32_t *count, const float *t,
                              const float *point, const float *normal, const uint32_t *mesh, const uint32_t *hit, crt_history_record *next,
                              float *out_rgb, float *out_var, uint8_t *out_valid) {
    const crt_temporal_rule rule{max_history, normal_min, sigma_plane};
    crt_temporal_pose p{};
    if (prev) {
        for (int i = 0; i < 3; i++) p.o[i] = pose[i];
        for (int i = 0; i < 9; i++) p.m[i] = pose[3 + i];
    }
    for (int32_t y = 0; y < height; y++)
        for (int32_t x = 0; x < width; x++) {
            const int64_t i = (int64_t)y * width + x;
            const crt_guide g = crt_guide_of(t[i], point + 3 * i, normal + 3 * i, mesh[i], hit[i]);
            const crt_temporal_out r = crt_temporal_pixel(rule, width, height, g, sum + 3 * i, sq[i], count[i], p, prev);
            next[i] = r.r;
            out_rgb[3 * i] = r.r.c[0]; out_rgb[3 * i + 1] = r.r.c[1]; out_rgb[3 * i + 2] = r.r.c[2];
            out_var[i] = r.v;
            out_valid[i] = (uint8_t)r.valid;
        }
}
