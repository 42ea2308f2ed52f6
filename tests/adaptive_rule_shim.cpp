// The host build of csrc/adaptive_rule.h behind a C entry point: tests/test_adaptive_host.py compiles this with g++ -ffp-contract=off
// and holds the numpy restatement of the rule (tests/adaptive_sets.py) to it.
#include "../course-assignment-danielhalachev_amd/csrc/adaptive_rule.h"

// one step for n pixels: colour, sum, mean 3 floats a pixel; keep one byte a pixel
extern "C" void shim_adaptive_step(uint32_t min_samples, uint32_t max_samples, float threshold, float floor, uint32_t s, const float *colour,
                                   uint64_t n, float *sum, float *sq, uint32_t *count, float *mean, uint8_t *keep) {
    const crt_adaptive_rule rule{min_samples, max_samples, threshold, floor};
    for (uint64_t i = 0; i < n; i++)
        keep[i] = crt_adaptive_step(rule, s, colour[3 * i], colour[3 * i + 1], colour[3 * i + 2], sum + 3 * i, sq + i, count + i, mean + 3 * i) ? 1 : 0;
}
