// The host build of csrc/split_rule.h behind C entry points: tests/test_split_host.py compiles this with g++ -ffp-contract=off and holds
// the numpy restatement of the rule (tests/split_sets.py) to it.
#include "../course-assignment-danielhalachev_amd/csrc/split_rule.h"

extern "C" void shim_split_direct(const uint8_t *status, const float *light, uint32_t gi_sample_size, uint64_t n, float *direct) {
    for (uint64_t i = 0; i < n; i++) crt_split_direct(status[i], light + 3 * i, gi_sample_size, direct + 3 * i);
}

// entry i is pixel i; the state is updated in place
extern "C" void shim_split_fold(uint32_t sample, const float *rgb, const float *direct, uint64_t n, float *dsum, float *rsum, float *rsq) {
    for (uint64_t i = 0; i < n; i++) crt_split_fold(sample, rgb + 3 * i, direct + 3 * i, dsum + 3 * i, rsum + 3 * i, rsq + i);
}

extern "C" void shim_split_recombine(const uint32_t *count, const float *filtered, const float *dsum, uint64_t n, float *out) {
    for (uint64_t i = 0; i < n; i++) crt_split_recombine(count[i], filtered + 3 * i, dsum + 3 * i, out + 3 * i);
}
