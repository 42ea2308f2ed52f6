// adaptive_rule.h -- the stopping rule of an adaptively sampled GI frame (include/crt_hip.h: "Adaptive sampling"; kernels:
// csrc/kernel_adaptive.h), one header for the host and the device build: every operation below is one float32 operation with one
// rounding (the whole build is -ffp-contract=off), so tests/adaptive_sets.py restates it in numpy and tests/adaptive_rule_shim.cpp
// holds that restatement to this file.
//
// State of a pixel: the fold's sum[3] (kernel_progressive.h), one float sq, one uint32 count.  Step for sample s with colour (r, g, b),
// n = s + 1:
//     sum_c   = (s == 0 ? 0.0f : sum_c) + c                      // unchanged: progressive_accumulate's expression
//     sq      = (s == 0 ? 0.0f : sq) + ((r*r + g*g) + b*b)
//     inv     = 1.0f / (float)n
//     mean_c  = sum_c * inv                                       // unchanged
//     q       = sq * inv
//     mm      = (mean_r*mean_r + mean_g*mean_g) + mean_b*mean_b
//     var     = q - mm
//     bound   = ((threshold*threshold) * (float)n) * (mm > floor ? mm : floor)
//     converged = (var <= bound)                                  // false when either side is NaN; a negative var converges
//     count   = n
//     keep    = (n < max_samples) && !(n >= min_samples && converged)
// The squared standard error of the mean, var / n, is at most threshold^2 x max(|mean|^2, floor): no division, no square root.  A pixel
// with a NaN or infinite sample never converges (inf - inf and NaN compare false) and runs to max_samples; a pixel of identical samples
// has var <= 0 up to rounding and stops at min_samples.
#pragma once

#include "filter_rule.h"

// what the rule reads of a crt_adaptive (include/crt_hip.h)
struct crt_adaptive_rule {
    uint32_t min_samples, max_samples;
    float threshold, floor;
};

// One step of a pixel's state; `mean` receives the three means.  Returns keep: the pixel is shot again.
CRT_HD bool crt_adaptive_step(const crt_adaptive_rule rule, const uint32_t s, const float r, const float g, const float b, float sum[3], float *sq,
                              uint32_t *count, float mean[3]) {
    const uint32_t n = s + 1u;
    sum[0] = (s == 0u ? 0.0f : sum[0]) + r;
    sum[1] = (s == 0u ? 0.0f : sum[1]) + g;
    sum[2] = (s == 0u ? 0.0f : sum[2]) + b;
    const float c[3] = {r, g, b};
    const float c2 = crt_sum3(c, c);
    *sq = (s == 0u ? 0.0f : *sq) + c2;
    const float inv = 1.0f / (float)n;
    mean[0] = sum[0] * inv;
    mean[1] = sum[1] * inv;
    mean[2] = sum[2] * inv;
    const float q = *sq * inv;
    const float mm = crt_sum3(mean, mean);
    const float var = q - mm;
    const float t2 = rule.threshold * rule.threshold;
    const float t2n = t2 * (float)n;
    const float bound = t2n * (mm > rule.floor ? mm : rule.floor);
    const bool converged = var <= bound;
    *count = n;
    return (n < rule.max_samples) && !(n >= rule.min_samples && converged);
}
