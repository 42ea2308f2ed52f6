// split_rule.h -- the additive split of a GI sample into its direct light and the rest (include/crt_hip.h: "Split GI frames"; kernels:
// csrc/kernel_split.h), one header for the host and the device build: every operation below is one float32 operation with one rounding
// (the whole build is -ffp-contract=off), so tests/split_sets.py restates it in numpy and tests/split_rule_shim.cpp holds that
// restatement to this file.
//
// Why additive.  The reference's calculateDiffusion (RayTracer.cpp:300-356) gives a diffuse hit
//     colour = (sum over lights of k * base + sum of the GI sample rays' colours) * (1 / (GI_SAMPLE_SIZE + 1))
// and the texture / albedo `base` multiplies the direct term alone.  Dividing the pixel by the albedo would stamp the inverse texture into
// the indirect light; subtracting the direct term takes every texel and every hard shadow edge out of what the filters see, and leaves
// them the only part with Monte-Carlo noise.
//
// The direct part of a sample (radiance_keep_direct), from the level-0 status of its ray and the level's colour array as the lighting
// launches left it (L: a DIFFUSE record's direct light, a BACKGROUND record's final colour), gi_inv = 1.0f / (float)(gi_sample_size + 1):
//     CRT_SHADE_DIFFUSE     direct_c = L_c * gi_inv
//     CRT_SHADE_BACKGROUND  direct_c = L_c                        // a miss or a constant material: no noise but the jitter's
//     otherwise             direct_c = 0.0f                       // mirrors, glass, invalid records: the whole colour is "rest"
// The fold (split_fold), entry i, pixel p:
//     r_c      = rgb[3i+c] - direct[3i+c]
//     dsum_c   = (sample == 0 ? 0.0f : dsum_c) + direct[3i+c]
//     rsum_c   = (sample == 0 ? 0.0f : rsum_c) + r_c
//     rsq      = (sample == 0 ? 0.0f : rsq) + ((r_r*r_r + r_g*r_g) + r_b*r_b)
// Putting it back (split_recombine), pixel p:
//     count == 0: out_c = filtered_c
//     else:       inv = 1.0f / (float)count; out_c = filtered_c + dsum_c * inv
// A sample with an infinite channel in both parts gives inf - inf = NaN in the rest.
#pragma once

#include "filter_rule.h"

// the CRT_SHADE_* values the rule tells apart (include/crt_hip.h)
enum : uint32_t { CRT_SPLIT_BACKGROUND = 0u, CRT_SPLIT_DIFFUSE = 1u };

CRT_HD void crt_split_direct(const uint32_t status, const float L[3], const uint32_t gi_sample_size, float direct[3]) {
    const float gi_inv = 1.0f / (float)(gi_sample_size + 1u);
    for (int c = 0; c < 3; c++) direct[c] = status == CRT_SPLIT_DIFFUSE ? L[c] * gi_inv : (status == CRT_SPLIT_BACKGROUND ? L[c] : 0.0f);
}

CRT_HD void crt_split_fold(const uint32_t sample, const float rgb[3], const float direct[3], float dsum[3], float rsum[3], float *rsq) {
    float r[3];
    for (int c = 0; c < 3; c++) {
        r[c] = rgb[c] - direct[c];
        dsum[c] = (sample == 0u ? 0.0f : dsum[c]) + direct[c];
        rsum[c] = (sample == 0u ? 0.0f : rsum[c]) + r[c];
    }
    const float r2 = crt_sum3(r, r);
    *rsq = (sample == 0u ? 0.0f : *rsq) + r2;
}

CRT_HD void crt_split_recombine(const uint32_t count, const float filtered[3], const float dsum[3], float out[3]) {
    if (count == 0u) {
        for (int c = 0; c < 3; c++) out[c] = filtered[c];
        return;
    }
    const float inv = 1.0f / (float)count;
    for (int c = 0; c < 3; c++) {
        const float dmean = dsum[c] * inv;
        out[c] = filtered[c] + dmean;
    }
}
