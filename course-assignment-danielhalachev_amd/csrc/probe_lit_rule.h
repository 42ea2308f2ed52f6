// probe_lit_rule.h -- the rule of the probe-lit radiance queries (include/crt_hip.h: "Probe-lit radiance"; kernel:
// csrc/kernel_probe_light.h): what a DIFFUSE record of a radiance query takes from an irradiance probe volume in place of the GI build's
// sample rays -- the EXPECTATION of those rays' colours, looked up in the volume's SH9 records -- and how it is put into the reference's own
// normalisation.  One header for the host and the device build: every operation below is one float32 operation with one rounding, in the
// order written (the whole build is -ffp-contract=off), so tests/probe_lit_sets.py restates it in numpy and tests/probe_lit_rule_shim.cpp
// holds that restatement to this file.  It adds two functions to csrc/probe_rule.h and csrc/probe_depth_rule.h and changes nothing of them.
//
// Derivation.  In the GI build a DIFFUSE record's colour is (direct + c_0 + ... + c_{S-1}) * (1 / (float)(S + 1)), S = gi_sample_size,
//   c_i the colour shootRay returns for sample ray i (radiance_combine<true>, csrc/kernel_radiance.h).  gi_sample_direction
//   (csrc/kernel_lane.h) draws angle1 = pi * u1 and angle2 = 2 pi * u2, forms (cos angle1, sin angle1, 0) in the (right, normal, forward)
//   frame and rotates it about the normal by angle2: the angle alpha between the sample and the normal is |pi/2 - angle1|, uniform on
//   [0, pi/2], and the azimuth is uniform.  The density per solid angle is p(omega) = 1 / (pi^2 sin alpha) on the normal's hemisphere; it
//   depends on the normal alone.  The expectation of one sample's colour, Lbar(x, n) = the integral of L(x, omega) p(omega) d omega, is a
//   zonal convolution of the incoming radiance, and by Funk-Hecke its SH band factors are
//       lambda_l = (2 / pi) * the integral over [0, pi/2] of P_l(cos alpha) d alpha:   lambda_0 = 1, lambda_1 = 2 / pi, lambda_2 = 1 / 4
//   where csrc/probe_rule.h's clamped-cosine lookup has A = 1, 2/3, 1/4.
// Zonal resolve.  csrc/probe_rule.h's lookup -- or, with a visibility, csrc/probe_depth_rule.h's -- in the finite test, the per-axis clamp,
//   the corner order, the skipped corners, the weights and the folds W and S[c][ch] (crt_probe_axis, crt_probe_sum_add, the depth tap and
//   the Chebyshev weight, all unchanged), resolved with the zonal table in place of A:
//     no corner used: status 0, Lbar = 0
//     e[ch] = the left fold over c = 0..8, starting from 0.0f, of (Z_c * Y_c(n)) * S[c][ch], Z = 1.0f, 0.63661975f (x3), 0.25f (x5)
//     q = e[ch] / W; Lbar[ch] = q > 0.0f ? q : 0.0f          (a NaN gives 0)
//     status = the number of corners used (1 to 8)
//   x is the record's point and n its normal as the crt_hit holds them (the normal radiance_scatter<true> hands to gi_sample_direction),
//   used as given and not normalised.  A point or normal that is not finite: status 0, Lbar = 0.
// Combine.  For a record whose status byte is CRT_SHADE_DIFFUSE, with direct[ch] the colour crt_shade_hits_device left:
//     ind = (float)S * Lbar[ch]
//     inv = 1.0f / (float)(S + 1u)
//     colour[ch] = (direct[ch] + ind) * inv
//   Every other record keeps its colour's bytes.  A DIFFUSE record of status 0 counts as UNLIT, every other DIFFUSE record as LIT.  With
//   S = 0 and a finite Lbar the colour is (direct + 0.0f) * 1.0f: direct as a float value.  The indirect term is multiplied by no albedo and
//   no texture: the reference's is not either (README, "Split GI frames").
//
// Known limits.
//   * The light is the volume's: as smooth as SH9 and the probe spacing make it, with the leaks the lookup in use has, and as old as the
//     last bake.  Re-baked volumes are not blended over time.
//   * Lbar is the mean of the GI build's estimator when the volume holds the radiance the sample rays would return; a volume baked with
//     max_depth - 1 and gi_sample_size S approximates that.  Nothing checks which options a volume was baked with.
//   * The indirect term carries no albedo (the reference has none).
//   * The frame kernels of crt_launch.hip do not read the volume: crt_render* give the bytes they gave.
//   * The query waits once a level: there is no enqueue-only or graph-capturable form.
//   * Single-device contexts only.
#pragma once

#include "probe_depth_rule.h"

// the Lbar and the status of a lookup whose corners have been added: crt_probe_resolve with the zonal table
CRT_HD uint32_t crt_probe_lit_resolve(const crt_probe_sum *s, const float n[3], float out[3]) {
    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
    if (s->used == 0u) return 0u;
    float Y[9];
    crt_probe_basis(n, Y);
    const float Z[9] = {1.0f, 0.63661975f, 0.63661975f, 0.63661975f, 0.25f, 0.25f, 0.25f, 0.25f, 0.25f};
    for (int ch = 0; ch < 3; ch++) {
        float e = 0.0f;
        for (int c = 0; c < 9; c++) {
            const float zy = Z[c] * Y[c];
            const float term = zy * s->S[3 * c + ch];
            e = e + term;
        }
        const float q = e / s->W;
        out[ch] = q > 0.0f ? q : 0.0f;
    }
    return s->used;
}

// one channel of a DIFFUSE record's colour
CRT_HD float crt_probe_lit_combine(const float direct, const float lbar, const uint32_t samples) {
    const float ind = (float)samples * lbar;
    const float inv = 1.0f / (float)(samples + 1u);
    const float sum = direct + ind;
    return sum * inv;
}
