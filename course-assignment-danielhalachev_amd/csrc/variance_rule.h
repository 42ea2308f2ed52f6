// variance_rule.h -- the rule of the GI frames' variance estimate (include/crt_hip.h: "Variance estimate"; kernel: csrc/kernel_variance.h):
// SVGF's variance-estimation stage.  Where a pixel's accumulated sample count is below a threshold, its variance of the mean is replaced by
// a 7x7 cross-bilateral estimate from the moments of geometrically similar neighbours.  Only the variance is replaced; the colour is never
// touched.  One header for the host and the device build: every operation below is one float32 operation with one rounding, in the order
// written (the whole build is -ffp-contract=off), so tests/variance_sets.py restates it in numpy and tests/variance_rule_shim.cpp holds that
// restatement to this file.  There is no exp, pow or sqrt in it.
//
// Definitions.  finite(x) is (x - x) == 0.0f.  A moment record is M = {c[3], m2, weight}, the fields of a crt_history_pixel (the record's
// own guide fields are not read).  usable(M): weight > 0 and c[0..2], m2, weight all finite.  A guide is G = {n[3], x[3], t, mesh}, taken
// from a crt_hit as the denoiser takes it (filter_rule.h: crt_guide_of; mesh = 0xFFFFFFFF when hit == 0).  V_in is the incoming
// variance of the mean.  The window radius is 3 and is not a setting.
//
// Centre p = (y, x) of a width x height image.  It passes through, V' = V_in, when
//     !usable(M_p), or mesh_p is a miss, or !(weight_p < min_history)
// Otherwise the centre is FLAGGED:
//     tol = sigma_plane * t_p
//     acc = {0,0,0}; accq = 0; wsum = 0
//     for dy in -3..3, dx in -3..3 (row-major), q = (y+dy, x+dx); the offsets are compared with the room the centre has before a coordinate is formed:
//         skip q outside the frame
//         skip q with !usable(M_q)
//         skip q with mesh_q != mesh_p
//         d  = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
//         d  = d > 0 ? d : 0
//         d  = d * d, normal_squarings times
//         e  = (n_p.x*(x_q.x - x_p.x) + n_p.y*(x_q.y - x_p.y)) + n_p.z*(x_q.z - x_p.z)
//         ae = fabsf(e)
//         skip unless ae <= tol                      // a NaN skips
//         wz = tol > 0 ? 1.0f - ae / tol : 1.0f
//         w  = d * wz
//         acc_c = acc_c + w * c_q,c
//         accq  = accq + w * m2_q
//         wsum  = wsum + w
//     if wsum > 0:
//         inv = 1.0f / wsum
//         Cb_c = acc_c * inv
//         qb  = accq * inv
//         mm  = (Cb_r*Cb_r + Cb_g*Cb_g) + Cb_b*Cb_b
//         var = qb - mm
//         iw  = 1.0f / weight_p
//         V'  = (var > 0 ? var : 0) * iw
//     else:
//         V' = V_in                                  // a flagged centre with no surviving tap, or a NaN weight sum
// The centre is its own tap (dy = dx = 0) and passes every test whose operands are finite, with d = |n_p|^2 squared and wz = 1.  A NaN that
// arises from overflow or from a non-finite guide is whatever these lines give: a NaN w makes wsum NaN, and the centre passes through.
//
// The geometry lines are the denoiser's own (filter_rule.h: crt_geometry_weight), with the same names.  weight_p is the number of samples
// the centre's record stands for, so V' is a variance OF THE MEAN, as the denoiser's and the temporal rule's V are.
//
// Known limits.
//   * A miss pixel is never estimated: it has no geometry to compare, and the a-trous filter averages misses under the colour weight alone.
//   * The estimate is spatial: where the neighbourhood is a texture or a shadow edge inside one mesh and plane, the detail counts as variance
//     and the filter smooths it more.  The split frames (csrc/split_rule.h) hand this rule the moments of the indirect light only.
//   * The window is 7x7 and dense; it does not widen where few taps survive.
#pragma once

#include "filter_rule.h"

#define CRT_VARIANCE_RADIUS 3   // the window is (2 * 3 + 1)^2 = 49 taps

// what the rule reads of a crt_variance_estimate (include/crt_hip.h)
struct crt_variance_rule {
    float min_history;
    uint32_t normal_squarings;
    float sigma_plane;
};

// The 12 words a tap needs, as three 16-byte vectors: {n, mesh}, {x, weight}, {c, m2}.  The kernel keeps each in a plane of its own.
struct alignas(16) crt_variance_tap_geometry {
    float n[3];
    uint32_t mesh;
};
struct alignas(16) crt_variance_tap_place {
    float x[3], weight;
};
struct alignas(16) crt_variance_tap_moments {
    float c[3], m2;
};

struct crt_variance_sums {
    float acc[3], accq, wsum;
};

// usable(M) of a tap's or the centre's moments (a function of the 16-byte vector, as the kernel reads it from its plane)
CRT_HD bool crt_variance_usable(const crt_variance_tap_moments m, const float weight) { return CRT_USABLE(m.c, m.m2, weight); }

// the centre test: true when the centre is FLAGGED, false when it passes through
CRT_HD bool crt_variance_flagged(const crt_variance_rule rule, const crt_variance_tap_moments m, const float weight, const uint32_t mesh) {
    if (!crt_variance_usable(m, weight)) return false;
    if (mesh == CRT_GUIDE_MISS) return false;
    return weight < rule.min_history;
}

CRT_HD crt_variance_sums crt_variance_begin() {
    crt_variance_sums s;
    s.acc[0] = 0.0f; s.acc[1] = 0.0f; s.acc[2] = 0.0f;
    s.accq = 0.0f;
    s.wsum = 0.0f;
    return s;
}

// One tap inside the frame against the flagged centre's guide GP and tol = sigma_plane * t_p.  A tap staged for a place outside the frame
// has weight 0 and is skipped as not usable.
CRT_HD void crt_variance_tap(const crt_variance_rule rule, const crt_guide GP, const float tol, const crt_variance_tap_geometry A,
                             const crt_variance_tap_place B, const crt_variance_tap_moments Q, crt_variance_sums &s) {
    if (!crt_variance_usable(Q, B.weight)) return;
    if (A.mesh != GP.mesh) return;
    float w;
    if (!crt_geometry_weight(GP, tol, rule.normal_squarings, A.n, B.x, &w)) return;
    const float w0 = w * Q.c[0], w1 = w * Q.c[1], w2 = w * Q.c[2];
    s.acc[0] = s.acc[0] + w0;
    s.acc[1] = s.acc[1] + w1;
    s.acc[2] = s.acc[2] + w2;
    const float wq = w * Q.m2;
    s.accq = s.accq + wq;
    s.wsum = s.wsum + w;
}

// behind the 49 taps of a flagged centre
CRT_HD float crt_variance_finish(const crt_variance_sums s, const float weight_p, const float v_in) {
    if (!(s.wsum > 0.0f)) return v_in;
    const float inv = 1.0f / s.wsum;
    const float cb[3] = {s.acc[0] * inv, s.acc[1] * inv, s.acc[2] * inv};
    const float qb = s.accq * inv;
    return crt_variance_of_mean(cb, qb, weight_p);
}

CRT_HD crt_variance_tap_moments crt_variance_moments_of(const crt_history_record r) {
    crt_variance_tap_moments m;
    m.c[0] = r.c[0]; m.c[1] = r.c[1]; m.c[2] = r.c[2];
    m.m2 = r.m2;
    return m;
}

// The rule at the centre (y, x) of a width x height image (width * height < 2^31, so both fit int32_t), every tap from the row-major arrays
// of the whole image: `moments` (of which c, m2 and weight are read) and `guides`.  Every tap offset is compared with the room the centre has
// BEFORE the coordinate is formed, so no signed sum overflows and no address outside the image exists.  The kernel runs the same three
// functions on a tile staged in LDS.
CRT_HD float crt_variance_pixel(const crt_variance_rule rule, const int32_t width, const int32_t height, const int32_t y, const int32_t x,
                                const crt_history_record *moments, const crt_guide *guides, const float v_in) {
    const int64_t at = (int64_t)y * width + x;
    const crt_history_record MP = moments[at];
    const crt_guide GP = guides[at];
    if (!crt_variance_flagged(rule, crt_variance_moments_of(MP), MP.weight, GP.mesh)) return v_in;
    const float tol = rule.sigma_plane * GP.t;
    crt_variance_sums s = crt_variance_begin();
    for (int32_t dy = -CRT_VARIANCE_RADIUS; dy <= CRT_VARIANCE_RADIUS; dy++) {
        if (dy < -y || dy >= height - y) continue;
        for (int32_t dx = -CRT_VARIANCE_RADIUS; dx <= CRT_VARIANCE_RADIUS; dx++) {
            if (dx < -x || dx >= width - x) continue;
            const int64_t q = (int64_t)(y + dy) * width + (x + dx);
            const crt_history_record MQ = moments[q];
            const crt_guide GQ = guides[q];
            crt_variance_tap_geometry A;
            A.n[0] = GQ.n[0]; A.n[1] = GQ.n[1]; A.n[2] = GQ.n[2];
            A.mesh = GQ.mesh;
            crt_variance_tap_place B;
            B.x[0] = GQ.x[0]; B.x[1] = GQ.x[1]; B.x[2] = GQ.x[2];
            B.weight = MQ.weight;
            crt_variance_tap(rule, GP, tol, A, B, crt_variance_moments_of(MQ), s);
        }
    }
    return crt_variance_finish(s, MP.weight, v_in);
}
