// probe_depth_rule.h -- the rule of the probe volume's visibility term (include/crt_hip.h: "Probe visibility"; kernels:
// csrc/kernel_probe_depth.h): the depth record a probe keeps beside its SH9 record -- the first two moments of the distance it sees, per
// direction --, the projection that makes it from the hit records of the probe's rays, the tap that reads it in a direction, and the lookup
// that weights every corner of csrc/probe_rule.h's lookup by a one-sided Chebyshev bound on "this probe sees the point".  One header for the
// host and the device build: every operation below is one float32 operation with one rounding, in the order written (the whole build is
// -ffp-contract=off), so tests/probe_depth_sets.py restates it in numpy and tests/probe_depth_rule_shim.cpp holds that restatement to this
// file.  sqrtf is the correctly rounded one; there is no pow and no exp.
//
// Depth record.  crt_probe_depth is 512 bytes: 64 pairs (mean, mean2) of float32, pair k = row * 8 + col the texel (col, row) of an 8 x 8
//   octahedral map of the sphere.  The side is CRT_PROBE_DEPTH_SIDE = 8: a wave's 64 lanes are a probe's 64 texels, and a tap is one
//   8-byte load.
// Texel direction.  e_k is the octahedral decode of the texel's centre:
//     qx = (((float)col + 0.5f) / 8.0f) * 2.0f - 1.0f, qy likewise from row
//     z = (1.0f - |qx|) - |qy|
//     (x, y) = (qx, qy) where z >= 0, otherwise the fold ((1.0f - |qy|) * sgn(qx), (1.0f - |qx|) * sgn(qy)), sgn(v) = v >= 0 ? 1.0f : -1.0f
//     len = sqrtf((x * x + y * y) + z * z); e_k = (x / len, y / len, z / len)
// Ray distance.  For ray j of the probe with the hit record h crt_trace_rays_device wrote:
//     r = (h.hit != 0 && h.t < max_distance) ? h.t : max_distance       (a NaN t gives max_distance)
//     r = r > 0.0f ? r : 0.0f
//   A back-face hit counts with its own distance.  d_j is the direction READ FROM THE RAY ARRAY as given.
// Projection.  For texel k, the left folds over j = 0 .. R - 1 in increasing order, each starting from 0.0f:
//     c = (d_j.x * e_k.x + d_j.y * e_k.y) + d_j.z * e_k.z; c = c > 0.0f ? c : 0.0f
//     w = c^16 by four squarings (w = c * c; w = w * w; w = w * w; w = w * w)
//     W = W + w; S1 = S1 + w * r; S2 = S2 + w * (r * r)
//   The folds run inside one lane: no cross-lane sum, no dependence on arrival.  Where W > 0.0f: mean = S1 / W, mean2 = S2 / W.  Otherwise
//   (nothing seen, or a NaN) the pair is (max_distance, max_distance * max_distance): the texel saw nothing and hides nothing.
// Depth tap.  For a direction u (a unit vector, but any floats are answered):
//     s = (|u.x| + |u.y|) + |u.z|; px = u.x / s; py = u.y / s
//     where u.z < 0.0f: (px, py) = ((1.0f - |py|) * sgn(px), (1.0f - |px|) * sgn(py)), both from the unfolded values
//     per axis: g = (p * 0.5f + 0.5f) * 8.0f - 0.5f, clamped as a float: g = g > -0.5f ? g : -0.5f (a NaN gives -0.5f), then
//         g = g < 7.5f ? g : 7.5f
//     i = (int32_t)g, lowered by one when (float)i > g: the floor, in [-1, 7]; f = g - (float)i
//     the four taps (tx, ty) = (ix + a, iy + b), b = 0, 1 outer, a = 0, 1 inner, have the weights (a ? fx : 1.0f - fx) * (b ? fy : 1.0f - fy)
//     an index outside [0, 7] wraps the octahedral way: tx < 0: tx = 0, ty = 7 - ty; tx > 7: tx = 7, ty = 7 - ty; then, with the new
//         values, ty < 0: ty = 0, tx = 7 - tx; ty > 7: ty = 7, tx = 7 - tx
//     k = ty * 8 + tx; it is compared with 64 as an integer before an address is formed
//     m1 = the left fold over the four taps, starting from 0.0f, of weight * mean_k; m2 likewise of weight * mean2_k
// Lookup.  csrc/probe_rule.h's lookup in the finite test, the per-axis clamp, the corner order, the trilinear weight wc = (wx * wy) * wz from
//   the point x, the skipped corners (wc == 0.0f, or not VALID), crt_probe_resolve and status = the corners used.  A used corner is added
//   with the weight w = wc * vis instead of wc.  With P the corner's crt_probe_position:
//     b.k = x.k + n.k * normal_bias; v.k = b.k - P.k
//     dist = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z)
//     if dist > 0.0f fails (the point AT the probe, or a NaN): vis = 1.0f
//     otherwise u.k = v.k / dist; (m1, m2) = the depth tap of the corner's record at u
//         var = m2 - m1 * m1; var = |var|; var = var > variance_floor ? var : variance_floor        (a NaN gives variance_floor)
//         if dist <= m1: ch = 1.0f
//         else e = dist - m1; ch = var / (var + e * e); ch = (ch * ch) * ch
//         vis = ch > min_weight ? ch : min_weight                                                    (a NaN gives min_weight)
//   There is no direction ("wrap") factor, so with every pair (max_distance, max_distance^2) and every corner within max_distance of b the
//   lookup is csrc/probe_rule.h's bit for bit.
// Parameters.  crt_probe_visibility { uint32_t size; float max_distance, normal_bias, variance_floor, min_weight; }, 20 bytes.  Valid:
//   size == 20, max_distance finite and > 0, normal_bias finite and >= 0, variance_floor finite and > 0, min_weight finite in (0, 1].
//   crt_probe_visibility_defaults fills it from a volume:
//     diag = sqrtf((sx * sx + sy * sy) + sz * sz) of the spacing; max_distance = 1.5f * diag
//     normal_bias = 0.02f * the smallest spacing
//     variance_floor = 1e-6f * (max_distance * max_distance)
//     min_weight = 0.01f
//
// Known limits.
//   * The map's side is fixed at 8: a wall thinner than a texel's footprint at its distance is blurred with what lies behind it.
//   * There is no direction factor: a probe behind the surface's tangent plane is not down-weighted for that.
//   * Back-face hits count with their own distance.
//   * One max_distance per volume.
//   * Static scenes: nothing blends a re-baked depth record over time.
//   * Single-device contexts only.
#pragma once

#include "probe_rule.h"

#define CRT_PROBE_DEPTH_SIDE 8
#define CRT_PROBE_DEPTH_TEXELS 64         // SIDE * SIDE: a wave's lanes

// crt_probe_visibility's layout
struct crt_probe_vis {
    uint32_t size;
    float max_distance, normal_bias, variance_floor, min_weight;
};

CRT_HD bool crt_probe_vis_valid(const crt_probe_vis &p) {
    if (p.size != 20u) return false;
    if (!crt_finite(p.max_distance) || !(p.max_distance > 0.0f)) return false;
    if (!crt_finite(p.normal_bias) || !(p.normal_bias >= 0.0f)) return false;
    if (!crt_finite(p.variance_floor) || !(p.variance_floor > 0.0f)) return false;
    return crt_finite(p.min_weight) && p.min_weight > 0.0f && p.min_weight <= 1.0f;
}

CRT_HD void crt_probe_vis_defaults(const crt_probe_grid &v, crt_probe_vis *p) {
    const float *s = v.spacing;
    const float diag = sqrtf(crt_sum3(s, s));
    float least = s[0];
    if (s[1] < least) least = s[1];
    if (s[2] < least) least = s[2];
    p->size = 20u;
    p->max_distance = 1.5f * diag;
    p->normal_bias = 0.02f * least;
    const float mm = p->max_distance * p->max_distance;
    p->variance_floor = 1e-6f * mm;
    p->min_weight = 0.01f;
}

CRT_HD float crt_probe_sgn(const float v) { return v >= 0.0f ? 1.0f : -1.0f; }

// e_k of texel k < 64
CRT_HD void crt_probe_depth_direction(const uint32_t k, float e[3]) {
    const uint32_t col = k % CRT_PROBE_DEPTH_SIDE, row = k / CRT_PROBE_DEPTH_SIDE;
    const float cx = ((float)col + 0.5f) / 8.0f, cy = ((float)row + 0.5f) / 8.0f;
    const float qx = cx * 2.0f - 1.0f, qy = cy * 2.0f - 1.0f;
    const float ax = fabsf(qx), ay = fabsf(qy);
    const float zx = 1.0f - ax;
    const float z = zx - ay;
    float x = qx, y = qy;
    if (z < 0.0f) {
        const float fx = 1.0f - ay, fy = 1.0f - ax;
        x = fx * crt_probe_sgn(qx);
        y = fy * crt_probe_sgn(qy);
    }
    const float d[3] = {x, y, z};
    const float len = sqrtf(crt_sum3(d, d));
    e[0] = x / len;
    e[1] = y / len;
    e[2] = z / len;
}

// the distance ray j counts with
CRT_HD float crt_probe_depth_distance(const uint32_t hit, const float t, const float max_distance) {
    const float r = (hit != 0u && t < max_distance) ? t : max_distance;
    return r > 0.0f ? r : 0.0f;
}

// a texel's folds
struct crt_probe_depth_sum {
    float W, S1, S2;
};

CRT_HD void crt_probe_depth_reset(crt_probe_depth_sum *s) { s->W = 0.0f; s->S1 = 0.0f; s->S2 = 0.0f; }

// one ray of direction d and distance r, seen from the texel of direction e
CRT_HD void crt_probe_depth_add(crt_probe_depth_sum *s, const float e[3], const float d[3], const float r) {
    float c = crt_sum3(d, e);
    c = c > 0.0f ? c : 0.0f;
    float w = c * c;
    w = w * w;
    w = w * w;
    w = w * w;
    const float wr = w * r;
    const float rr = r * r;
    const float wrr = w * rr;
    s->W = s->W + w;
    s->S1 = s->S1 + wr;
    s->S2 = s->S2 + wrr;
}

CRT_HD void crt_probe_depth_pair(const crt_probe_depth_sum *s, const float max_distance, float pair[2]) {
    if (s->W > 0.0f) {
        pair[0] = s->S1 / s->W;
        pair[1] = s->S2 / s->W;
    } else {
        pair[0] = max_distance;
        pair[1] = max_distance * max_distance;
    }
}

// one axis of the tap: the floor of the texel coordinate, in [-1, 7], and the fraction
CRT_HD void crt_probe_depth_axis(const float p, int32_t *i, float *f) {
    const float h = p * 0.5f + 0.5f;
    const float h8 = h * 8.0f;
    float g = h8 - 0.5f;
    g = g > -0.5f ? g : -0.5f;
    g = g < 7.5f ? g : 7.5f;
    int32_t k = (int32_t)g;   // -0.5 <= g <= 7.5
    if ((float)k > g) k--;
    *i = k;
    *f = g - (float)k;
}

// the texel (tx, ty), each in [-1, 8], wrapped the octahedral way -> k < 64
CRT_HD uint32_t crt_probe_depth_wrap(int32_t tx, int32_t ty) {
    if (tx < 0) { tx = 0; ty = 7 - ty; }
    else if (tx > 7) { tx = 7; ty = 7 - ty; }
    if (ty < 0) { ty = 0; tx = 7 - tx; }
    else if (ty > 7) { ty = 7; tx = 7 - tx; }
    return (uint32_t)(ty * CRT_PROBE_DEPTH_SIDE + tx);
}

// where the four taps of a direction lie and what they weigh
struct crt_probe_depth_taps {
    uint32_t k[4];
    float w[4];
};

CRT_HD void crt_probe_depth_tap(const float u[3], crt_probe_depth_taps *t) {
    const float ax = fabsf(u[0]), ay = fabsf(u[1]), az = fabsf(u[2]);
    const float axy = ax + ay;
    const float s = axy + az;
    float px = u[0] / s, py = u[1] / s;
    if (u[2] < 0.0f) {
        const float fx = 1.0f - fabsf(py), fy = 1.0f - fabsf(px);
        const float sx = crt_probe_sgn(px), sy = crt_probe_sgn(py);
        px = fx * sx;
        py = fy * sy;
    }
    int32_t ix, iy;
    float fx, fy;
    crt_probe_depth_axis(px, &ix, &fx);
    crt_probe_depth_axis(py, &iy, &fy);
    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
    for (int b = 0; b < 2; b++)
        for (int a = 0; a < 2; a++) {
            t->k[2 * b + a] = crt_probe_depth_wrap(ix + a, iy + b);
            t->w[2 * b + a] = wx[a] * wy[b];
        }
}

// the moments of the four pairs pairs[i] = (mean, mean2) of texel t->k[i]
CRT_HD void crt_probe_depth_blend(const crt_probe_depth_taps *t, const float pairs[4][2], float *m1, float *m2) {
    float a = 0.0f, b = 0.0f;
    for (int i = 0; i < 4; i++) {
        const float ta = t->w[i] * pairs[i][0], tb = t->w[i] * pairs[i][1];
        a = a + ta;
        b = b + tb;
    }
    *m1 = a;
    *m2 = b;
}

// v = (x + n * normal_bias) - P and its length
CRT_HD float crt_probe_vis_offset(const crt_probe_vis &p, const float x[3], const float n[3], const float P[3], float v[3]) {
    for (int k = 0; k < 3; k++) {
        const float nb = n[k] * p.normal_bias;
        const float b = x[k] + nb;
        v[k] = b - P[k];
    }
    return sqrtf(crt_sum3(v, v));
}

// the Chebyshev weight of a corner at distance dist > 0 whose tap gave (m1, m2)
CRT_HD float crt_probe_vis_weight(const crt_probe_vis &p, const float dist, const float m1, const float m2) {
    const float mm = m1 * m1;
    float var = m2 - mm;
    var = fabsf(var);
    var = var > p.variance_floor ? var : p.variance_floor;
    float ch = 1.0f;
    if (!(dist <= m1)) {
        const float e = dist - m1;
        const float ee = e * e;
        const float den = var + ee;
        ch = var / den;
        const float c2 = ch * ch;
        ch = c2 * ch;
    }
    return ch > p.min_weight ? ch : p.min_weight;
}
