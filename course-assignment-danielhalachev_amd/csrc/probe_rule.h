// probe_rule.h -- the rule of the irradiance probe volume (include/crt_hip.h: "Irradiance probes"; kernels: csrc/kernel_probes.h): where
// the probes of a volume stand, the rays of a probe, the projection of the colours those rays return onto nine spherical-harmonic
// coefficients per channel (SH9), which probes count as inside geometry, and the lookup that turns a volume of such probes into the diffuse
// light at a point with a normal.  One header for the host and the device build: every operation below is one float32 operation with one
// rounding, in the order written (the whole build is -ffp-contract=off), so tests/probe_sets.py restates it in numpy and
// tests/probe_rule_shim.cpp holds that restatement to this file.  sqrtf is the correctly rounded one; sine and cosine are
// csrc/glibc_sincosf.h's.
//
// Volume.  crt_probe_volume { float origin[3], spacing[3]; uint32_t nx, ny, nz, rays; uint32_t gi_seed; float backface_limit; }.
//   Probe p = (iz * ny + iy) * nx + ix stands at position.k = origin.k + (float)i_k * spacing.k (the product is rounded, then the sum).
//   Valid volumes have nx, ny, nz >= 1, 1 <= rays <= 4096, nx * ny * nz < 2^24, finite origin, spacing finite and > 0, and backface_limit
//   finite in [0, 1].
// Directions.  Ray j of R = rays is a spherical Fibonacci point, the same set for every probe:
//     z = 1.0f - (float)(2j + 1) / (float)R
//     r = sqrtf(max(0, 1.0f - z * z))                   (m = 1.0f - z * z; m > 0 ? m : 0)
//     t = (float)j * 0.618034f, then t = t - (float)(int32_t)t
//     phi = t * 6.2831855f
//     d = (r * crt_cosf(phi), r * crt_sinf(phi), z)      (phi lies in [0, 2 pi], inside the |y| < 120 range of csrc/glibc_sincosf.h)
//   The ray is {probe position, d}, shot as CRT_RAY_REFLECTION (back faces are not culled).  Its GI key is
//   crt_gi_mix(crt_gi_mix(gi_seed, p), j).
// Basis.  Nine real SH functions of a direction (x, y, z), in the fixed order 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2:
//     Y0 = 0.282095f
//     Y1 = 0.488603f * y; Y2 = 0.488603f * z; Y3 = 0.488603f * x
//     Y4 = 1.092548f * (x * y); Y5 = 1.092548f * (y * z); Y7 = 1.092548f * (x * z)
//     Y6 = 0.315392f * (3.0f * (z * z) - 1.0f)
//     Y8 = 0.546274f * (x * x - y * y)
// Projection.  For probe p, coefficient c, channel ch, with L the colour shootRay returned for ray (p, j) and d_j the direction READ FROM
//   THE RAY ARRAY as given (so the projection also serves a caller's own uniform direction set):
//     lane partial: part[l], l = 0..63, is the left fold, starting from 0.0f, over j = l, l + 64, ... in increasing order of
//         L[p][j][ch] * Y_c(d_j)
//     tree: for step = 32, 16, 8, 4, 2, 1: part[l] = part[l] + part[l + step] for l < step
//     coef[c][ch] = part[0] * (12.566371f / (float)R)
//   That is what a wave of 64 lanes does with cross-lane moves; numpy restates it with a reshape.
// Validity.  Optional, and off when backface_limit == 1.0f.  The same rays go through crt_trace_rays_device; back counts the hits with
//   (n.x * d.x + n.y * d.y) + n.z * d.z > 0.0f (n the hit's normal), miss the rays without a hit.  The probe is INVALID when
//   (float)back > backface_limit * (float)R, otherwise VALID.  The counts are integers (ballot and popcount): no order dependence.
// Record.  crt_probe is 128 bytes, one cache line: 27 floats coef[c][ch], then uint32 rays, back, miss, state, and one pad word written
//   as 0.  state: CRT_PROBE_INVALID = 0, CRT_PROBE_VALID = 1; the lookup takes every other value as INVALID.  The projection writes
//   back = 0, miss = 0, state = VALID; the validity pass writes back, miss and state over them.
// Lookup.  For a point x with normal n, used as given and not normalised:
//     if any coordinate of x or n is not finite ((v - v) == 0.0f fails): status 0, colour 0; decided before any conversion to an integer
//     per axis k: g = (x.k - origin.k) / spacing.k, clamped as a float: g < 0 ? 0 : (g > (float)(n_k - 1) ? (float)(n_k - 1) : g)
//         i0 = (int32_t)g, lowered to n_k - 2 when n_k > 1 and i0 > n_k - 2; f = g - (float)i0
//         the two corners i0 and i0 + 1 have the weights 1.0f - f and f; with n_k == 1 only i0 = 0 with weight 1.0f exists
//     corners run in the order dz, dy, dx (dx fastest), with weight w = (wx * wy) * wz
//     an INVALID corner and a corner of weight 0 are skipped; every corner index is compared with nx * ny * nz as an integer before an
//         address is formed
//     W = the left fold of the used weights, S[c][ch] = the left fold of w * coef[c][ch], both starting from 0.0f
//     no corner used: status 0, colour 0
//     e[ch] = the left fold over c = 0..8, starting from 0.0f, of (A_c * Y_c(n)) * S[c][ch], A = 1.0f, 0.6666667f (x3), 0.25f (x5)
//     q = e[ch] / W; out[ch] = q > 0.0f ? q : 0.0f          (a NaN gives 0)
//     status = the number of corners used (1 to 8)
//   A_c is the clamped-cosine convolution divided by pi: the result is the colour a white Lambertian surface would show.
//
// Known limits.
//   * Every probe uses the same direction set: there is no per-probe rotation, and re-baked volumes are not blended over time.
//   * There is no visibility (Chebyshev) term, so light leaks through thin walls.
//   * SH9 rings under hard directional light.
//   * The volume is not fed into the frame kernels: a frame does not read it.
//   * Single-device contexts only.
#pragma once

#include "filter_rule.h"
#include "gi_random.h"
#include "glibc_sincosf.h"

#define CRT_PROBE_STATE_INVALID 0u
#define CRT_PROBE_STATE_VALID 1u
#define CRT_PROBE_MAX_RAYS 4096u
#define CRT_PROBE_MAX_PROBES (1u << 24)   // nx * ny * nz stays below it
#define CRT_PROBE_COEFS 27                // coef[c][ch] at 3 * c + ch
// the record's words behind the 27 coefficients
#define CRT_PROBE_WORD_RAYS 27
#define CRT_PROBE_WORD_BACK 28
#define CRT_PROBE_WORD_MISS 29
#define CRT_PROBE_WORD_STATE 30
#define CRT_PROBE_WORD_PAD 31

// the volume as the rule reads it (crt_probe_volume's layout)
struct crt_probe_grid {
    float origin[3], spacing[3];
    uint32_t n[3], rays;
    uint32_t gi_seed;
    float backface_limit;
};

CRT_HD bool crt_probe_grid_valid(const crt_probe_grid &v) {
    for (int k = 0; k < 3; k++)
        if (v.n[k] == 0u || !crt_finite(v.origin[k]) || !crt_finite(v.spacing[k]) || !(v.spacing[k] > 0.0f)) return false;
    if (v.rays == 0u || v.rays > CRT_PROBE_MAX_RAYS) return false;
    if ((uint64_t)v.n[0] * v.n[1] >= CRT_PROBE_MAX_PROBES || (uint64_t)v.n[0] * v.n[1] * v.n[2] >= CRT_PROBE_MAX_PROBES) return false;
    return crt_finite(v.backface_limit) && v.backface_limit >= 0.0f && v.backface_limit <= 1.0f;
}

CRT_HD uint32_t crt_probe_count(const crt_probe_grid &v) { return v.n[0] * v.n[1] * v.n[2]; }

// where probe p < crt_probe_count stands
CRT_HD void crt_probe_position(const crt_probe_grid &v, const uint32_t p, float position[3]) {
    const uint32_t ix = p % v.n[0], rest = p / v.n[0];
    const uint32_t i[3] = {ix, rest % v.n[1], rest / v.n[1]};
    for (int k = 0; k < 3; k++) {
        const float step = (float)i[k] * v.spacing[k];
        position[k] = v.origin[k] + step;
    }
}

// direction j < rays of a set of `rays` directions
CRT_HD void crt_probe_direction(const uint32_t j, const uint32_t rays, float d[3]) {
    const float q = (float)(2u * j + 1u) / (float)rays;
    const float z = 1.0f - q;
    const float zz = z * z;
    const float m = 1.0f - zz;
    const float r = sqrtf(m > 0.0f ? m : 0.0f);
    float t = (float)j * 0.618034f;
    t = t - (float)(int32_t)t;
    const float phi = t * 6.2831855f;
    d[0] = r * crt_cosf(phi);
    d[1] = r * crt_sinf(phi);
    d[2] = z;
}

CRT_HD uint32_t crt_probe_key(const uint32_t gi_seed, const uint32_t p, const uint32_t j) { return crt_gi_mix(crt_gi_mix(gi_seed, p), j); }

// the nine basis functions of a direction
CRT_HD void crt_probe_basis(const float d[3], float Y[9]) {
    const float x = d[0], y = d[1], z = d[2];
    const float xy = x * y, yz = y * z, xz = x * z, xx = x * x, yy = y * y, zz = z * z;
    const float z3 = 3.0f * zz;
    const float zm = z3 - 1.0f;
    const float xmy = xx - yy;
    Y[0] = 0.282095f;
    Y[1] = 0.488603f * y;
    Y[2] = 0.488603f * z;
    Y[3] = 0.488603f * x;
    Y[4] = 1.092548f * xy;
    Y[5] = 1.092548f * yz;
    Y[6] = 0.315392f * zm;
    Y[7] = 1.092548f * xz;
    Y[8] = 0.546274f * xmy;
}

// one ray of a lane's partial sums: acc[3 * c + ch] = acc[3 * c + ch] + L[ch] * Y_c(d)
CRT_HD void crt_probe_accumulate(const float L[3], const float d[3], float acc[CRT_PROBE_COEFS]) {
    float Y[9];
    crt_probe_basis(d, Y);
    for (int c = 0; c < 9; c++)
        for (int ch = 0; ch < 3; ch++) {
            const float term = L[ch] * Y[c];
            acc[3 * c + ch] = acc[3 * c + ch] + term;
        }
}

// what part[0] is multiplied by
CRT_HD float crt_probe_scale(const uint32_t rays) { return 12.566371f / (float)rays; }

// whether a hit with normal n counts as a back face for a ray of direction d
CRT_HD bool crt_probe_backfacing(const float n[3], const float d[3]) { return crt_sum3(n, d) > 0.0f; }

CRT_HD uint32_t crt_probe_state_of(const uint32_t back, const uint32_t rays, const float backface_limit) {
    const float most = backface_limit * (float)rays;
    return (float)back > most ? CRT_PROBE_STATE_INVALID : CRT_PROBE_STATE_VALID;
}

CRT_HD bool crt_probe_point_finite(const float x[3], const float n[3]) {
    return crt_finite(x[0]) && crt_finite(x[1]) && crt_finite(x[2]) && crt_finite(n[0]) && crt_finite(n[1]) && crt_finite(n[2]);
}

// one axis of the lookup for a finite coordinate: the lower corner and the two weights; count: the axis' corners, 1 or 2
CRT_HD void crt_probe_axis(const float x, const float origin, const float spacing, const uint32_t n, uint32_t *i0, float w[2], uint32_t *count) {
    const float o = x - origin;
    float g = o / spacing;
    const float hi = (float)(n - 1u);
    g = g < 0.0f ? 0.0f : (g > hi ? hi : g);
    if (n == 1u) {
        *i0 = 0u; w[0] = 1.0f; w[1] = 0.0f; *count = 1u;
        return;
    }
    int32_t i = (int32_t)g;   // 0 <= g <= n - 1 < 2^24
    if (i > (int32_t)n - 2) i = (int32_t)n - 2;
    const float f = g - (float)i;
    *i0 = (uint32_t)i;
    w[0] = 1.0f - f;
    w[1] = f;
    *count = 2u;
}

// the lookup's state between corners: W, S and the corners used
struct crt_probe_sum {
    float W, S[CRT_PROBE_COEFS];
    uint32_t used;
};

CRT_HD void crt_probe_sum_reset(crt_probe_sum *s) {
    s->W = 0.0f;
    for (int i = 0; i < CRT_PROBE_COEFS; i++) s->S[i] = 0.0f;
    s->used = 0u;
}

// a VALID corner of weight w != 0 with the coefficients coef[27]
CRT_HD void crt_probe_sum_add(crt_probe_sum *s, const float w, const float coef[CRT_PROBE_COEFS]) {
    s->W = s->W + w;
    for (int i = 0; i < CRT_PROBE_COEFS; i++) {
        const float term = w * coef[i];
        s->S[i] = s->S[i] + term;
    }
    s->used++;
}

// the colour and the status of a lookup whose corners have been added
CRT_HD uint32_t crt_probe_resolve(const crt_probe_sum *s, const float n[3], float out[3]) {
    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
    if (s->used == 0u) return 0u;
    float Y[9];
    crt_probe_basis(n, Y);
    const float A[9] = {1.0f, 0.6666667f, 0.6666667f, 0.6666667f, 0.25f, 0.25f, 0.25f, 0.25f, 0.25f};
    for (int ch = 0; ch < 3; ch++) {
        float e = 0.0f;
        for (int c = 0; c < 9; c++) {
            const float ay = A[c] * Y[c];
            const float term = ay * s->S[3 * c + ch];
            e = e + term;
        }
        const float q = e / s->W;
        out[ch] = q > 0.0f ? q : 0.0f;
    }
    return s->used;
}
