// denoise_rule.h -- the rule of the GI frames' denoiser (include/crt_hip.h: "Denoising"; kernels: csrc/kernel_denoise.h): a spatial,
// variance-guided, edge-avoiding a-trous wavelet filter on first-hit guides -- SVGF's spatial half, with no temporal part.  One header for
// the host and the device build: every operation below is one float32 operation with one rounding, in the order written (the whole build
// is -ffp-contract=off), so tests/denoise_sets.py restates it in numpy and tests/denoise_rule_shim.cpp holds that restatement to this file.
//
// Definitions.  finite(x) is (x - x) == 0.0f.  A pixel is usable when its three colour channels and its variance are all finite.  A guide is
// {n[3], x[3], t, mesh}, taken from a crt_hit: normal, point, t and mesh; mesh = 0xFFFFFFFF when hit == 0.
// h = {1/16, 1/4, 3/8, 1/4, 1/16}.  g3 = {1,2,1; 2,4,2; 1,2,1} as floats.
//
// From the fold's state (crt_sample_variance_device).  n = count.  When n == 0, colour and variance are 0.  Otherwise:
//     inv = 1.0f / (float)n
//     C_c = sum_c * inv                              // adaptive_rule.h's mean
//     q   = sq * inv
//     mm  = (C_r*C_r + C_g*C_g) + C_b*C_b
//     var = q - mm
//     V   = (var > 0 ? var : 0) * inv                // the variance OF THE MEAN
//
// Iteration k (step = 1 << k), centre p = (y, x).  A centre that is not usable passes through: C' = C, V' = V.  Otherwise:
//     vnum = 0; vden = 0
//     for dy in -1..1, dx in -1..1 (row-major), q = (y+dy, x+dx) inside the frame and finite(V_q):
//         vnum = vnum + g3[dy+1][dx+1] * V_q
//         vden = vden + g3[dy+1][dx+1]
//     vp  = vnum / vden
//     s2  = sigma_colour * sigma_colour
//     den = s2 * vp + floor
//     tol = sigma_plane * t_p
//     acc = {0,0,0}; accv = 0; wsum = 0
//     for dy in -2..2, dx in -2..2 (row-major), q = (y + dy*step, x + dx*step) in signed arithmetic:
//         skip q outside the frame
//         skip q not usable
//         skip q with mesh_q != mesh_p
//         if mesh_p is a hit:
//             d  = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
//             d  = d > 0 ? d : 0
//             d  = d * d, normal_squarings times
//             e  = (n_p.x*(x_q.x - x_p.x) + n_p.y*(x_q.y - x_p.y)) + n_p.z*(x_q.z - x_p.z)
//             ae = fabsf(e)
//             skip unless ae <= tol                  // a NaN skips
//             wz = tol > 0 ? 1.0f - ae / tol : 1.0f
//             g  = d * wz
//         else:
//             g = 1.0f
//         dr, dg, db = C_q - C_p
//         d2 = (dr*dr + dg*dg) + db*db
//         wl = den / (den + d2)
//         w  = ((h[dy+2] * h[dx+2]) * g) * wl
//         acc_c = acc_c + w * C_q,c
//         accv  = accv + (w*w) * V_q
//         wsum  = wsum + w
//     if wsum > 0:
//         inv = 1.0f / wsum
//         C'_c = acc_c * inv
//         V'   = accv * (inv * inv)
//     else:
//         pass through
// iterations == 0 copies input to output.  A NaN that arises from overflow is whatever these lines give.
//
// There is no exp, pow or sqrt in it: the colour weight is the rational den / (den + d2) -- 1 at d2 = 0, 1/2 where the squared colour
// distance equals sigma_colour^2 times the local variance of the mean -- the normal weight is a power of two of the cosine by repeated
// squaring, and the plane weight is a tent.  Each is one correctly rounded IEEE operation a line, the same on every device and host.
//
// Known limits.
//   * There is no albedo demodulation, because the library has no albedo query.  Texture detail inside one mesh is protected by the colour
//     weight alone.  The split frames (csrc/split_rule.h) feed this rule the indirect light only and add the direct light, which carries
//     the texels, back untouched.
//   * Reflections in a flat mirror are guided by the mirror's own plane.
//   * With count == 1 every variance is 0, so the filter hardly smooths.  Use at least 2 samples -- or the variance estimate
//     (csrc/variance_rule.h), which replaces the variance of such pixels before this rule runs.
#pragma once

#include "filter_rule.h"

// what the rule reads of a crt_denoise (include/crt_hip.h)
struct crt_denoise_rule {
    uint32_t normal_squarings;
    float sigma_colour, sigma_plane, floor;
};

// the work area's records (kernel_denoise.h: denoise_pack): a crt_guide and this one, 16 bytes, aligned to its size
struct alignas(16) crt_denoise_pixel {
    float c[3], v;
};

CRT_HD bool crt_denoise_usable(const crt_denoise_pixel p) { return crt_finite(p.c[0]) && crt_finite(p.c[1]) && crt_finite(p.c[2]) && crt_finite(p.v); }

// From the fold's state: the mean and the variance of the mean.
CRT_HD crt_denoise_pixel crt_denoise_variance(const float sum[3], const float sq, const uint32_t count) {
    crt_denoise_pixel p;
    p.c[0] = 0.0f; p.c[1] = 0.0f; p.c[2] = 0.0f; p.v = 0.0f;
    if (count == 0u) return p;
    const float n = (float)count;
    const float inv = 1.0f / n;
    const float C[3] = {sum[0] * inv, sum[1] * inv, sum[2] * inv};
    p.c[0] = C[0]; p.c[1] = C[1]; p.c[2] = C[2];
    const float q = sq * inv;
    p.v = crt_variance_of_mean(C, q, n);   // the rule's "* inv": the same division of the same operands gives the same float
    return p;
}

// One iteration at the centre (y, x) of a width x height image (width * height < 2^31, so both fit int32_t): `in` and `guides` are the
// row-major records of the whole image.  Every tap offset is compared with the room the centre has BEFORE the coordinate is formed, so no
// signed sum overflows and no address outside the image exists.
CRT_HD crt_denoise_pixel crt_denoise_atrous(const crt_denoise_rule rule, const int32_t width, const int32_t height, const int32_t step, const int32_t y,
                                            const int32_t x, const crt_denoise_pixel *in, const crt_guide *guides) {
    const float H5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float G3[3][3] = {{1.0f, 2.0f, 1.0f}, {2.0f, 4.0f, 2.0f}, {1.0f, 2.0f, 1.0f}};
    const int64_t at = (int64_t)y * width + x;
    const crt_denoise_pixel P = in[at];
    if (!crt_denoise_usable(P)) return P;
    float vnum = 0.0f, vden = 0.0f;
    for (int32_t dy = -1; dy <= 1; dy++) {
        if (dy < -y || dy >= height - y) continue;
        for (int32_t dx = -1; dx <= 1; dx++) {
            if (dx < -x || dx >= width - x) continue;
            const float vq = in[(int64_t)(y + dy) * width + (x + dx)].v;
            if (!crt_finite(vq)) continue;
            const float gv = G3[dy + 1][dx + 1] * vq;
            vnum = vnum + gv;
            vden = vden + G3[dy + 1][dx + 1];
        }
    }
    const float vp = vnum / vden;
    const float s2 = rule.sigma_colour * rule.sigma_colour;
    const float s2v = s2 * vp;
    const float den = s2v + rule.floor;
    const crt_guide GP = guides[at];
    const float tol = rule.sigma_plane * GP.t;
    float acc[3] = {0.0f, 0.0f, 0.0f}, accv = 0.0f, wsum = 0.0f;
    for (int32_t dy = -2; dy <= 2; dy++) {
        const int32_t oy = dy * step;
        if (oy < -y || oy >= height - y) continue;
        for (int32_t dx = -2; dx <= 2; dx++) {
            const int32_t ox = dx * step;
            if (ox < -x || ox >= width - x) continue;
            const int64_t q = (int64_t)(y + oy) * width + (x + ox);
            const crt_denoise_pixel Q = in[q];
            if (!crt_denoise_usable(Q)) continue;
            const crt_guide GQ = guides[q];
            if (GQ.mesh != GP.mesh) continue;
            float g = 1.0f;
            if (GP.mesh != CRT_GUIDE_MISS && !crt_geometry_weight(GP, tol, rule.normal_squarings, GQ.n, GQ.x, &g)) continue;
            const float dc[3] = {Q.c[0] - P.c[0], Q.c[1] - P.c[1], Q.c[2] - P.c[2]};
            const float d2 = crt_sum3(dc, dc);
            const float dd = den + d2;
            const float wl = den / dd;
            const float hh = H5[dy + 2] * H5[dx + 2];
            const float hg = hh * g;
            const float w = hg * wl;
            const float w0 = w * Q.c[0], w1 = w * Q.c[1], w2 = w * Q.c[2];
            acc[0] = acc[0] + w0;
            acc[1] = acc[1] + w1;
            acc[2] = acc[2] + w2;
            const float ww = w * w;
            const float wv = ww * Q.v;
            accv = accv + wv;
            wsum = wsum + w;
        }
    }
    if (!(wsum > 0.0f)) return P;
    const float inv = 1.0f / wsum;
    crt_denoise_pixel R;
    R.c[0] = acc[0] * inv;
    R.c[1] = acc[1] * inv;
    R.c[2] = acc[2] * inv;
    const float i2 = inv * inv;
    R.v = accv * i2;
    return R;
}
