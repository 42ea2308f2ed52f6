// filter_rule.h -- what the rules of the GI frames' filter stages share (denoise_rule.h, temporal_rule.h, variance_rule.h, adaptive_rule.h,
// split_rule.h): the guide of a first hit, the history record, the geometry test of a tap against a centre's guide, and the moments.  One
// header for the host and the device build.  Every function is a sequence of single float32 operations with one rounding each, in the order
// written (the whole build is -ffp-contract=off); the rules' own headers state what these lines compute, and the tests' numpy restatements
// hold them to it.  A stage that is still to come takes its geometry test and its variance of the mean from here.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef CRT_HD   // (the math headers glibc_powf.h, glibc_sincosf.h and gi_random.h stand alone and carry the same definition)
#if defined(__HIPCC__) || defined(__HIP__)
#define CRT_HD __host__ __device__ __forceinline__
#else
#define CRT_HD static inline
#endif
#endif

#define CRT_GUIDE_MISS 0xFFFFFFFFu   // a guide's mesh where the camera's ray hit nothing

// the guide record: 32 bytes, aligned 16, so that a tap reads it with two 16-byte loads
struct alignas(16) crt_guide {
    float n[3], t;
    float x[3];
    uint32_t mesh;
};

// crt_history_pixel's layout (include/crt_hip.h), aligned so that a record is four 16-byte loads
struct alignas(16) crt_history_record {
    crt_guide g;
    float c[3], m2;
    float weight, pad[3];
};

CRT_HD bool crt_finite(const float x) { return (x - x) == 0.0f; }

// the guide of a first hit: (t, point, normal, mesh, hit) of a crt_hit
CRT_HD crt_guide crt_guide_of(const float t, const float point[3], const float normal[3], const uint32_t mesh, const uint32_t hit) {
    crt_guide g;
    g.n[0] = normal[0]; g.n[1] = normal[1]; g.n[2] = normal[2];
    g.t = t;
    g.x[0] = point[0]; g.x[1] = point[1]; g.x[2] = point[2];
    g.mesh = hit ? mesh : CRT_GUIDE_MISS;
    return g;
}

// (a0*b0 + a1*b1) + a2*b2: three products, then two sums in this association
CRT_HD float crt_sum3(const float a[3], const float b[3]) {
    const float p0 = a[0] * b[0], p1 = a[1] * b[1], p2 = a[2] * b[2];
    const float p01 = p0 + p1;
    return p01 + p2;
}

// ---- the geometry of a tap with normal n[3] at x[3] against the centre's guide GP

// d = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
CRT_HD float crt_normal_dot(const crt_guide GP, const float n[3]) { return crt_sum3(GP.n, n); }

// ae = fabsf(e), e = (n_p.x*(x_q.x - x_p.x) + n_p.y*(x_q.y - x_p.y)) + n_p.z*(x_q.z - x_p.z)
CRT_HD float crt_plane_distance(const crt_guide GP, const float x[3]) {
    const float o[3] = {x[0] - GP.x[0], x[1] - GP.x[1], x[2] - GP.x[2]};
    const float e = crt_sum3(GP.n, o);
    return fabsf(e);
}

// The denoiser's and the variance estimate's weight of a tap of the centre's mesh, tol = sigma_plane * t_p: the clamped cosine squared
// normal_squarings times, by the tent over the plane distance.  False: the tap is skipped (a NaN distance skips), and *g is not written.
CRT_HD bool crt_geometry_weight(const crt_guide GP, const float tol, const uint32_t normal_squarings, const float n[3], const float x[3], float *g) {
    float d = crt_normal_dot(GP, n);
    d = d > 0.0f ? d : 0.0f;
    for (uint32_t k = 0; k < normal_squarings; k++) d = d * d;
    const float ae = crt_plane_distance(GP, x);
    if (!(ae <= tol)) return false;
    float wz = 1.0f;
    if (tol > 0.0f) {
        const float r = ae / tol;
        wz = 1.0f - r;
    }
    *g = d * wz;
    return true;
}

// ---- the moments {c[3], m2, weight} of a history record

// usable(M): weight > 0 and c[0..2], m2, weight all finite.  A macro, not a function: as a function temporal_reproject takes 54 vector
// registers, expanded in place 52 (tools/kernel_regs.sh).  `weight` is evaluated twice: pass it a value, not an expression with an effect.
#define CRT_USABLE(c, m2, weight) \
    ((weight) > 0.0f && crt_finite((c)[0]) && crt_finite((c)[1]) && crt_finite((c)[2]) && crt_finite(m2) && crt_finite(weight))

// V = (var > 0 ? var : 0) * (1.0f / n) with var = q - ((C_r*C_r + C_g*C_g) + C_b*C_b): the variance OF THE MEAN C of n samples whose mean
// of r*r + g*g + b*b is q
CRT_HD float crt_variance_of_mean(const float C[3], const float q, const float n) {
    const float mm = crt_sum3(C, C);
    const float var = q - mm;
    const float inv = 1.0f / n;
    return (var > 0.0f ? var : 0.0f) * inv;
}
