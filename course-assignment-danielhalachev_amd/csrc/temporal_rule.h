// temporal_rule.h -- the rule of the GI frames' temporal accumulation (include/crt_hip.h: "Temporal accumulation"; kernel:
// csrc/kernel_temporal.h): SVGF's temporal half for a camera that moves through a static scene.  A pixel's first hit is projected into the
// previous frame's camera, the previous frame's accumulated moments are fetched there with a bilinear tap whose four corners are tested
// against the pixel's own guide (mesh, normal, plane), and what survives is merged with this frame's moments by sample count.  One header
// for the host and the device build: every operation below is one float32 operation with one rounding, in the order written (the whole
// build is -ffp-contract=off), so tests/temporal_sets.py restates it in numpy and tests/temporal_rule_shim.cpp holds that restatement to
// this file.  There is no exp, pow or sqrt in it; floorf is exact.
//
// Records.  A history pixel is 64 bytes, aligned 16: {n[3], t, x[3], mesh, c[3], m2, weight, pad[3]}.  n[3], t, x[3], mesh is the guide of
// the frame that wrote it (filter_rule.h: crt_guide_of; mesh = 0xFFFFFFFF is a miss), c[3] the accumulated mean colour, m2 the
// accumulated mean of r*r + g*g + b*b, weight the number of samples the record stands for, as a float; pad is written as 0.  A tap reads it
// with four 16-byte loads from one 64-byte half line.  A pose is {position[3], matrix[9]}, what crt_set_camera takes: (o, m) below.
// finite(x) is (x - x) == 0.0f.
//
// Pixel p = (y, x) of a width x height frame, with the guide G_p = {n_p, t_p, x_p, mesh_p} of the pixel's crt_hit, the fold's state sum[3],
// sq, count, the previous pose (o, m) and the previous history array:
//   current:
//     n_c = (float)count
//     count == 0: C_c = 0, q_c = 0
//     else: inv = 1.0f / n_c; C_c = sum_c * inv; q_c = sq * inv
//   reproject:
//     no history array, or mesh_p is a miss: no history (n_h = 0, valid = 0)
//     w_j = x_p.j - o.j, j = 0..2
//     v_i = (w_0*m[3i] + w_1*m[3i+1]) + w_2*m[3i+2], i = 0..2
//     depth = 0.0f - v_2
//     skip unless depth > 0                          // a NaN skips
//     sx = v_0 / depth; sy = v_1 / depth
//     aspect = (float)width / (float)height
//     sx = sx / aspect
//     fx = ((sx + 1.0f) * 0.5f) * (float)width - 0.5f
//     fy = ((1.0f - sy) * 0.5f) * (float)height - 0.5f
//     skip unless fx > -1.0f && fx < (float)width && fy > -1.0f && fy < (float)height
//     x0 = floorf(fx); y0 = floorf(fy)
//     ax = fx - x0; ay = fy - y0
//     bx = 1.0f - ax; by = 1.0f - ay
//     tol = sigma_plane * t_p
//     acc = {0,0,0}; accq = 0; accn = 0; wsum = 0; valid = 0
//     taps q in the order (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1) with b = by*bx, by*ax, ay*bx, ay*ax:
//         skip q outside the frame                   // integer comparison, before any address is formed
//         skip unless weight_q > 0 and c_q[0..2], m2_q, weight_q are all finite
//         skip unless mesh_q == mesh_p
//         d = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
//         skip unless d >= normal_min
//         e = (n_p.x*(x_q.x - x_p.x) + n_p.y*(x_q.y - x_p.y)) + n_p.z*(x_q.z - x_p.z)
//         skip unless fabsf(e) <= tol
//         wsum = wsum + b
//         acc_c = acc_c + b * c_q,c
//         accq = accq + b * m2_q
//         accn = accn + b * weight_q
//         valid = valid + 1
//     wsum > 0: inv = 1.0f / wsum; C_h,c = acc_c * inv; q_h = accq * inv; n_h = accn * inv
//     else: n_h = 0
//   merge:
//     n_h = n_h < max_history ? n_h : max_history
//     n_h == 0: C = C_c, q = q_c, n = n_c            // exactly: a pixel without history is the denoiser's own input
//     else: n = n_h + n_c; inv = 1.0f / n; a_h = n_h * inv; a_c = n_c * inv
//           C_c' = a_h * C_h,c + a_c * C_c,c
//           q = a_h * q_h + a_c * q_c
//     n == 0: C = 0, q = 0, V = 0
//     else: mm = (C_r*C_r + C_g*C_g) + C_b*C_b
//           var = q - mm
//           V = (var > 0 ? var : 0) * (1.0f / n)
//   write:
//     next[p] = {G_p, C, q, n}; out_rgb[p] = C; out_var[p] = V; out_valid[p] = valid (0..4)
// The matrix product is the transpose of getRay's row-vector product: the reference's camera matrices are products of rotations, whose
// inverse is the transpose.  A non-finite current sample gives a non-finite record; the next frame skips such a record as a tap, so a NaN
// lives for one frame.
//
// Known limits.
//   * A miss pixel keeps no history.
//   * A matrix that is not a rotation reprojects wrongly.  The geometry tests reject most of those taps, but not a slide within one plane.
//   * Reflections are reprojected as if painted on the mirror.
//   * The history holds the unfiltered moments: the filtered colour is not fed back.
#pragma once

#include "filter_rule.h"

// what the rule reads of a crt_temporal (include/crt_hip.h)
struct crt_temporal_rule {
    float max_history, normal_min, sigma_plane;
};

// crt_camera_pose's fields
struct crt_temporal_pose {
    float o[3], m[9];
};

// what a pixel gives beside its record
struct crt_temporal_out {
    crt_history_record r;
    float v;
    uint32_t valid;
};

// The pixel (y, x) of a width x height frame (width * height < 2^31, so both fit int32_t); `prev` is the previous frame's row-major records
// or null.  A tap's coordinates are compared with the frame as integers before its address is formed.
CRT_HD crt_temporal_out crt_temporal_pixel(const crt_temporal_rule rule, const int32_t width, const int32_t height, const crt_guide GP,
                                           const float sum[3], const float sq, const uint32_t count, const crt_temporal_pose pose,
                                           const crt_history_record *prev) {
    // current
    const float nc = (float)count;
    float cc[3] = {0.0f, 0.0f, 0.0f}, qc = 0.0f;
    if (count != 0u) {
        const float inv = 1.0f / nc;
        cc[0] = sum[0] * inv;
        cc[1] = sum[1] * inv;
        cc[2] = sum[2] * inv;
        qc = sq * inv;
    }
    // reproject
    float ch[3] = {0.0f, 0.0f, 0.0f}, qh = 0.0f, nh = 0.0f;
    uint32_t valid = 0u;
    if (prev && GP.mesh != CRT_GUIDE_MISS) {
        const float w0 = GP.x[0] - pose.o[0], w1 = GP.x[1] - pose.o[1], w2 = GP.x[2] - pose.o[2];
        float v[3];
        for (int i = 0; i < 3; i++) {
            const float a = w0 * pose.m[3 * i], b = w1 * pose.m[3 * i + 1], c = w2 * pose.m[3 * i + 2];
            const float ab = a + b;
            v[i] = ab + c;
        }
        const float depth = 0.0f - v[2];
        if (depth > 0.0f) {
            float sx = v[0] / depth;
            const float sy = v[1] / depth;
            const float fw = (float)width, fh = (float)height;
            const float aspect = fw / fh;
            sx = sx / aspect;
            const float ux = sx + 1.0f, uy = 1.0f - sy;
            const float hx = ux * 0.5f, hy = uy * 0.5f;
            const float px = hx * fw, py = hy * fh;
            const float fx = px - 0.5f, fy = py - 0.5f;
            if (fx > -1.0f && fx < fw && fy > -1.0f && fy < fh) {
                const float x0 = floorf(fx), y0 = floorf(fy);
                const float ax = fx - x0, ay = fy - y0;
                const float bx = 1.0f - ax, by = 1.0f - ay;
                const int32_t ix = (int32_t)x0, iy = (int32_t)y0;   // -1 .. width - 1, -1 .. height - 1
                const float tol = rule.sigma_plane * GP.t;
                const float B[4] = {by * bx, by * ax, ay * bx, ay * ax};
                float acc[3] = {0.0f, 0.0f, 0.0f}, accq = 0.0f, accn = 0.0f, wsum = 0.0f;
                for (int k = 0; k < 4; k++) {
                    const int32_t qx = ix + (k & 1), qy = iy + (k >> 1);
                    if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;
                    const crt_history_record Q = prev[(int64_t)qy * width + qx];
                    if (!CRT_USABLE(Q.c, Q.m2, Q.weight)) continue;
                    if (Q.g.mesh != GP.mesh) continue;
                    const float d = crt_normal_dot(GP, Q.g.n);
                    if (!(d >= rule.normal_min)) continue;
                    const float ae = crt_plane_distance(GP, Q.g.x);
                    if (!(ae <= tol)) continue;
                    const float b = B[k];
                    wsum = wsum + b;
                    const float b0 = b * Q.c[0], b1 = b * Q.c[1], b2 = b * Q.c[2];
                    acc[0] = acc[0] + b0;
                    acc[1] = acc[1] + b1;
                    acc[2] = acc[2] + b2;
                    const float bq = b * Q.m2;
                    accq = accq + bq;
                    const float bn = b * Q.weight;
                    accn = accn + bn;
                    valid = valid + 1u;
                }
                if (wsum > 0.0f) {
                    const float inv = 1.0f / wsum;
                    ch[0] = acc[0] * inv;
                    ch[1] = acc[1] * inv;
                    ch[2] = acc[2] * inv;
                    qh = accq * inv;
                    nh = accn * inv;
                }
            }
        }
    }
    // merge
    nh = nh < rule.max_history ? nh : rule.max_history;
    float C[3] = {cc[0], cc[1], cc[2]}, q = qc, n = nc;
    if (!(nh == 0.0f)) {
        n = nh + nc;
        const float inv = 1.0f / n;
        const float ah = nh * inv, ac = nc * inv;
        for (int c = 0; c < 3; c++) {
            const float h = ah * ch[c], u = ac * cc[c];
            C[c] = h + u;
        }
        const float h = ah * qh, u = ac * qc;
        q = h + u;
    }
    float V = 0.0f;
    if (n == 0.0f) {
        C[0] = 0.0f; C[1] = 0.0f; C[2] = 0.0f;
        q = 0.0f;
    } else {
        V = crt_variance_of_mean(C, q, n);
    }
    // write
    crt_temporal_out R;
    R.r.g = GP;
    R.r.c[0] = C[0]; R.r.c[1] = C[1]; R.r.c[2] = C[2];
    R.r.m2 = q;
    R.r.weight = n;
    R.r.pad[0] = 0.0f; R.r.pad[1] = 0.0f; R.r.pad[2] = 0.0f;
    R.v = V;
    R.valid = valid;
    return R;
}
