// bake_rule.h -- the rule of lightmap baking (include/crt_hip.h: "Lightmap baking"; kernels: csrc/kernel_bake.h): where the texels of a
// mesh's UV layout lie in the world, which triangle owns a texel, the probe ray a texel is lit through, the keys and the fold of its GI
// samples, and the dilation that fills the texels beside a chart.  One header for the host and the device build: every operation below is
// one float32 operation with one rounding, in the order written (the whole build is -ffp-contract=off), so tests/bake_sets.py restates it
// in numpy and tests/bake_rule_shim.cpp holds that restatement to this file.  There is no exp, pow or sqrt in it.
//
// Texel centres.  Texel (row, col) of a W x H map, row 0 the top, has the centre
//     q.x = ((float)col + 0.5f) / (float)W
//     q.y = 1.0f - ((float)row + 0.5f) / (float)H
//   the convention of BitmapTexture::getColor (Texture.cpp:62-72: x = (int)(uv.x * W), y = (int)((1 - uv.y) * H)): a baked map read back
//   as a bitmap texture lands on the texel that was baked.
// Coverage.  a, b, c are the x and y of the three vertex_uvs of a triangle, finite(x) is (x - x) == 0.0f:
//     A = (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x)
//     the triangle covers nothing unless finite(A) and A != 0
//     box: umin, umax, vmin, vmax the smallest and largest of the three x and of the three y
//         f0 = umin * (float)W; f1 = umax * (float)W; g0 = (1.0f - vmax) * (float)H; g1 = (1.0f - vmin) * (float)H
//         each clamped: f < 0 ? 0 : (f > (float)W ? (float)W : f), with (float)H for g
//         col0 = max((int)f0 - 1, 0); col1 = min((int)f1 + 1, W - 1); row0 = max((int)g0 - 1, 0); row1 = min((int)g1 + 1, H - 1)
//     only texels with col0 <= col <= col1 and row0 <= row <= row1 are considered: integer comparison, before any address is formed
//     e1 = (q.x - a.x) * (c.y - a.y) - (q.y - a.y) * (c.x - a.x)
//     e2 = (b.x - a.x) * (q.y - a.y) - (b.y - a.y) * (q.x - a.x)
//     e0 = (b.x - q.x) * (c.y - q.y) - (b.y - q.y) * (c.x - q.x)
//     covered: A > 0 ? (e0 >= 0 && e1 >= 0 && e2 >= 0) : (e0 <= 0 && e1 <= 0 && e2 <= 0)
//   The test is inclusive, so both triangles at a shared edge cover the texels on it; a NaN covers nothing.
// Ownership.  A texel's owner is the covering triangle of the mesh with the LOWEST global triangle index; no covering triangle: EMPTY.
// Record.  With the owner's crt_triangle (v0, v1, v2, the unit face normal nx, ny, nz):
//     u = e1 / A; v = e2 / A
//     w = (1.0f - u) - v
//     point.k = (v0.k * w + v1.k * u) + v2.k * v, k = 0..2
//     normal = (nx, ny, nz)
//   u is the weight of vertex 1 and v the weight of vertex 2, the (u, v) of crt_hit and of Texture::getColor.
// Probe ray.  origin.k = point.k + normal.k * probe_offset; direction.k = -normal.k; the ray type is CRT_RAY_REFLECTION, so back faces
//   are not culled.  A texel's colour is DEFINED as what shootRay returns for that ray.
// Keys in the GI mode.  Sample s of texel p = row * W + col has the key crt_gi_mix(crt_gi_mix(gi_seed, p), s); every sample of a texel
//   uses the same probe ray.  The fold: sum = (s == 0 ? 0 : sum) + c_s; mean = sum * (1.0f / (float)(s + 1)).
// Dilation.  A pass reads the statuses and colours as they are at the START of the pass.  A texel with status EMPTY takes the colour of
//   the first of its neighbours, in the order (row - 1, col) (row + 1, col) (row, col - 1) (row, col + 1) (row - 1, col - 1)
//   (row - 1, col + 1) (row + 1, col - 1) (row + 1, col + 1), whose status is not EMPTY, and becomes DILATED; every other texel keeps
//   what it has.  A pass copies and does no arithmetic; neighbours outside the map are skipped by integer comparison.  After max(W, H)
//   passes nothing can change any more, so no more than that are run.
//
// Known limits.
//   * There is no jitter inside a texel: every sample of a texel goes through its centre.
//   * Overlapping UV charts resolve to the lowest triangle index.
//   * A probe can meet another surface lying within probe_offset in front of the texel.
//   * Mirrors and glass are baked as seen along the normal.
//   * Multi-device contexts are not supported.
#pragma once

#include "filter_rule.h"
#include "gi_random.h"

#define CRT_BAKE_STATUS_EMPTY 0u
#define CRT_BAKE_STATUS_COVERED 1u
#define CRT_BAKE_STATUS_DILATED 2u
#define CRT_BAKE_NO_OWNER 0xFFFFFFFFu

// the x and y of a triangle's three vertex_uvs
struct crt_bake_uv {
    float ax, ay, bx, by, cx, cy;
};

// a triangle's clipped box of texels, both ends inclusive; col0 > col1: empty
struct crt_bake_box {
    int32_t col0, col1, row0, row1;
};

CRT_HD void crt_bake_centre(const int32_t width, const int32_t height, const int32_t row, const int32_t col, float *qx, float *qy) {
    const float cx = (float)col + 0.5f, cy = (float)row + 0.5f;
    const float x = cx / (float)width, y = cy / (float)height;
    *qx = x;
    *qy = 1.0f - y;
}

CRT_HD float crt_bake_area(const crt_bake_uv t) {
    const float e1x = t.bx - t.ax, e1y = t.by - t.ay, e2x = t.cx - t.ax, e2y = t.cy - t.ay;
    const float p = e1x * e2y, q = e1y * e2x;
    return p - q;
}

CRT_HD bool crt_bake_area_usable(const float area) { return crt_finite(area) && area != 0.0f; }

CRT_HD float crt_bake_clamp(const float f, const float hi) { return f < 0.0f ? 0.0f : (f > hi ? hi : f); }

// the box of a triangle whose area is usable (every coordinate is then finite); width * height < 2^31
CRT_HD crt_bake_box crt_bake_box_of(const crt_bake_uv t, const int32_t width, const int32_t height) {
    float umin = t.ax < t.bx ? t.ax : t.bx, umax = t.ax > t.bx ? t.ax : t.bx;
    float vmin = t.ay < t.by ? t.ay : t.by, vmax = t.ay > t.by ? t.ay : t.by;
    umin = umin < t.cx ? umin : t.cx; umax = umax > t.cx ? umax : t.cx;
    vmin = vmin < t.cy ? vmin : t.cy; vmax = vmax > t.cy ? vmax : t.cy;
    const float fw = (float)width, fh = (float)height;
    const float tv0 = 1.0f - vmax, tv1 = 1.0f - vmin;
    const float f0 = crt_bake_clamp(umin * fw, fw), f1 = crt_bake_clamp(umax * fw, fw);
    const float g0 = crt_bake_clamp(tv0 * fh, fh), g1 = crt_bake_clamp(tv1 * fh, fh);
    const int64_t c0 = (int64_t)f0 - 1, c1 = (int64_t)f1 + 1, r0 = (int64_t)g0 - 1, r1 = (int64_t)g1 + 1;
    crt_bake_box b;
    b.col0 = (int32_t)(c0 < 0 ? 0 : c0);
    b.col1 = (int32_t)(c1 > (int64_t)width - 1 ? (int64_t)width - 1 : c1);
    b.row0 = (int32_t)(r0 < 0 ? 0 : r0);
    b.row1 = (int32_t)(r1 > (int64_t)height - 1 ? (int64_t)height - 1 : r1);
    return b;
}

// whether the triangle (its area usable) covers q, and the two edge functions the record is made of
CRT_HD bool crt_bake_covers(const crt_bake_uv t, const float area, const float qx, const float qy, float *e1, float *e2) {
    const float e1x = t.bx - t.ax, e1y = t.by - t.ay, e2x = t.cx - t.ax, e2y = t.cy - t.ay;
    const float dx = qx - t.ax, dy = qy - t.ay;
    const float p1 = dx * e2y, q1 = dy * e2x;
    const float f1 = p1 - q1;
    const float p2 = e1x * dy, q2 = e1y * dx;
    const float f2 = p2 - q2;
    const float bqx = t.bx - qx, bqy = t.by - qy, cqx = t.cx - qx, cqy = t.cy - qy;
    const float p0 = bqx * cqy, q0 = bqy * cqx;
    const float f0 = p0 - q0;
    *e1 = f1;
    *e2 = f2;
    return area > 0.0f ? (f0 >= 0.0f && f1 >= 0.0f && f2 >= 0.0f) : (f0 <= 0.0f && f1 <= 0.0f && f2 <= 0.0f);
}

// a covered texel's record: (u, v) and the point; v0, v1, v2 are the owner's corners
CRT_HD void crt_bake_record(const float area, const float e1, const float e2, const float v0[3], const float v1[3], const float v2[3], float *u,
                            float *v, float point[3]) {
    const float uu = e1 / area, vv = e2 / area;
    const float w1 = 1.0f - uu;
    const float w = w1 - vv;
    for (int k = 0; k < 3; k++) {
        const float a = v0[k] * w, b = v1[k] * uu, c = v2[k] * vv;
        const float ab = a + b;
        point[k] = ab + c;
    }
    *u = uu;
    *v = vv;
}

// the probe ray of a record
CRT_HD void crt_bake_probe(const float point[3], const float normal[3], const float probe_offset, float origin[3], float direction[3]) {
    for (int k = 0; k < 3; k++) {
        const float d = normal[k] * probe_offset;
        origin[k] = point[k] + d;
        direction[k] = -normal[k];
    }
}

// the key of sample s of texel p
CRT_HD uint32_t crt_bake_key(const uint32_t gi_seed, const uint32_t p, const uint32_t s) { return crt_gi_mix(crt_gi_mix(gi_seed, p), s); }

// one step of the fold for one channel: the new sum; *mean is the colour the sum stands for after sample s
CRT_HD float crt_bake_fold(const uint32_t s, const float sum, const float c, float *mean) {
    const float next = (s == 0u ? 0.0f : sum) + c;
    const float scale = 1.0f / (float)(s + 1u);
    *mean = next * scale;
    return next;
}

// Dilation, one texel of one pass: the row-major index of the texel whose colour (row, col) takes, or -1 when it keeps what it has.
// `status` is the map's status plane at the start of the pass.  A neighbour's coordinates are compared with the map as integers before
// its address is formed.
CRT_HD int64_t crt_bake_dilate_source(const int32_t width, const int32_t height, const int32_t row, const int32_t col, const uint8_t *status) {
    if (status[(int64_t)row * width + col] != CRT_BAKE_STATUS_EMPTY) return -1;
    const int32_t dr[8] = {-1, 1, 0, 0, -1, -1, 1, 1};
    const int32_t dc[8] = {0, 0, -1, 1, -1, 1, -1, 1};
    for (int k = 0; k < 8; k++) {
        const int32_t r = row + dr[k], c = col + dc[k];
        if (r < 0 || r >= height || c < 0 || c >= width) continue;
        const int64_t i = (int64_t)r * width + c;
        if (status[i] != CRT_BAKE_STATUS_EMPTY) return i;
    }
    return -1;
}

// passes that can still change a map
CRT_HD uint32_t crt_bake_dilate_passes(const uint32_t width, const uint32_t height, const uint32_t passes) {
    const uint32_t most = width > height ? width : height;
    return passes < most ? passes : most;
}
