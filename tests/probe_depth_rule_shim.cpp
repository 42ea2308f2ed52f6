// The host build of csrc/probe_depth_rule.h behind C entry points: tests/test_probe_depth_host.py compiles this with g++ -ffp-contract=off and
// holds the numpy restatement of the rule (tests/probe_depth_sets.py) to it.  With PROBE_DEPTH_RULE_MAIN it is a stand-alone program that
// runs the same entry points over seeded cases of its own, for a run under -fsanitize=address,undefined.
#include "../course-assignment-danielhalachev_amd/csrc/probe_depth_rule.h"

#include <cstdio>
#include <cstring>
#include <vector>

struct shim_probe {
    float coef[27];
    uint32_t rays, back, miss, state, pad;
};
static_assert(sizeof(shim_probe) == 128 && sizeof(crt_probe_grid) == 48 && sizeof(crt_probe_vis) == 20, "crt_probe, crt_probe_volume, crt_probe_visibility");

extern "C" void shim_depth_directions(float *out) {   // 64 x 3
    for (uint32_t k = 0; k < CRT_PROBE_DEPTH_TEXELS; k++) crt_probe_depth_direction(k, out + 3 * k);
}

extern "C" void shim_depth_defaults(const crt_probe_grid *grid, crt_probe_vis *out) { crt_probe_vis_defaults(*grid, out); }
extern "C" int shim_depth_vis_valid(const crt_probe_vis *p) { return crt_probe_vis_valid(*p) ? 1 : 0; }

// rays: 6 floats each; hit: a word a ray; t: a float a ray; depth: 128 floats a probe
extern "C" void shim_depth_project(const float *rays, const uint32_t *hit, const float *t, uint32_t count, uint32_t R, float max_distance, float *depth) {
    for (uint32_t p = 0; p < count; p++)
        for (uint32_t k = 0; k < CRT_PROBE_DEPTH_TEXELS; k++) {
            float e[3];
            crt_probe_depth_direction(k, e);
            crt_probe_depth_sum s;
            crt_probe_depth_reset(&s);
            for (uint32_t j = 0; j < R; j++) {
                const uint64_t i = (uint64_t)p * R + j;
                crt_probe_depth_add(&s, e, rays + 6 * i + 3, crt_probe_depth_distance(hit[i], t[i], max_distance));
            }
            crt_probe_depth_pair(&s, max_distance, depth + 128 * (uint64_t)p + 2 * k);
        }
}

// the four texels and weights of n directions, and the blended moments in one map (128 floats)
extern "C" void shim_depth_tap(const float *u, uint64_t n, const float *map, uint32_t *k, float *w, float *m) {
    for (uint64_t i = 0; i < n; i++) {
        crt_probe_depth_taps t;
        crt_probe_depth_tap(u + 3 * i, &t);
        float pairs[4][2];
        for (int a = 0; a < 4; a++) {
            k[4 * i + a] = t.k[a];
            w[4 * i + a] = t.w[a];
            const uint32_t at = t.k[a] < CRT_PROBE_DEPTH_TEXELS ? t.k[a] : 0u;
            pairs[a][0] = map[2 * at];
            pairs[a][1] = map[2 * at + 1];
        }
        crt_probe_depth_blend(&t, pairs, m + 2 * i, m + 2 * i + 1);
    }
}

extern "C" void shim_depth_lookup(const crt_probe_grid *grid, const crt_probe_vis *vis, const shim_probe *probes, const float *depth, const float *points,
                                  const float *normals, uint64_t n, float *rgb, uint8_t *status) {
    const uint64_t total = (uint64_t)grid->n[0] * grid->n[1] * grid->n[2];
    for (uint64_t i = 0; i < n; i++) {
        const float *x = points + 3 * i, *nn = normals + 3 * i;
        float *out = rgb + 3 * i;
        out[0] = out[1] = out[2] = 0.0f;
        status[i] = 0;
        if (!crt_probe_point_finite(x, nn)) continue;
        uint32_t i0[3], cnt[3];
        float w[3][2];
        for (int k = 0; k < 3; k++) crt_probe_axis(x[k], grid->origin[k], grid->spacing[k], grid->n[k], &i0[k], w[k], &cnt[k]);
        crt_probe_sum s;
        crt_probe_sum_reset(&s);
        for (uint32_t dz = 0; dz < cnt[2]; dz++)
            for (uint32_t dy = 0; dy < cnt[1]; dy++)
                for (uint32_t dx = 0; dx < cnt[0]; dx++) {
                    const float wxy = w[0][dx] * w[1][dy];
                    const float wc = wxy * w[2][dz];
                    if (wc == 0.0f) continue;
                    const uint64_t p = ((uint64_t)(i0[2] + dz) * grid->n[1] + (i0[1] + dy)) * grid->n[0] + (i0[0] + dx);
                    if (p >= total || probes[p].state != CRT_PROBE_STATE_VALID) continue;
                    float pos[3], v[3];
                    crt_probe_position(*grid, (uint32_t)p, pos);
                    const float dist = crt_probe_vis_offset(*vis, x, nn, pos, v);
                    float visible = 1.0f;
                    if (dist > 0.0f) {
                        const float u[3] = {v[0] / dist, v[1] / dist, v[2] / dist};
                        crt_probe_depth_taps t;
                        crt_probe_depth_tap(u, &t);
                        float pairs[4][2];
                        for (int a = 0; a < 4; a++) {
                            const uint32_t at = t.k[a] < CRT_PROBE_DEPTH_TEXELS ? t.k[a] : 0u;
                            pairs[a][0] = depth[128 * p + 2 * at];
                            pairs[a][1] = depth[128 * p + 2 * at + 1];
                        }
                        float m1, m2;
                        crt_probe_depth_blend(&t, pairs, &m1, &m2);
                        visible = crt_probe_vis_weight(*vis, dist, m1, m2);
                    }
                    const float wv = wc * visible;
                    crt_probe_sum_add(&s, wv, probes[p].coef);
                }
        status[i] = (uint8_t)crt_probe_resolve(&s, nn, out);
    }
}

#ifdef PROBE_DEPTH_RULE_MAIN
static uint32_t g_state = 2463534242u;
static float draw() {   // [-1, 3)
    g_state = g_state * 1664525u + 1013904223u;
    return -1.0f + 4.0f * (float)(g_state >> 8) * 0x1p-24f;
}
int main() {
    const uint32_t ray_counts[] = {1, 63, 64, 65, 100, 256};
    const uint32_t dims[][3] = {{1, 1, 1}, {2, 3, 1}, {3, 2, 4}};
    for (const uint32_t R : ray_counts)
        for (const auto &dim : dims) {
            crt_probe_grid g{{-1.0f, 0.5f, -4.0f}, {0.75f, 1.25f, 0.5f}, {dim[0], dim[1], dim[2]}, R, 7u, 1.0f};
            crt_probe_vis vis;
            shim_depth_defaults(&g, &vis);
            if (!shim_depth_vis_valid(&vis)) return 1;
            const uint32_t count = crt_probe_count(g);
            const size_t n = (size_t)count * R;
            std::vector<float> rays(6 * n), t(n), depth(128 * (size_t)count);
            std::vector<uint32_t> hit(n);
            std::vector<shim_probe> probes(count);
            for (uint32_t p = 0; p < count; p++) {
                for (int k = 0; k < 27; k++) probes[p].coef[k] = draw();
                probes[p].rays = R; probes[p].back = probes[p].miss = probes[p].pad = 0;
                probes[p].state = (p % 5u == 3u) ? CRT_PROBE_STATE_INVALID : CRT_PROBE_STATE_VALID;
                for (uint32_t j = 0; j < R; j++) {
                    const size_t i = (size_t)p * R + j;
                    crt_probe_position(g, p, rays.data() + 6 * i);
                    crt_probe_direction(j, R, rays.data() + 6 * i + 3);
                    t[i] = draw();
                    hit[i] = (g_state >> 5) & 1u;
                }
            }
            if (n > 4) { t[0] = NAN; t[1] = INFINITY; t[2] = -0.0f; t[3] = 1e-42f; rays[3] = NAN; }
            shim_depth_project(rays.data(), hit.data(), t.data(), count, R, vis.max_distance, depth.data());
            const size_t points = 257;
            std::vector<float> x(3 * points), nn(3 * points), out(3 * points), m(2 * points), w(4 * points);
            std::vector<uint32_t> k(4 * points);
            std::vector<uint8_t> status(points);
            for (size_t i = 0; i < 3 * points; i++) { x[i] = 2.0f * draw() - 3.0f; nn[i] = draw(); }
            x[0] = NAN; x[4] = INFINITY; nn[8] = -INFINITY; x[9] = 3e38f; x[13] = -3e38f; nn[15] = 3e38f; nn[19] = 0.0f; nn[20] = 0.0f; nn[18] = 0.0f;
            shim_depth_tap(nn.data(), points, depth.data(), k.data(), w.data(), m.data());
            for (size_t i = 0; i < 4 * points; i++)
                if (k[i] >= CRT_PROBE_DEPTH_TEXELS) return 2;
            shim_depth_lookup(&g, &vis, probes.data(), depth.data(), x.data(), nn.data(), points, out.data(), status.data());
            unsigned lit = 0;
            for (size_t i = 0; i < points; i++) lit += status[i] != 0;
            printf("%u rays, %u x %u x %u: %u of %zu points lit\n", R, dim[0], dim[1], dim[2], lit, points);
        }
    return 0;
}
#endif
