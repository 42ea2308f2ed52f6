// The host build of csrc/probe_lit_rule.h behind one C entry point: tests/test_probe_lit_host.py compiles this with g++ -ffp-contract=off and
// holds the numpy restatement of the rule (tests/probe_lit_sets.py) to it.  With PROBE_LIT_RULE_MAIN it is a stand-alone program that runs
// the same entry point over seeded cases of its own, for a run under -fsanitize=address,undefined.
#include "../course-assignment-danielhalachev_amd/csrc/probe_lit_rule.h"

#include <cstdio>
#include <cstring>
#include <vector>

struct shim_probe {
    float coef[27];
    uint32_t rays, back, miss, state, pad;
};
static_assert(sizeof(shim_probe) == 128 && sizeof(crt_probe_grid) == 48 && sizeof(crt_probe_vis) == 20, "crt_probe, crt_probe_volume, crt_probe_visibility");

// The primitive for n records: points and normals 3 floats each, status a byte each, rgb 3 floats each in place; vis and depth (128 floats a
// probe) null: the plain lookup.  counts[0] += LIT, counts[1] += UNLIT.  Only records of status 1 (CRT_SHADE_DIFFUSE) change.
extern "C" void shim_lit_light(const crt_probe_grid *grid, const crt_probe_vis *vis, const shim_probe *probes, const float *depth, const float *points,
                               const float *normals, const uint8_t *status, uint64_t n, uint32_t samples, float *rgb, uint64_t *counts) {
    const uint64_t count = crt_probe_count(*grid);
    for (uint64_t i = 0; i < n; i++) {
        if (status[i] != 1u) continue;
        const float *x = points + 3 * i, *nn = normals + 3 * i;
        float lbar[3] = {0.0f, 0.0f, 0.0f};
        uint32_t used = 0u;
        if (crt_probe_point_finite(x, nn)) {
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
                        if (p >= count || probes[p].state != CRT_PROBE_STATE_VALID) continue;
                        float wv = wc;
                        if (vis) {
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
                                    const uint32_t at = t.k[a] < (uint32_t)CRT_PROBE_DEPTH_TEXELS ? t.k[a] : 0u;
                                    pairs[a][0] = depth[128 * p + 2 * at];
                                    pairs[a][1] = depth[128 * p + 2 * at + 1];
                                }
                                float m1, m2;
                                crt_probe_depth_blend(&t, pairs, &m1, &m2);
                                visible = crt_probe_vis_weight(*vis, dist, m1, m2);
                            }
                            wv = wc * visible;
                        }
                        crt_probe_sum_add(&s, wv, probes[p].coef);
                    }
            used = crt_probe_lit_resolve(&s, nn, lbar);
        }
        for (int ch = 0; ch < 3; ch++) rgb[3 * i + ch] = crt_probe_lit_combine(rgb[3 * i + ch], lbar[ch], samples);
        if (counts) counts[used ? 0 : 1]++;
    }
}

#ifdef PROBE_LIT_RULE_MAIN
static uint32_t g_state = 2463534242u;
static float draw() {   // [-1, 3)
    g_state = g_state * 1664525u + 1013904223u;
    return -1.0f + 4.0f * (float)(g_state >> 8) * 0x1p-24f;
}
int main() {
    const uint32_t dims[][3] = {{1, 1, 1}, {2, 2, 2}, {2, 3, 1}, {3, 2, 4}};
    const uint32_t samples[] = {0, 1, 2, 7};
    for (const auto &dim : dims)
        for (const uint32_t S : samples)
            for (int visible = 0; visible < 2; visible++) {
                crt_probe_grid g{{-1.0f, 0.5f, -4.0f}, {0.75f, 1.25f, 0.5f}, {dim[0], dim[1], dim[2]}, 64u, 7u, 1.0f};
                crt_probe_vis vis;
                crt_probe_vis_defaults(g, &vis);
                const uint32_t count = crt_probe_count(g);
                std::vector<shim_probe> probes(count);
                std::vector<float> depth(128 * (size_t)count);
                for (uint32_t p = 0; p < count; p++) {
                    for (int k = 0; k < 27; k++) probes[p].coef[k] = draw();
                    probes[p].rays = 64; probes[p].back = probes[p].miss = probes[p].pad = 0;
                    probes[p].state = (p % 5u == 3u) ? CRT_PROBE_STATE_INVALID : CRT_PROBE_STATE_VALID;
                    for (int k = 0; k < 64; k++) {
                        const float m = 0.5f + 0.25f * draw();
                        depth[128 * p + 2 * k] = m;
                        depth[128 * p + 2 * k + 1] = m * m + 0.01f;
                    }
                }
                const size_t n = 257;
                std::vector<float> x(3 * n), nn(3 * n), rgb(3 * n);
                std::vector<uint8_t> status(n);
                for (size_t i = 0; i < 3 * n; i++) { x[i] = 2.0f * draw() - 3.0f; nn[i] = draw(); rgb[i] = draw(); }
                for (size_t i = 0; i < n; i++) status[i] = (uint8_t)((g_state = g_state * 1664525u + 1013904223u) >> 30);
                status[0] = status[1] = status[2] = status[3] = status[4] = status[5] = status[6] = 1;
                x[0] = NAN; x[4] = INFINITY; nn[8] = -INFINITY; x[9] = 3e38f; x[13] = -3e38f; nn[15] = 3e38f; nn[19] = 0.0f; nn[20] = 0.0f; nn[18] = 0.0f;
                uint64_t counts[2] = {0, 0};
                shim_lit_light(&g, visible ? &vis : nullptr, probes.data(), visible ? depth.data() : nullptr, x.data(), nn.data(), status.data(), n, S,
                               rgb.data(), counts);
                printf("%u x %u x %u, S = %u, %s: %llu lit, %llu unlit\n", dim[0], dim[1], dim[2], S, visible ? "visible" : "plain",
                       (unsigned long long)counts[0], (unsigned long long)counts[1]);
            }
    return 0;
}
#endif
