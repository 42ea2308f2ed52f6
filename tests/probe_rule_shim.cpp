// The host build of csrc/probe_rule.h behind C entry points: tests/test_probes_host.py compiles this with g++ -ffp-contract=off and holds the
// numpy restatement of the rule (tests/probe_sets.py) to it.  With PROBE_RULE_MAIN it is a stand-alone program that runs the same entry
// points over seeded cases of its own, for a run under -fsanitize=address,undefined.
#include "../course-assignment-danielhalachev_amd/csrc/probe_rule.h"

#include <cstdio>
#include <cstring>
#include <vector>

struct shim_probe {
    float coef[27];
    uint32_t rays, back, miss, state, pad;
};
static_assert(sizeof(shim_probe) == 128 && sizeof(crt_probe_grid) == 48, "crt_probe's 128 and crt_probe_volume's 48 bytes");

// rays: 6 floats each, keys: may be null
extern "C" void shim_probe_rays(const crt_probe_grid *grid, uint32_t first, uint32_t count, float *rays, uint32_t *keys) {
    for (uint32_t q = 0; q < count; q++)
        for (uint32_t j = 0; j < grid->rays; j++) {
            const uint64_t i = (uint64_t)q * grid->rays + j;
            crt_probe_position(*grid, first + q, rays + 6 * i);
            crt_probe_direction(j, grid->rays, rays + 6 * i + 3);
            if (keys) keys[i] = crt_probe_key(grid->gi_seed, first + q, j);
        }
}

extern "C" void shim_probe_basis(const float *d, uint64_t n, float *out) {
    for (uint64_t i = 0; i < n; i++) crt_probe_basis(d + 3 * i, out + 9 * i);
}

// the projection as 64 lanes do it
extern "C" void shim_probe_project(const float *rays, const float *rgb, uint32_t count, uint32_t R, shim_probe *out) {
    for (uint32_t p = 0; p < count; p++) {
        float part[64][CRT_PROBE_COEFS];
        for (uint32_t l = 0; l < 64; l++) {
            for (int k = 0; k < CRT_PROBE_COEFS; k++) part[l][k] = 0.0f;
            for (uint32_t j = l; j < R; j += 64) {
                const uint64_t i = (uint64_t)p * R + j;
                crt_probe_accumulate(rgb + 3 * i, rays + 6 * i + 3, part[l]);
            }
        }
        for (uint32_t step = 32; step >= 1; step >>= 1)
            for (uint32_t l = 0; l < step; l++)
                for (int k = 0; k < CRT_PROBE_COEFS; k++) part[l][k] = part[l][k] + part[l + step][k];
        const float scale = crt_probe_scale(R);
        shim_probe rec;
        memset(&rec, 0, sizeof(rec));
        for (int k = 0; k < CRT_PROBE_COEFS; k++) rec.coef[k] = part[0][k] * scale;
        rec.rays = R;
        rec.state = CRT_PROBE_STATE_VALID;
        out[p] = rec;
    }
}

// hit: a byte a ray, normals: 3 floats a ray
extern "C" void shim_probe_validity(const float *rays, const uint8_t *hit, const float *normals, uint32_t count, uint32_t R, float limit, shim_probe *probes) {
    for (uint32_t p = 0; p < count; p++) {
        uint32_t back = 0, miss = 0;
        for (uint32_t j = 0; j < R; j++) {
            const uint64_t i = (uint64_t)p * R + j;
            if (!hit[i]) miss++;
            else if (crt_probe_backfacing(normals + 3 * i, rays + 6 * i + 3)) back++;
        }
        probes[p].back = back;
        probes[p].miss = miss;
        probes[p].state = crt_probe_state_of(back, R, limit);
        probes[p].pad = 0;
    }
}

extern "C" void shim_probe_lookup(const crt_probe_grid *grid, const shim_probe *probes, const float *points, const float *normals, uint64_t n, float *rgb,
                                  uint8_t *status) {
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
                    crt_probe_sum_add(&s, wc, probes[p].coef);
                }
        status[i] = (uint8_t)crt_probe_resolve(&s, nn, out);
    }
}

extern "C" int shim_probe_grid_valid(const crt_probe_grid *grid) { return crt_probe_grid_valid(*grid) ? 1 : 0; }

#ifdef PROBE_RULE_MAIN
static uint32_t g_state = 12345u;
static float draw() {   // [-1, 3)
    g_state = g_state * 1664525u + 1013904223u;
    return -1.0f + 4.0f * (float)(g_state >> 8) * 0x1p-24f;
}
int main() {
    const uint32_t ray_counts[] = {1, 63, 64, 65, 100, 256, 4096};
    const uint32_t dims[][3] = {{1, 1, 1}, {2, 3, 1}, {3, 2, 4}};
    for (const uint32_t R : ray_counts)
        for (const auto &dim : dims) {
            crt_probe_grid g{{-1.0f, 0.5f, -4.0f}, {0.75f, 1.25f, 0.5f}, {dim[0], dim[1], dim[2]}, R, 7u, 0.25f};
            if (!shim_probe_grid_valid(&g)) return 1;
            const uint32_t count = crt_probe_count(g);
            const size_t n = (size_t)count * R;
            std::vector<float> rays(6 * n), rgb(3 * n), normals(3 * n);
            std::vector<uint32_t> keys(n);
            std::vector<uint8_t> hit(n);
            std::vector<shim_probe> probes(count);
            shim_probe_rays(&g, 0, count, rays.data(), keys.data());
            for (size_t i = 0; i < 3 * n; i++) { rgb[i] = draw(); normals[i] = draw(); }
            for (size_t i = 0; i < n; i++) hit[i] = (keys[i] & 3u) != 0u;
            if (n > 9) { rgb[2] = -0.0f; rgb[5] = INFINITY; rgb[8] = NAN; }
            shim_probe_project(rays.data(), rgb.data(), count, R, probes.data());
            shim_probe_validity(rays.data(), hit.data(), normals.data(), count, R, g.backface_limit, probes.data());
            const size_t points = 257;
            std::vector<float> x(3 * points), nn(3 * points), out(3 * points);
            std::vector<uint8_t> status(points);
            for (size_t i = 0; i < 3 * points; i++) { x[i] = 2.0f * draw() - 3.0f; nn[i] = draw(); }
            x[0] = NAN; x[4] = INFINITY; nn[8] = -INFINITY; x[9] = 3e38f; x[13] = -3e38f;
            shim_probe_lookup(&g, probes.data(), x.data(), nn.data(), points, out.data(), status.data());
            unsigned lit = 0, invalid = 0;
            for (size_t i = 0; i < points; i++) lit += status[i] != 0;
            for (uint32_t p = 0; p < count; p++) invalid += probes[p].state != CRT_PROBE_STATE_VALID;
            printf("%u rays, %u x %u x %u: %u invalid probes, %u of %zu points lit\n", R, dim[0], dim[1], dim[2], invalid, lit, points);
        }
    return 0;
}
#endif
