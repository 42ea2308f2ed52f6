// kernel_probe_light.h -- the kernel of the probe-lit radiance queries (include/crt_hip.h: crt_probe_light_hits_device, crt_shoot_rays_lit*,
// crt_render_probe_lit); the rule, one header for host and device: csrc/probe_lit_rule.h.
//   probe_light_records<VISIBLE>   one lane per record of a level.  The lane loads the record's status byte first and does nothing more
//                          unless it is CRT_SHADE_DIFFUSE.  Then the point and the normal of the record's crt_hit -- the normal
//                          radiance_scatter<true> hands to gi_sample_direction --, and the cell's corners as probe_lookup (VISIBLE false) or
//                          probe_lookup_visible (true) walk them: a corner's state word is read first; the other 112 bytes of the SH record
//                          and, VISIBLE, the four 8-byte depth taps only for a VALID corner of weight != 0; every corner index is compared
//                          with the probe count, and every texel index with 64, as an integer before an address is formed.  The sums are
//                          resolved with the zonal table (crt_probe_lit_resolve), the record's colour is read from the level's colour
//                          array and the combined colour written over it.  Every lane stays to the end: two ballots count the wave's LIT
//                          and UNLIT records, and lane 0 adds each count that is not zero to its counter, words nobody orders by.
// As in kernel_probes.h: this kernel and nothing else is enqueued by the primitive, 64-bit indices are formed from unmasked 32-bit values,
// all stores are plain vector stores, no LDS, and no kernel waits for another.
#pragma once

#include "probe_lit_rule.h"

struct ProbeLightArgs {
    crt_probe_grid grid;
    crt_probe_vis vis;                   // VISIBLE alone
    const float4 *probes;                // 8 x float4 per record, the grid's probes
    const float2 *depth;                 // VISIBLE alone: 64 pairs per probe
    const crt_hit *hits;                 // the level's records
    const uint8_t *status;               // ... CRT_SHADE_* of each
    uint64_t n;
    uint32_t samples;                    // S
    float *rgb;                          // 3 floats a record: direct light in, the lit colour out
    unsigned long long *counts;          // or null: [0] += LIT records, [1] += UNLIT records
};
template <bool VISIBLE>
__global__ __launch_bounds__(BLOCK) void probe_light_records(const ProbeLightArgs P) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;   // (every lane stays to the end: the ballots are the wave's)
    const bool diffuse = i < P.n && P.status[i] == (uint8_t)CRT_SHADE_DIFFUSE;
    uint32_t used = 0u;
    if (diffuse) {
        const crt_hit *h = P.hits + i;
        const float x[3] = {h->point[0], h->point[1], h->point[2]}, n[3] = {h->normal[0], h->normal[1], h->normal[2]};
        float lbar[3] = {0.0f, 0.0f, 0.0f};
        if (crt_probe_point_finite(x, n)) {
            uint32_t i0[3], cnt[3];
            float w[3][2];
#pragma unroll
            for (int k = 0; k < 3; k++) crt_probe_axis(x[k], P.grid.origin[k], P.grid.spacing[k], P.grid.n[k], &i0[k], w[k], &cnt[k]);
            const uint64_t probes = (uint64_t)P.grid.n[0] * P.grid.n[1] * P.grid.n[2];
            crt_probe_sum s;
            crt_probe_sum_reset(&s);
            for (uint32_t dz = 0; dz < cnt[2]; dz++)
                for (uint32_t dy = 0; dy < cnt[1]; dy++)
                    for (uint32_t dx = 0; dx < cnt[0]; dx++) {
                        const float wxy = w[0][dx] * w[1][dy];
                        const float wc = wxy * w[2][dz];
                        if (wc == 0.0f) continue;
                        const uint64_t p = ((uint64_t)(i0[2] + dz) * P.grid.n[1] + (i0[1] + dy)) * P.grid.n[0] + (i0[0] + dx);
                        if (p >= probes) continue;   // (never true for a valid grid)
                        const float4 *rec = P.probes + 8 * p;
                        const uint4 tail = reinterpret_cast<const uint4 *>(rec)[7];
                        if (tail.z != CRT_PROBE_STATE_VALID) continue;
                        float wv = wc;
                        if constexpr (VISIBLE) {
                            float pos[3], v[3];
                            crt_probe_position(P.grid, (uint32_t)p, pos);
                            const float dist = crt_probe_vis_offset(P.vis, x, n, pos, v);
                            float vis = 1.0f;
                            if (dist > 0.0f) {
                                const float u[3] = {v[0] / dist, v[1] / dist, v[2] / dist};
                                crt_probe_depth_taps taps;
                                crt_probe_depth_tap(u, &taps);
                                const float2 *map = P.depth + p * CRT_PROBE_DEPTH_TEXELS;
                                float pairs[4][2];
#pragma unroll
                                for (int t = 0; t < 4; t++) {
                                    const uint32_t k = taps.k[t] < (uint32_t)CRT_PROBE_DEPTH_TEXELS ? taps.k[t] : 0u;   // (never the other for the rule's wrap)
                                    const float2 m = map[k];
                                    pairs[t][0] = m.x; pairs[t][1] = m.y;
                                }
                                float m1, m2;
                                crt_probe_depth_blend(&taps, pairs, &m1, &m2);
                                vis = crt_probe_vis_weight(P.vis, dist, m1, m2);
                            }
                            wv = wc * vis;
                        }
                        float coef[28];
#pragma unroll
                        for (int k = 0; k < 7; k++) {
                            const float4 c = rec[k];
                            coef[4 * k] = c.x; coef[4 * k + 1] = c.y; coef[4 * k + 2] = c.z; coef[4 * k + 3] = c.w;
                        }
                        crt_probe_sum_add(&s, wv, coef);
                    }
            used = crt_probe_lit_resolve(&s, n, lbar);
        }
        float *c = P.rgb + 3 * i;
        const float r = crt_probe_lit_combine(c[0], lbar[0], P.samples), g = crt_probe_lit_combine(c[1], lbar[1], P.samples),
                    b = crt_probe_lit_combine(c[2], lbar[2], P.samples);
        c[0] = r; c[1] = g; c[2] = b;
    }
    const unsigned long long lit = __ballot(diffuse && used != 0u), unlit = __ballot(diffuse && used == 0u);
    if (P.counts && (threadIdx.x & 63u) == 0u) {
        if (lit) atomicAdd(P.counts, (unsigned long long)__popcll(lit));
        if (unlit) atomicAdd(P.counts + 1, (unsigned long long)__popcll(unlit));
    }
}
