// kernel_probe_depth.h -- the kernels of the probe volume's visibility term (include/crt_hip.h: crt_probe_depth_device,
// crt_probe_irradiance_visible_device, crt_bake_probes_visible); the rule, one header for host and device: csrc/probe_depth_rule.h.
//   probe_depth            ONE WAVE per probe, lane k = texel k of its 8 x 8 map.  The rays are consumed 64 at a time: lane l loads the
//                          direction of ray base + l and the (t, hit) of its crt_hit and makes its distance r -- consecutive lanes,
//                          consecutive records --, then every lane walks the staged rays j = 0, 1, ... of the chunk in order, each read from
//                          lane j with a wave-uniform index (v_readlane: four a ray), so a lane's folds see j increasing.  The last chunk is
//                          partial when R % 64 != 0; what its idle lanes hold is never read.  Lane k stores its pair as one 8-byte store: a
//                          record is one 512-byte coalesced store per wave.  Two runs give the same bytes: nothing depends on arrival.
//   probe_lookup_visible   one thread per point, probe_lookup's structure.  A corner's state word is read first; the other 112 bytes of the
//                          SH record and the four 8-byte depth taps only for a VALID corner of weight != 0.  Every corner index is compared
//                          with the probe count, and every texel index with 64, as an integer before an address is formed.
// As in kernel_probes.h: these kernels and nothing else are enqueued (no memset or copy node between them), 64-bit indices are formed from
// unmasked 32-bit values, all stores are plain vector stores, no LDS.
#pragma once

#include "probe_depth_rule.h"

struct ProbeDepthArgs {
    const crt_ray *rays;         // count * rays entries
    const crt_hit *hits;         // one a ray
    uint32_t count, rays_per_probe;
    float max_distance;
    float2 *depth;               // 64 pairs a probe
};
__global__ __launch_bounds__(BLOCK) void probe_depth(const ProbeDepthArgs P) {
    const uint64_t p = (uint64_t)blockIdx.x * PROBE_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (p >= P.count) return;    // (wave-uniform: every lane of a wave meets every cross-lane read)
    const uint32_t R = P.rays_per_probe;
    float e[3];
    crt_probe_depth_direction(lane, e);
    crt_probe_depth_sum s;
    crt_probe_depth_reset(&s);
    for (uint32_t base = 0; base < R; base += 64u) {
        const uint32_t j = base + lane;
        float dx = 0.0f, dy = 0.0f, dz = 0.0f, r = 0.0f;
        if (j < R) {
            const uint64_t i = p * R + j;
            const crt_ray ray = P.rays[i];
            const crt_hit *h = P.hits + i;
            dx = ray.direction[0]; dy = ray.direction[1]; dz = ray.direction[2];
            r = crt_probe_depth_distance(h->hit, h->t, P.max_distance);
        }
        const uint32_t live = R - base < 64u ? R - base : 64u;   // (wave-uniform)
        for (uint32_t l = 0; l < live; l++) {
            const float d[3] = {__int_as_float(__builtin_amdgcn_readlane(__float_as_int(dx), (int)l)),
                                __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dy), (int)l)),
                                __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dz), (int)l))};
            const float rl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r), (int)l));
            crt_probe_depth_add(&s, e, d, rl);
        }
    }
    float pair[2];
    crt_probe_depth_pair(&s, P.max_distance, pair);
    P.depth[p * CRT_PROBE_DEPTH_TEXELS + lane] = make_float2(pair[0], pair[1]);
}

struct ProbeLookupVisibleArgs {
    crt_probe_grid grid;
    crt_probe_vis vis;
    const float4 *probes;        // 8 x float4 per record, the grid's probes
    const float2 *depth;         // 64 pairs per probe
    const float *points, *normals;   // 3 floats per point
    uint64_t n;
    float *rgb;                  // 3 floats per point
    uint8_t *status;             // or null
};
__global__ __launch_bounds__(BLOCK) void probe_lookup_visible(const ProbeLookupVisibleArgs P) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const float *xp = P.points + 3 * i, *np = P.normals + 3 * i;
    const float x[3] = {xp[0], xp[1], xp[2]}, n[3] = {np[0], np[1], np[2]};
    float out[3] = {0.0f, 0.0f, 0.0f};
    uint32_t status = 0u;
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
                    float coef[28];
#pragma unroll
                    for (int k = 0; k < 7; k++) {
                        const float4 c = rec[k];
                        coef[4 * k] = c.x; coef[4 * k + 1] = c.y; coef[4 * k + 2] = c.z; coef[4 * k + 3] = c.w;
                    }
                    const float wv = wc * vis;
                    crt_probe_sum_add(&s, wv, coef);
                }
        status = crt_probe_resolve(&s, n, out);
    }
    float *o = P.rgb + 3 * i;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
    if (P.status) P.status[i] = (uint8_t)status;
}
