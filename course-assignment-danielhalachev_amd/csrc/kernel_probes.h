// kernel_probes.h -- the kernels of the irradiance probe volume (include/crt_hip.h: crt_probe_rays_device, crt_probe_project_device,
// crt_probe_validity_device, crt_probe_irradiance_device, crt_bake_probes); the rule, one header for host and device: csrc/probe_rule.h.
//   probe_rays      one thread per ray of the probes [first, first + count): position, direction j of the set, the GI key.  A ray is 24
//                   bytes, so ray i lies at a multiple of 16 bytes when i is even and 8 bytes behind one when i is odd: it is written as a
//                   16-byte and an 8-byte store, in the order its parity asks for.  The direction is recomputed by every thread (its sine
//                   and cosine run in binary64: csrc/glibc_sincosf.h); a 16^3 volume at 256 rays is a million of them.
//   probe_project   ONE WAVE per probe.  Lane l keeps the 27 partial sums of rays l, l + 64, ... in registers -- the direction is READ from
//                   the ray array --, then six cross-lane steps per value in the rule's order (__shfl_down by 32, 16, 8, 4, 2, 1: lane l
//                   adds lane l + step's value to its own; what lanes >= step hold afterwards is never read by a lane below step), and lane 0
//                   writes the 128-byte record as eight 16-byte stores.  Two runs give the same bytes: nothing depends on arrival.
//   probe_validity  ONE WAVE per probe: a ballot and a popcount over the crt_hit records of its rays, 64 at a time; lane 0 writes back,
//                   miss, state and the pad word as the record's last 16-byte store.
//   probe_lookup    one thread per point.  A corner's record is one 128-byte line out of L2: its last 16 bytes (back, miss, state, pad)
//                   are read first, and the other 112 bytes -- seven 16-byte loads -- only for a VALID corner of weight != 0.  Every
//                   corner index is compared with the probe count as an integer before its address is formed.
//   probe_count_invalid   crt_bake_probes' statistic: one atomicAdd per wave on a word nobody orders by.
// The primitives enqueue these kernels and nothing else (no memset or copy node between them: DESIGN.md section 8f), so a captured chain
// replays in order.  64-bit indices are formed from unmasked 32-bit values (kernel_progressive.h says why).  All stores are plain vector
// stores.  No LDS.
#pragma once

#include "probe_rule.h"

constexpr uint32_t PROBE_WAVES = BLOCK / 64;
static_assert(BLOCK % 64 == 0 && PROBE_WAVES >= 1, "a workgroup is whole waves");

struct ProbeRaysArgs {
    crt_probe_grid grid;
    uint32_t first, count;       // first + count <= the grid's probes
    crt_ray *rays;               // count * rays entries, aligned to 16 bytes
    uint32_t *keys;              // or null
};
__global__ __launch_bounds__(BLOCK) void probe_rays(const ProbeRaysArgs P) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t R = P.grid.rays;
    if (i >= (uint64_t)P.count * R) return;
    const uint32_t q = (uint32_t)(i / R);            // (count * rays < 2^36; q < count)
    const uint32_t j = (uint32_t)(i - (uint64_t)q * R);
    const uint32_t p = P.first + q;
    float o[3], d[3];
    crt_probe_position(P.grid, p, o);
    crt_probe_direction(j, R, d);
    char *at = reinterpret_cast<char *>(P.rays) + 24u * i;
    if ((i & 1u) == 0u) {
        *reinterpret_cast<float4 *>(at) = make_float4(o[0], o[1], o[2], d[0]);
        *reinterpret_cast<float2 *>(at + 16) = make_float2(d[1], d[2]);
    } else {
        *reinterpret_cast<float2 *>(at) = make_float2(o[0], o[1]);
        *reinterpret_cast<float4 *>(at + 8) = make_float4(o[2], d[0], d[1], d[2]);
    }
    if (P.keys) P.keys[i] = crt_probe_key(P.grid.gi_seed, p, j);
}

struct ProbeProjectArgs {
    const crt_ray *rays;         // count * rays entries
    const float *rgb;            // 3 floats per ray
    uint32_t count, rays_per_probe;
    float4 *probes;              // 8 x float4 per record
};
__global__ __launch_bounds__(BLOCK) void probe_project(const ProbeProjectArgs P) {
    const uint64_t p = (uint64_t)blockIdx.x * PROBE_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (p >= P.count) return;    // (wave-uniform)
    const uint32_t R = P.rays_per_probe;
    float acc[CRT_PROBE_COEFS];
#pragma unroll
    for (int k = 0; k < CRT_PROBE_COEFS; k++) acc[k] = 0.0f;
    for (uint32_t j = lane; j < R; j += 64u) {
        const uint64_t i = p * R + j;
        const crt_ray ray = P.rays[i];
        const float *c = P.rgb + 3 * i;
        const float L[3] = {c[0], c[1], c[2]};
        crt_probe_accumulate(L, ray.direction, acc);
    }
#pragma unroll
    for (int k = 0; k < CRT_PROBE_COEFS; k++) {
        float v = acc[k];
#pragma unroll
        for (uint32_t step = 32u; step >= 1u; step >>= 1) {
            const float other = __shfl_down(v, step);
            v = v + other;
        }
        acc[k] = v;
    }
    if (lane != 0u) return;
    const float scale = crt_probe_scale(R);
#pragma unroll
    for (int k = 0; k < CRT_PROBE_COEFS; k++) acc[k] = acc[k] * scale;
    float4 *out = P.probes + 8 * p;
#pragma unroll
    for (int k = 0; k < 6; k++) out[k] = make_float4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
    out[6] = make_float4(acc[24], acc[25], acc[26], __uint_as_float(R));
    reinterpret_cast<uint4 *>(out)[7] = make_uint4(0u, 0u, CRT_PROBE_STATE_VALID, 0u);
}

struct ProbeValidityArgs {
    const crt_ray *rays;
    const crt_hit *hits;
    uint32_t count, rays_per_probe;
    float backface_limit;
    float4 *probes;
};
__global__ __launch_bounds__(BLOCK) void probe_validity(const ProbeValidityArgs P) {
    const uint64_t p = (uint64_t)blockIdx.x * PROBE_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (p >= P.count) return;    // (wave-uniform: every lane of a wave meets every ballot)
    const uint32_t R = P.rays_per_probe;
    uint32_t back = 0, miss = 0;
    for (uint32_t base = 0; base < R; base += 64u) {
        const uint32_t j = base + lane;
        bool is_back = false, is_miss = false;
        if (j < R) {
            const uint64_t i = p * R + j;
            const crt_hit h = P.hits[i];
            const crt_ray ray = P.rays[i];
            is_miss = h.hit == 0u;
            is_back = !is_miss && crt_probe_backfacing(h.normal, ray.direction);
        }
        back += (uint32_t)__popcll(__ballot(is_back));
        miss += (uint32_t)__popcll(__ballot(is_miss));
    }
    if (lane == 0u) reinterpret_cast<uint4 *>(P.probes + 8 * p)[7] = make_uint4(back, miss, crt_probe_state_of(back, R, P.backface_limit), 0u);
}

struct ProbeLookupArgs {
    crt_probe_grid grid;
    const float4 *probes;        // 8 x float4 per record, the grid's probes
    const float *points, *normals;   // 3 floats per point
    uint64_t n;
    float *rgb;                  // 3 floats per point
    uint8_t *status;             // or null
};
__global__ __launch_bounds__(BLOCK) void probe_lookup(const ProbeLookupArgs P) {
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
                    float coef[28];
#pragma unroll
                    for (int k = 0; k < 7; k++) {
                        const float4 v = rec[k];
                        coef[4 * k] = v.x; coef[4 * k + 1] = v.y; coef[4 * k + 2] = v.z; coef[4 * k + 3] = v.w;
                    }
                    crt_probe_sum_add(&s, wc, coef);
                }
        status = crt_probe_resolve(&s, n, out);
    }
    float *o = P.rgb + 3 * i;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
    if (P.status) P.status[i] = (uint8_t)status;
}

// *count += the probes p < n whose state is not VALID
__global__ __launch_bounds__(BLOCK) void probe_count_invalid(const float4 *probes, const uint64_t n, uint32_t *count) {
    const uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool invalid = p < n && reinterpret_cast<const uint4 *>(probes)[8 * p + 7].z != CRT_PROBE_STATE_VALID;
    const unsigned long long mask = __ballot(invalid);
    if ((threadIdx.x & 63u) == 0u && mask) atomicAdd(count, (uint32_t)__popcll(mask));
}
