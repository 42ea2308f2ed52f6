// kernel_radiance.h -- radiance queries (crt_shoot_rays*): what RayTracer::shootRay (RayTracer.cpp:419-451, the non-GI build) returns
// for rays the CALLER supplies, level by level.  The walks and the direct lighting are the queries that exist (kernel_query.h:
// query_walk / query_reroute, kernel_shade.h: query_direct / query_direct_reroute); the three small kernels here are the recursion
// around them, and the host loop (crt_query.hip) runs them one level behind the other:
//
//   radiance_prepare   level 0 only: the caller's rays into the level's ray array, normalised as shootRay's entry does it;
//   (trace, direct light: the level's crt_hit, colour and status arrays; background, constant and diffuse records are final)
//   radiance_scatter   a lane per ray of the level; a record whose status is CRT_SHADE_RECURSES gets a node (TNode, kernel_stream.h: kind,
//                      albedo or Fresnel coefficient, two child indices) and its child rays in level g + 1's ray array;
//   radiance_combine   from the deepest level up: a lane per recursing record mixes its children's colours into its own.
//
// DEVN = true: the builds of crt_shoot_rays*_enqueue, whose host loop never learns a level's size.  The launch is sized for the level's
// CAPACITY (n, child_n) and the kernel reads how many rays the level holds from the word radiance_scatter counted them in, clamped to
// that capacity; radiance_report turns the words into the call's crt_shoot_report.  The other builds are what they were.
//
// Every level has arrays of its own (rays, records, colours, status, nodes): a parent holds its children's indices in the next level's
// arrays, so the ORDER in which a level's children are appended may differ between two runs and no colour does.  Nothing of a frame is
// used: no FrameArgs queue, no level queue, no ray tree of a pixel.
//
// GI = true: the builds of crt_shoot_rays_gi*, the reference's GI mode (RayTracer.cpp:331-354; oracle/cpu_ref.c: shoot_ray with use_gi)
// with the generator of gi_random.h.  Every ray of a level has a KEY beside it (the key of its shootRay invocation); a DIFFUSE record
// is a node too -- its gi_samples sample rays are gi_samples CONSECUTIVE rays of level g + 1, the first one's index in the node -- and
// the up-sweep folds it as stream_resolve does: (direct + (((0 + c_0) + c_1) + ...)) * (1 / (gi_samples + 1)).  The plain builds carry
// none of this (as kernel_stream.h's kernels do with their GI parameter).
#pragma once

#include "kernel_stream.h"
#include "kernel_shade.h"

struct RadianceArgs {
    const crt_ray *in_rays;             // radiance_prepare: the caller's rays
    crt_ray *rays;                      // this level's rays, directions as shootRay holds them (normalised on entry)
    const crt_hit *hits;                // ... their closest hits
    const uint8_t *status;              // ... CRT_SHADE_* of each
    float *rgb;                         // ... colours, 3 floats a ray (level 0: the caller's output)
    float4 *nodes;                      // ... nodes, 2 x float4 a ray; written and read for CRT_SHADE_RECURSES records only
    crt_ray *child_rays;                // level g + 1's ray array
    const float *child_rgb;             // level g + 1's colours (radiance_combine)
    uint32_t *child_count;              // rays appended to level g + 1
    unsigned long long *diffuse_total;  // CRT_SHADE_DIFFUSE records over all levels of the call
    uint32_t n;                         // rays of this level
    uint32_t child_cap;                 // records level g + 1's arrays hold (the host allocates 2 n before the launch: never reached)
    uint32_t child_n;                   // radiance_combine: rays of level g + 1
    uint32_t spawn;                     // g + 1 <= max_depth: children are traced (else CHILD_BG: background without tracing, RayTracer.cpp:427-429)
    float reflection_bias, refraction_bias;
    // the GI builds alone (crt_shoot_rays_gi*)
    const uint32_t *in_keys;            // radiance_prepare<true>: the caller's keys, or null: mix(mix(gi_seed, key_first + r), 0)
    uint32_t *keys;                     // this level's keys, one a ray
    uint32_t *child_keys;               // level g + 1's
    uint32_t gi_samples;                // GI_SAMPLE_SIZE
    uint32_t gi_seed, key_first;        // in_keys == null: the seed, and the index in the CALL of this pass's first ray
    float monte_carlo_bias;
    // the DEVN builds alone (crt_shoot_rays*_enqueue); null: n / child_n are the counts themselves (level 0's n is the caller's)
    const uint32_t *n_dev;              // rays appended to this level: it holds min(*n_dev, n)
    const uint32_t *child_n_dev;        // ... to level g + 1 (radiance_combine): it holds min(*child_n_dev, child_n)
};

// rays of a level whose capacity is `cap`: one load for the wave
template <bool DEVN>
__device__ __forceinline__ uint32_t radiance_count(const uint32_t *dev, const uint32_t cap) {
    if constexpr (DEVN) {
        if (dev) {
            const uint32_t have = (uint32_t)__builtin_amdgcn_readfirstlane(*dev);
            return have < cap ? have : cap;
        }
    }
    return cap;
}

// shootRay's entry (RayTracer.cpp:420) for the caller's rays: normalize3 leaves a zero direction as it is.  GI: and the rays' keys --
// the caller's, or those of a frame's pixels key_first + r, sample 0 (kernel_stream.h: level0_key).
template <bool GI>
__global__ __launch_bounds__(BLOCK) void radiance_prepare(const RadianceArgs G) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= G.n) return;
    crt_ray q = G.in_rays[r];
    normalize3(q.direction[0], q.direction[1], q.direction[2]);
    G.rays[r] = q;
    if constexpr (GI) G.keys[r] = G.in_keys ? G.in_keys[r] : crt_gi_mix(crt_gi_mix(G.gi_seed, G.key_first + (uint32_t)r), 0u);
}

// shootRay's dispatch for a mirror or glass hit (RayTracer.cpp:437-442) up to the recursive calls: the node and the child rays.  The
// arithmetic is shade_hit's (kernel_stream.h), in one body for both: mirror_glass_children (kernel_common.h).  A child is stored the
// way the next level walks it: normalised once more, which is the child's own shootRay entry (stream_trace_shade does that when it
// fetches a queued ray).  The children of a wave are appended with ONE atomic (kernel_query.h: query_append's pattern): the
// reflection rays of its lanes first, then the transmission rays, then -- GI -- gi_samples consecutive rays for each DIFFUSE lane.
// GI: a DIFFUSE record's sample rays (RayTracer.cpp:333-350; the expressions of shade_and_emit<.., true>, kernel_stream.h): sample i
// leaves point + normal * monte_carlo_bias in gi_sample_direction(incoming direction, normal, u(key, 2 + 2i), u(key, 3 + 2i)) with key
// child_key(key, 2 + i); the mirror and glass children get child_key(key, 0) and (key, 1).  The record's node holds the first sample's
// index (CHILD_BG: nothing is traced -- no samples, or they would enter shootRay beyond max_depth).
template <bool GI, bool DEVN = false>
__global__ __launch_bounds__(BLOCK) void radiance_scatter(const KernelArgs A, const RadianceArgs G) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;   // (every lane stays to the end: the ballots are the wave's)
    const uint32_t level_n = radiance_count<DEVN>(G.n_dev, G.n);
    const uint32_t status = r < level_n ? (uint32_t)G.status[r] : (uint32_t)CRT_SHADE_BACKGROUND;
    const unsigned long long diffuse = __ballot(r < level_n && status == (uint32_t)CRT_SHADE_DIFFUSE);
    if (lane == 0 && diffuse) atomicAdd(G.diffuse_total, (unsigned long long)__popcll(diffuse));
    const bool recurses = r < level_n && status == (uint32_t)CRT_SHADE_RECURSES;
    const bool gi_record = GI && r < level_n && status == (uint32_t)CRT_SHADE_DIFFUSE;
    const bool samples = gi_record && G.spawn != 0u && G.gi_samples > 0u;
    uint32_t key = 0;
    if constexpr (GI) if (recurses || samples) key = G.keys[r];
    TNode N;
    N.cx = N.cy = N.cz = 0; N.kind = TN_CONST; N.a = 0; N.b = 0; N.f = 0; N.pad = 0;
    bool reflect = false, transmit = false;
    float rox = 0, roy = 0, roz = 0, rdx = 0, rdy = 0, rdz = 0, tox = 0, toy = 0, toz = 0, tdx = 0, tdy = 0, tdz = 0;
    if (recurses) {
        const crt_ray q = G.rays[r];
        const crt_hit h = G.hits[r];
        // (CRT_SHADE_RECURSES: shade_load has compared h.mesh with the scene's count and found one of the two materials)
        const DMaterial M = A.s->materials[A.s->meshes[h.mesh].material];
        const bool refractive = M.type == CRT_MAT_REFRACTIVE;
        const bool through = mirror_glass_children(refractive, M.ior, q.direction[0], q.direction[1], q.direction[2], h.point[0], h.point[1],
                                                   h.point[2], h.normal[0], h.normal[1], h.normal[2], &G.reflection_bias, &G.refraction_bias,
                                                   N.f, rox, roy, roz, rdx, rdy, rdz, tox, toy, toz, tdx, tdy, tdz);
        if (refractive) N.kind = TN_REFRACT;
        else {
            N.kind = TN_REFLECT;
            N.cx = M.ax; N.cy = M.ay; N.cz = M.az;
        }
        N.a = CHILD_BG;
        N.b = refractive ? (through ? CHILD_BG : CHILD_NONE) : 0u;
        reflect = G.spawn != 0u;
        transmit = G.spawn != 0u && through;
    }
    const unsigned long long m1 = __ballot(reflect), m2 = __ballot(transmit);
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long m3 = GI ? __ballot(samples) : 0ull;
    const uint32_t n1 = (uint32_t)__popcll(m1), n2 = (uint32_t)__popcll(m2), n3 = GI ? (uint32_t)__popcll(m3) * G.gi_samples : 0u;
    uint32_t base = 0;
    if (m1 | m3) {   // (wave-uniform)
        const uint32_t first = (uint32_t)(__ffsll((long long)(m1 | m3)) - 1);
        if (lane == first) base = atomicAdd(G.child_count, n1 + n2 + n3);
        base = __shfl(base, first);
    }
    if (reflect) {
        const uint32_t i1 = base + (uint32_t)__popcll(m1 & below);
        if (i1 < G.child_cap) {
            crt_ray c;
            normalize3(rdx, rdy, rdz);   // the child's shootRay entry (RayTracer.cpp:420)
            c.origin[0] = rox; c.origin[1] = roy; c.origin[2] = roz; c.direction[0] = rdx; c.direction[1] = rdy; c.direction[2] = rdz;
            G.child_rays[i1] = c;
            if constexpr (GI) G.child_keys[i1] = crt_gi_child_key(key, 0u);
            N.a = i1;
        }
        if (transmit) {
            const uint32_t i2 = base + n1 + (uint32_t)__popcll(m2 & below);
            if (i2 < G.child_cap) {
                crt_ray c;
                normalize3(tdx, tdy, tdz);
                c.origin[0] = tox; c.origin[1] = toy; c.origin[2] = toz; c.direction[0] = tdx; c.direction[1] = tdy; c.direction[2] = tdz;
                G.child_rays[i2] = c;
                if constexpr (GI) G.child_keys[i2] = crt_gi_child_key(key, 1u);
                N.b = i2;
            }
        }
    }
    if constexpr (GI) {
        if (gi_record) {
            N.a = CHILD_BG;
            // (64-bit: the block's end is compared with the capacity before anything of it is written)
            const uint64_t i3 = (uint64_t)base + n1 + n2 + (uint64_t)__popcll(m3 & below) * G.gi_samples;
            if (samples && i3 + G.gi_samples <= (uint64_t)G.child_cap) {
                const crt_ray q = G.rays[r];
                const crt_hit h = G.hits[r];
                const float ox = h.point[0] + h.normal[0] * G.monte_carlo_bias, oy = h.point[1] + h.normal[1] * G.monte_carlo_bias,
                            oz = h.point[2] + h.normal[2] * G.monte_carlo_bias;
                for (uint32_t i = 0; i < G.gi_samples; i++) {
                    float dx, dy, dz;
                    gi_sample_direction(q.direction[0], q.direction[1], q.direction[2], h.normal[0], h.normal[1], h.normal[2],
                                        crt_gi_uniform(key, 2u + 2u * i), crt_gi_uniform(key, 3u + 2u * i), dx, dy, dz);
                    normalize3(dx, dy, dz);   // the child's shootRay entry
                    crt_ray c;
                    c.origin[0] = ox; c.origin[1] = oy; c.origin[2] = oz; c.direction[0] = dx; c.direction[1] = dy; c.direction[2] = dz;
                    G.child_rays[i3 + i] = c;
                    G.child_keys[i3 + i] = crt_gi_child_key(key, 2u + i);
                }
                N.a = (uint32_t)i3;
            }
            G.nodes[2 * r + 1] = make_float4(__uint_as_float(N.a), 0.0f, 0.0f, 0.0f);   // (a DIFFUSE record's node is this word alone)
        }
    }
    if (recurses) {
        G.nodes[2 * r] = make_float4(N.cx, N.cy, N.cz, __uint_as_float(N.kind));
        G.nodes[2 * r + 1] = make_float4(__uint_as_float(N.a), __uint_as_float(N.b), N.f, 0.0f);
    }
}

// the colour shootRay returned for child `index` of the next level (CHILD_BG: the depth rule, RayTracer.cpp:427-429)
__device__ __forceinline__ void radiance_child(const KernelArgs &A, const RadianceArgs &G, const uint32_t child_n, const uint32_t index, float &x,
                                               float &y, float &z) {
    x = A.s->bgx; y = A.s->bgy; z = A.s->bgz;
    if (index < child_n) { x = G.child_rgb[3 * (size_t)index]; y = G.child_rgb[3 * (size_t)index + 1]; z = G.child_rgb[3 * (size_t)index + 2]; }
}

// What calculateReflection / calculateRefraction return once their recursive calls have (RayTracer.cpp:368-372, 414-416): the
// expressions of stream_resolve (kernel_stream.h), a lane per recursing record of the level.  Level g + 1's colours are final when
// this runs for level g.  GI: and what calculateDiffusion returns once its sample rays have (RayTracer.cpp:349-353): the record's
// colour is its direct light until then; the samples' colours are added in sample order to an indirect sum that starts at 0, a sample
// that was not traced is the background, and no samples at all is (direct + 0) * (1 / 1).
template <bool GI, bool DEVN = false>
__global__ __launch_bounds__(BLOCK) void radiance_combine(const KernelArgs A, const RadianceArgs G) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t child_n = radiance_count<DEVN>(G.child_n_dev, G.child_n);
    if (r >= radiance_count<DEVN>(G.n_dev, G.n)) return;
    if constexpr (GI) {
        if (G.status[r] == (uint8_t)CRT_SHADE_DIFFUSE) {
            const uint32_t first = __float_as_uint(G.nodes[2 * r + 1].x);
            const float gi_inv = 1.0f / (float)(G.gi_samples + 1u);
            float ix = 0.0f, iy = 0.0f, iz = 0.0f;
            for (uint32_t i = 0; i < G.gi_samples; i++) {
                float cx, cy, cz;
                radiance_child(A, G, child_n, first == CHILD_BG ? CHILD_BG : first + i, cx, cy, cz);
                ix = ix + cx; iy = iy + cy; iz = iz + cz;
            }
            G.rgb[3 * r] = (G.rgb[3 * r] + ix) * gi_inv; G.rgb[3 * r + 1] = (G.rgb[3 * r + 1] + iy) * gi_inv; G.rgb[3 * r + 2] = (G.rgb[3 * r + 2] + iz) * gi_inv;
            return;
        }
    }
    if (G.status[r] != (uint8_t)CRT_SHADE_RECURSES) return;
    const float4 n0 = G.nodes[2 * r], n1 = G.nodes[2 * r + 1];
    const uint32_t kind = __float_as_uint(n0.w) & TN_KIND_MASK;
    float cx, cy, cz;
    radiance_child(A, G, child_n, __float_as_uint(n1.x), cx, cy, cz);   // the reflection ray is shot first (RayTracer.cpp:366, 398-400)
    if (kind == TN_REFLECT) {
        cx = 0.0f + n0.x * cx; cy = 0.0f + n0.y * cy; cz = 0.0f + n0.z * cz;   // RayTracer.cpp:368-372
    } else {
        const uint32_t refr = __float_as_uint(n1.y);
        if (refr != CHILD_NONE) {   // (CHILD_NONE: `return reflectionColor`, RayTracer.cpp:416)
            float tx, ty, tz;
            radiance_child(A, G, child_n, refr, tx, ty, tz);
            const float f = n1.z;
            cx = f * cx + (1 - f) * tx; cy = f * cy + (1 - f) * ty; cz = f * cz + (1 - f) * tz;   // RayTracer.cpp:414
        }
    }
    G.rgb[3 * r] = cx; G.rgb[3 * r + 1] = cy; G.rgb[3 * r + 2] = cz;
}

// The call's crt_shoot_report from the device words, behind the last radiance_combine: one wave, lane g for level g.  Level 0 holds the
// caller's rays; level g >= 1 holds min(count[g], cap[g]) of the count[g] children radiance_scatter appended to it, and the rest did not
// fit (cap[g] = 0 behind the last level the host launched).  Written to `out` and `out2`, whichever is not null, with plain stores.
struct ReportArgs {
    const uint32_t *count;               // [g]: rays appended to level g (g >= 1)
    const unsigned long long *hits0;     // the caller's rays with a hit
    const unsigned long long *diffuse;   // DIFFUSE records over all levels
    const unsigned long long *rerouted;  // the constituent launches' rerouted rays and records
    crt_shoot_report *out, *out2;
    uint32_t n;                          // the caller's rays
    uint32_t cap[MAX_GENERATIONS];
};
__global__ __launch_bounds__(64) void radiance_report(const ReportArgs P) {
    const uint32_t g = threadIdx.x;
    const uint32_t appended = g == 0 ? P.n : P.count[g];
    const uint32_t held = g == 0 ? P.n : (appended < P.cap[g] ? appended : P.cap[g]);
    const unsigned long long lost = __ballot(appended > held);
    unsigned long long dropped = appended - held;
    for (int off = 32; off > 0; off >>= 1) dropped += __shfl_down(dropped, off);
    const uint32_t levels = (uint32_t)__popcll(__ballot(held > 0u));   // (level g + 1 holds children of level g: the levels with rays are the first ones)
    crt_shoot_report *const outs[2] = {P.out, P.out2};
    for (int k = 0; k < 2; k++) {
        crt_shoot_report *o = outs[k];
        if (!o) continue;
        o->level_rays[g] = held;
        if (g == 0) {
            o->levels = levels;
            o->overflow = lost ? (uint32_t)__ffsll((long long)lost) - 1u : 0u;   // level g + 1 is lane g + 1: 1 + g
            o->dropped = dropped;
            o->hits = *P.hits0;
            o->shadow_records = *P.diffuse;
            o->rerouted = *P.rerouted;
        }
    }
}
