// kernel_guides.h -- filter guides that follow mirrors and glass to the surface they show (include/crt_hip.h: "Chain guides";
// crt_guide_rays*).  One kernel, guide_step, launched behind every trace of a call's live chains (crt_query.hip runs the loop, the walks
// are the ray queries': kernel_query.h).  A lane per live entry of level k: the segment's ray, its closest hit, the pixel it belongs to,
// the path length before it and the mesh of the chain's first hit.  The lane either FINALISES its pixel -- record, status byte, terminal
// ray -- or APPENDS the chain's next segment to level k + 1's compact list.
//
// The child ray is mirror_glass_children's (kernel_common.h), the one body shade_hit and radiance_scatter share, normalised once more as
// the child's shootRay entry does (RayTracer.cpp:420): nothing of the parity argument is restated here.
//
// The append is radiance_scatter's: one ballot and one atomic per wave, so the ORDER of a level's list may differ between two runs and no
// pixel's result does -- a pixel's chain is a function of its own ray alone, and every lane writes its own pixel.  Every level's capacity
// is the caller's n (a chain has at most one live segment), so nothing can overflow; every index is still compared with that capacity
// before an address is formed from it.
#pragma once

#include "kernel_common.h"

constexpr uint32_t GUIDE_CUT = 0x80u;          // status bit 7: the chain was cut at max_bounces on a mirror or glass hit
constexpr uint32_t GUIDE_MAX_BOUNCES = 63u;    // status bits 0-5

struct GuideArgs {
    scene_args_p s;
    const crt_ray *rays;          // level k's rays as they were traced (level 0: the caller's, as given)
    const crt_hit *hits;          // ... their closest hits
    const uint32_t *pixel;        // ... the pixel of each; null at level 0: entry e is pixel e
    const float *tsum;            // ... (t_0 + ...) + t_(k-1); null at level 0
    const uint32_t *mesh0;        // ... the mesh of h_0; null at level 0
    const uint32_t *n_dev;        // entries appended to level k; null at level 0: n of them
    crt_ray *child_rays;          // level k + 1's list: ray, pixel, path length so far, first mesh
    uint32_t *child_pixel;
    float *child_tsum;
    uint32_t *child_mesh0;
    uint32_t *child_count;        // entries appended to level k + 1
    crt_hit *out_hits;            // one record a pixel
    uint8_t *out_status;          // one byte a pixel, or null
    crt_ray *out_last_rays;       // the terminal segment's ray, one a pixel, or null
    uint32_t n;                   // the caller's rays: the capacity of every level and of the outputs
    uint32_t level;               // k
    uint32_t max_bounces;
    float reflection_bias, refraction_bias;
};

__global__ __launch_bounds__(BLOCK) void guide_step(const GuideArgs G) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;   // (every lane stays to the end: the ballot is the wave's)
    uint32_t level_n = G.n;
    if (G.n_dev) {
        const uint32_t have = (uint32_t)__builtin_amdgcn_readfirstlane(*G.n_dev);
        level_n = have < G.n ? have : G.n;
    }
    bool spawn = false;
    uint32_t pixel = 0, first_mesh = 0;
    float t = 0;
    float cox = 0, coy = 0, coz = 0, cdx = 0, cdy = 0, cdz = 0;   // the child ray
    if (e < level_n) {
        pixel = G.pixel ? G.pixel[e] : (uint32_t)e;
        if (pixel < G.n) {
            // (the two records word by word: a whole-struct copy of their float[3] members ends up in LDS with this compiler)
            const float *const qw = reinterpret_cast<const float *>(G.rays + e);
            const float qox = qw[0], qoy = qw[1], qoz = qw[2], qdx = qw[3], qdy = qw[4], qdz = qw[5];
            const float *const hw = reinterpret_cast<const float *>(G.hits + e);
            const uint32_t *const hu = reinterpret_cast<const uint32_t *>(G.hits + e);
            const float h_t = hw[0], hpx = hw[1], hpy = hw[2], hpz = hw[3], hnx = hw[4], hny = hw[5], hnz = hw[6], h_u = hw[7], h_v = hw[8];
            const uint32_t h_mesh = hu[9], h_triangle = hu[10], h_hit = hu[11];
            t = G.tsum ? G.tsum[e] + h_t : h_t;
            first_mesh = G.mesh0 ? G.mesh0[e] : h_mesh;
            const uint32_t n_meshes = G.s->n_meshes;
            uint32_t status = G.level;
            // the mesh is compared with the scene's count before anything is read through it (a record of a trace is in range)
            if (h_hit != 0 && h_mesh < n_meshes) {
                const DMaterial M = G.s->materials[G.s->meshes[h_mesh].material];
                const bool refractive = M.type == CRT_MAT_REFRACTIVE;
                if (refractive || M.type == CRT_MAT_REFLECTIVE) {
                    if (G.level >= G.max_bounces) status |= GUIDE_CUT;
                    else {
                        float fresnel = 0, rox, roy, roz, rdx, rdy, rdz, tox = 0, toy = 0, toz = 0, tdx = 0, tdy = 0, tdz = 0;
                        const bool through = mirror_glass_children(refractive, M.ior, qdx, qdy, qdz, hpx,
                                                                   hpy, hpz, hnx, hny, hnz, &G.reflection_bias,
                                                                   &G.refraction_bias, fresnel, rox, roy, roz, rdx, rdy, rdz, tox, toy, toz, tdx, tdy,
                                                                   tdz);
                        // glass: the transmission ray; under total internal reflection, and on a mirror, the reflection ray
                        if (through) { rox = tox; roy = toy; roz = toz; rdx = tdx; rdy = tdy; rdz = tdz; }
                        normalize3(rdx, rdy, rdz);   // the child's shootRay entry (RayTracer.cpp:420)
                        cox = rox; coy = roy; coz = roz; cdx = rdx; cdy = rdy; cdz = rdz;
                        spawn = true;
                    }
                }
            }
            if (!spawn) {
                const bool hit = h_hit != 0;   // (a miss stays all-zero, as the trace wrote it)
                float *const ow = reinterpret_cast<float *>(G.out_hits + pixel);
                uint32_t *const ou = reinterpret_cast<uint32_t *>(G.out_hits + pixel);
                ow[0] = hit ? t : h_t; ow[1] = hpx; ow[2] = hpy; ow[3] = hpz; ow[4] = hnx; ow[5] = hny; ow[6] = hnz; ow[7] = h_u; ow[8] = h_v;
                ou[9] = hit && G.level != 0u ? h_mesh + n_meshes * (1u + first_mesh) : h_mesh;
                ou[10] = h_triangle; ou[11] = h_hit;
                if (G.out_status) G.out_status[pixel] = (uint8_t)status;
                if (G.out_last_rays) {
                    float *const lw = reinterpret_cast<float *>(G.out_last_rays + pixel);
                    lw[0] = qox; lw[1] = qoy; lw[2] = qoz; lw[3] = qdx; lw[4] = qdy; lw[5] = qdz;
                }
            }
        }
    }
    const unsigned long long m = __ballot(spawn);
    if (m) {   // (wave-uniform)
        const uint32_t first = (uint32_t)(__ffsll((long long)m) - 1);
        uint32_t base = 0;
        if (lane == first) base = atomicAdd(G.child_count, (uint32_t)__popcll(m));
        base = __shfl(base, first);
        const uint32_t i = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (spawn && i < G.n) {
            float *const cw = reinterpret_cast<float *>(G.child_rays + i);
            cw[0] = cox; cw[1] = coy; cw[2] = coz; cw[3] = cdx; cw[4] = cdy; cw[5] = cdz;
            G.child_pixel[i] = pixel;
            G.child_tsum[i] = t;
            G.child_mesh0[i] = first_mesh;
        }
    }
}
