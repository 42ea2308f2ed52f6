// kernel_shade.h -- direct lighting for records the CALLER supplies (crt_shade_hits*, crt_light_points*): the reference's one
// non-recursive stage below shootRay, RayTracer::calculateDiffusion of the non-GI build (RayTracer.cpp:300-330), and the cases of
// shootRay that need no further ray (RayTracer.cpp:443-450: no hit or a constant material -- the background).
//
// The design is the ray queries' (kernel_query.h): persistent waves, a lane per record, the candidate filter's shadow walk, and a
// record the filter cannot answer goes ALONE to the reference-order walk behind it.  What is new is the light loop inside a lane:
//   * a lane owns its record from load to store.  The reference adds the lights' contributions in scene order and float addition
//     does not commute, so the sum stays where it is formed: one record's lights are never split over lanes;
//   * every light is light_setup's shadow ray (kernel_common.h, the bias from the query's arguments) walked like query_walk<.., true>
//     walks a caller's ray: to distance (1 + 2^-16), to the first verified occluder;
//   * when ANY of a record's shadow rays cannot be taken by the filter -- a non-finite coordinate (a record at t = inf / NaN), a
//     zero direction (a light AT the point), a stack that runs out -- the whole record is listed and query_direct_reroute redoes
//     every light of it in the reference's order.  Its colour is written once, by the kernel that finishes it.
#pragma once

#include "kernel_query.h"

struct ShadeArgs {
    QueryArgs q;                  // n, words, list, spill, direct, chunk: as the ray queries use them (rays / hits / occluded unused)
    const crt_hit *hits;          // crt_shade_hits
    const float *points, *normals;  // crt_light_points: 3 floats per record each
    float *out;                   // 3 floats per record (crt_shade_hits) or one (crt_light_points)
    uint8_t *status;              // CRT_SHADE_* per record, or null
    float shadow_bias;
};

// What the light loop needs of a record: the point, the normal and the colour an unoccluded light's factor multiplies.
struct ShadeRecord { float px, py, pz, nx, ny, nz, bx, by, bz; };

// shootRay's switch on the hit (RayTracer.cpp:430-450) for a record of the caller's; DIFFUSE: H is filled in.  Both indices are
// compared with the scene's counts BEFORE anything is read through them; what in-range indices lead to is in range by crt_create's
// checks (crt_scene.hip: mesh -> material -> texture, triangle -> vertices -> uvs, texels clamped to the bitmap).
template <bool POINTS>
__device__ __forceinline__ uint32_t shade_load(const KernelArgs &A, const ShadeArgs &S, const uint32_t r, ShadeRecord &H) {
    if (POINTS) {
        H.px = S.points[3 * (size_t)r]; H.py = S.points[3 * (size_t)r + 1]; H.pz = S.points[3 * (size_t)r + 2];
        H.nx = S.normals[3 * (size_t)r]; H.ny = S.normals[3 * (size_t)r + 1]; H.nz = S.normals[3 * (size_t)r + 2];
        H.bx = H.by = H.bz = 1.0f;   // a white, untextured diffuse surface: k * 1 = k
        return CRT_SHADE_DIFFUSE;
    }
    const crt_hit h = S.hits[r];
    if (h.hit == 0) return CRT_SHADE_BACKGROUND;
    if (h.mesh >= A.s->n_meshes || h.triangle >= A.s->n_triangles) return CRT_SHADE_INVALID;
    const DMaterial M = A.s->materials[A.s->meshes[h.mesh].material];
    if (M.type == CRT_MAT_REFLECTIVE || M.type == CRT_MAT_REFRACTIVE) return CRT_SHADE_RECURSES;
    if (M.type != CRT_MAT_DIFFUSE) return CRT_SHADE_BACKGROUND;   // RayTracer.cpp:443-446
    H.px = h.point[0]; H.py = h.point[1]; H.pz = h.point[2];
    H.nx = h.normal[0]; H.ny = h.normal[1]; H.nz = h.normal[2];
    if (M.texture >= 0) {
        bool is_bitmap;
        texture_color<false>(A, A.s->textures[M.texture], h.triangle, h.u, h.v, 1.0f - h.u - h.v, H.bx, H.by, H.bz, is_bitmap);
    } else { H.bx = M.ax; H.by = M.ay; H.bz = M.az; }
    return CRT_SHADE_DIFFUSE;
}

// a record's answer; (x, y, z): the light sum of a DIFFUSE record
template <bool POINTS>
__device__ __forceinline__ void shade_store(const KernelArgs &A, const ShadeArgs &S, const uint32_t r, const uint32_t status, float x, float y,
                                            float z) {
    if (POINTS) { S.out[r] = x; return; }
    if (status == CRT_SHADE_BACKGROUND) { x = A.s->bgx; y = A.s->bgy; z = A.s->bgz; }   // RayTracer.cpp:449-450
    else if (status != CRT_SHADE_DIFFUSE) { x = 0.0f; y = 0.0f; z = 0.0f; }
    S.out[3 * (size_t)r] = x; S.out[3 * (size_t)r + 1] = y; S.out[3 * (size_t)r + 2] = z;
    if (S.status) S.status[r] = (uint8_t)status;
}

// query_walk<.., true>'s state machine with a light index inside the lane: BVH_FETCH (wants a record), BVH_SHADOWS (between two lights:
// sets up the next shadow ray, or is through), BVH_WALK, BVH_FINISHED (its record is to be stored or listed), BVH_OUT.
// EVERY: the GI build's occlusion rule -- no mesh is skipped (AccelerationStructure.cpp:67-71) -- as a build of its own, for the levels
// of crt_shoot_rays_gi*: the plain build is what it was, instruction for instruction.
template <int MODE, bool POINTS, bool EVERY = false, bool DEVN = false>
__global__ __launch_bounds__(BLOCK) void query_direct(const KernelArgs A, const ShadeArgs S) {
    __shared__ uint32_t stack_lds[BVH_LDS_STACK * BLOCK];
    const uint32_t lane = threadIdx.x & 63u;
    const QueryArgs &Q = S.q;
    const uint32_t n = query_count<DEVN>(Q);
    const BvhStack stack = query_stack_of(Q, stack_lds);
    const uint32_t n_lights = A.s->n_lights;
    uint32_t nbox = 0, ntri = 0, n_diffuse = 0;
    Ray R = query_no_ray();
    BvhWalk W;
    bvh_walk_begin(W, INFINITY);
    ShadeRecord H;
    H.px = H.py = H.pz = H.nx = H.ny = H.nz = H.bx = H.by = H.bz = 0;
    float accx = 0, accy = 0, accz = 0, kfac = 0, light_dist = 0;
    uint32_t li = 0, r = 0;
    bool reroute = false;
    int state = BVH_FETCH;
    WaveChunk chunk{0u, 0u};
    for (;;) {
        const uint32_t n_free = (uint32_t)__popcll(__ballot(state == BVH_FETCH || state == BVH_FINISHED));
        if (n_free >= BVH_BATCH || (n_free && !__ballot(state == BVH_WALK || state == BVH_SHADOWS))) {
            if (state == BVH_FINISHED) {
                // a shadow ray the filter cannot take: the record (not the launch) goes to the reference-order walk, all of its lights
                query_append(Q, reroute, r, lane);
                if (!reroute) {
                    shade_store<POINTS>(A, S, r, CRT_SHADE_DIFFUSE, accx, accy, accz);
                    n_diffuse++;
                }
                state = BVH_FETCH;
            }
            // one fetch per free lane and round: no inner loop, no `continue` (compiler notes)
            const uint32_t claimed = wave_fetch_chunked(Q.words + QW_CURSOR, lane, state == BVH_FETCH, chunk, Q.chunk, n);
            if (state == BVH_FETCH) {
                r = claimed;
                if (r >= n) state = BVH_OUT;
                else {
                    const uint32_t status = shade_load<POINTS>(A, S, r, H);
                    if (status != CRT_SHADE_DIFFUSE) shade_store<POINTS>(A, S, r, status, 0.0f, 0.0f, 0.0f);   // (the lane fetches again next round)
                    else { accx = accy = accz = 0; li = 0; reroute = false; state = BVH_SHADOWS; }
                }
            }
        }
        if (!__ballot(state != BVH_OUT)) break;
        if (state == BVH_SHADOWS) {   // the next light (RayTracer.cpp:308-318), or none is left
            if (li >= n_lights) state = BVH_FINISHED;
            else {
                light_setup(A, li, H.px, H.py, H.pz, H.nx, H.ny, H.nz, S.shadow_bias, R, light_dist, kfac);
                // an occluding hit has length(d t) <= distance with |d| = 1 up to rounding: t <= distance (1 + 2^-16) (NaN: no bound)
                bvh_walk_begin(W, light_dist * (1.0f + 0x1p-16f));
                // query_walk's entry conditions.  A light at distance 0 leaves a zero direction (normalize3 returns it as it is), a
                // non-finite point or normal a non-finite ray: neither is the filter's.
                if (!(bvh_ray_setup(A, R, W.B) && query_direction_is_unit(R))) { reroute = true; state = BVH_FINISHED; }
                // No walk for a factor of +-0 (the light behind the surface: angle = max(0, l . n) = 0, or intensity 0) and a finite base:
                // the light would add +-0 to each channel if it is unoccluded and nothing if it is not, and adding +-0 changes no bit of
                // the sum -- a NaN stays that NaN, a non-zero stays itself, and a zero sum is +0 (it starts as +0, and no sum of
                // round-to-nearest additions gives -0 unless both terms are -0), to which +-0 adds up to +0.  (kernel_plan.h has the
                // argument for a frame.)  A NaN factor is not zero; an infinite or NaN base would make the product a NaN: both walk.
                else if (kfac == 0.0f && fabsf(H.bx) < INFINITY && fabsf(H.by) < INFINITY && fabsf(H.bz) < INFINITY) li++;
                else state = BVH_WALK;
            }
        }
        if (state == BVH_WALK) {
            for (int it = 0; it < BVH_STEPS; ++it)
                if (state == BVH_WALK && !bvh_step<1, MODE>(A, R, false, light_dist, EVERY, W, stack, nbox, ntri)) {
                    if (W.give_up) { reroute = true; state = BVH_FINISHED; }
                    else {
                        if (!W.have) {   // RayTracer.cpp:319-328: color = color + k * base
                            accx += kfac * H.bx;
                            if (!POINTS) { accy += kfac * H.by; accz += kfac * H.bz; }
                        }
                        li++;
                        state = BVH_SHADOWS;
                    }
                }
        }
    }
    wave_add_u64(Q.words + QW_HITS, n_diffuse, lane);
}

// The records query_direct listed (or, `direct`, every record of the launch: a scene without a filter, crt_tuning::bvh == 0), a lane per
// record, every light of it walked in the reference's order as render_lanes walks a diffuse hit's shadow rays (kernel_lane.h:
// traversal_begin / traversal_step<false>, rtype SHADOW; that walk reads the occlusion rule from the frame block, A.f->use_gi: the
// queries have an all-zero block and one with use_gi = 1).  The grid is sized for the worst case; a workgroup without a record leaves.
template <bool POINTS, bool DEVN = false>
__global__ __launch_bounds__(BLOCK) void query_direct_reroute(const KernelArgs A, const ShadeArgs S) {
    const QueryArgs &Q = S.q;
    const uint32_t count = Q.direct ? query_count<DEVN>(Q) : Q.words[QW_LIST];
    if ((uint64_t)blockIdx.x * BLOCK >= count) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_lights = A.s->n_lights;
    Ray R = query_no_ray();
    LaneWalk L;
    traversal_begin(L, A.s->top_root);
    L.rtype = RAY_SHADOW; L.light_dist = 0;
    ShadeRecord H;
    H.px = H.py = H.pz = H.nx = H.ny = H.nz = H.bx = H.by = H.bz = 0;
    float accx = 0, accy = 0, accz = 0, kfac = 0;
    uint32_t li = 0, r = 0, n_diffuse = 0;
    bool next_light = false;
    int state = ST_FETCH;
    for (;;) {
        const uint32_t n_free = (uint32_t)__popcll(__ballot(state == ST_FETCH));
        if (n_free >= BVH_BATCH || (n_free && !__ballot(state == ST_TRAVERSE))) {
            if (state == ST_FETCH) {
                const uint32_t k = wave_fetch(Q.words + QW_RCURSOR, lane);
                if (k >= count) state = ST_DONE;
                else {
                    r = Q.direct ? k : Q.list[k];
                    const uint32_t status = shade_load<POINTS>(A, S, r, H);
                    if (status != CRT_SHADE_DIFFUSE) shade_store<POINTS>(A, S, r, status, 0.0f, 0.0f, 0.0f);   // (`direct` only: nothing else is listed)
                    else { accx = accy = accz = 0; li = 0; next_light = true; state = ST_TRAVERSE; }
                }
            }
        }
        if (!__ballot(state != ST_DONE)) break;
        if (state == ST_TRAVERSE && next_light) {
            next_light = false;
            if (li < n_lights) {
                light_setup(A, li, H.px, H.py, H.pz, H.nx, H.ny, H.nz, S.shadow_bias, R, L.light_dist, kfac);
                L.rtype = RAY_SHADOW;
                traversal_begin(L, A.s->top_root);
            } else {
                shade_store<POINTS>(A, S, r, CRT_SHADE_DIFFUSE, accx, accy, accz);
                n_diffuse++;
                state = ST_FETCH;
            }
        }
        for (int it = 0; it < 32; ++it)
            if (state == ST_TRAVERSE && !next_light && !traversal_step<false>(L, R, A, nullptr)) {
                if (!L.occluded) {   // RayTracer.cpp:319-328
                    accx += kfac * H.bx;
                    if (!POINTS) { accy += kfac * H.by; accz += kfac * H.bz; }
                }
                li++;
                next_light = true;
            }
    }
    wave_add_u64(Q.words + QW_HITS, n_diffuse, lane);
    wave_add_u64(Q.words + QW_REROUTED, n_diffuse, lane);   // (the records redone here are the DIFFUSE ones: the others need no walk)
}
