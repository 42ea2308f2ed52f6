// kernel_query.h -- ray queries: closest hit and occlusion for rays the CALLER supplies (crt_trace_rays*, crt_occluded_rays*), and
// the camera's rays as such a set (crt_camera_rays_device).  The reference's seam below shootRay: AccelerationStructure::intersect
// (KDTree.cpp:127-192) and AccelerationStructure::checkForIntersection (AccelerationStructure.cpp:56-94).
//
// Nothing of the parity argument is restated here: the filter walk is kernel_bvh.h's (bvh_ray_setup, bvh_step, bvh_line_setup,
// bvh_miss_step -- candidates from the filter, the reference's triangle test, every accepted candidate verified against the
// reference's own trees), the reference-order walk is kernel_lane.h's (traversal_begin / traversal_step<false>), the record of a
// hit is surface_at's (kernel_common.h).  What differs from a frame's kernels:
//   * a ray comes out of the caller's array AS GIVEN (the reference's Ray holds what it is handed; camera rays and shootRay
//     normalise before they build one) and its answer goes to the caller's array: no ray tree, no queues, no shading;
//   * a ray the filter cannot answer -- a direction that is not of unit length (QUERY_UNIT_TOL), a non-finite coordinate, a miss
//     that the miss check refutes, a stack that runs out -- does NOT condemn the launch, as it condemns a frame: the lane of
//     query_walk appends the ray's index to a list (one atomic per wave and round) and query_reroute, launched behind on the same stream, walks the
//     listed rays in the reference's order.  No host round trip: the device variants stay asynchronous.
//   * the launches have scratch of their own (walk-stack spill columns, list, counter words: crt_query.hip), never a frame's.
#pragma once

#include "kernel_bvh.h"
#include "kernel_lane.h"
#include "shoot_caps.h"

// The filter's error analysis (kernel_bvh.h, top of the file and bvh_ray_setup) takes t for the distance travelled: |d| = 1 up to
// rounding.  It has a factor of twelve in hand (a slack of 256 unit roundoffs where about 20 are needed), the shadow walk's
// segment end one of 2^8 (t <= distance (1 + 2^-16) where |d| >= 1 - 2^-24 would do), the miss check's cones 1e-4 rad against
// |d . n| < 4 u.  A direction with | dx^2 + dy^2 + dz^2 - 1 | <= 2^-20, the sum evaluated in float32 as written below (its own
// rounding is below 2^-22), has | |d| - 1 | < 2^-20: a change of one part in a million to bounds that have those factors in hand.
// Every float32-rounded unit vector qualifies (each square is off by at most 2^-23 of itself: the sum by less than 2^-21), and so
// does every vector that normalize3 has produced.  What does not qualify is answered by the reference-order walk: same answer.
constexpr float QUERY_UNIT_TOL = 0x1p-20f;

// the query launches' words (uint32 offsets), 256 bytes apart: the filter kernel's cursor, the reroute list's length, the reroute
// kernel's cursor; hits / rerouted rays of the call (64-bit, over all of its launches)
enum : int { QW_CURSOR = 0, QW_LIST = 64, QW_RCURSOR = 128, QW_HITS = 192, QW_REROUTED = 256, QW_WORDS = 320 };

struct QueryArgs {
    const crt_ray *rays;
    const float *max_distance;    // occlusion only
    crt_hit *hits;                // closest hit only
    uint8_t *occluded;            // occlusion only
    uint32_t n;                   // rays of this launch (< 2^31)
    uint32_t ray_type;            // CRT_RAY_*: only PRIMARY differs (Ray.cpp:13)
    uint32_t *words;              // QW_*
    uint32_t *list;               // indices of the rays left to query_reroute
    uint32_t *spill;              // the walks' stacks beyond their LDS part: one column per thread of this grid
    uint32_t direct;              // query_reroute: no list -- every ray of the launch (a scene without a filter, crt_tuning::bvh == 0)
    uint32_t chunk;               // indices a wave claims per atomic (kernel_stream.h: wave_fetch_chunked)
    // the DEVN builds alone (crt_shoot_rays*_enqueue: a level's size stays on the device)
    const uint32_t *count;        // rays of the whole LEVEL, of which this launch has [first, first + n): n is the launch's capacity
    uint32_t first;
};

// rays of this launch.  DEVN: clamp(*count - first, 0, n) (shoot_caps.h) -- one load for the wave, from a word that
// the launches before this one have finished with.  The other builds read n and are what they were.
template <bool DEVN>
__device__ __forceinline__ uint32_t query_count(const QueryArgs &Q) {
    if constexpr (DEVN) return shoot_part_count((uint32_t)__builtin_amdgcn_readfirstlane(*Q.count), Q.first, Q.n);
    else return Q.n;
}

__device__ __forceinline__ void query_load_ray(const QueryArgs &Q, const uint32_t r, Ray &R) {
    const crt_ray q = Q.rays[r];
    R.ox = q.origin[0]; R.oy = q.origin[1]; R.oz = q.origin[2];
    R.dx = q.direction[0]; R.dy = q.direction[1]; R.dz = q.direction[2];   // as given: nothing is normalised
    ray_prepare(R);
}
__device__ __forceinline__ bool query_direction_is_unit(const Ray &R) {
    const float s = R.dx * R.dx + R.dy * R.dy + R.dz * R.dz;
    return fabsf(s - 1.0f) <= QUERY_UNIT_TOL;   // (NaN: false)
}
// what AccelerationStructure::intersect hands back (KDTree.cpp:168-190: point, face or interpolated normal, (u, v)), or zeros
__device__ __forceinline__ void query_write_hit(const KernelArgs &A, const QueryArgs &Q, const uint32_t r, const Ray &R, const bool have,
                                                const float t, const uint32_t tri, const uint32_t mesh) {
    crt_hit h;
    h.t = 0; h.point[0] = h.point[1] = h.point[2] = 0; h.normal[0] = h.normal[1] = h.normal[2] = 0; h.u = h.v = 0;
    h.mesh = 0; h.triangle = 0; h.hit = 0;
    if (have) {
        Surface S;
        surface_at(A, R, t, tri, mesh, S);
        h.t = t; h.point[0] = S.px; h.point[1] = S.py; h.point[2] = S.pz;
        h.normal[0] = S.nx; h.normal[1] = S.ny; h.normal[2] = S.nz; h.u = S.u; h.v = S.v;
        h.mesh = mesh; h.triangle = tri; h.hit = 1u;
    }
    Q.hits[r] = h;
}
// the lanes of the wave for which `mine` holds append r to the reroute list: one atomic for all of them
__device__ __forceinline__ void query_append(const QueryArgs &Q, const bool mine, const uint32_t r, const uint32_t lane) {
    const unsigned long long m = __ballot(mine);
    if (mine) {
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        uint32_t base = 0;
        if (rank == 0) base = atomicAdd(Q.words + QW_LIST, (uint32_t)__popcll(m));
        base = __shfl(base, __ffsll((long long)m) - 1);
        Q.list[base + rank] = r;
    }
}
// the wave's sum of n, added to the 64-bit counter at `word` by one atomic
__device__ __forceinline__ void wave_add_u64(uint32_t *word, const uint32_t n, const uint32_t lane) {
    unsigned long long v = n;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0 && v) atomicAdd(reinterpret_cast<unsigned long long *>(word), v);
}
// the Ray of a lane that holds none yet
__device__ __forceinline__ Ray query_no_ray() {
    Ray R;
    R.ox = R.oy = R.oz = R.dx = R.dy = R.dz = R.ix = R.iy = R.iz = 0; R.parmask = 0;
    return R;
}
// a walk that ended without a hit starts over as the miss check (kernel_bvh.h: bvh_miss_step)
__device__ __forceinline__ void query_begin_miss_check(const KernelArgs &A, const Ray &R, BvhWalk &W) {
    W.cur = 0; W.sp = 0; W.cache_mesh = NONE; W.cache_k2 = NONE;
    bvh_line_setup(A, R, W.B);
}
__device__ __forceinline__ BvhStack query_stack_of(const QueryArgs &Q, uint32_t *stack_lds) {
    BvhStack S;
    S.lds = stack_lds + threadIdx.x;
    S.stride = gridDim.x * BLOCK;
    S.spill = Q.spill + (size_t)blockIdx.x * BLOCK + threadIdx.x;
    S.room = 0;   // (read by the bounds-checked build only, and the query kernels have none)
    return S;
}

// The filter kernel of both ray queries: persistent waves, a lane per ray, bvh_shade_level's state machine (kernel_bvh.h) with the
// shading replaced by the answer's store.  Work indices are claimed per wave in chunks, as level 0 claims its primary rays; a wave
// looks after its free lanes when BVH_BATCH of them have gathered.
//   closest hit (OCCLUDED = false): the walk has no end, and a ray without a hit goes through the miss check.
//   occlusion (OCCLUDED = true): checkForIntersection(ray, max_distance) of the non-GI build for a shadow ray
//     (AccelerationStructure.cpp:56-94): refractive meshes skipped, a mesh occludes when its closest hit lies within
//     length(point - origin) <= max_distance.  The walk is bvh_shadow_rays' (kernel_bvh.h): it ends at max_distance (1 + 2^-16) and at
//     the first verified occluder.  A max_distance that is not finite lets a mesh's closest hit at t = +inf count as well (length = inf
//     <= inf), and such a hit is no candidate of the filter: those rays (and only those) go through the miss check when the walk found
//     no occluder, like a closest-hit ray without a hit -- nothing found (all but certain): not occluded; something found: the
//     reference-order walk decides.
template <int MODE, bool OCCLUDED, bool DEVN = false>
__global__ __launch_bounds__(BLOCK) void query_walk(const KernelArgs A, const QueryArgs Q) {
    __shared__ uint32_t stack_lds[BVH_LDS_STACK * BLOCK];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = query_count<DEVN>(Q);
    const BvhStack stack = query_stack_of(Q, stack_lds);
    const bool primary = !OCCLUDED && Q.ray_type == (uint32_t)RAY_PRIMARY;
    uint32_t nbox = 0, ntri = 0, n_hits = 0;
    Ray R = query_no_ray();
    BvhWalk W;
    bvh_walk_begin(W, INFINITY);
    float light_dist = 0;   // (occlusion only)
    int state = BVH_FETCH;
    uint32_t r = 0;
    WaveChunk chunk{0u, 0u};
    for (;;) {
        const uint32_t n_free = (uint32_t)__popcll(__ballot(state == BVH_FETCH || state == BVH_FINISHED));
        if (n_free >= BVH_BATCH || (n_free && !__ballot(state == BVH_WALK || state == BVH_MISS_CHECK))) {
            if (state == BVH_FINISHED) {
                // a ray the filter cannot take, a miss refuted: the ray (not the launch) goes to the reference-order walk
                query_append(Q, W.give_up, r, lane);
                if (!W.give_up) {
                    if constexpr (OCCLUDED) Q.occluded[r] = W.have ? 1 : 0;
                    else query_write_hit(A, Q, r, R, W.have, W.best, W.btri, W.bmesh);
                    n_hits += W.have ? 1u : 0u;
                }
                state = BVH_FETCH;
            }
            // one fetch per free lane and round: no inner loop, no `continue` (compiler notes)
            const uint32_t claimed = wave_fetch_chunked(Q.words + QW_CURSOR, lane, state == BVH_FETCH, chunk, Q.chunk, n);
            if (state == BVH_FETCH) {
                r = claimed;
                if (r >= n) state = BVH_OUT;
                else {
                    query_load_ray(Q, r, R);
                    if constexpr (OCCLUDED) {
                        light_dist = Q.max_distance[r];
                        // an occluding hit has length(d t) <= max_distance with |d| = 1 up to QUERY_UNIT_TOL: t <= max_distance (1 + 2^-16)
                        bvh_walk_begin(W, light_dist * (1.0f + 0x1p-16f));
                    } else bvh_walk_begin(W, INFINITY);
                    if (bvh_ray_setup(A, R, W.B) && query_direction_is_unit(R)) state = BVH_WALK;
                    else { W.give_up = true; state = BVH_FINISHED; }
                }
            }
        }
        if (!__ballot(state != BVH_OUT)) break;
        if (state == BVH_WALK) {
            for (int it = 0; it < BVH_STEPS; ++it)
                if (state == BVH_WALK && !bvh_step<OCCLUDED ? 1 : 0, MODE>(A, R, primary, light_dist, false, W, stack, nbox, ntri)) {
                    if (W.have || W.give_up || (OCCLUDED && light_dist < INFINITY)) state = BVH_FINISHED;
                    else { query_begin_miss_check(A, R, W); state = BVH_MISS_CHECK; }
                }
        }
        if (state == BVH_MISS_CHECK) {
            for (int it = 0; it < BVH_STEPS; ++it)
                if (state == BVH_MISS_CHECK && !bvh_miss_step<MODE>(A, R, primary, W, stack, nbox, ntri)) state = BVH_FINISHED;
        }
    }
    wave_add_u64(Q.words + QW_HITS, n_hits, lane);
}

// The rays the filter kernel listed (or, `direct`, every ray of the launch), walked in the reference's order, a lane per ray:
// render_lanes' walk (kernel_lane.h) without the recursion.  Launched behind the filter kernel with a grid for the worst case --
// every ray listed --; the list is all but always empty or short, and a workgroup that sees no ray for one of its lanes leaves.
template <bool OCCLUDED, bool DEVN = false>
__global__ __launch_bounds__(BLOCK) void query_reroute(const KernelArgs A, const QueryArgs Q) {
    const uint32_t count = Q.direct ? query_count<DEVN>(Q) : Q.words[QW_LIST];
    if (blockIdx.x == 0 && threadIdx.x == 0 && count) atomicAdd(reinterpret_cast<unsigned long long *>(Q.words + QW_REROUTED), (unsigned long long)count);
    if ((uint64_t)blockIdx.x * BLOCK >= count) return;
    const uint32_t lane = threadIdx.x & 63u;
    Ray R = query_no_ray();
    LaneWalk L;
    traversal_begin(L, A.s->top_root);
    L.rtype = RAY_REFLECTION; L.light_dist = 0;
    int state = ST_FETCH;
    uint32_t r = 0, n_hits = 0;
    for (;;) {
        const uint32_t n_free = (uint32_t)__popcll(__ballot(state == ST_FETCH));
        if (n_free >= BVH_BATCH || (n_free && !__ballot(state == ST_TRAVERSE))) {
            if (state == ST_FETCH) {
                const uint32_t k = wave_fetch(Q.words + QW_RCURSOR, lane);
                if (k >= count) state = ST_DONE;
                else {
                    r = Q.direct ? k : Q.list[k];
                    query_load_ray(Q, r, R);
                    traversal_begin(L, A.s->top_root);
                    // (reflection and refraction rays behave alike in the walk; only PRIMARY culls back faces, Ray.cpp:13)
                    L.rtype = OCCLUDED ? RAY_SHADOW : (Q.ray_type == (uint32_t)RAY_PRIMARY ? RAY_PRIMARY : RAY_REFLECTION);
                    if (OCCLUDED) L.light_dist = Q.max_distance[r];
                    state = ST_TRAVERSE;
                }
            }
        }
        if (!__ballot(state != ST_DONE)) break;
        for (int it = 0; it < 32; ++it)
            if (state == ST_TRAVERSE && !traversal_step<false>(L, R, A, nullptr)) {
                if (OCCLUDED) { Q.occluded[r] = L.occluded ? 1 : 0; n_hits += L.occluded ? 1u : 0u; }
                else { query_write_hit(A, Q, r, R, L.have, L.bt, L.btri, L.bmesh); n_hits += L.have ? 1u : 0u; }
                state = ST_FETCH;
            }
    }
    wave_add_u64(Q.words + QW_HITS, n_hits, lane);
}

// crt_shoot_rays*_enqueue: what the other calls do with hipMemsetAsync and a small copy, as ONE kernel -- a captured call is then a
// chain of kernel nodes and nothing else.  Copies src to dst (64 bits; null: nothing) and then zeroes a[0 .. na) and b[0 .. nb): the
// counter words before a launch that starts counting again.  One workgroup; plain stores.
struct ResetArgs {
    uint32_t *a, *b;
    uint32_t na, nb;
    const unsigned long long *src;
    unsigned long long *dst;
};
__global__ __launch_bounds__(BLOCK) void query_reset(const ResetArgs P) {
    if (threadIdx.x == 0 && P.src) *P.dst = *P.src;
    for (uint32_t i = threadIdx.x; i < P.na; i += BLOCK) P.a[i] = 0u;
    for (uint32_t i = threadIdx.x; i < P.nb; i += BLOCK) P.b[i] = 0u;
}

// RayTracer::getRay (RayTracer.cpp:61-80) at the pixel centre, one thread per pixel, row-major: the direction normalised ONCE, as
// getRay returns it (primary_ray, kernel_common.h, is getRay FOLLOWED by shootRay's own normalisation, RayTracer.cpp:420: the ray a
// frame walks.  A query walks the ray it is given, so a caller who wants the frame's ray normalises once more).
__global__ __launch_bounds__(BLOCK) void query_camera_rays(const QueryCamera C, crt_ray *out) {
    const uint64_t gid = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (gid >= (uint64_t)C.width * C.height) return;
    const uint32_t px = (uint32_t)(gid % C.width), py = (uint32_t)(gid / C.width);
    float x = (float)px + 0.5f;
    float y = (float)py + 0.5f;
    x = x / (float)C.width;
    y = y / (float)C.height;
    x = (2.0f * x) - 1.0f;
    y = 1.0f - (2.0f * y);
    x = x * ((float)C.width / (float)C.height);
    const float z = -1.0f;
    float dx = x * C.m[0] + y * C.m[3] + z * C.m[6];   // row vector x matrix, Matrix.h:137-142
    float dy = x * C.m[1] + y * C.m[4] + z * C.m[7];
    float dz = x * C.m[2] + y * C.m[5] + z * C.m[8];
    normalize3(dx, dy, dz);
    crt_ray q;
    q.origin[0] = C.pos[0]; q.origin[1] = C.pos[1]; q.origin[2] = C.pos[2];
    q.direction[0] = dx; q.direction[1] = dy; q.direction[2] = dz;
    out[gid] = q;
}
