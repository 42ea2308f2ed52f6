// crt_query.hip -- ray queries (include/crt_hip.h: crt_trace_rays*, crt_occluded_rays*, crt_camera_rays_device, crt_get_query_stats):
// closest hit and occlusion for rays the caller supplies; and direct lighting for the caller's hit records and points (crt_shade_hits*,
// crt_light_points*: RayTracer::calculateDiffusion, RayTracer.cpp:300-330; kernels: csrc/kernel_shade.h), on the same scratch.  Replaces AccelerationStructure::intersect (KDTree.cpp:127-192) and
// AccelerationStructure::checkForIntersection (AccelerationStructure.cpp:56-94) as entry points of their own; the kernels are
// csrc/kernel_query.h.  A query reads the context's scene and nothing of its frames: the scratch below is the queries' own.
// Radiance queries (crt_shoot_rays*: RayTracer::shootRay, RayTracer.cpp:419-451) are a host loop over those launches, one recursion
// level behind the other, with three small kernels of their own around them (csrc/kernel_radiance.h): at the end of this file.
#include "crt_internal.h"
#include "glibc_powf.h"

namespace {

// (the frame kernels of these headers are crt_launch.hip's: this file launches none of them)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "kernel_lane.h"
#include "kernel_stream.h"
#include "kernel_bvh.h"
#include "kernel_query.h"
#include "kernel_shade.h"
#include "kernel_radiance.h"
#pragma clang diagnostic pop

// rays per launch: indices, the cursor's overshoot (claimed and dropped) and the list's length stay well inside 31 bits
constexpr uint64_t QUERY_LAUNCH_RAYS = 1ull << 27;
// rays per round trip of the host variants (their device copies: 24 + 48 bytes a ray)
constexpr uint64_t QUERY_HOST_RAYS = 1ull << 22;
// radiance queries: the caller's rays per pass (every level of a pass has arrays of its own: 117 bytes a ray), and what a level may
// hold at most (a level is at most twice as wide as the one above it; indices and counts stay inside 31 bits)
constexpr uint64_t SHOOT_PASS_RAYS = 1ull << 22;
constexpr uint64_t SHOOT_LEVEL_RAYS = 1ull << 30;
// the radiance queries' own words (uint32 offsets): rays appended to level g at [g], the call's DIFFUSE records (64-bit) behind them
enum : int { SW_COUNT = 0, SW_DIFFUSE = MAX_GENERATIONS + 2, SW_WORDS = MAX_GENERATIONS + 4 };
// ... and what comes back through pinned memory (uint64 slots): a level's count, level 0's hits, the DIFFUSE records, the rerouted ones
enum : int { SH_COUNT = 0, SH_HITS0 = 1, SH_DIFFUSE = 2, SH_REROUTED = 3, SH_SLOTS = 4 };

// one recursion level of a radiance query: rays, their records, colours, status and nodes, `cap` of each
struct ShootLevel {
    crt_ray *rays = nullptr;
    crt_hit *hits = nullptr;
    float *rgb = nullptr;
    uint8_t *status = nullptr;
    float4 *nodes = nullptr;
    uint64_t cap = 0;
};

}  // namespace

struct crt_query_state {
    FrameArgs *d_frame = nullptr;     // an all-zero frame block: the reference-order walk reads use_gi (0: shadow rays skip refractive meshes)
    uint32_t *d_words = nullptr;      // QW_*
    uint32_t *h_words = nullptr;      // pinned: the words of the last call, copied behind its last launch
    uint32_t *d_list = nullptr;       // reroute list
    uint64_t list_cap = 0;
    uint32_t *d_spill = nullptr;      // walk-stack spill columns of the query grid (never FrameArgs::bvh_spill: a frame's kernels may run beside)
    crt_ray *d_rays = nullptr;        // device copies of the host variants' arrays
    float *d_dist = nullptr;
    crt_hit *d_hits = nullptr;
    uint8_t *d_occ = nullptr;
    uint64_t stage_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the launches of the last device call
    hipStream_t last_stream = nullptr;
    bool open = false;                // ... whose words and events have not been read yet
    crt_query_stats stats{};          // of the last call
    // radiance queries (crt_shoot_rays*)
    ShootLevel lv[MAX_GENERATIONS];
    crt_ray *d_shoot_in = nullptr;    // the host variant's device copy of the caller's rays
    uint64_t shoot_in_cap = 0;
    uint32_t *d_swords = nullptr;     // SW_*
    uint64_t *h_shoot = nullptr;      // pinned, SH_*
    hipEvent_t sev0 = nullptr, sev1 = nullptr;   // around the launches of the last radiance call
    bool shoot_open = false;          // ... whose last pass has not been read yet
    crt_shoot_stats shoot{};          // of the last radiance call
};

static void shoot_level_free(ShootLevel &L) {
    for (void *p : {(void *)L.rays, (void *)L.hits, (void *)L.rgb, (void *)L.status, (void *)L.nodes}) if (p) (void)hipFree(p);
    L = ShootLevel{};
}

void query_destroy(crt_ctx *ctx) {
    crt_query_state *q = ctx->query;
    if (!q) return;
    if (q->d_frame) (void)hipFree(q->d_frame);
    if (q->d_words) (void)hipFree(q->d_words);
    if (q->h_words) (void)hipHostFree(q->h_words);
    if (q->d_list) (void)hipFree(q->d_list);
    if (q->d_spill) (void)hipFree(q->d_spill);
    if (q->d_rays) (void)hipFree(q->d_rays);
    if (q->d_dist) (void)hipFree(q->d_dist);
    if (q->d_hits) (void)hipFree(q->d_hits);
    if (q->d_occ) (void)hipFree(q->d_occ);
    if (q->ev0) (void)hipEventDestroy(q->ev0);
    if (q->ev1) (void)hipEventDestroy(q->ev1);
    for (ShootLevel &L : q->lv) shoot_level_free(L);
    if (q->d_shoot_in) (void)hipFree(q->d_shoot_in);
    if (q->d_swords) (void)hipFree(q->d_swords);
    if (q->h_shoot) (void)hipHostFree(q->h_shoot);
    if (q->sev0) (void)hipEventDestroy(q->sev0);
    if (q->sev1) (void)hipEventDestroy(q->sev1);
    delete q;
    ctx->query = nullptr;
}

// the words and events of the last device call, once: waits for it
static void shoot_fold(crt_query_state *q);
static int query_harvest(crt_ctx *ctx) {
    crt_query_state *q = ctx->query;
    if (q && q->shoot_open) {   // a radiance call: its last pass's numbers, and what crt_get_query_stats says of it
        CRT_HIP_CHECK(ctx, hipEventSynchronize(q->sev1));
        q->shoot_open = false;
        float ms = 0;
        CRT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, q->sev0, q->sev1));
        q->shoot.kernel_ms = ms;
        shoot_fold(q);
        q->stats.rerouted = q->shoot.rerouted;
        q->stats.kernel_ms = q->shoot.kernel_ms;
    }
    if (!q || !q->open) return CRT_OK;
    CRT_HIP_CHECK(ctx, hipEventSynchronize(q->ev1));
    q->open = false;
    float ms = 0;
    CRT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, q->ev0, q->ev1));
    q->stats.kernel_ms += ms;
    memcpy(&q->stats.hits, q->h_words + QW_HITS, sizeof(uint64_t));          // (totals of the call: its launches add to the same words)
    memcpy(&q->stats.rerouted, q->h_words + QW_REROUTED, sizeof(uint64_t));
    return CRT_OK;
}

static bool uses_filter(const crt_ctx *ctx) { return ctx->scene.bvh_ok && ctx->tuning.bvh; }

// what every query needs, allocated by the first one; the list follows the largest launch asked for
static int query_prepare(crt_ctx *ctx, uint64_t launch_rays, hipStream_t stream) {
    if (ctx->pending) {   // a frame enqueued by crt_render_async: finish it first, as a second crt_render_async does
        int rc = crt_wait(ctx);
        if (rc) return rc;
    }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (!ctx->query) ctx->query = new (std::nothrow) crt_query_state;
    crt_query_state *q = ctx->query;
    if (!q) { ctx->error = "out of memory"; return CRT_ERR_NOMEM; }
    if (!q->d_words) {
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&q->d_frame, sizeof(FrameArgs)));
        CRT_HIP_CHECK(ctx, hipMemset(q->d_frame, 0, sizeof(FrameArgs)));
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&q->d_words, QW_WORDS * sizeof(uint32_t)));
        CRT_HIP_CHECK(ctx, hipHostMalloc((void **)&q->h_words, QW_WORDS * sizeof(uint32_t)));
        memset(q->h_words, 0, QW_WORDS * sizeof(uint32_t));
        // one region: every filter launch of a query (query_closest / query_occluded / query_direct, the levels of crt_shoot_rays* among
        // them) has at most grid_blocks workgroups and follows the previous one on ONE stream (query_prepare makes a call on another
        // stream, and a pending frame, wait first): no two of them run side by side
        if (ctx->bvh_spill_words())
            CRT_HIP_CHECK(ctx, hipMalloc((void **)&q->d_spill, ctx->bvh_spill_words() * sizeof(uint32_t)));
        CRT_HIP_CHECK(ctx, hipEventCreate(&q->ev0));
        CRT_HIP_CHECK(ctx, hipEventCreate(&q->ev1));
    }
    // the scratch is one call's at a time: a call on another stream waits for the previous call's last launch (and any call for a
    // radiance call before it: that one's statistics are read through the words this one is about to clear)
    if ((q->open && q->last_stream != stream) || q->shoot_open) {
        int rc = query_harvest(ctx);
        if (rc) return rc;
    }
    if (uses_filter(ctx) && launch_rays > q->list_cap) {
        CRT_HIP_CHECK(ctx, hipDeviceSynchronize());   // nothing may still be writing the old list
        if (q->d_list) (void)hipFree(q->d_list);
        q->d_list = nullptr;
        q->list_cap = 0;
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&q->d_list, launch_rays * sizeof(uint32_t)));
        q->list_cap = launch_rays;
    }
    return CRT_OK;
}

// the launches of n rays, at most QUERY_LAUNCH_RAYS at a time, on the scratch query_prepare has made; `clean`: the cursors and the list's
// length are zero already
static int query_launches(crt_ctx *ctx, bool occluded, const crt_ray *d_rays, const float *d_dist, uint64_t n, uint32_t ray_type, crt_hit *d_hits,
                          uint8_t *d_occ, hipStream_t stream, bool clean) {
    crt_query_state *q = ctx->query;
    KernelArgs A{};
    A.s = (scene_args_p)ctx->d_scene;
    A.f = (frame_args_p)q->d_frame;
    const bool filter = uses_filter(ctx);
    for (uint64_t done = 0; done < n; done += QUERY_LAUNCH_RAYS) {
        const uint32_t m = (uint32_t)std::min(n - done, QUERY_LAUNCH_RAYS);
        if (done || !clean) CRT_HIP_CHECK(ctx, hipMemsetAsync(q->d_words, 0, QW_HITS * sizeof(uint32_t), stream));   // cursors and list length; the totals stay
        QueryArgs Q{};
        Q.rays = d_rays + done;
        Q.max_distance = occluded ? d_dist + done : nullptr;
        Q.hits = occluded ? nullptr : d_hits + done;
        Q.occluded = occluded ? d_occ + done : nullptr;
        Q.n = m;
        Q.ray_type = ray_type;
        Q.words = q->d_words;
        Q.list = q->d_list;
        Q.spill = q->d_spill;
        Q.direct = filter ? 0u : 1u;
        Q.chunk = std::max(64u, (ctx->tuning.fetch_chunk >> 16) & ~63u);   // (level 0's claim size, crt_tuning::fetch_chunk)
        const uint32_t blocks = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(ctx->grid_blocks, ((uint64_t)m + BLOCK - 1) / BLOCK));
        if (filter) {
            if (occluded) hipLaunchKernelGGL(query_occluded<BVH_PLAIN>, dim3(blocks), dim3(BLOCK), 0, stream, A, Q);
            else hipLaunchKernelGGL(query_closest<BVH_PLAIN>, dim3(blocks), dim3(BLOCK), 0, stream, A, Q);
            CRT_HIP_CHECK(ctx, hipGetLastError());
        }
        // behind it, for what it listed (all but always nothing: the workgroups leave at once) -- or for every ray
        if (occluded) hipLaunchKernelGGL(query_reroute<true>, dim3(blocks), dim3(BLOCK), 0, stream, A, Q);
        else hipLaunchKernelGGL(query_reroute<false>, dim3(blocks), dim3(BLOCK), 0, stream, A, Q);
        CRT_HIP_CHECK(ctx, hipGetLastError());
    }
    return CRT_OK;
}

// one device call: n rays; `first`: the call's counters start at zero
static int query_run(crt_ctx *ctx, bool occluded, const crt_ray *d_rays, const float *d_dist, uint64_t n, uint32_t ray_type, crt_hit *d_hits,
                     uint8_t *d_occ, hipStream_t stream, bool first) {
    int rc = query_prepare(ctx, std::min(n, QUERY_LAUNCH_RAYS), stream);
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    // (a previous call still under way is on the same stream: this one is ordered behind it, and supersedes its statistics)
    if (first) {
        q->stats = crt_query_stats{};
        CRT_HIP_CHECK(ctx, hipMemsetAsync(q->d_words, 0, QW_WORDS * sizeof(uint32_t), stream));
    }
    q->stats.rays += n;
    CRT_HIP_CHECK(ctx, hipEventRecord(q->ev0, stream));
    rc = query_launches(ctx, occluded, d_rays, d_dist, n, ray_type, d_hits, d_occ, stream, first);
    if (rc) return rc;
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->h_words, q->d_words, QW_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipEventRecord(q->ev1, stream));
    q->last_stream = stream;
    q->open = true;
    return CRT_OK;
}

static int query_check(crt_ctx *ctx, const void *rays, const void *extra, const void *out, uint32_t ray_type, const char *what) {
    if (!rays || !extra || !out) { ctx->error = std::string(what) + ": NULL array with n > 0"; return CRT_ERR_INVALID; }
    if (ray_type > (uint32_t)CRT_RAY_REFRACTION) { ctx->error = std::string(what) + ": unknown ray_type " + std::to_string(ray_type); return CRT_ERR_INVALID; }
    return CRT_OK;
}

extern "C" int crt_trace_rays_device(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, crt_hit *d_out, void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = query_check(ctx, d_rays, d_rays, d_out, ray_type, "crt_trace_rays_device");
    if (rc) return rc;
    return query_run(ctx, false, d_rays, nullptr, n, ray_type, d_out, nullptr, (hipStream_t)stream, true);
}

extern "C" int crt_occluded_rays_device(crt_ctx *ctx, const crt_ray *d_rays, const float *d_max_distance, uint64_t n, uint8_t *d_out, void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = query_check(ctx, d_rays, d_max_distance, d_out, CRT_RAY_SHADOW, "crt_occluded_rays_device");
    if (rc) return rc;
    return query_run(ctx, true, d_rays, d_max_distance, n, CRT_RAY_SHADOW, nullptr, d_out, (hipStream_t)stream, true);
}

// the device copies of the host variants' arrays, kept for the next call: room for `cap` records
static int query_stage(crt_ctx *ctx, const uint64_t cap) {
    crt_query_state *q = ctx->query;
    if (cap > q->stage_cap) {
        CRT_HIP_CHECK(ctx, hipDeviceSynchronize());
        for (void *p : {(void *)q->d_rays, (void *)q->d_dist, (void *)q->d_hits, (void *)q->d_occ}) if (p) (void)hipFree(p);
        q->d_rays = nullptr; q->d_dist = nullptr; q->d_hits = nullptr; q->d_occ = nullptr;
        q->stage_cap = 0;
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&q->d_rays, cap * sizeof(crt_ray)));
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&q->d_dist, cap * sizeof(float)));
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&q->d_hits, cap * sizeof(crt_hit)));
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&q->d_occ, cap));
        q->stage_cap = cap;
    }
    return CRT_OK;
}

// the host variants: copy in, run, copy out, QUERY_HOST_RAYS at a time through device copies that are kept for the next call
static int query_host(crt_ctx *ctx, bool occluded, const crt_ray *rays, const float *dist, uint64_t n, uint32_t ray_type, crt_hit *hits, uint8_t *occ) {
    int rc = query_prepare(ctx, std::min(n, QUERY_HOST_RAYS), ctx->stream);
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    rc = query_stage(ctx, std::min(n, QUERY_HOST_RAYS));
    if (rc) return rc;
    for (uint64_t done = 0; done < n; done += QUERY_HOST_RAYS) {
        const uint64_t m = std::min(n - done, QUERY_HOST_RAYS);
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->d_rays, rays + done, m * sizeof(crt_ray), hipMemcpyHostToDevice, ctx->stream));
        if (occluded) CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->d_dist, dist + done, m * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        rc = query_run(ctx, occluded, q->d_rays, q->d_dist, m, ray_type, q->d_hits, q->d_occ, ctx->stream, done == 0);
        if (rc) return rc;
        if (occluded) CRT_HIP_CHECK(ctx, hipMemcpyAsync(occ + done, q->d_occ, m, hipMemcpyDeviceToHost, ctx->stream));
        else CRT_HIP_CHECK(ctx, hipMemcpyAsync(hits + done, q->d_hits, m * sizeof(crt_hit), hipMemcpyDeviceToHost, ctx->stream));
        CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        rc = query_harvest(ctx);
        if (rc) return rc;
    }
    return CRT_OK;
}

extern "C" int crt_trace_rays(crt_ctx *ctx, const crt_ray *rays, uint64_t n, uint32_t ray_type, crt_hit *out) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = query_check(ctx, rays, rays, out, ray_type, "crt_trace_rays");
    if (rc) return rc;
    return query_host(ctx, false, rays, nullptr, n, ray_type, out, nullptr);
}

extern "C" int crt_occluded_rays(crt_ctx *ctx, const crt_ray *rays, const float *max_distance, uint64_t n, uint8_t *out) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = query_check(ctx, rays, max_distance, out, CRT_RAY_SHADOW, "crt_occluded_rays");
    if (rc) return rc;
    return query_host(ctx, true, rays, max_distance, n, CRT_RAY_SHADOW, nullptr, out);
}

// ---- direct lighting (csrc/kernel_shade.h): n records in launches of at most QUERY_LAUNCH_RAYS, on the ray queries' scratch (words, list,
// spill columns); `points`: crt_light_points (d_a = points, d_b = normals), else crt_shade_hits (d_a = records); `clean`: as query_launches
static int shade_launches(crt_ctx *ctx, bool points, const void *d_a, const float *d_b, uint64_t n, float shadow_bias, float *d_out, uint8_t *d_status,
                          hipStream_t stream, bool clean) {
    crt_query_state *q = ctx->query;
    KernelArgs A{};
    A.s = (scene_args_p)ctx->d_scene;
    A.f = (frame_args_p)q->d_frame;   // all zero (use_gi = 0: shadow rays skip refractive meshes); the bias travels in ShadeArgs
    const bool filter = uses_filter(ctx);
    for (uint64_t done = 0; done < n; done += QUERY_LAUNCH_RAYS) {
        const uint32_t m = (uint32_t)std::min(n - done, QUERY_LAUNCH_RAYS);
        if (done || !clean) CRT_HIP_CHECK(ctx, hipMemsetAsync(q->d_words, 0, QW_HITS * sizeof(uint32_t), stream));   // cursors and list length; the totals stay
        ShadeArgs S{};
        S.q.n = m;
        S.q.words = q->d_words;
        S.q.list = q->d_list;
        S.q.spill = q->d_spill;
        S.q.direct = filter ? 0u : 1u;
        S.q.chunk = std::max(64u, (ctx->tuning.fetch_chunk >> 16) & ~63u);
        if (points) { S.points = (const float *)d_a + 3 * done; S.normals = d_b + 3 * done; S.out = d_out + done; }
        else { S.hits = (const crt_hit *)d_a + done; S.out = d_out + 3 * done; S.status = d_status ? d_status + done : nullptr; }
        S.shadow_bias = shadow_bias;
        const uint32_t blocks = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(ctx->grid_blocks, ((uint64_t)m + BLOCK - 1) / BLOCK));
        if (filter) {
            if (points) hipLaunchKernelGGL((query_direct<BVH_PLAIN, true>), dim3(blocks), dim3(BLOCK), 0, stream, A, S);
            else hipLaunchKernelGGL((query_direct<BVH_PLAIN, false>), dim3(blocks), dim3(BLOCK), 0, stream, A, S);
            CRT_HIP_CHECK(ctx, hipGetLastError());
        }
        // behind it, for the records it listed (all but always none) -- or for every record
        if (points) hipLaunchKernelGGL(query_direct_reroute<true>, dim3(blocks), dim3(BLOCK), 0, stream, A, S);
        else hipLaunchKernelGGL(query_direct_reroute<false>, dim3(blocks), dim3(BLOCK), 0, stream, A, S);
        CRT_HIP_CHECK(ctx, hipGetLastError());
    }
    return CRT_OK;
}

// one device call
static int shade_run(crt_ctx *ctx, bool points, const void *d_a, const float *d_b, uint64_t n, float shadow_bias, float *d_out, uint8_t *d_status,
                     hipStream_t stream, bool first) {
    int rc = query_prepare(ctx, std::min(n, QUERY_LAUNCH_RAYS), stream);
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    if (first) {
        q->stats = crt_query_stats{};
        CRT_HIP_CHECK(ctx, hipMemsetAsync(q->d_words, 0, QW_WORDS * sizeof(uint32_t), stream));
    }
    q->stats.rays += n;
    CRT_HIP_CHECK(ctx, hipEventRecord(q->ev0, stream));
    rc = shade_launches(ctx, points, d_a, d_b, n, shadow_bias, d_out, d_status, stream, first);
    if (rc) return rc;
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->h_words, q->d_words, QW_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipEventRecord(q->ev1, stream));
    q->last_stream = stream;
    q->open = true;
    return CRT_OK;
}

static int shade_check(crt_ctx *ctx, const void *a, const void *b, const void *out, const crt_options *options, const char *what) {
    if (!a || !b || !out) { ctx->error = std::string(what) + ": NULL array with n > 0"; return CRT_ERR_INVALID; }
    if (options && options->use_gi) {
        ctx->error = std::string(what) + ": use_gi is not offered (the GI build's occlusion rule and its division by GI_SAMPLE_SIZE + 1)";
        return CRT_ERR_INVALID;
    }
    return CRT_OK;
}

extern "C" int crt_shade_hits_device(crt_ctx *ctx, const crt_hit *d_hits, uint64_t n, const crt_options *options, float *d_rgb, uint8_t *d_status,
                                     void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shade_check(ctx, d_hits, options, d_rgb, options, "crt_shade_hits_device");
    if (rc) return rc;
    return shade_run(ctx, false, d_hits, nullptr, n, options->shadow_bias, d_rgb, d_status, (hipStream_t)stream, true);
}

extern "C" int crt_light_points_device(crt_ctx *ctx, const float *d_points, const float *d_normals, uint64_t n, float shadow_bias, float *d_out,
                                       void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shade_check(ctx, d_points, d_normals, d_out, nullptr, "crt_light_points_device");
    if (rc) return rc;
    return shade_run(ctx, true, d_points, d_normals, n, shadow_bias, d_out, nullptr, (hipStream_t)stream, true);
}

// The host variants, QUERY_HOST_RAYS at a time, through the ray queries' device copies: a record's 48 bytes in d_hits, its colour (12
// bytes) in d_rays (24 a record), its status in d_occ; a point and its normal (12 + 12 bytes) in the two halves of d_rays, its sum in d_dist
static int shade_host(crt_ctx *ctx, bool points, const void *a, const float *b, uint64_t n, float shadow_bias, float *out, uint8_t *status) {
    int rc = query_prepare(ctx, std::min(n, QUERY_HOST_RAYS), ctx->stream);
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    rc = query_stage(ctx, std::min(n, QUERY_HOST_RAYS));
    if (rc) return rc;
    float *d_lo = reinterpret_cast<float *>(q->d_rays), *d_hi = d_lo + 3 * q->stage_cap;
    for (uint64_t done = 0; done < n; done += QUERY_HOST_RAYS) {
        const uint64_t m = std::min(n - done, QUERY_HOST_RAYS);
        if (points) {
            CRT_HIP_CHECK(ctx, hipMemcpyAsync(d_lo, (const float *)a + 3 * done, m * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            CRT_HIP_CHECK(ctx, hipMemcpyAsync(d_hi, b + 3 * done, m * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            rc = shade_run(ctx, true, d_lo, d_hi, m, shadow_bias, q->d_dist, nullptr, ctx->stream, done == 0);
            if (rc) return rc;
            CRT_HIP_CHECK(ctx, hipMemcpyAsync(out + done, q->d_dist, m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        } else {
            CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->d_hits, (const crt_hit *)a + done, m * sizeof(crt_hit), hipMemcpyHostToDevice, ctx->stream));
            rc = shade_run(ctx, false, q->d_hits, nullptr, m, shadow_bias, d_lo, q->d_occ, ctx->stream, done == 0);
            if (rc) return rc;
            CRT_HIP_CHECK(ctx, hipMemcpyAsync(out + 3 * done, d_lo, m * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
            if (status) CRT_HIP_CHECK(ctx, hipMemcpyAsync(status + done, q->d_occ, m, hipMemcpyDeviceToHost, ctx->stream));
        }
        CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        rc = query_harvest(ctx);
        if (rc) return rc;
    }
    return CRT_OK;
}

extern "C" int crt_shade_hits(crt_ctx *ctx, const crt_hit *hits, uint64_t n, const crt_options *options, float *out_rgb, uint8_t *out_status) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shade_check(ctx, hits, options, out_rgb, options, "crt_shade_hits");
    if (rc) return rc;
    return shade_host(ctx, false, hits, nullptr, n, options->shadow_bias, out_rgb, out_status);
}

extern "C" int crt_light_points(crt_ctx *ctx, const float *points, const float *normals, uint64_t n, float shadow_bias, float *out) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shade_check(ctx, points, normals, out, nullptr, "crt_light_points");
    if (rc) return rc;
    return shade_host(ctx, true, points, normals, n, shadow_bias, out, nullptr);
}

extern "C" int crt_camera_rays_device(crt_ctx *ctx, crt_ray *d_rays, void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (!d_rays) { ctx->error = "crt_camera_rays_device: d_rays is NULL"; return CRT_ERR_INVALID; }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    QueryCamera cam;
    memcpy(cam.pos, ctx->frame.cam_pos, sizeof(cam.pos));   // the camera of the NEXT frame: crt_set_camera's last word
    memcpy(cam.m, ctx->frame.cam, sizeof(cam.m));
    cam.width = ctx->width; cam.height = ctx->height;
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    if (pixels == 0) return CRT_OK;
    hipLaunchKernelGGL(query_camera_rays, dim3((uint32_t)((pixels + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, cam, d_rays);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

extern "C" int crt_get_query_stats(crt_ctx *ctx, crt_query_stats *out) {
    if (!ctx || !out) return CRT_ERR_INVALID;
    if (!ctx->query) { *out = crt_query_stats{}; return CRT_OK; }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int rc = query_harvest(ctx);
    if (rc) return rc;
    *out = ctx->query->stats;
    return CRT_OK;
}

// ---- radiance queries (csrc/kernel_radiance.h): RayTracer::shootRay for the caller's rays, level-synchronous.  For level g = 0 ..
// max_depth: trace the level's rays (query_launches), light their records (shade_launches: background, constant and diffuse records are
// final), radiance_scatter the recursing ones into level g + 1, read that level's size back -- the one wait of a level --; then
// radiance_combine from the deepest level up.  Level 0's colours are the caller's array.

// the pass's numbers, once its last copy has arrived
static void shoot_fold(crt_query_state *q) {
    q->stats.hits += q->h_shoot[SH_HITS0];
    q->shoot.shadow_records += q->h_shoot[SH_DIFFUSE];
    q->shoot.rerouted += q->h_shoot[SH_REROUTED];
}

// room for `cap` rays at level g (`own_rgb`: with colours of its own; level 0 writes the caller's array)
static int shoot_level_reserve(crt_ctx *ctx, const uint32_t g, const uint64_t cap, const bool own_rgb) {
    ShootLevel &L = ctx->query->lv[g];
    if (cap <= L.cap && (L.rgb || !own_rgb)) return CRT_OK;
    const uint64_t want = std::max(cap, L.cap);
    CRT_HIP_CHECK(ctx, hipDeviceSynchronize());   // nothing may still be using the old arrays
    shoot_level_free(L);
    CRT_HIP_CHECK(ctx, hipMalloc((void **)&L.rays, want * sizeof(crt_ray)));
    CRT_HIP_CHECK(ctx, hipMalloc((void **)&L.hits, want * sizeof(crt_hit)));
    CRT_HIP_CHECK(ctx, hipMalloc((void **)&L.status, want));
    CRT_HIP_CHECK(ctx, hipMalloc((void **)&L.nodes, want * 2 * sizeof(float4)));
    if (own_rgb) CRT_HIP_CHECK(ctx, hipMalloc((void **)&L.rgb, want * 3 * sizeof(float)));
    L.cap = want;
    return CRT_OK;
}

// one pass: m <= SHOOT_PASS_RAYS rays of the caller's, every level of them; leaves the pass's numbers on their way to h_shoot
static int shoot_pass(crt_ctx *ctx, const crt_ray *d_rays, const uint32_t m, const uint32_t ray_type, const crt_options *o, float *d_rgb,
                      hipStream_t stream) {
    crt_query_state *q = ctx->query;
    KernelArgs A{};
    A.s = (scene_args_p)ctx->d_scene;
    A.f = (frame_args_p)q->d_frame;
    CRT_HIP_CHECK(ctx, hipMemsetAsync(q->d_words, 0, QW_WORDS * sizeof(uint32_t), stream));
    CRT_HIP_CHECK(ctx, hipMemsetAsync(q->d_swords, 0, SW_WORDS * sizeof(uint32_t), stream));
    uint32_t count[MAX_GENERATIONS + 1] = {m};
    uint32_t last = 0;
    for (uint32_t g = 0; g <= o->max_depth; g++) {
        const uint32_t n = count[g];
        last = g;
        int rc = query_prepare(ctx, n, stream);   // (the reroute list follows the widest level)
        if (rc) return rc;
        rc = shoot_level_reserve(ctx, g, n, g > 0);
        if (rc) return rc;
        const ShootLevel &L = q->lv[g];
        float *rgb = g == 0 ? d_rgb : L.rgb;
        const uint32_t blocks = (uint32_t)(((uint64_t)n + BLOCK - 1) / BLOCK);
        RadianceArgs G{};
        G.in_rays = d_rays; G.rays = L.rays; G.hits = L.hits; G.status = L.status; G.rgb = rgb; G.nodes = L.nodes; G.n = n;
        G.diffuse_total = reinterpret_cast<unsigned long long *>(q->d_swords + SW_DIFFUSE);
        G.reflection_bias = o->reflection_bias; G.refraction_bias = o->refraction_bias;
        if (g == 0) {
            hipLaunchKernelGGL(radiance_prepare, dim3(blocks), dim3(BLOCK), 0, stream, G);
            CRT_HIP_CHECK(ctx, hipGetLastError());
        }
        // children are REFLECTION or REFRACTION rays, which walk alike: only the caller's own ray can be PRIMARY (Ray.cpp:13)
        rc = query_launches(ctx, false, L.rays, nullptr, n, g == 0 ? ray_type : (uint32_t)CRT_RAY_REFLECTION, L.hits, nullptr, stream, g == 0);
        if (rc) return rc;
        if (g == 0) CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->h_shoot + SH_HITS0, q->d_words + QW_HITS, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        rc = shade_launches(ctx, false, L.hits, nullptr, n, o->shadow_bias, rgb, L.status, stream, false);
        if (rc) return rc;
        // the next level holds at most two rays for each of this one: room for that BEFORE the launch that fills it
        const bool spawn = g + 1 <= o->max_depth;   // a child enters shootRay with depth g + 1 (RayTracer.cpp:427)
        if (spawn) {
            if (2ull * n > SHOOT_LEVEL_RAYS) { ctx->error = "crt_shoot_rays: a recursion level wider than 2^30 rays"; return CRT_ERR_NOMEM; }
            rc = shoot_level_reserve(ctx, g + 1, 2ull * n, true);
            if (rc) return rc;
            G.child_rays = q->lv[g + 1].rays;
            G.child_cap = (uint32_t)std::min<uint64_t>(q->lv[g + 1].cap, SHOOT_LEVEL_RAYS);
        }
        G.child_count = q->d_swords + SW_COUNT + g + 1;
        G.spawn = spawn ? 1u : 0u;
        hipLaunchKernelGGL(radiance_scatter, dim3(blocks), dim3(BLOCK), 0, stream, A, G);
        CRT_HIP_CHECK(ctx, hipGetLastError());
        if (!spawn) break;
        // the one wait of a level: four bytes through pinned memory, to size the next one
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->h_shoot + SH_COUNT, G.child_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));
        count[g + 1] = (uint32_t)std::min<uint64_t>(*reinterpret_cast<const uint32_t *>(q->h_shoot + SH_COUNT), 2ull * n);
        if (count[g + 1] == 0) break;
    }
    for (uint32_t g = 0; g <= last; g++) q->shoot.level_rays[g] += count[g];
    q->shoot.levels = std::max(q->shoot.levels, last + 1);
    // the up-sweep: level g's recursing records from level g + 1's colours, which are final by then
    for (uint32_t g = last + 1; g-- > 0;) {
        const ShootLevel &L = q->lv[g];
        RadianceArgs G{};
        G.status = L.status; G.nodes = L.nodes; G.rgb = g == 0 ? d_rgb : L.rgb; G.n = count[g];
        G.child_rgb = g < last ? q->lv[g + 1].rgb : nullptr;
        G.child_n = g < last ? count[g + 1] : 0u;
        hipLaunchKernelGGL(radiance_combine, dim3((uint32_t)(((uint64_t)count[g] + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, A, G);
        CRT_HIP_CHECK(ctx, hipGetLastError());
    }
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->h_shoot + SH_DIFFUSE, q->d_swords + SW_DIFFUSE, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->h_shoot + SH_REROUTED, q->d_words + QW_REROUTED, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    return CRT_OK;
}

static int shoot_check(crt_ctx *ctx, const void *rays, const crt_options *options, const void *out, uint32_t ray_type, const char *what) {
    if (!rays || !options || !out) { ctx->error = std::string(what) + ": NULL array or options with n > 0"; return CRT_ERR_INVALID; }
    if (ray_type > (uint32_t)CRT_RAY_REFRACTION) { ctx->error = std::string(what) + ": unknown ray_type " + std::to_string(ray_type); return CRT_ERR_INVALID; }
    if (options->use_gi) {
        ctx->error = std::string(what) + ": use_gi is not offered (the GI build's random sample rays, its occlusion rule and its division by GI_SAMPLE_SIZE + 1)";
        return CRT_ERR_INVALID;
    }
    if ((uint64_t)options->max_depth + 1 > (uint64_t)MAX_GENERATIONS) {   // (a frame's rule: crt_launch.hip)
        ctx->error = std::string(what) + ": max_depth too large: " + std::to_string(options->max_depth) + " + 1 levels, at most " + std::to_string(MAX_GENERATIONS);
        return CRT_ERR_INVALID;
    }
    return CRT_OK;
}

static int shoot_run(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *d_rgb, hipStream_t stream) {
    int rc = query_prepare(ctx, std::min(n, SHOOT_PASS_RAYS), stream);   // (waits for a pending frame, and for the previous query on another stream)
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    if (q->open) {   // a ray or lighting query before this one, on this stream: its words are about to be cleared
        rc = query_harvest(ctx);
        if (rc) return rc;
    }
    if (!q->d_swords) {
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&q->d_swords, SW_WORDS * sizeof(uint32_t)));
        CRT_HIP_CHECK(ctx, hipHostMalloc((void **)&q->h_shoot, SH_SLOTS * sizeof(uint64_t)));
        memset(q->h_shoot, 0, SH_SLOTS * sizeof(uint64_t));
        CRT_HIP_CHECK(ctx, hipEventCreate(&q->sev0));
        CRT_HIP_CHECK(ctx, hipEventCreate(&q->sev1));
    }
    q->stats = crt_query_stats{};
    q->stats.rays = n;
    q->shoot = crt_shoot_stats{};
    q->shoot.rays = n;
    CRT_HIP_CHECK(ctx, hipEventRecord(q->sev0, stream));
    for (uint64_t done = 0; done < n; done += SHOOT_PASS_RAYS) {
        if (done) {   // the previous pass's numbers leave the pinned slots before this pass writes them
            CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));
            shoot_fold(q);
        }
        rc = shoot_pass(ctx, d_rays + done, (uint32_t)std::min(n - done, SHOOT_PASS_RAYS), ray_type, options, d_rgb + 3 * done, stream);
        if (rc) return rc;
    }
    CRT_HIP_CHECK(ctx, hipEventRecord(q->sev1, stream));
    q->last_stream = stream;
    q->shoot_open = true;
    return CRT_OK;
}

extern "C" int crt_shoot_rays_device(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *d_rgb,
                                     void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shoot_check(ctx, d_rays, options, d_rgb, ray_type, "crt_shoot_rays_device");
    if (rc) return rc;
    return shoot_run(ctx, d_rays, n, ray_type, options, d_rgb, (hipStream_t)stream);
}

// the host variant: copy in, run, copy out, SHOOT_PASS_RAYS at a time; the colours' device copy is level 0's own colour array
extern "C" int crt_shoot_rays(crt_ctx *ctx, const crt_ray *rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *out_rgb) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shoot_check(ctx, rays, options, out_rgb, ray_type, "crt_shoot_rays");
    if (rc) return rc;
    const uint64_t m = std::min(n, SHOOT_PASS_RAYS);
    rc = query_prepare(ctx, m, ctx->stream);
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    rc = shoot_level_reserve(ctx, 0, m, true);
    if (rc) return rc;
    if (m > q->shoot_in_cap) {
        CRT_HIP_CHECK(ctx, hipDeviceSynchronize());
        if (q->d_shoot_in) (void)hipFree(q->d_shoot_in);
        q->d_shoot_in = nullptr;
        q->shoot_in_cap = 0;
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&q->d_shoot_in, m * sizeof(crt_ray)));
        q->shoot_in_cap = m;
    }
    crt_shoot_stats total{};
    crt_query_stats qtotal{};
    for (uint64_t done = 0; done < n; done += SHOOT_PASS_RAYS) {
        const uint64_t k = std::min(n - done, SHOOT_PASS_RAYS);
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->d_shoot_in, rays + done, k * sizeof(crt_ray), hipMemcpyHostToDevice, ctx->stream));
        rc = shoot_run(ctx, q->d_shoot_in, k, ray_type, options, q->lv[0].rgb, ctx->stream);
        if (rc) return rc;
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb + 3 * done, q->lv[0].rgb, k * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        rc = query_harvest(ctx);
        if (rc) return rc;
        // the call's statistics are the sum of its passes'
        total.rays += q->shoot.rays; total.levels = std::max(total.levels, q->shoot.levels);
        for (int g = 0; g < MAX_GENERATIONS; g++) total.level_rays[g] += q->shoot.level_rays[g];
        total.shadow_records += q->shoot.shadow_records; total.rerouted += q->shoot.rerouted; total.kernel_ms += q->shoot.kernel_ms;
        qtotal.rays += q->stats.rays; qtotal.hits += q->stats.hits; qtotal.rerouted += q->stats.rerouted; qtotal.kernel_ms += q->stats.kernel_ms;
    }
    q->shoot = total;
    q->stats = qtotal;
    return CRT_OK;
}

extern "C" int crt_get_shoot_stats(crt_ctx *ctx, crt_shoot_stats *out) {
    if (!ctx || !out) return CRT_ERR_INVALID;
    if (!ctx->query) { *out = crt_shoot_stats{}; return CRT_OK; }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int rc = query_harvest(ctx);
    if (rc) return rc;
    *out = ctx->query->shoot;
    return CRT_OK;
}
