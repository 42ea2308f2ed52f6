// crt_query.hip -- the queries for what the CALLER supplies (include/crt_hip.h), behind one call path:
//   ray queries        crt_trace_rays*, crt_occluded_rays*, crt_camera_rays_device: closest hit and occlusion, in place of
//                      AccelerationStructure::intersect (KDTree.cpp:127-192) and AccelerationStructure::checkForIntersection
//                      (AccelerationStructure.cpp:56-94) as entry points of their own; kernels: csrc/kernel_query.h
//   direct lighting    crt_shade_hits*, crt_light_points*: RayTracer::calculateDiffusion (RayTracer.cpp:300-330) for the caller's hit
//                      records and points; kernels: csrc/kernel_shade.h
//   radiance queries   crt_shoot_rays*: RayTracer::shootRay (RayTracer.cpp:419-451), a host loop over the launches of the other two, one
//                      recursion level behind the other, with three small kernels of its own around them (csrc/kernel_radiance.h): at
//                      the end of this file; crt_shoot_rays_gi*: the same loop for the GI build (a key per ray, sample rays at DIFFUSE
//                      records, no mesh skipped by a shadow ray)
// and their statistics (crt_get_query_stats, crt_get_shoot_stats).  A query reads the context's scene and nothing of its frames: the
// scratch below is the queries' own.
#include "crt_internal.h"
#include "glibc_powf.h"
#include "gi_random.h"
#include "shoot_caps.h"

static void query_scratch_changed(crt_ctx *ctx);   // (below crt_query_state)

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

// radiance queries: what a level may hold at most is SHOOT_LEVEL_RAYS (shoot_caps.h: a level is at most twice as wide as the one above
// it; indices and counts stay inside 31 bits)
// ... and in the GI mode, where a level is up to max(2, gi_sample_size) times as wide as the one above it: what the DEEPEST level of one
// pass may hold in the worst case (every ray of every level a DIFFUSE hit); about 8 GB of level arrays.  A call's pass size follows it.
constexpr uint64_t SHOOT_GI_DEEPEST_RAYS = 1ull << 26;
// the radiance queries' own words (uint32 offsets): rays appended to level g at [g], the call's DIFFUSE records (64-bit) behind them
enum : int { SW_COUNT = 0, SW_DIFFUSE = MAX_GENERATIONS + 2, SW_WORDS = MAX_GENERATIONS + 4 };
// ... and what comes back through pinned memory (uint64 slots): a level's count, level 0's hits, the DIFFUSE records, the rerouted ones
enum : int { SH_COUNT = 0, SH_HITS0 = 1, SH_DIFFUSE = 2, SH_REROUTED = 3, SH_SLOTS = 4 };

// A device array that only grows and is kept for the next call; freed with its owner.
template <typename T>
struct DeviceArray {
    T *p = nullptr;
    uint64_t cap = 0;
    DeviceArray() = default;
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
    ~DeviceArray() { release(); }
    int reserve(crt_ctx *ctx, const uint64_t n) {
        if (n <= cap) return CRT_OK;
        if (p) CRT_HIP_CHECK(ctx, hipDeviceSynchronize());   // nothing may still be using the old array
        release();
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&p, n * sizeof(T)));
        cap = n;
        query_scratch_changed(ctx);   // a graph captured from an enqueue call holds the old pointer (crt_query_scratch_generation)
        return CRT_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// one recursion level of a radiance query: rays, their records, colours (level 0 writes the caller's array), status and nodes
struct ShootLevel {
    DeviceArray<crt_ray> rays;
    DeviceArray<crt_hit> hits;
    DeviceArray<float> rgb;        // 3 a ray
    DeviceArray<uint8_t> status;
    DeviceArray<float4> nodes;     // 2 a ray
    DeviceArray<uint32_t> keys;    // crt_shoot_rays_gi*: the key of each ray's shootRay invocation (gi_random.h)
};

// One call of the ray or lighting queries: which filter / reroute kernel pair answers it, and the arrays of its n rays or records (the
// caller's, or the host variants' device copies).
enum QueryKind { Q_CLOSEST, Q_OCCLUDED, Q_SHADE_HITS, Q_LIGHT_POINTS };
struct QueryCall {
    QueryKind kind;
    uint64_t n;
    const crt_ray *rays;          // Q_CLOSEST, Q_OCCLUDED
    const float *max_distance;    // Q_OCCLUDED
    crt_hit *hits;                // Q_CLOSEST: the answer
    uint8_t *occluded;            // Q_OCCLUDED: the answer
    const crt_hit *records;       // Q_SHADE_HITS
    const float *points, *normals;   // Q_LIGHT_POINTS: 3 floats a record each
    float *out;                   // Q_SHADE_HITS: 3 floats a record, Q_LIGHT_POINTS: one
    uint8_t *status;              // Q_SHADE_HITS, or null
    uint32_t ray_type;
    float shadow_bias;
    bool every_mesh;              // Q_SHADE_HITS: the GI build's occlusion rule (the levels of crt_shoot_rays_gi*)
    // a level of crt_shoot_rays*_enqueue (Q_CLOSEST, Q_SHADE_HITS): n is the level's CAPACITY, and the kernels read how many rays it
    // holds from this device word (null: n rays); record `count_first` of the level is the first of this call's arrays
    const uint32_t *d_count;
    uint32_t count_first;
    bool kernels_only;            // an enqueue call: the words are cleared by query_reset, not by hipMemsetAsync (level 0 as well)
};
QueryCall closest_call(const crt_ray *rays, uint64_t n, uint32_t ray_type, crt_hit *hits) {
    QueryCall c{};
    c.kind = Q_CLOSEST; c.n = n; c.rays = rays; c.ray_type = ray_type; c.hits = hits;
    return c;
}
QueryCall occluded_call(const crt_ray *rays, const float *max_distance, uint64_t n, uint8_t *occluded) {
    QueryCall c{};
    c.kind = Q_OCCLUDED; c.n = n; c.rays = rays; c.max_distance = max_distance; c.ray_type = CRT_RAY_SHADOW; c.occluded = occluded;
    return c;
}
QueryCall shade_call(const crt_hit *records, uint64_t n, float shadow_bias, float *rgb, uint8_t *status, bool every_mesh = false) {
    QueryCall c{};
    c.kind = Q_SHADE_HITS; c.n = n; c.records = records; c.shadow_bias = shadow_bias; c.out = rgb; c.status = status; c.every_mesh = every_mesh;
    return c;
}
QueryCall points_call(const float *points, const float *normals, uint64_t n, float shadow_bias, float *sums) {
    QueryCall c{};
    c.kind = Q_LIGHT_POINTS; c.n = n; c.points = points; c.normals = normals; c.shadow_bias = shadow_bias; c.out = sums;
    return c;
}
// records [first, first + m) of a call
QueryCall call_part(QueryCall c, const uint64_t first, const uint64_t m) {
    c.n = m;
    if (c.rays) c.rays += first;
    if (c.max_distance) c.max_distance += first;
    if (c.hits) c.hits += first;
    if (c.occluded) c.occluded += first;
    if (c.records) c.records += first;
    if (c.points) c.points += 3 * first;
    if (c.normals) c.normals += 3 * first;
    if (c.out) c.out += (c.kind == Q_LIGHT_POINTS ? 1 : 3) * first;
    if (c.status) c.status += first;
    c.count_first += (uint32_t)first;   // (a level holds at most 2^30 rays)
    return c;
}

// The call still under way: a device call returns with its launches enqueued, and its words and events are read later, once
// (query_harvest).  The scratch is one call's at a time, so before a call starts (query_begin):
//   * a frame enqueued by crt_render_async is waited for, as a second crt_render_async does;
//   * a call on ANOTHER stream waits for the open call's last launch (one on the same stream is ordered behind it, and supersedes its
//     statistics);
//   * any call after a radiance call waits for it: that one's statistics are read through the words this one is about to clear;
//   * a radiance call after any call harvests that one first, for the same reason.
struct OpenCall {
    bool open = false, radiance = false;
    bool enqueue = false;   // a radiance call of the enqueue kind: its numbers are the report's (h_report), not h_shoot's
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around its launches
};

}  // namespace

struct crt_query_state {
    DeviceArray<FrameArgs> frame;     // two frame blocks, all zero but for use_gi = 1 in the second: the reference-order walk reads use_gi
                                      // (0: shadow rays skip refractive meshes; 1, the levels of crt_shoot_rays_gi*: they skip none)
    DeviceArray<uint32_t> words;      // QW_*
    uint32_t *h_words = nullptr;      // pinned: the words of the last call, copied behind its last launch
    DeviceArray<uint32_t> list;       // reroute list: follows the largest launch asked for
    DeviceArray<uint32_t> spill;      // walk-stack spill columns of the query grid (never FrameArgs::bvh_spill: a frame's kernels may run beside)
    OpenCall call;
    crt_query_stats stats{};          // of the last call
    // device copies of the host variants' arrays, each family's reserved by its first call
    DeviceArray<crt_ray> s_rays;      // ray queries
    DeviceArray<float> s_dist;
    DeviceArray<crt_hit> s_hits;
    DeviceArray<uint8_t> s_occ;
    DeviceArray<crt_hit> s_records;   // crt_shade_hits
    DeviceArray<float> s_rgb;
    DeviceArray<uint8_t> s_status;
    DeviceArray<float> s_points, s_normals, s_sums;   // crt_light_points
    // radiance queries (crt_shoot_rays*)
    ShootLevel lv[MAX_GENERATIONS];
    DeviceArray<crt_ray> shoot_in;    // the host variant's device copy of the caller's rays
    DeviceArray<uint32_t> shoot_keys; // ... and of the caller's keys (crt_shoot_rays_gi)
    DeviceArray<uint32_t> swords;     // SW_*
    uint64_t *h_shoot = nullptr;      // pinned, SH_*
    crt_shoot_stats shoot{};          // of the last radiance call
    // crt_shoot_rays*_enqueue
    DeviceArray<crt_shoot_report> d_report;   // what radiance_report writes for the library's own statistics (outside a capture)
    DeviceArray<unsigned long long> d_hits0;  // level 0's hits: QW_HITS as the level's trace left it (the lighting launches add to that word)
    crt_shoot_report *h_report = nullptr;     // pinned: d_report, copied behind the last launch
    crt_shoot_report report{};                // of the last enqueue call outside a capture
    uint64_t generation = 0;                  // crt_query_scratch_generation
    ~crt_query_state() {
        if (h_words) (void)hipHostFree(h_words);
        if (h_shoot) (void)hipHostFree(h_shoot);
        if (h_report) (void)hipHostFree(h_report);
        if (call.ev0) (void)hipEventDestroy(call.ev0);
        if (call.ev1) (void)hipEventDestroy(call.ev1);
    }
};

static void query_scratch_changed(crt_ctx *ctx) {
    if (ctx->query) ctx->query->generation++;
}

void query_destroy(crt_ctx *ctx) {
    delete ctx->query;
    ctx->query = nullptr;
}

// a radiance pass's numbers, once its last copy has arrived
static void shoot_fold(crt_query_state *q) {
    q->stats.hits += q->h_shoot[SH_HITS0];
    q->shoot.shadow_records += q->h_shoot[SH_DIFFUSE];
    q->shoot.rerouted += q->h_shoot[SH_REROUTED];
}

// the words and events of the open call, once: waits for it
static int query_harvest(crt_ctx *ctx) {
    crt_query_state *q = ctx->query;
    if (!q || !q->call.open) return CRT_OK;
    CRT_HIP_CHECK(ctx, hipEventSynchronize(q->call.ev1));
    q->call.open = false;
    float ms = 0;
    CRT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, q->call.ev0, q->call.ev1));
    if (q->call.radiance) {   // its last pass's numbers, and what crt_get_query_stats says of it
        q->shoot.kernel_ms = ms;
        if (q->call.enqueue) {   // (one pass, and the device has done the sums)
            q->report = *q->h_report;
            q->shoot.levels = q->report.levels;
            memcpy(q->shoot.level_rays, q->report.level_rays, sizeof(q->shoot.level_rays));
            q->shoot.shadow_records = q->report.shadow_records;
            q->shoot.rerouted = q->report.rerouted;
            q->stats.hits = q->report.hits;
        } else shoot_fold(q);
        q->stats.rerouted = q->shoot.rerouted;
        q->stats.kernel_ms = q->shoot.kernel_ms;
    } else {
        q->stats.kernel_ms += ms;
        memcpy(&q->stats.hits, q->h_words + QW_HITS, sizeof(uint64_t));          // (totals of the call: its launches add to the same words)
        memcpy(&q->stats.rerouted, q->h_words + QW_REROUTED, sizeof(uint64_t));
    }
    return CRT_OK;
}

static bool uses_filter(const crt_ctx *ctx) { return ctx->scene.bvh_ok && ctx->tuning.bvh; }

// before a call on `stream`: the waiting rules (OpenCall), and what every query needs, allocated by the first one
static int query_begin(crt_ctx *ctx, hipStream_t stream, bool radiance, bool enqueue = false) {
    if (ctx->pending) {
        int rc = crt_wait(ctx);
        if (rc) return rc;
    }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (!ctx->query) ctx->query = new (std::nothrow) crt_query_state;
    crt_query_state *q = ctx->query;
    if (!q) { ctx->error = "out of memory"; return CRT_ERR_NOMEM; }
    if (!q->h_words) {
        int rc;
        if ((rc = q->frame.reserve(ctx, 2)) || (rc = q->words.reserve(ctx, QW_WORDS))) return rc;
        CRT_HIP_CHECK(ctx, hipMemset(q->frame.p, 0, 2 * sizeof(FrameArgs)));
        const uint32_t one = 1u;
        CRT_HIP_CHECK(ctx, hipMemcpy(&q->frame.p[1].use_gi, &one, sizeof(one), hipMemcpyHostToDevice));
        // one region: every filter launch of a query (query_walk / query_direct, the levels of crt_shoot_rays* among them) has at most
        // grid_blocks workgroups and follows the previous one on ONE stream (a call on another stream, and a pending frame, are waited
        // for first): no two of them run side by side
        if ((rc = q->spill.reserve(ctx, ctx->bvh_spill_words()))) return rc;
        if (!q->call.ev0) CRT_HIP_CHECK(ctx, hipEventCreate(&q->call.ev0));
        if (!q->call.ev1) CRT_HIP_CHECK(ctx, hipEventCreate(&q->call.ev1));
        CRT_HIP_CHECK(ctx, hipHostMalloc((void **)&q->h_words, QW_WORDS * sizeof(uint32_t)));
        memset(q->h_words, 0, QW_WORDS * sizeof(uint32_t));
    }
    // (an enqueue call behind an enqueue call on the same stream is ordered behind it and supersedes its statistics, which come through
    // a report of their own, not through the words: no wait)
    if (q->call.open && enqueue && q->call.radiance && q->call.enqueue && q->call.stream == stream) return CRT_OK;
    if (q->call.open && (q->call.stream != stream || q->call.radiance || radiance)) return query_harvest(ctx);
    return CRT_OK;
}

// room in the reroute list for the largest launch of n rays or records: before the call's first event, so that growing it is no part of kernel_ms
static int query_list_reserve(crt_ctx *ctx, const uint64_t n) {
    return uses_filter(ctx) ? ctx->query->list.reserve(ctx, std::min(n, ctx->query_launch_rays)) : CRT_OK;
}

// query_reset (kernel_query.h): dst = src, then a[0 .. na) = b[0 .. nb) = 0
static void launch_reset(uint32_t *a, uint32_t na, uint32_t *b, uint32_t nb, const unsigned long long *src, unsigned long long *dst, hipStream_t stream) {
    ResetArgs P{};
    P.a = a; P.na = na; P.b = b; P.nb = nb; P.src = src; P.dst = dst;
    hipLaunchKernelGGL(query_reset, dim3(1), dim3(BLOCK), 0, stream, P);
}

template <typename Args>
static hipError_t launch_pair(void (*filter)(KernelArgs, Args), void (*reroute)(KernelArgs, Args), bool use_filter, uint32_t blocks, hipStream_t stream,
                              const KernelArgs &A, const Args &args) {
    if (use_filter) {
        hipLaunchKernelGGL(filter, dim3(blocks), dim3(BLOCK), 0, stream, A, args);
        if (hipError_t e = hipGetLastError()) return e;
    }
    // behind it, for what it listed (all but always nothing: the workgroups leave at once) -- or for everything
    hipLaunchKernelGGL(reroute, dim3(blocks), dim3(BLOCK), 0, stream, A, args);
    return hipGetLastError();
}

// the launches of a call's rays or records, at most query_launch_rays at a time, on the scratch query_begin and query_list_reserve have made; `clean`: the cursors
// and the list's length are zero already
static int query_launches(crt_ctx *ctx, const QueryCall &C, hipStream_t stream, bool clean) {
    crt_query_state *q = ctx->query;
    KernelArgs A{};
    A.s = (scene_args_p)ctx->d_scene;
    A.f = (frame_args_p)(q->frame.p + (C.every_mesh ? 1 : 0));   // all zero but for use_gi (0: shadow rays skip refractive meshes); the bias travels in ShadeArgs
    const bool filter = uses_filter(ctx);
    // (an enqueue call grows nothing inside a capture: its parts are what the reroute list holds)
    const uint64_t part = C.d_count && filter ? std::min<uint64_t>(ctx->query_launch_rays, q->list.cap) : ctx->query_launch_rays;
    if (part == 0) { ctx->error = "query_launches: no reroute list"; return CRT_ERR_INVALID; }
    for (uint64_t done = 0; done < C.n; done += part) {
        const QueryCall c = call_part(C, done, std::min(C.n - done, part));
        if ((done || !clean) && C.kernels_only) {
            launch_reset(q->words.p, QW_HITS, nullptr, 0, nullptr, nullptr, stream);
            CRT_HIP_CHECK(ctx, hipGetLastError());
        } else if (done || !clean) CRT_HIP_CHECK(ctx, hipMemsetAsync(q->words.p, 0, QW_HITS * sizeof(uint32_t), stream));   // cursors and list length; the totals stay
        ShadeArgs S{};   // (the ray queries' arguments are its first member)
        QueryArgs &Q = S.q;
        Q.n = (uint32_t)c.n;
        Q.words = q->words.p;
        Q.list = q->list.p;
        Q.spill = q->spill.p;
        Q.direct = filter ? 0u : 1u;
        Q.chunk = std::max(64u, (ctx->tuning.fetch_chunk >> 16) & ~63u);   // (level 0's claim size, crt_tuning::fetch_chunk)
        Q.rays = c.rays; Q.max_distance = c.max_distance; Q.hits = c.hits; Q.occluded = c.occluded; Q.ray_type = c.ray_type;
        Q.count = c.d_count; Q.first = c.count_first;
        S.hits = c.records; S.points = c.points; S.normals = c.normals; S.out = c.out; S.status = c.status; S.shadow_bias = c.shadow_bias;
        const uint32_t blocks = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(ctx->grid_blocks, (c.n + BLOCK - 1) / BLOCK));
        hipError_t e = hipSuccess;
        if (c.d_count) {   // the DEVN builds: the levels of crt_shoot_rays*_enqueue
            if (c.kind == Q_CLOSEST) e = launch_pair(query_walk<BVH_PLAIN, false, true>, query_reroute<false, true>, filter, blocks, stream, A, Q);
            else if (c.kind != Q_SHADE_HITS) e = hipErrorInvalidValue;
            else if (c.every_mesh) e = launch_pair(query_direct<BVH_PLAIN, false, true, true>, query_direct_reroute<false, true>, filter, blocks, stream, A, S);
            else e = launch_pair(query_direct<BVH_PLAIN, false, false, true>, query_direct_reroute<false, true>, filter, blocks, stream, A, S);
        } else switch (c.kind) {
            case Q_CLOSEST: e = launch_pair(query_walk<BVH_PLAIN, false>, query_reroute<false>, filter, blocks, stream, A, Q); break;
            case Q_OCCLUDED: e = launch_pair(query_walk<BVH_PLAIN, true>, query_reroute<true>, filter, blocks, stream, A, Q); break;
            case Q_SHADE_HITS:
                e = c.every_mesh ? launch_pair(query_direct<BVH_PLAIN, false, true>, query_direct_reroute<false>, filter, blocks, stream, A, S)
                                 : launch_pair(query_direct<BVH_PLAIN, false>, query_direct_reroute<false>, filter, blocks, stream, A, S);
                break;
            case Q_LIGHT_POINTS: e = launch_pair(query_direct<BVH_PLAIN, true>, query_direct_reroute<true>, filter, blocks, stream, A, S); break;
        }
        CRT_HIP_CHECK(ctx, e);
    }
    return CRT_OK;
}

// one device call; `first`: the call's counters start at zero (the host variants make one call of every round trip)
static int query_run(crt_ctx *ctx, const QueryCall &C, hipStream_t stream, bool first) {
    int rc = query_begin(ctx, stream, false);
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    if ((rc = query_list_reserve(ctx, C.n))) return rc;
    if (first) {
        q->stats = crt_query_stats{};
        CRT_HIP_CHECK(ctx, hipMemsetAsync(q->words.p, 0, QW_WORDS * sizeof(uint32_t), stream));
    }
    q->stats.rays += C.n;
    CRT_HIP_CHECK(ctx, hipEventRecord(q->call.ev0, stream));
    rc = query_launches(ctx, C, stream, first);
    if (rc) return rc;
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->h_words, q->words.p, QW_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipEventRecord(q->call.ev1, stream));
    q->call.stream = stream;
    q->call.radiance = q->call.enqueue = false;
    q->call.open = true;
    return CRT_OK;
}

// The host variants: H holds the caller's host arrays.  Copy in, run, copy out, query_host_rays at a time, through the family's device
// copies, which are kept for the next call.
static int query_host(crt_ctx *ctx, const QueryCall &H) {
    int rc = query_begin(ctx, ctx->stream, false);
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    const uint64_t cap = std::min(H.n, ctx->query_host_rays);
    QueryCall D = H;   // the same call on the device copies
    switch (H.kind) {
        case Q_CLOSEST:
            if ((rc = q->s_rays.reserve(ctx, cap)) || (rc = q->s_hits.reserve(ctx, cap))) return rc;
            D.rays = q->s_rays.p; D.hits = q->s_hits.p;
            break;
        case Q_OCCLUDED:
            if ((rc = q->s_rays.reserve(ctx, cap)) || (rc = q->s_dist.reserve(ctx, cap)) || (rc = q->s_occ.reserve(ctx, cap))) return rc;
            D.rays = q->s_rays.p; D.max_distance = q->s_dist.p; D.occluded = q->s_occ.p;
            break;
        case Q_SHADE_HITS:
            if ((rc = q->s_records.reserve(ctx, cap)) || (rc = q->s_rgb.reserve(ctx, 3 * cap)) || (rc = q->s_status.reserve(ctx, cap))) return rc;
            D.records = q->s_records.p; D.out = q->s_rgb.p; D.status = q->s_status.p;
            break;
        case Q_LIGHT_POINTS:
            if ((rc = q->s_points.reserve(ctx, 3 * cap)) || (rc = q->s_normals.reserve(ctx, 3 * cap)) || (rc = q->s_sums.reserve(ctx, cap))) return rc;
            D.points = q->s_points.p; D.normals = q->s_normals.p; D.out = q->s_sums.p;
            break;
    }
    const uint64_t out_floats = H.kind == Q_LIGHT_POINTS ? 1 : 3;
    for (uint64_t done = 0; done < H.n; done += ctx->query_host_rays) {
        const QueryCall h = call_part(H, done, std::min(H.n - done, ctx->query_host_rays));
        D.n = h.n;
        if (h.rays) CRT_HIP_CHECK(ctx, hipMemcpyAsync((void *)D.rays, h.rays, h.n * sizeof(crt_ray), hipMemcpyHostToDevice, ctx->stream));
        if (h.max_distance) CRT_HIP_CHECK(ctx, hipMemcpyAsync((void *)D.max_distance, h.max_distance, h.n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        if (h.records) CRT_HIP_CHECK(ctx, hipMemcpyAsync((void *)D.records, h.records, h.n * sizeof(crt_hit), hipMemcpyHostToDevice, ctx->stream));
        if (h.points) CRT_HIP_CHECK(ctx, hipMemcpyAsync((void *)D.points, h.points, h.n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        if (h.normals) CRT_HIP_CHECK(ctx, hipMemcpyAsync((void *)D.normals, h.normals, h.n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        rc = query_run(ctx, D, ctx->stream, done == 0);
        if (rc) return rc;
        if (h.hits) CRT_HIP_CHECK(ctx, hipMemcpyAsync(h.hits, D.hits, h.n * sizeof(crt_hit), hipMemcpyDeviceToHost, ctx->stream));
        if (h.occluded) CRT_HIP_CHECK(ctx, hipMemcpyAsync(h.occluded, D.occluded, h.n, hipMemcpyDeviceToHost, ctx->stream));
        if (h.out) CRT_HIP_CHECK(ctx, hipMemcpyAsync(h.out, D.out, h.n * out_floats * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (h.status) CRT_HIP_CHECK(ctx, hipMemcpyAsync(h.status, D.status, h.n, hipMemcpyDeviceToHost, ctx->stream));
        CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        rc = query_harvest(ctx);
        if (rc) return rc;
    }
    return CRT_OK;
}

static int query_check(crt_ctx *ctx, const void *rays, const void *extra, const void *out, uint32_t ray_type, const char *what) {
    if (!rays || !extra || !out) { ctx->error = std::string(what) + ": NULL array with n > 0"; return CRT_ERR_INVALID; }
    if (ray_type > (uint32_t)CRT_RAY_REFRACTION) { ctx->error = std::string(what) + ": unknown ray_type " + std::to_string(ray_type); return CRT_ERR_INVALID; }
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

extern "C" int crt_trace_rays_device(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, crt_hit *d_out, void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = query_check(ctx, d_rays, d_rays, d_out, ray_type, "crt_trace_rays_device");
    if (rc) return rc;
    return query_run(ctx, closest_call(d_rays, n, ray_type, d_out), (hipStream_t)stream, true);
}

extern "C" int crt_occluded_rays_device(crt_ctx *ctx, const crt_ray *d_rays, const float *d_max_distance, uint64_t n, uint8_t *d_out, void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = query_check(ctx, d_rays, d_max_distance, d_out, CRT_RAY_SHADOW, "crt_occluded_rays_device");
    if (rc) return rc;
    return query_run(ctx, occluded_call(d_rays, d_max_distance, n, d_out), (hipStream_t)stream, true);
}

extern "C" int crt_trace_rays(crt_ctx *ctx, const crt_ray *rays, uint64_t n, uint32_t ray_type, crt_hit *out) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = query_check(ctx, rays, rays, out, ray_type, "crt_trace_rays");
    if (rc) return rc;
    return query_host(ctx, closest_call(rays, n, ray_type, out));
}

extern "C" int crt_occluded_rays(crt_ctx *ctx, const crt_ray *rays, const float *max_distance, uint64_t n, uint8_t *out) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = query_check(ctx, rays, max_distance, out, CRT_RAY_SHADOW, "crt_occluded_rays");
    if (rc) return rc;
    return query_host(ctx, occluded_call(rays, max_distance, n, out));
}

extern "C" int crt_shade_hits_device(crt_ctx *ctx, const crt_hit *d_hits, uint64_t n, const crt_options *options, float *d_rgb, uint8_t *d_status,
                                     void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shade_check(ctx, d_hits, options, d_rgb, options, "crt_shade_hits_device");
    if (rc) return rc;
    return query_run(ctx, shade_call(d_hits, n, options->shadow_bias, d_rgb, d_status), (hipStream_t)stream, true);
}

extern "C" int crt_light_points_device(crt_ctx *ctx, const float *d_points, const float *d_normals, uint64_t n, float shadow_bias, float *d_out,
                                       void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shade_check(ctx, d_points, d_normals, d_out, nullptr, "crt_light_points_device");
    if (rc) return rc;
    return query_run(ctx, points_call(d_points, d_normals, n, shadow_bias, d_out), (hipStream_t)stream, true);
}

extern "C" int crt_shade_hits(crt_ctx *ctx, const crt_hit *hits, uint64_t n, const crt_options *options, float *out_rgb, uint8_t *out_status) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shade_check(ctx, hits, options, out_rgb, options, "crt_shade_hits");
    if (rc) return rc;
    return query_host(ctx, shade_call(hits, n, options->shadow_bias, out_rgb, out_status));
}

extern "C" int crt_light_points(crt_ctx *ctx, const float *points, const float *normals, uint64_t n, float shadow_bias, float *out) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shade_check(ctx, points, normals, out, nullptr, "crt_light_points");
    if (rc) return rc;
    return query_host(ctx, points_call(points, normals, n, shadow_bias, out));
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
// max_depth: trace the level's rays and light their records (query_launches, twice: background, constant and diffuse records are
// final), radiance_scatter the recursing ones into level g + 1, read that level's size back -- the one wait of a level --; then
// radiance_combine from the deepest level up.  Level 0's colours are the caller's array.
// crt_shoot_rays_gi*: the same loop with the kernels' GI builds.  A level has a key array beside its rays; the lighting launches skip no
// mesh; a DIFFUSE record is not final but spawns gi_sample_size rays, so level g + 1 holds up to max(2, gi_sample_size) rays for each
// of level g.

// what a GI call adds to a pass's arguments (null: a plain call)
struct ShootGi {
    const uint32_t *d_keys;   // the pass's keys on the device, or null: those of a frame's pixels key_first ..., sample 0
    uint32_t key_first;       // the index in the call of the pass's first ray
};

// rays of level g + 1 for each ray of level g, at most
static uint64_t shoot_fan(const crt_options *o, const bool gi) { return gi ? std::max(2u, o->gi_sample_size) : 2u; }

// GI: the rays of one pass -- as many as keep the worst-case deepest level (every hit of every level DIFFUSE) at SHOOT_GI_DEEPEST_RAYS,
// between 64 and shoot_pass_rays; 0 when 64 rays do not fit.  *product: max(2, gi_sample_size)^max_depth (saturated above the bound).
static uint64_t shoot_gi_pass_rays(const crt_ctx *ctx, const crt_options *o, uint64_t *product) {
    const uint64_t fan = shoot_fan(o, true);   // (<= 64: the product below stays under 2^33)
    uint64_t p = 1;
    for (uint32_t d = 0; d < o->max_depth && p <= SHOOT_GI_DEEPEST_RAYS; d++) p *= fan;
    *product = p;
    if (64u * p > SHOOT_GI_DEEPEST_RAYS) return 0;
    return std::min(std::max<uint64_t>(SHOOT_GI_DEEPEST_RAYS / p, 64u), ctx->shoot_pass_rays);
}

// room for `cap` rays at level g (`own_rgb`: with colours of its own; level 0 writes the caller's array; `keys`: a GI call)
static int shoot_level_reserve(crt_ctx *ctx, const uint32_t g, const uint64_t cap, const bool own_rgb, const bool keys) {
    ShootLevel &L = ctx->query->lv[g];
    int rc;
    if ((rc = L.rays.reserve(ctx, cap)) || (rc = L.hits.reserve(ctx, cap)) || (rc = L.status.reserve(ctx, cap)) || (rc = L.nodes.reserve(ctx, 2 * cap))) return rc;
    if (keys && (rc = L.keys.reserve(ctx, cap))) return rc;
    return own_rgb ? L.rgb.reserve(ctx, 3 * cap) : CRT_OK;
}

// what crt_shoot_rays*_enqueue adds to a pass's arguments (null: the host reads every level's size back): the levels' capacities, in
// place of the sizes.  The scratch holds them already (shoot_enqueue has seen to it): the pass reserves, waits for and reads nothing.
struct ShootDev {
    uint32_t cap[MAX_GENERATIONS];   // shoot_level_caps (shoot_caps.h)
    crt_shoot_report *d_report;      // the caller's, or null
    bool capturing;                  // the stream is being captured: the library's own copy of the report is not made
};

// one pass: m rays of the caller's (at most shoot_pass_rays, or what shoot_gi_pass_rays allows), every level of them; leaves the pass's
// numbers on their way to h_shoot (dev: to h_report)
static int shoot_pass(crt_ctx *ctx, const crt_ray *d_rays, const uint32_t m, const uint32_t ray_type, const crt_options *o, float *d_rgb,
                      hipStream_t stream, const ShootGi *gi, const ShootDev *dev = nullptr) {
    crt_query_state *q = ctx->query;
    KernelArgs A{};
    A.s = (scene_args_p)ctx->d_scene;
    A.f = (frame_args_p)q->frame.p;
    const uint64_t fan = shoot_fan(o, gi != nullptr);
    if (dev) {   // (kernel launches alone: shoot_enqueue)
        launch_reset(q->words.p, QW_WORDS, q->swords.p, SW_WORDS, nullptr, nullptr, stream);
        CRT_HIP_CHECK(ctx, hipGetLastError());
    } else {
        CRT_HIP_CHECK(ctx, hipMemsetAsync(q->words.p, 0, QW_WORDS * sizeof(uint32_t), stream));
        CRT_HIP_CHECK(ctx, hipMemsetAsync(q->swords.p, 0, SW_WORDS * sizeof(uint32_t), stream));
    }
    uint32_t count[MAX_GENERATIONS + 1] = {m};   // dev: the capacities -- what the launches are sized for
    uint32_t *const d_count = q->swords.p + SW_COUNT;   // [g]: rays appended to level g
    uint32_t last = 0;
    for (uint32_t g = 0; g <= o->max_depth; g++) {
        const uint32_t n = count[g];
        last = g;
        int rc;
        if (!dev && ((rc = query_list_reserve(ctx, n)) || (rc = shoot_level_reserve(ctx, g, n, g > 0, gi != nullptr)))) return rc;   // (the list follows the widest level)
        const bool devn = dev && g > 0;   // (level 0's size is the caller's n: its launches are those of the other calls)
        const ShootLevel &L = q->lv[g];
        float *rgb = g == 0 ? d_rgb : L.rgb.p;
        const uint32_t blocks = (uint32_t)(((uint64_t)n + BLOCK - 1) / BLOCK);
        RadianceArgs G{};
        G.in_rays = d_rays; G.rays = L.rays.p; G.hits = L.hits.p; G.status = L.status.p; G.rgb = rgb; G.nodes = L.nodes.p; G.n = n;
        G.diffuse_total = reinterpret_cast<unsigned long long *>(q->swords.p + SW_DIFFUSE);
        G.reflection_bias = o->reflection_bias; G.refraction_bias = o->refraction_bias;
        if (gi) {
            G.in_keys = gi->d_keys; G.keys = L.keys.p; G.gi_samples = o->gi_sample_size; G.gi_seed = o->gi_seed; G.key_first = gi->key_first;
            G.monte_carlo_bias = o->monte_carlo_bias;
        }
        if (devn) G.n_dev = d_count + g;
        if (g == 0) {
            if (gi) hipLaunchKernelGGL(radiance_prepare<true>, dim3(blocks), dim3(BLOCK), 0, stream, G);
            else hipLaunchKernelGGL(radiance_prepare<false>, dim3(blocks), dim3(BLOCK), 0, stream, G);
            CRT_HIP_CHECK(ctx, hipGetLastError());
        }
        // children are REFLECTION or REFRACTION rays, which walk alike: only the caller's own ray can be PRIMARY (Ray.cpp:13)
        QueryCall trace = closest_call(L.rays.p, n, g == 0 ? ray_type : (uint32_t)CRT_RAY_REFLECTION, L.hits.p);
        QueryCall light = shade_call(L.hits.p, n, o->shadow_bias, rgb, L.status.p, gi != nullptr);
        if (devn) trace.d_count = light.d_count = d_count + g;
        trace.kernels_only = light.kernels_only = dev != nullptr;
        rc = query_launches(ctx, trace, stream, g == 0);
        if (rc) return rc;
        if (g == 0 && dev) {
            launch_reset(nullptr, 0, nullptr, 0, reinterpret_cast<const unsigned long long *>(q->words.p + QW_HITS), q->d_hits0.p, stream);
            CRT_HIP_CHECK(ctx, hipGetLastError());
        } else if (g == 0) CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->h_shoot + SH_HITS0, q->words.p + QW_HITS, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        rc = query_launches(ctx, light, stream, false);
        if (rc) return rc;
        // the next level holds at most `fan` rays for each of this one: room for that BEFORE the launch that fills it
        const bool spawn = g + 1 <= o->max_depth;   // a child enters shootRay with depth g + 1 (RayTracer.cpp:427)
        if (spawn) {
            if (!dev) {
                if (fan * n > SHOOT_LEVEL_RAYS) { ctx->error = "crt_shoot_rays: a recursion level wider than 2^30 rays"; return CRT_ERR_NOMEM; }
                rc = shoot_level_reserve(ctx, g + 1, fan * n, true, gi != nullptr);
                if (rc) return rc;
            }
            G.child_rays = q->lv[g + 1].rays.p;
            G.child_keys = q->lv[g + 1].keys.p;
            G.child_cap = (uint32_t)std::min<uint64_t>(q->lv[g + 1].rays.cap, SHOOT_LEVEL_RAYS);
            if (gi) G.child_cap = (uint32_t)std::min<uint64_t>(G.child_cap, q->lv[g + 1].keys.cap);
            if (dev) G.child_cap = dev->cap[g + 1];   // (at most what the arrays hold: shoot_enqueue; a child beyond it is the background)
        }
        G.child_count = d_count + g + 1;
        G.spawn = spawn ? 1u : 0u;
        if (devn) {
            if (gi) hipLaunchKernelGGL((radiance_scatter<true, true>), dim3(blocks), dim3(BLOCK), 0, stream, A, G);
            else hipLaunchKernelGGL((radiance_scatter<false, true>), dim3(blocks), dim3(BLOCK), 0, stream, A, G);
        } else if (gi) hipLaunchKernelGGL(radiance_scatter<true>, dim3(blocks), dim3(BLOCK), 0, stream, A, G);
        else hipLaunchKernelGGL(radiance_scatter<false>, dim3(blocks), dim3(BLOCK), 0, stream, A, G);
        CRT_HIP_CHECK(ctx, hipGetLastError());
        if (!spawn) break;
        if (dev) count[g + 1] = dev->cap[g + 1];   // no wait: the next level is launched for what it may hold, and counts for itself
        else {
            // the one wait of a level: four bytes through pinned memory, to size the next one
            CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->h_shoot + SH_COUNT, G.child_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));
            count[g + 1] = (uint32_t)std::min<uint64_t>(*reinterpret_cast<const uint32_t *>(q->h_shoot + SH_COUNT), fan * n);
        }
        if (count[g + 1] == 0) break;
    }
    if (!dev) {
        for (uint32_t g = 0; g <= last; g++) q->shoot.level_rays[g] += count[g];
        q->shoot.levels = std::max(q->shoot.levels, last + 1);
    }
    // the up-sweep: level g's recursing records from level g + 1's colours, which are final by then
    for (uint32_t g = last + 1; g-- > 0;) {
        const ShootLevel &L = q->lv[g];
        RadianceArgs G{};
        G.status = L.status.p; G.nodes = L.nodes.p; G.rgb = g == 0 ? d_rgb : L.rgb.p; G.n = count[g];
        G.child_rgb = g < last ? q->lv[g + 1].rgb.p : nullptr;
        G.child_n = g < last ? count[g + 1] : 0u;
        G.gi_samples = gi ? o->gi_sample_size : 0u;
        const dim3 grid((uint32_t)(((uint64_t)count[g] + BLOCK - 1) / BLOCK));
        if (dev) {
            G.n_dev = g > 0 ? d_count + g : nullptr;
            G.child_n_dev = g < last ? d_count + g + 1 : nullptr;
            if (gi) hipLaunchKernelGGL((radiance_combine<true, true>), grid, dim3(BLOCK), 0, stream, A, G);
            else hipLaunchKernelGGL((radiance_combine<false, true>), grid, dim3(BLOCK), 0, stream, A, G);
        } else if (gi) hipLaunchKernelGGL(radiance_combine<true>, grid, dim3(BLOCK), 0, stream, A, G);
        else hipLaunchKernelGGL(radiance_combine<false>, grid, dim3(BLOCK), 0, stream, A, G);
        CRT_HIP_CHECK(ctx, hipGetLastError());
    }
    if (dev) {   // the call's numbers, summed where they are
        ReportArgs P{};
        P.count = d_count;
        P.hits0 = q->d_hits0.p;
        P.diffuse = reinterpret_cast<const unsigned long long *>(q->swords.p + SW_DIFFUSE);
        P.rerouted = reinterpret_cast<const unsigned long long *>(q->words.p + QW_REROUTED);
        P.out = dev->d_report;
        P.out2 = dev->capturing ? nullptr : q->d_report.p;
        P.n = m;
        for (uint32_t g = 0; g <= last; g++) P.cap[g] = count[g];   // (0 behind the last level launched)
        hipLaunchKernelGGL(radiance_report, dim3(1), dim3(64), 0, stream, P);
        CRT_HIP_CHECK(ctx, hipGetLastError());
        if (!dev->capturing) CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->h_report, q->d_report.p, sizeof(crt_shoot_report), hipMemcpyDeviceToHost, stream));
        return CRT_OK;
    }
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->h_shoot + SH_DIFFUSE, q->swords.p + SW_DIFFUSE, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->h_shoot + SH_REROUTED, q->words.p + QW_REROUTED, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
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

// crt_shoot_rays_gi*: the arguments, and *pass = the rays of one pass (null: no pass size is asked for, and none can be refused)
static int shoot_gi_check(crt_ctx *ctx, const void *rays, const crt_options *options, const void *out, uint32_t ray_type, const char *what, uint64_t *pass) {
    if (!rays || !options || !out) { ctx->error = std::string(what) + ": NULL array or options with n > 0"; return CRT_ERR_INVALID; }
    if (ray_type > (uint32_t)CRT_RAY_REFRACTION) { ctx->error = std::string(what) + ": unknown ray_type " + std::to_string(ray_type); return CRT_ERR_INVALID; }
    if (!options->use_gi) {
        ctx->error = std::string(what) + ": use_gi is 0: the deterministic build's colours are crt_shoot_rays' (crt_shoot_rays_device's)";
        return CRT_ERR_INVALID;
    }
    if (options->gi_sample_size > 64u) {   // (a frame's rule: crt_launch.hip)
        ctx->error = std::string(what) + ": gi_sample_size too large: " + std::to_string(options->gi_sample_size) + ", at most 64";
        return CRT_ERR_INVALID;
    }
    if ((uint64_t)options->max_depth + 1 > (uint64_t)MAX_GENERATIONS) {
        ctx->error = std::string(what) + ": max_depth too large: " + std::to_string(options->max_depth) + " + 1 levels, at most " + std::to_string(MAX_GENERATIONS);
        return CRT_ERR_INVALID;
    }
    if (!pass) return CRT_OK;   // (crt_shoot_rays_gi_enqueue: one pass, whose levels the capacities bound)
    uint64_t product = 0;
    *pass = shoot_gi_pass_rays(ctx, options, &product);
    if (*pass == 0) {
        ctx->error = std::string(what) + ": the deepest level of a pass of 64 rays may hold 64 x max(2, gi_sample_size)^max_depth = 64 x " +
                     std::to_string(shoot_fan(options, true)) + "^" + std::to_string(options->max_depth) +
                     (product > SHOOT_GI_DEEPEST_RAYS ? " > 64 x 2^26" : " = " + std::to_string(64u * product)) + " rays, more than 2^26";
        return CRT_ERR_INVALID;
    }
    return CRT_OK;
}

// the radiance queries' own words and pinned slots, the enqueue calls' among them: made by the first radiance call of a context, so that
// an enqueue call inside a capture finds them
static int shoot_words_reserve(crt_ctx *ctx) {
    crt_query_state *q = ctx->query;
    if (q->h_shoot) return CRT_OK;
    int rc;
    if ((rc = q->swords.reserve(ctx, SW_WORDS)) || (rc = q->d_report.reserve(ctx, 1)) || (rc = q->d_hits0.reserve(ctx, 1))) return rc;
    if (!q->h_report) {
        CRT_HIP_CHECK(ctx, hipHostMalloc((void **)&q->h_report, sizeof(crt_shoot_report)));
        memset(q->h_report, 0, sizeof(crt_shoot_report));
    }
    CRT_HIP_CHECK(ctx, hipHostMalloc((void **)&q->h_shoot, SH_SLOTS * sizeof(uint64_t)));
    memset(q->h_shoot, 0, SH_SLOTS * sizeof(uint64_t));
    return CRT_OK;
}

// one device call: n rays, `pass` at a time
static int shoot_run(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *d_rgb, hipStream_t stream,
                     const uint64_t pass, const ShootGi *gi) {
    int rc = query_begin(ctx, stream, true);
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    if ((rc = shoot_words_reserve(ctx))) return rc;
    q->stats = crt_query_stats{};
    q->stats.rays = n;
    q->shoot = crt_shoot_stats{};
    q->shoot.rays = n;
    CRT_HIP_CHECK(ctx, hipEventRecord(q->call.ev0, stream));
    for (uint64_t done = 0; done < n; done += pass) {
        if (done) {   // the previous pass's numbers leave the pinned slots before this pass writes them
            CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));
            shoot_fold(q);
        }
        ShootGi part{};
        if (gi) { part.d_keys = gi->d_keys ? gi->d_keys + done : nullptr; part.key_first = gi->key_first + (uint32_t)done; }
        rc = shoot_pass(ctx, d_rays + done, (uint32_t)std::min(n - done, pass), ray_type, options, d_rgb + 3 * done, stream, gi ? &part : nullptr);
        if (rc) return rc;
    }
    CRT_HIP_CHECK(ctx, hipEventRecord(q->call.ev1, stream));
    q->call.stream = stream;
    q->call.radiance = true;
    q->call.enqueue = false;
    q->call.open = true;
    return CRT_OK;
}

// rays level g's arrays hold now (`own_rgb`, `keys`: as shoot_level_reserve takes them)
static uint64_t shoot_level_room(const crt_query_state *q, const uint32_t g, const bool own_rgb, const bool keys) {
    const ShootLevel &L = q->lv[g];
    uint64_t room = std::min(std::min(L.rays.cap, L.hits.cap), std::min(L.status.cap, L.nodes.cap / 2));
    if (own_rgb) room = std::min(room, L.rgb.cap / 3);
    if (keys) room = std::min(room, L.keys.cap);
    return room;
}

// crt_shoot_rays*_enqueue: one pass whose levels' sizes stay on the device (shoot_pass with a ShootDev).  Everything that waits,
// allocates or records an event happens HERE, before the first launch, and none of it inside a capture: what a capture would need of
// it is refused while nothing is enqueued yet, so that the capture stays valid.
static int shoot_enqueue(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *o, float *d_rgb,
                         const uint32_t *level_cap, crt_shoot_report *d_report, hipStream_t stream, const ShootGi *gi, const char *what) {
    if (n > SHOOT_ENQUEUE_RAYS) {
        ctx->error = std::string(what) + ": a call is one pass: n = " + std::to_string(n) + " > 2^22 rays; split the rays over several calls";
        return CRT_ERR_INVALID;
    }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    CRT_HIP_CHECK(ctx, hipStreamIsCapturing(stream, &capture));
    const bool capturing = capture != hipStreamCaptureStatusNone;
    const auto refuse = [&](const char *why) {
        ctx->error = std::string(what) + ": the stream is being captured and " + why;
        return CRT_ERR_INVALID;
    };
    int rc;
    if (capturing) {
        if (capture != hipStreamCaptureStatusActive) return refuse("the capture is invalidated");
        if (ctx->pending) return refuse("a crt_render_async frame is pending: the call would have to wait for it (crt_wait before the capture)");
        if (!ctx->query || !ctx->query->h_words || !ctx->query->h_shoot)
            return refuse("the query scratch would have to grow (the context has none yet): size it with a radiance call before the capture");
        if (ctx->query->call.open)
            return refuse("an open call would have to be harvested, which waits (crt_get_shoot_stats or crt_get_query_stats before the capture)");
    } else if ((rc = query_begin(ctx, stream, true, true)) || (rc = shoot_words_reserve(ctx))) return rc;
    crt_query_state *q = ctx->query;
    // the capacities, and room for them
    const bool keys = gi != nullptr;
    uint64_t have[MAX_GENERATIONS];
    for (uint32_t g = 0; g < (uint32_t)MAX_GENERATIONS; g++) have[g] = shoot_level_room(q, g, true, keys);
    ShootDev dev{};
    shoot_level_caps(n, shoot_fan(o, keys), o->max_depth, level_cap, have, dev.cap);
    uint64_t widest = n;
    bool fits = shoot_level_room(q, 0, false, keys) >= n;
    for (uint32_t g = 1; g <= o->max_depth; g++) {
        widest = std::max<uint64_t>(widest, dev.cap[g]);
        fits = fits && have[g] >= dev.cap[g];
    }
    if (capturing) {
        // (the reroute list need not follow the widest level here: a level's launches are cut to what the list holds, query_launches)
        if (!fits || (uses_filter(ctx) && q->list.cap < std::min(n, ctx->query_launch_rays)))
            return refuse("the query scratch would have to grow for these rays and capacities: make the same call once before the capture");
    } else {
        if ((rc = query_list_reserve(ctx, widest)) || (rc = shoot_level_reserve(ctx, 0, n, false, keys))) return rc;
        for (uint32_t g = 1; g <= o->max_depth && dev.cap[g]; g++)
            if ((rc = shoot_level_reserve(ctx, g, dev.cap[g], true, keys))) return rc;
        q->stats = crt_query_stats{};
        q->stats.rays = n;
        q->shoot = crt_shoot_stats{};
        q->shoot.rays = n;
        CRT_HIP_CHECK(ctx, hipEventRecord(q->call.ev0, stream));
    }
    dev.d_report = d_report;
    dev.capturing = capturing;
    rc = shoot_pass(ctx, d_rays, (uint32_t)n, ray_type, o, d_rgb, stream, gi, &dev);
    if (rc || capturing) return rc;   // (a captured call leaves no open call behind: the replays' numbers are d_report's)
    CRT_HIP_CHECK(ctx, hipEventRecord(q->call.ev1, stream));
    q->call.stream = stream;
    q->call.radiance = q->call.enqueue = true;
    q->call.open = true;
    return CRT_OK;
}

// the host variants: copy in, run, copy out, `pass` rays at a time; the colours' device copy is level 0's own colour array
static int shoot_host(crt_ctx *ctx, const crt_ray *rays, const uint32_t *keys, uint64_t n, uint32_t ray_type, const crt_options *options, float *out_rgb,
                      const uint64_t pass, const bool gi) {
    const uint64_t m = std::min(n, pass);
    int rc = query_begin(ctx, ctx->stream, true);
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    if ((rc = shoot_level_reserve(ctx, 0, m, true, gi)) || (rc = q->shoot_in.reserve(ctx, m))) return rc;
    if (keys && (rc = q->shoot_keys.reserve(ctx, m))) return rc;
    crt_shoot_stats total{};
    crt_query_stats qtotal{};
    for (uint64_t done = 0; done < n; done += pass) {
        const uint64_t k = std::min(n - done, pass);
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->shoot_in.p, rays + done, k * sizeof(crt_ray), hipMemcpyHostToDevice, ctx->stream));
        if (keys) CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->shoot_keys.p, keys + done, k * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        const ShootGi part{keys ? q->shoot_keys.p : nullptr, (uint32_t)done};
        rc = shoot_run(ctx, q->shoot_in.p, k, ray_type, options, q->lv[0].rgb.p, ctx->stream, pass, gi ? &part : nullptr);
        if (rc) return rc;
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb + 3 * done, q->lv[0].rgb.p, k * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
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

extern "C" int crt_shoot_rays_device(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *d_rgb,
                                     void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shoot_check(ctx, d_rays, options, d_rgb, ray_type, "crt_shoot_rays_device");
    if (rc) return rc;
    return shoot_run(ctx, d_rays, n, ray_type, options, d_rgb, (hipStream_t)stream, ctx->shoot_pass_rays, nullptr);
}

extern "C" int crt_shoot_rays(crt_ctx *ctx, const crt_ray *rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *out_rgb) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shoot_check(ctx, rays, options, out_rgb, ray_type, "crt_shoot_rays");
    if (rc) return rc;
    return shoot_host(ctx, rays, nullptr, n, ray_type, options, out_rgb, ctx->shoot_pass_rays, false);
}

extern "C" int crt_shoot_rays_gi_device(crt_ctx *ctx, const crt_ray *d_rays, const uint32_t *d_keys, uint64_t n, uint32_t ray_type,
                                        const crt_options *options, float *d_rgb, void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    uint64_t pass = 0;
    int rc = shoot_gi_check(ctx, d_rays, options, d_rgb, ray_type, "crt_shoot_rays_gi_device", &pass);
    if (rc) return rc;
    const ShootGi gi{d_keys, 0u};
    return shoot_run(ctx, d_rays, n, ray_type, options, d_rgb, (hipStream_t)stream, pass, &gi);
}

extern "C" int crt_shoot_rays_gi(crt_ctx *ctx, const crt_ray *rays, const uint32_t *keys, uint64_t n, uint32_t ray_type, const crt_options *options,
                                 float *out_rgb) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    uint64_t pass = 0;
    int rc = shoot_gi_check(ctx, rays, options, out_rgb, ray_type, "crt_shoot_rays_gi", &pass);
    if (rc) return rc;
    return shoot_host(ctx, rays, keys, n, ray_type, options, out_rgb, pass, true);
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

extern "C" int crt_shoot_rays_enqueue(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *d_rgb,
                                      const uint32_t *level_cap, crt_shoot_report *d_report, void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shoot_check(ctx, d_rays, options, d_rgb, ray_type, "crt_shoot_rays_enqueue");
    if (rc) return rc;
    return shoot_enqueue(ctx, d_rays, n, ray_type, options, d_rgb, level_cap, d_report, (hipStream_t)stream, nullptr, "crt_shoot_rays_enqueue");
}

extern "C" int crt_shoot_rays_gi_enqueue(crt_ctx *ctx, const crt_ray *d_rays, const uint32_t *d_keys, uint64_t n, uint32_t ray_type,
                                         const crt_options *options, float *d_rgb, const uint32_t *level_cap, crt_shoot_report *d_report,
                                         void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    int rc = shoot_gi_check(ctx, d_rays, options, d_rgb, ray_type, "crt_shoot_rays_gi_enqueue", nullptr);
    if (rc) return rc;
    const ShootGi gi{d_keys, 0u};
    return shoot_enqueue(ctx, d_rays, n, ray_type, options, d_rgb, level_cap, d_report, (hipStream_t)stream, &gi, "crt_shoot_rays_gi_enqueue");
}

extern "C" int crt_get_shoot_report(crt_ctx *ctx, crt_shoot_report *out) {
    if (!ctx || !out) return CRT_ERR_INVALID;
    if (!ctx->query) { *out = crt_shoot_report{}; return CRT_OK; }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int rc = query_harvest(ctx);
    if (rc) return rc;
    *out = ctx->query->report;
    return CRT_OK;
}

extern "C" uint64_t crt_query_scratch_generation(const crt_ctx *ctx) { return ctx && ctx->query ? ctx->query->generation : 0; }
