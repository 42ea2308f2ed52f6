// crt_query.hip -- the queries for what the CALLER supplies (include/crt_hip.h), behind one call path:
//   ray queries        crt_trace_rays*, crt_occluded_rays*, crt_camera_rays_device: closest hit and occlusion, in place of
//                      AccelerationStructure::intersect (KDTree.cpp:127-192) and AccelerationStructure::checkForIntersection
//                      (AccelerationStructure.cpp:56-94) as entry points of their own; kernels: csrc/kernel_query.h
//   direct lighting    crt_shade_hits*, crt_light_points*: RayTracer::calculateDiffusion (RayTracer.cpp:300-330) for the caller's hit
//                      records and points; kernels: csrc/kernel_shade.h
//   radiance queries   crt_shoot_rays*: RayTracer::shootRay (RayTracer.cpp:419-451), a host loop over the launches of the other two, one
//                      recursion level behind the other, with three small kernels of its own around them (csrc/kernel_radiance.h): behind
//                      them in this file; crt_shoot_rays_gi*: the same loop for the GI build (a key per ray, sample rays at DIFFUSE
//                      records, no mesh skipped by a shadow ray)
//   chain guides       crt_guide_rays*: a ray's chain of closest-hit walks through mirrors and glass, level behind level without a wait;
//                      the step kernel and the work area: crt_guides.hip
// and their statistics (crt_get_query_stats, crt_get_shoot_stats).  A query reads the context's scene and nothing of its frames: the
// scratch below is the queries' own.  The GI frame calls (crt_giframe.hip) run queries through the few functions crt_internal.h lists
// and see nothing else of this file, nor this file anything of theirs.  The shape of the file:
//   an entry point    query_entry: the preamble and the one argument check (query_check, told what the call needs by a CallCheck)
//   a call            query_begin (the waiting rule: call_wait.h), then its launches between call_open and call_close
//   its launches      query_launches: the filter / reroute pair of the call's kind from one table (PAIRS); clear_words clears every word
//   a radiance pass   shoot_pass: shoot_down (level behind level), shoot_up, shoot_numbers.  The synchronous and the enqueue form part in
//                     shoot_children (a level's room and size), clear_words and shoot_numbers -- and in shoot_up's choice of build --,
//                     and nowhere in the level loop
#include "device_array.h"
#include "glibc_powf.h"
#include "gi_random.h"
#include "shoot_caps.h"

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
//   * a radiance call after any call harvests that one first, for the same reason;
//   * but an enqueue call behind an enqueue call on the same stream does not wait: that one's statistics come through a report of
//     their own, not through the words.
// call_waits (call_wait.h) is this rule, and query_begin asks nothing else.
struct OpenCall {
    bool open = false;
    CallKind kind = CALL_QUERY;   // CALL_ENQUEUE: its numbers are the report's (QueryPinned::report), not the SH_* slots'
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around its launches
};

// what comes back through pinned memory, in one block that query_begin makes with the rest of the scratch
struct QueryPinned {
    uint32_t words[QW_WORDS];   // the words of the last call, copied behind its last launch
    uint64_t shoot[SH_SLOTS];   // SH_*
    crt_shoot_report report;    // crt_query_state::d_report, copied behind the last launch of an enqueue call
};

}  // namespace

struct crt_query_state {
    DeviceArray<FrameArgs> frame;     // two frame blocks, all zero but for use_gi = 1 in the second: the reference-order walk reads use_gi
                                      // (0: shadow rays skip refractive meshes; 1, the levels of crt_shoot_rays_gi*: they skip none)
    DeviceArray<uint32_t> words;      // QW_*
    QueryPinned *pin = nullptr;
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
    DeviceArray<float> shoot_direct;  // ... and the device copy of the direct parts it gets back (crt_shoot_rays_gi_split)
    DeviceArray<uint32_t> swords;     // SW_*
    crt_shoot_stats shoot{};          // of the last radiance call
    // crt_shoot_rays*_enqueue
    DeviceArray<crt_shoot_report> d_report;   // what radiance_report writes for the library's own statistics (outside a capture)
    DeviceArray<unsigned long long> d_hits0;  // level 0's hits: QW_HITS as the level's trace left it (the lighting launches add to that word)
    crt_shoot_report report{};                // of the last enqueue call outside a capture
    // crt_guide_rays: the host variant's device copies of the status bytes and terminal rays, and its work area
    DeviceArray<uint8_t> g_status;
    DeviceArray<crt_ray> g_last;
    DeviceArray<float4> g_work;
    uint64_t level_peak[MAX_GENERATIONS] = {};   // the widest level g of a pass since query_level_peaks_reset (shoot_numbers)
    // the radiance queries' own device words: made by the first radiance call of a context (shoot_words_reserve)
    bool shoot_words_made() const { return swords.p && d_report.p && d_hits0.p; }
    ~crt_query_state() {
        if (pin) (void)hipHostFree(pin);
        if (call.ev0) (void)hipEventDestroy(call.ev0);
        if (call.ev1) (void)hipEventDestroy(call.ev1);
    }
};

void query_destroy(crt_ctx *ctx) {
    delete ctx->query;
    ctx->query = nullptr;
}

// a radiance pass's numbers, once its last copy has arrived
static void shoot_fold(crt_query_state *q) {
    q->stats.hits += q->pin->shoot[SH_HITS0];
    q->shoot.shadow_records += q->pin->shoot[SH_DIFFUSE];
    q->shoot.rerouted += q->pin->shoot[SH_REROUTED];
}

// the words and events of the open call, once: waits for it
static int query_harvest(crt_ctx *ctx) {
    crt_query_state *q = ctx->query;
    if (!q || !q->call.open) return CRT_OK;
    CRT_HIP_CHECK(ctx, hipEventSynchronize(q->call.ev1));
    q->call.open = false;
    float ms = 0;
    CRT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, q->call.ev0, q->call.ev1));
    if (q->call.kind != CALL_QUERY) {   // its last pass's numbers, and what crt_get_query_stats says of it
        q->shoot.kernel_ms = ms;
        if (q->call.kind == CALL_ENQUEUE) {   // (one pass, and the device has done the sums)
            q->report = q->pin->report;
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
        memcpy(&q->stats.hits, q->pin->words + QW_HITS, sizeof(uint64_t));          // (totals of the call: its launches add to the same words)
        memcpy(&q->stats.rerouted, q->pin->words + QW_REROUTED, sizeof(uint64_t));
    }
    return CRT_OK;
}

static bool uses_filter(const crt_ctx *ctx) { return ctx->scene.bvh_ok && ctx->tuning.bvh; }

// before a call on `stream`: the waiting rules (OpenCall), and what every query needs, allocated by the first one
int query_begin(crt_ctx *ctx, hipStream_t stream, const CallKind kind) {
    if (ctx->pending) {
        int rc = crt_wait(ctx);
        if (rc) return rc;
    }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (!ctx->query) ctx->query = new (std::nothrow) crt_query_state;
    crt_query_state *q = ctx->query;
    if (!q) { ctx->error = "out of memory"; return CRT_ERR_NOMEM; }
    if (!q->pin) {
        if (int rc = reserve_all(ctx, q->frame, 2, q->words, QW_WORDS)) return rc;
        CRT_HIP_CHECK(ctx, hipMemset(q->frame.p, 0, 2 * sizeof(FrameArgs)));
        const uint32_t one = 1u;
        CRT_HIP_CHECK(ctx, hipMemcpy(&q->frame.p[1].use_gi, &one, sizeof(one), hipMemcpyHostToDevice));
        // one region: every filter launch of a query (query_walk / query_direct, the levels of crt_shoot_rays* among them) has at most
        // grid_blocks workgroups and follows the previous one on ONE stream (a call on another stream, and a pending frame, are waited
        // for first): no two of them run side by side
        if (int rc = q->spill.reserve(ctx, ctx->bvh_spill_words())) return rc;
        if (!q->call.ev0) CRT_HIP_CHECK(ctx, hipEventCreate(&q->call.ev0));
        if (!q->call.ev1) CRT_HIP_CHECK(ctx, hipEventCreate(&q->call.ev1));
        CRT_HIP_CHECK(ctx, hipHostMalloc((void **)&q->pin, sizeof(QueryPinned)));
        memset(q->pin, 0, sizeof(QueryPinned));
    }
    return call_waits(q->call.open, q->call.kind, kind, q->call.stream == stream) ? query_harvest(ctx) : CRT_OK;
}

// A call's bracket.  call_open: the statistics of a call of `kind` for n rays start again (`first` false: a later round trip of a host
// variant adds to them) and ev0 is recorded; call_close: ev1 behind the last launch, and the call is the open one.
static int call_open(crt_ctx *ctx, const CallKind kind, const uint64_t n, hipStream_t stream, const bool first = true) {
    crt_query_state *q = ctx->query;
    if (first) q->stats = crt_query_stats{};
    q->stats.rays += n;
    if (kind != CALL_QUERY) {
        q->shoot = crt_shoot_stats{};
        q->shoot.rays = n;
    }
    CRT_HIP_CHECK(ctx, hipEventRecord(q->call.ev0, stream));
    return CRT_OK;
}
static int call_close(crt_ctx *ctx, const CallKind kind, hipStream_t stream) {
    OpenCall &call = ctx->query->call;
    CRT_HIP_CHECK(ctx, hipEventRecord(call.ev1, stream));
    call.stream = stream;
    call.kind = kind;
    call.open = true;
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

// The one way to clear counter words: a[0 .. na) and b[0 .. nb) (nb 0: none) become zero, by hipMemsetAsync -- or, `kernels_only` (an
// enqueue call, which a graph must be able to capture as a single chain of kernels), by query_reset.
static int clear_words(crt_ctx *ctx, uint32_t *a, uint32_t na, uint32_t *b, uint32_t nb, const bool kernels_only, hipStream_t stream) {
    if (kernels_only) {
        launch_reset(a, na, b, nb, nullptr, nullptr, stream);
        CRT_HIP_CHECK(ctx, hipGetLastError());
        return CRT_OK;
    }
    CRT_HIP_CHECK(ctx, hipMemsetAsync(a, 0, na * sizeof(uint32_t), stream));
    if (nb) CRT_HIP_CHECK(ctx, hipMemsetAsync(b, 0, nb * sizeof(uint32_t), stream));
    return CRT_OK;
}

// a filter / reroute kernel pair, launched: the ray queries' arguments are the first member of the lighting queries'
static const QueryArgs &pair_args(const ShadeArgs &S, void (*)(KernelArgs, QueryArgs)) { return S.q; }
static const ShadeArgs &pair_args(const ShadeArgs &S, void (*)(KernelArgs, ShadeArgs)) { return S; }
template <auto FILTER, auto REROUTE>
static hipError_t launch_pair(bool use_filter, uint32_t blocks, hipStream_t stream, const KernelArgs &A, const ShadeArgs &S) {
    if (use_filter) {
        hipLaunchKernelGGL(FILTER, dim3(blocks), dim3(BLOCK), 0, stream, A, pair_args(S, FILTER));
        if (hipError_t e = hipGetLastError()) return e;
    }
    // behind it, for what it listed (all but always nothing: the workgroups leave at once) -- or for everything
    hipLaunchKernelGGL(REROUTE, dim3(blocks), dim3(BLOCK), 0, stream, A, pair_args(S, REROUTE));
    return hipGetLastError();
}
using PairLaunch = hipError_t (*)(bool, uint32_t, hipStream_t, const KernelArgs &, const ShadeArgs &);
template <bool OCCLUDED, bool DEVN>
constexpr PairLaunch WALK = launch_pair<query_walk<BVH_PLAIN, OCCLUDED, DEVN>, query_reroute<OCCLUDED, DEVN>>;
template <bool POINTS, bool EVERY, bool DEVN>
constexpr PairLaunch DIRECT = launch_pair<query_direct<BVH_PLAIN, POINTS, EVERY, DEVN>, query_direct_reroute<POINTS, DEVN>>;
// Kernel choice: [QueryKind; 4: Q_SHADE_HITS by the GI build's occlusion rule (every_mesh)][the DEVN build: the level's size is a device
// word, crt_shoot_rays*_enqueue].  Null: no such build.
static const PairLaunch PAIRS[5][2] = {{WALK<false, false>, WALK<false, true>},
                                       {WALK<true, false>, nullptr},
                                       {DIRECT<false, false, false>, DIRECT<false, false, true>},
                                       {DIRECT<true, false, false>, nullptr},
                                       {DIRECT<false, true, false>, DIRECT<false, true, true>}};
// ... and the radiance queries' own kernels: [GI], [GI][DEVN]
static void (*const PREPARE[2])(RadianceArgs) = {radiance_prepare<false>, radiance_prepare<true>};
static void (*const SCATTER[2][2])(KernelArgs, RadianceArgs) = {{radiance_scatter<false>, radiance_scatter<false, true>},
                                                                {radiance_scatter<true>, radiance_scatter<true, true>}};
static void (*const COMBINE[2][2])(KernelArgs, RadianceArgs) = {{radiance_combine<false>, radiance_combine<false, true>},
                                                                {radiance_combine<true>, radiance_combine<true, true>}};

// the launches of a call's rays or records, at most query_launch_rays at a time, on the scratch query_begin and query_list_reserve have made; `clean`: the cursors
// and the list's length are zero already
static int query_launches(crt_ctx *ctx, const QueryCall &C, hipStream_t stream, bool clean) {
    crt_query_state *q = ctx->query;
    KernelArgs A{};
    A.s = (scene_args_p)ctx->d_scene;
    A.f = (frame_args_p)(q->frame.p + (C.every_mesh ? 1 : 0));   // all zero but for use_gi (0: shadow rays skip refractive meshes); the bias travels in ShadeArgs
    const bool filter = uses_filter(ctx);
    const PairLaunch launch = PAIRS[C.kind == Q_SHADE_HITS && C.every_mesh ? 4 : C.kind][C.d_count ? 1 : 0];
    if (!launch) CRT_HIP_CHECK(ctx, hipErrorInvalidValue);
    // (an enqueue call grows nothing inside a capture: its parts are what the reroute list holds)
    const uint64_t part = C.d_count && filter ? std::min<uint64_t>(ctx->query_launch_rays, q->list.cap) : ctx->query_launch_rays;
    if (part == 0) { ctx->error = "query_launches: no reroute list"; return CRT_ERR_INVALID; }
    for (uint64_t done = 0; done < C.n; done += part) {
        const QueryCall c = call_part(C, done, std::min(C.n - done, part));
        if (done || !clean)   // cursors and list length; the totals stay
            if (int rc = clear_words(ctx, q->words.p, QW_HITS, nullptr, 0, C.kernels_only, stream)) return rc;
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
        CRT_HIP_CHECK(ctx, launch(filter, blocks, stream, A, S));
    }
    return CRT_OK;
}

// one device call; `first`: the call's counters start at zero (the host variants make one call of every round trip)
static int query_run(crt_ctx *ctx, const QueryCall &C, hipStream_t stream, bool first) {
    int rc = query_begin(ctx, stream, CALL_QUERY);
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    if ((rc = query_list_reserve(ctx, C.n))) return rc;
    if (first && (rc = clear_words(ctx, q->words.p, QW_WORDS, nullptr, 0, false, stream))) return rc;
    if ((rc = call_open(ctx, CALL_QUERY, C.n, stream, first)) || (rc = query_launches(ctx, C, stream, first))) return rc;
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->pin->words, q->words.p, QW_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    return call_close(ctx, CALL_QUERY, stream);
}

// The host variants: H holds the caller's host arrays.  Copy in, run, copy out, query_host_rays at a time, through the family's device
// copies, which are kept for the next call.
static int query_host(crt_ctx *ctx, const QueryCall &H) {
    int rc = query_begin(ctx, ctx->stream, CALL_QUERY);
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    const uint64_t cap = std::min(H.n, ctx->query_host_rays);
    QueryCall D = H;   // the same call on the device copies
    switch (H.kind) {
        case Q_CLOSEST:
            if ((rc = reserve_all(ctx, q->s_rays, cap, q->s_hits, cap))) return rc;
            D.rays = q->s_rays.p; D.hits = q->s_hits.p;
            break;
        case Q_OCCLUDED:
            if ((rc = reserve_all(ctx, q->s_rays, cap, q->s_dist, cap, q->s_occ, cap))) return rc;
            D.rays = q->s_rays.p; D.max_distance = q->s_dist.p; D.occluded = q->s_occ.p;
            break;
        case Q_SHADE_HITS:
            if ((rc = reserve_all(ctx, q->s_records, cap, q->s_rgb, 3 * cap, q->s_status, cap))) return rc;
            D.records = q->s_records.p; D.out = q->s_rgb.p; D.status = q->s_status.p;
            break;
        case Q_LIGHT_POINTS:
            if ((rc = reserve_all(ctx, q->s_points, 3 * cap, q->s_normals, 3 * cap, q->s_sums, cap))) return rc;
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

// rays of level g + 1 for each ray of level g of a radiance query, at most
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

// What a call needs of its arguments: the one check of every entry point that takes n > 0 rays or records.
struct CallCheck {
    const char *what;             // the entry point
    const void *p[3];             // its arrays, and its options where it cannot do without them: none may be NULL
    uint32_t ray_type;            // one of crt_ray_type (CRT_RAY_SHADOW where the call takes none)
    const crt_options *options;   // or null: nothing of them is looked at.  use_gi must be 0 ...
    bool radiance;                // crt_shoot_rays*: max_depth + 1 levels must exist
    bool gi;                      // crt_shoot_rays_gi*: ... no: use_gi must be 1, and gi_sample_size a frame's
    uint64_t *pass;               // crt_shoot_rays_gi*, or null: the rays of one pass are wanted, and 64 of them must fit
};
static int query_check(crt_ctx *ctx, const CallCheck &k) {
    const auto refuse = [&](const std::string &why) {
        ctx->error = std::string(k.what) + ": " + why;
        return (int)CRT_ERR_INVALID;
    };
    const crt_options *o = k.options;
    if (!k.p[0] || !k.p[1] || !k.p[2]) return refuse(k.radiance ? "NULL array or options with n > 0" : "NULL array with n > 0");
    if (k.ray_type > (uint32_t)CRT_RAY_REFRACTION) return refuse("unknown ray_type " + std::to_string(k.ray_type));
    if (o && o->use_gi && !k.gi)
        return refuse(std::string("use_gi is not offered (the GI build's ") + (k.radiance ? "random sample rays, its " : "") +
                      "occlusion rule and its division by GI_SAMPLE_SIZE + 1)");
    if (k.gi && !o->use_gi) return refuse("use_gi is 0: the deterministic build's colours are crt_shoot_rays' (crt_shoot_rays_device's)");
    if (k.gi && o->gi_sample_size > 64u)   // (a frame's rule: crt_launch.hip)
        return refuse("gi_sample_size too large: " + std::to_string(o->gi_sample_size) + ", at most 64");
    if (k.radiance && (uint64_t)o->max_depth + 1 > (uint64_t)MAX_GENERATIONS)   // (a frame's rule as well)
        return refuse("max_depth too large: " + std::to_string(o->max_depth) + " + 1 levels, at most " + std::to_string(MAX_GENERATIONS));
    if (!k.pass) return CRT_OK;   // (crt_shoot_rays_gi_enqueue asks for none: one pass, whose levels the capacities bound)
    uint64_t product = 0;
    *k.pass = shoot_gi_pass_rays(ctx, o, &product);
    if (*k.pass == 0)
        return refuse("the deepest level of a pass of 64 rays may hold 64 x max(2, gi_sample_size)^max_depth = 64 x " + std::to_string(shoot_fan(o, true)) +
                      "^" + std::to_string(o->max_depth) + (product > SHOOT_GI_DEEPEST_RAYS ? " > 64 x 2^26" : " = " + std::to_string(64u * product)) +
                      " rays, more than 2^26");
    return CRT_OK;
}

// the preamble of those entry points: no context is an error, no rays are no work; then the check, then the call
template <typename Run>
static int query_entry(crt_ctx *ctx, const uint64_t n, const CallCheck &k, Run &&run) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    if (int rc = query_check(ctx, k)) return rc;
    return run();
}

extern "C" int crt_trace_rays_device(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, crt_hit *d_out, void *stream) {
    return query_entry(ctx, n, {"crt_trace_rays_device", {d_rays, d_rays, d_out}, ray_type},
                       [&] { return query_run(ctx, closest_call(d_rays, n, ray_type, d_out), (hipStream_t)stream, true); });
}

extern "C" int crt_occluded_rays_device(crt_ctx *ctx, const crt_ray *d_rays, const float *d_max_distance, uint64_t n, uint8_t *d_out, void *stream) {
    return query_entry(ctx, n, {"crt_occluded_rays_device", {d_rays, d_max_distance, d_out}, CRT_RAY_SHADOW},
                       [&] { return query_run(ctx, occluded_call(d_rays, d_max_distance, n, d_out), (hipStream_t)stream, true); });
}

extern "C" int crt_trace_rays(crt_ctx *ctx, const crt_ray *rays, uint64_t n, uint32_t ray_type, crt_hit *out) {
    return query_entry(ctx, n, {"crt_trace_rays", {rays, rays, out}, ray_type}, [&] { return query_host(ctx, closest_call(rays, n, ray_type, out)); });
}

extern "C" int crt_occluded_rays(crt_ctx *ctx, const crt_ray *rays, const float *max_distance, uint64_t n, uint8_t *out) {
    return query_entry(ctx, n, {"crt_occluded_rays", {rays, max_distance, out}, CRT_RAY_SHADOW},
                       [&] { return query_host(ctx, occluded_call(rays, max_distance, n, out)); });
}

extern "C" int crt_shade_hits_device(crt_ctx *ctx, const crt_hit *d_hits, uint64_t n, const crt_options *options, float *d_rgb, uint8_t *d_status,
                                     void *stream) {
    return query_entry(ctx, n, {"crt_shade_hits_device", {d_hits, options, d_rgb}, CRT_RAY_SHADOW, options},
                       [&] { return query_run(ctx, shade_call(d_hits, n, options->shadow_bias, d_rgb, d_status), (hipStream_t)stream, true); });
}

extern "C" int crt_light_points_device(crt_ctx *ctx, const float *d_points, const float *d_normals, uint64_t n, float shadow_bias, float *d_out,
                                       void *stream) {
    return query_entry(ctx, n, {"crt_light_points_device", {d_points, d_normals, d_out}, CRT_RAY_SHADOW},
                       [&] { return query_run(ctx, points_call(d_points, d_normals, n, shadow_bias, d_out), (hipStream_t)stream, true); });
}

extern "C" int crt_shade_hits(crt_ctx *ctx, const crt_hit *hits, uint64_t n, const crt_options *options, float *out_rgb, uint8_t *out_status) {
    return query_entry(ctx, n, {"crt_shade_hits", {hits, options, out_rgb}, CRT_RAY_SHADOW, options},
                       [&] { return query_host(ctx, shade_call(hits, n, options->shadow_bias, out_rgb, out_status)); });
}

extern "C" int crt_light_points(crt_ctx *ctx, const float *points, const float *normals, uint64_t n, float shadow_bias, float *out) {
    return query_entry(ctx, n, {"crt_light_points", {points, normals, out}, CRT_RAY_SHADOW},
                       [&] { return query_host(ctx, points_call(points, normals, n, shadow_bias, out)); });
}

extern "C" int crt_camera_rays_device(crt_ctx *ctx, crt_ray *d_rays, void *stream) {
    if (!ctx) return CRT_ERR_INVALID;
    if (!d_rays) { ctx->error = "crt_camera_rays_device: d_rays is NULL"; return CRT_ERR_INVALID; }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    if (pixels == 0) return CRT_OK;
    hipLaunchKernelGGL(query_camera_rays, dim3((uint32_t)((pixels + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, ctx->camera(), d_rays);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

// the statistics of the last call, harvested first
template <typename T>
static int stats_of(crt_ctx *ctx, T *out, T crt_query_state::*member) {
    if (!ctx || !out) return CRT_ERR_INVALID;
    if (!ctx->query) { *out = T{}; return CRT_OK; }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = query_harvest(ctx)) return rc;
    *out = ctx->query->*member;
    return CRT_OK;
}
extern "C" int crt_get_query_stats(crt_ctx *ctx, crt_query_stats *out) { return stats_of(ctx, out, &crt_query_state::stats); }
extern "C" int crt_get_shoot_stats(crt_ctx *ctx, crt_shoot_stats *out) { return stats_of(ctx, out, &crt_query_state::shoot); }
extern "C" int crt_get_shoot_report(crt_ctx *ctx, crt_shoot_report *out) { return stats_of(ctx, out, &crt_query_state::report); }

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
    float *d_direct;          // crt_shoot_rays_gi_split*: the pass's slice of the direct parts, or null: nothing more is launched
    const ProbeLight *lit;    // crt_shoot_rays_lit*: the volume every level's DIFFUSE records are lit from, or null: nothing more is launched
};

// room for `cap` rays at level g (`own_rgb`: with colours of its own; level 0 writes the caller's array; `keys`: a GI call)
static int shoot_level_reserve(crt_ctx *ctx, const uint32_t g, const uint64_t cap, const bool own_rgb, const bool keys) {
    ShootLevel &L = ctx->query->lv[g];
    return reserve_all(ctx, L.rays, cap, L.hits, cap, L.status, cap, L.nodes, 2 * cap, L.keys, keys ? cap : 0, L.rgb, own_rgb ? 3 * cap : 0);
}

// what crt_shoot_rays*_enqueue adds to a pass's arguments (null: the host reads every level's size back): the levels' capacities, in
// place of the sizes.  The scratch holds them already (shoot_enqueue has seen to it): the pass reserves, waits for and reads nothing.
struct ShootDev {
    uint32_t cap[MAX_GENERATIONS];   // shoot_level_caps (shoot_caps.h)
    crt_shoot_report *d_report;      // the caller's, or null
    bool capturing;                  // the stream is being captured: the library's own copy of the report is not made
};

// A level as its launches see it: n rays -- exactly; or, `count` not null, at most, and that device word says how many (the launches
// are the DEVN builds, sized for what the level may hold).  Level 0's size is the caller's: its launches are those of the other calls.
struct LevelSize { uint32_t n; const uint32_t *count; };

// One pass: m rays of the caller's (at most shoot_pass_rays, or what shoot_gi_pass_rays allows) and every level of them; level 0's
// room is the caller's business.  Leaves the pass's numbers on their way to the pinned SH_* slots (dev: to the pinned report).
struct ShootPass {
    const crt_ray *d_rays; uint32_t m, ray_type; const crt_options *o; float *d_rgb; hipStream_t stream;
    const ShootGi *gi;                       // or null
    const ShootDev *dev;                     // or null
    KernelArgs A;                            // (shoot_pass fills in what follows)
    bool kernels_only;                       // how words are cleared (clear_words), by the levels' launches as well
    LevelSize level[MAX_GENERATIONS + 1];    // the down-sweep's: levels 0 .. last, and {0, null} behind them
    uint32_t last;
};

// Where a pass's numbers go -- the ONE place that tells: through the pinned SH_* slots, which shoot_fold adds up, or (dev) into
// radiance_report's sums and their copy.  `level0`: level 0's hits, QW_HITS as its trace left it (the lighting launches add to that
// word); else the rest, behind the up-sweep.
static int shoot_numbers(crt_ctx *ctx, const ShootPass &P, const bool level0) {
    crt_query_state *q = ctx->query;
    const auto hits = reinterpret_cast<const unsigned long long *>(q->words.p + QW_HITS), diffuse = reinterpret_cast<const unsigned long long *>(q->swords.p + SW_DIFFUSE);
    if (!P.dev) {
        if (level0) {
            CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->pin->shoot + SH_HITS0, hits, sizeof(uint64_t), hipMemcpyDeviceToHost, P.stream));
            return CRT_OK;
        }
        for (uint32_t g = 0; g <= P.last; g++) {
            q->shoot.level_rays[g] += P.level[g].n;
            q->level_peak[g] = std::max<uint64_t>(q->level_peak[g], P.level[g].n);
        }
        q->shoot.levels = std::max(q->shoot.levels, P.last + 1);
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->pin->shoot + SH_DIFFUSE, diffuse, sizeof(uint64_t), hipMemcpyDeviceToHost, P.stream));
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->pin->shoot + SH_REROUTED, q->words.p + QW_REROUTED, sizeof(uint64_t), hipMemcpyDeviceToHost, P.stream));
    } else if (level0) {
        launch_reset(nullptr, 0, nullptr, 0, hits, q->d_hits0.p, P.stream);
        CRT_HIP_CHECK(ctx, hipGetLastError());
    } else {   // the call's numbers, summed where they are
        ReportArgs R{};
        R.count = q->swords.p + SW_COUNT;
        R.hits0 = q->d_hits0.p;
        R.diffuse = diffuse;
        R.rerouted = reinterpret_cast<const unsigned long long *>(q->words.p + QW_REROUTED);
        R.out = P.dev->d_report;
        R.out2 = P.dev->capturing ? nullptr : q->d_report.p;
        R.n = P.m;
        for (uint32_t g = 0; g <= P.last; g++) R.cap[g] = P.level[g].n;   // (0 behind the last level launched)
        hipLaunchKernelGGL(radiance_report, dim3(1), dim3(64), 0, P.stream, R);
        CRT_HIP_CHECK(ctx, hipGetLastError());
        if (!P.dev->capturing) CRT_HIP_CHECK(ctx, hipMemcpyAsync(&q->pin->report, q->d_report.p, sizeof(crt_shoot_report), hipMemcpyDeviceToHost, P.stream));
    }
    return CRT_OK;
}

// radiance_scatter of level g (G: its arguments), and how level g + 1 gets its room -- BEFORE the launch that fills it -- and its size,
// behind it: the ONE place that tells.  Read back through pinned memory and reserve; or (dev) take the capacity, and wait for nothing.
static int shoot_children(crt_ctx *ctx, ShootPass &P, const uint32_t g, RadianceArgs &G) {
    crt_query_state *q = ctx->query;
    const bool gi = P.gi != nullptr;
    const LevelSize S = P.level[g];
    const auto scatter = [&] {
        if (G.spawn) { G.child_rays = q->lv[g + 1].rays.p; G.child_keys = q->lv[g + 1].keys.p; }
        hipLaunchKernelGGL(SCATTER[gi][S.count ? 1 : 0], dim3((uint32_t)(((uint64_t)S.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, P.stream, P.A, G);
        return hipGetLastError();
    };
    if (!G.spawn) {   // the deepest level a ray may reach: no children, and the level behind it stays {0, null}
        CRT_HIP_CHECK(ctx, scatter());
        return CRT_OK;
    }
    if (P.dev) {   // no wait: the next level is launched for what it may hold, and counts for itself
        G.child_cap = P.dev->cap[g + 1];   // (at most what the arrays hold: shoot_enqueue; a child beyond it is the background)
        P.level[g + 1] = {G.child_cap, G.child_count};
        CRT_HIP_CHECK(ctx, scatter());
        return CRT_OK;
    }
    // the next level holds at most `fan` rays for each of this one
    const uint64_t most = shoot_fan(P.o, gi) * S.n;
    if (most > SHOOT_LEVEL_RAYS) { ctx->error = "crt_shoot_rays: a recursion level wider than 2^30 rays"; return CRT_ERR_NOMEM; }
    if (int rc = shoot_level_reserve(ctx, g + 1, most, true, gi)) return rc;
    G.child_cap = (uint32_t)std::min<uint64_t>(q->lv[g + 1].rays.cap, SHOOT_LEVEL_RAYS);
    if (gi) G.child_cap = (uint32_t)std::min<uint64_t>(G.child_cap, q->lv[g + 1].keys.cap);
    CRT_HIP_CHECK(ctx, scatter());
    // the one wait of a level: four bytes through pinned memory, to size the next one
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->pin->shoot + SH_COUNT, G.child_count, sizeof(uint32_t), hipMemcpyDeviceToHost, P.stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(P.stream));
    P.level[g + 1] = {(uint32_t)std::min<uint64_t>(*reinterpret_cast<const uint32_t *>(q->pin->shoot + SH_COUNT), most), nullptr};
    return query_list_reserve(ctx, P.level[g + 1].n);   // (the list follows the widest level)
}

// the down-sweep: level after level, until one has no children
static int shoot_down(crt_ctx *ctx, ShootPass &P) {
    crt_query_state *q = ctx->query;
    const crt_options *o = P.o;
    const bool gi = P.gi != nullptr;
    uint32_t *const d_count = q->swords.p + SW_COUNT;   // [g]: rays appended to level g
    P.level[0] = {P.m, nullptr};
    for (uint32_t g = 0; g <= o->max_depth; g++) {
        const LevelSize S = P.level[g];
        P.last = g;
        const ShootLevel &L = q->lv[g];
        float *rgb = g == 0 ? P.d_rgb : L.rgb.p;
        RadianceArgs G{};
        G.in_rays = P.d_rays; G.rays = L.rays.p; G.hits = L.hits.p; G.status = L.status.p; G.rgb = rgb; G.nodes = L.nodes.p; G.n = S.n; G.n_dev = S.count;
        G.diffuse_total = reinterpret_cast<unsigned long long *>(q->swords.p + SW_DIFFUSE);
        G.reflection_bias = o->reflection_bias; G.refraction_bias = o->refraction_bias;
        if (gi) {
            G.in_keys = P.gi->d_keys; G.keys = L.keys.p; G.gi_samples = o->gi_sample_size; G.gi_seed = o->gi_seed; G.key_first = P.gi->key_first;
            G.monte_carlo_bias = o->monte_carlo_bias;
        }
        if (g == 0) {
            hipLaunchKernelGGL(PREPARE[gi], dim3((uint32_t)(((uint64_t)S.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, P.stream, G);
            CRT_HIP_CHECK(ctx, hipGetLastError());
        }
        // children are REFLECTION or REFRACTION rays, which walk alike: only the caller's own ray can be PRIMARY (Ray.cpp:13)
        QueryCall trace = closest_call(L.rays.p, S.n, g == 0 ? P.ray_type : (uint32_t)CRT_RAY_REFLECTION, L.hits.p);
        QueryCall light = shade_call(L.hits.p, S.n, o->shadow_bias, rgb, L.status.p, gi);
        trace.d_count = light.d_count = S.count;
        trace.kernels_only = light.kernels_only = P.kernels_only;
        int rc = query_launches(ctx, trace, P.stream, g == 0);
        if (rc || (g == 0 && (rc = shoot_numbers(ctx, P, true))) || (rc = query_launches(ctx, light, P.stream, false))) return rc;
        // a split call: level 0's colours are its records' direct light now, and the up-sweep overwrites them (csrc/split_rule.h)
        if (g == 0 && gi && P.gi->d_direct && (rc = split_launch_keep_direct(ctx, L.status.p, rgb, S.n, o->gi_sample_size, P.gi->d_direct, P.stream)))
            return rc;
        // a probe-lit call: the level's DIFFUSE records take their bounce light from the volume now (csrc/probe_lit_rule.h); the pass runs
        // with gi_sample_size = 0, so the up-sweep leaves them as they are
        if (gi && P.gi->lit && (rc = probe_light_launch(ctx, *P.gi->lit, L.hits.p, L.status.p, S.n, rgb, P.stream))) return rc;
        G.child_count = d_count + g + 1;
        G.spawn = g + 1 <= o->max_depth ? 1u : 0u;   // a child enters shootRay with depth g + 1 (RayTracer.cpp:427)
        if ((rc = shoot_children(ctx, P, g, G))) return rc;
        if (P.level[g + 1].n == 0) break;
    }
    return CRT_OK;
}

// the up-sweep: level g's recursing records from level g + 1's colours, which are final by then
static int shoot_up(crt_ctx *ctx, const ShootPass &P) {
    crt_query_state *q = ctx->query;
    for (uint32_t g = P.last + 1; g-- > 0;) {
        const ShootLevel &L = q->lv[g];
        const LevelSize S = P.level[g], C = g < P.last ? P.level[g + 1] : LevelSize{0u, nullptr};
        RadianceArgs G{};
        G.status = L.status.p; G.nodes = L.nodes.p; G.rgb = g == 0 ? P.d_rgb : L.rgb.p; G.n = S.n; G.n_dev = S.count;
        G.child_rgb = g < P.last ? q->lv[g + 1].rgb.p : nullptr;
        G.child_n = C.n; G.child_n_dev = C.count;
        G.gi_samples = P.gi ? P.o->gi_sample_size : 0u;
        // (an enqueue call's up-sweep is the DEVN build at every level, level 0 among them: the sizes it reads are its children's too)
        hipLaunchKernelGGL(COMBINE[P.gi ? 1 : 0][P.dev ? 1 : 0], dim3((uint32_t)(((uint64_t)S.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, P.stream, P.A, G);
        CRT_HIP_CHECK(ctx, hipGetLastError());
    }
    return CRT_OK;
}

static int shoot_pass(crt_ctx *ctx, ShootPass &P) {
    crt_query_state *q = ctx->query;
    P.A.s = (scene_args_p)ctx->d_scene;
    P.A.f = (frame_args_p)q->frame.p;
    P.kernels_only = P.dev != nullptr;   // (kernel launches alone: shoot_enqueue)
    int rc;
    if ((rc = clear_words(ctx, q->words.p, QW_WORDS, q->swords.p, SW_WORDS, P.kernels_only, P.stream)) || (rc = shoot_down(ctx, P)) || (rc = shoot_up(ctx, P))) return rc;
    return shoot_numbers(ctx, P, false);
}

// the radiance queries' own words, the enqueue calls' among them: made by the first radiance call of a context, so that an enqueue
// call inside a capture finds them
static int shoot_words_reserve(crt_ctx *ctx) {
    crt_query_state *q = ctx->query;
    return q->shoot_words_made() ? CRT_OK : reserve_all(ctx, q->swords, SW_WORDS, q->d_report, 1, q->d_hits0, 1);
}

// one device call: n rays, `pass` at a time
static int shoot_run(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *d_rgb, hipStream_t stream,
                     const uint64_t pass, const ShootGi *gi) {
    int rc;
    if ((rc = query_begin(ctx, stream, CALL_RADIANCE)) || (rc = shoot_words_reserve(ctx)) || (rc = call_open(ctx, CALL_RADIANCE, n, stream))) return rc;
    crt_query_state *q = ctx->query;
    for (uint64_t done = 0; done < n; done += pass) {
        if (done) {   // the previous pass's numbers leave the pinned slots before this pass writes them
            CRT_HIP_CHECK(ctx, hipStreamSynchronize(stream));
            shoot_fold(q);
        }
        const uint32_t m = (uint32_t)std::min(n - done, pass);
        ShootGi part{};
        if (gi) {
            part.d_keys = gi->d_keys ? gi->d_keys + done : nullptr;
            part.key_first = gi->key_first + (uint32_t)done;
            part.d_direct = gi->d_direct ? gi->d_direct + 3 * done : nullptr;
            part.lit = gi->lit;
        }
        ShootPass P{d_rays + done, m, ray_type, options, d_rgb + 3 * done, stream, gi ? &part : nullptr, nullptr};
        if ((rc = query_list_reserve(ctx, m)) || (rc = shoot_level_reserve(ctx, 0, m, false, gi != nullptr)) || (rc = shoot_pass(ctx, P))) return rc;
    }
    return call_close(ctx, CALL_RADIANCE, stream);
}

// rays level g's arrays hold now (`own_rgb`, `keys`: as shoot_level_reserve takes them)
static uint64_t shoot_level_room(const crt_query_state *q, const uint32_t g, const bool own_rgb, const bool keys) {
    const ShootLevel &L = q->lv[g];
    uint64_t room = std::min(std::min(L.rays.cap, L.hits.cap), std::min(L.status.cap, L.nodes.cap / 2));
    if (own_rgb) room = std::min(room, L.rgb.cap / 3);
    if (keys) room = std::min(room, L.keys.cap);
    return room;
}

// The start of a call that only enqueues (shoot_enqueue, guide_enqueue) and so may be captured.  Inside a capture nothing may wait,
// allocate or record an event: what the call would need of that is refused, while nothing is enqueued yet, so that the capture stays
// valid.  `made`: the scratch the call cannot do without exists -- else `no_scratch` is the refusal, and `open_call` that of a call
// that would have to be harvested.  Outside a capture: query_begin.
struct Capture {
    crt_ctx *ctx;
    const char *what;
    bool on = false;
    int refuse(const char *why) const {
        ctx->error = std::string(what) + ": the stream is being captured and " + why;
        return CRT_ERR_INVALID;
    }
};
static int capture_begin(crt_ctx *ctx, hipStream_t stream, const CallKind kind, Capture &capture, const bool made, const char *no_scratch,
                         const char *open_call) {
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    CRT_HIP_CHECK(ctx, hipStreamIsCapturing(stream, &status));
    capture.on = status != hipStreamCaptureStatusNone;
    if (!capture.on) return query_begin(ctx, stream, kind);
    if (status != hipStreamCaptureStatusActive) return capture.refuse("the capture is invalidated");
    if (ctx->pending) return capture.refuse("a crt_render_async frame is pending: the call would have to wait for it (crt_wait before the capture)");
    if (!made) return capture.refuse(no_scratch);
    if (ctx->query->call.open) return capture.refuse(open_call);
    return CRT_OK;
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
    Capture capture{ctx, what};
    int rc;
    if ((rc = capture_begin(ctx, stream, CALL_ENQUEUE, capture, ctx->query && ctx->query->shoot_words_made(),
                            "the query scratch would have to grow (the context has none yet): size it with a radiance call before the capture",
                            "an open call would have to be harvested, which waits (crt_get_shoot_stats or crt_get_query_stats before the capture)")) ||
        (!capture.on && (rc = shoot_words_reserve(ctx))))
        return rc;
    const bool capturing = capture.on;
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
            return capture.refuse("the query scratch would have to grow for these rays and capacities: make the same call once before the capture");
    } else {
        if ((rc = query_list_reserve(ctx, widest)) || (rc = shoot_level_reserve(ctx, 0, n, false, keys))) return rc;
        for (uint32_t g = 1; g <= o->max_depth && dev.cap[g]; g++)
            if ((rc = shoot_level_reserve(ctx, g, dev.cap[g], true, keys))) return rc;
        if ((rc = call_open(ctx, CALL_ENQUEUE, n, stream))) return rc;
    }
    dev.d_report = d_report;
    dev.capturing = capturing;
    ShootPass P{d_rays, (uint32_t)n, ray_type, o, d_rgb, stream, gi, &dev};
    rc = shoot_pass(ctx, P);
    if (rc || capturing) return rc;   // (a captured call opens and closes nothing: the replays' numbers are d_report's)
    return call_close(ctx, CALL_ENQUEUE, stream);
}

// the host variants: copy in, run, copy out, `pass` rays at a time; the colours' device copy is level 0's own colour array
static int shoot_host(crt_ctx *ctx, const crt_ray *rays, const uint32_t *keys, uint64_t n, uint32_t ray_type, const crt_options *options, float *out_rgb,
                      const uint64_t pass, const bool gi, float *out_direct = nullptr) {
    const uint64_t m = std::min(n, pass);
    int rc = query_begin(ctx, ctx->stream, CALL_RADIANCE);
    if (rc) return rc;
    crt_query_state *q = ctx->query;
    if ((rc = shoot_level_reserve(ctx, 0, m, true, gi)) || (rc = reserve_all(ctx, q->shoot_in, m, q->shoot_keys, keys ? m : 0, q->shoot_direct, out_direct ? 3 * m : 0)))
        return rc;
    crt_shoot_stats total{};
    crt_query_stats qtotal{};
    for (uint64_t done = 0; done < n; done += pass) {
        const uint64_t k = std::min(n - done, pass);
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->shoot_in.p, rays + done, k * sizeof(crt_ray), hipMemcpyHostToDevice, ctx->stream));
        if (keys) CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->shoot_keys.p, keys + done, k * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        const ShootGi part{keys ? q->shoot_keys.p : nullptr, (uint32_t)done, out_direct ? q->shoot_direct.p : nullptr};
        rc = shoot_run(ctx, q->shoot_in.p, k, ray_type, options, q->lv[0].rgb.p, ctx->stream, pass, gi ? &part : nullptr);
        if (rc) return rc;
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb + 3 * done, q->lv[0].rgb.p, k * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (out_direct) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_direct + 3 * done, q->shoot_direct.p, k * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
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

// the radiance entry points' check: the arrays and the options, ray_type, use_gi as the build has it, max_depth; `pass`: a GI pass's size
static CallCheck shoot_needs(const char *what, const void *rays, const crt_options *options, const void *out, uint32_t ray_type, bool gi, uint64_t *pass) {
    return {what, {rays, options, out}, ray_type, options, true, gi, pass};
}

extern "C" int crt_shoot_rays_device(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *d_rgb,
                                     void *stream) {
    return query_entry(ctx, n, shoot_needs("crt_shoot_rays_device", d_rays, options, d_rgb, ray_type, false, nullptr),
                       [&] { return shoot_run(ctx, d_rays, n, ray_type, options, d_rgb, (hipStream_t)stream, ctx->shoot_pass_rays, nullptr); });
}

extern "C" int crt_shoot_rays(crt_ctx *ctx, const crt_ray *rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *out_rgb) {
    return query_entry(ctx, n, shoot_needs("crt_shoot_rays", rays, options, out_rgb, ray_type, false, nullptr),
                       [&] { return shoot_host(ctx, rays, nullptr, n, ray_type, options, out_rgb, ctx->shoot_pass_rays, false); });
}

extern "C" int crt_shoot_rays_gi_device(crt_ctx *ctx, const crt_ray *d_rays, const uint32_t *d_keys, uint64_t n, uint32_t ray_type,
                                        const crt_options *options, float *d_rgb, void *stream) {
    uint64_t pass = 0;
    const ShootGi gi{d_keys, 0u};
    return query_entry(ctx, n, shoot_needs("crt_shoot_rays_gi_device", d_rays, options, d_rgb, ray_type, true, &pass),
                       [&] { return shoot_run(ctx, d_rays, n, ray_type, options, d_rgb, (hipStream_t)stream, pass, &gi); });
}

extern "C" int crt_shoot_rays_gi(crt_ctx *ctx, const crt_ray *rays, const uint32_t *keys, uint64_t n, uint32_t ray_type, const crt_options *options,
                                 float *out_rgb) {
    uint64_t pass = 0;
    return query_entry(ctx, n, shoot_needs("crt_shoot_rays_gi", rays, options, out_rgb, ray_type, true, &pass),
                       [&] { return shoot_host(ctx, rays, keys, n, ray_type, options, out_rgb, pass, true); });
}

// the split calls (csrc/split_rule.h): the same passes, and radiance_keep_direct behind level 0's lighting in each
static int split_direct_check(crt_ctx *ctx, const char *what, const void *direct, const uint64_t n) {
    if (!ctx || n == 0 || direct) return CRT_OK;   // (no context, no rays: query_entry's business)
    ctx->error = std::string(what) + ": d_direct is NULL with n > 0 (crt_shoot_rays_gi* is the call without it)";
    return CRT_ERR_INVALID;
}

extern "C" int crt_shoot_rays_gi_split_device(crt_ctx *ctx, const crt_ray *d_rays, const uint32_t *d_keys, uint64_t n, uint32_t ray_type,
                                              const crt_options *options, float *d_rgb, float *d_direct, void *stream) {
    const char *what = "crt_shoot_rays_gi_split_device";
    if (int rc = split_direct_check(ctx, what, d_direct, n)) return rc;
    uint64_t pass = 0;
    const ShootGi gi{d_keys, 0u, d_direct};
    return query_entry(ctx, n, shoot_needs(what, d_rays, options, d_rgb, ray_type, true, &pass),
                       [&] { return shoot_run(ctx, d_rays, n, ray_type, options, d_rgb, (hipStream_t)stream, pass, &gi); });
}

extern "C" int crt_shoot_rays_gi_split(crt_ctx *ctx, const crt_ray *rays, const uint32_t *keys, uint64_t n, uint32_t ray_type, const crt_options *options,
                                       float *out_rgb, float *out_direct) {
    const char *what = "crt_shoot_rays_gi_split";
    if (int rc = split_direct_check(ctx, what, out_direct, n)) return rc;
    uint64_t pass = 0;
    return query_entry(ctx, n, shoot_needs(what, rays, options, out_rgb, ray_type, true, &pass),
                       [&] { return shoot_host(ctx, rays, keys, n, ray_type, options, out_rgb, pass, true, out_direct); });
}

extern "C" int crt_shoot_rays_enqueue(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, float *d_rgb,
                                      const uint32_t *level_cap, crt_shoot_report *d_report, void *stream) {
    const char *what = "crt_shoot_rays_enqueue";
    return query_entry(ctx, n, shoot_needs(what, d_rays, options, d_rgb, ray_type, false, nullptr), [&] {
        return shoot_enqueue(ctx, d_rays, n, ray_type, options, d_rgb, level_cap, d_report, (hipStream_t)stream, nullptr, what);
    });
}

extern "C" int crt_shoot_rays_gi_enqueue(crt_ctx *ctx, const crt_ray *d_rays, const uint32_t *d_keys, uint64_t n, uint32_t ray_type,
                                         const crt_options *options, float *d_rgb, const uint32_t *level_cap, crt_shoot_report *d_report,
                                         void *stream) {
    const char *what = "crt_shoot_rays_gi_enqueue";
    const ShootGi gi{d_keys, 0u};
    return query_entry(ctx, n, shoot_needs(what, d_rays, options, d_rgb, ray_type, true, nullptr), [&] {
        return shoot_enqueue(ctx, d_rays, n, ray_type, options, d_rgb, level_cap, d_report, (hipStream_t)stream, &gi, what);
    });
}

// ---- what the GI frame calls (crt_giframe.hip) run of the above: the camera's rays are PRIMARY rays, the arrays are the context's

int query_gi_check(crt_ctx *ctx, const char *what, const crt_options *options, uint64_t *pass) {
    return query_check(ctx, shoot_needs(what, ctx, options, ctx, CRT_RAY_PRIMARY, true, pass));
}

// what crt_shoot_rays_device (use_gi == 0) or crt_shoot_rays_gi_device (use_gi != 0) would refuse of `options` for REFLECTION rays in the
// caller's arrays, asked before anything is enqueued: the entry points' own check, so the rules cannot drift apart
int query_shoot_check(crt_ctx *ctx, const char *what, const crt_options *options) {
    uint64_t pass = 0;
    const bool gi = options->use_gi != 0;
    return query_check(ctx, shoot_needs(what, ctx, options, ctx, CRT_RAY_REFLECTION, gi, gi ? &pass : nullptr));
}

int query_gi_run(crt_ctx *ctx, const crt_ray *d_rays, const uint32_t *d_keys, uint64_t n, const crt_options *options, float *d_rgb, float *d_direct,
                 const uint64_t pass, hipStream_t stream) {
    const ShootGi gi{d_keys, 0u, d_direct};
    return shoot_run(ctx, d_rays, n, CRT_RAY_PRIMARY, options, d_rgb, stream, pass, &gi);
}

// ---- what the probe-lit radiance queries (crt_probes.hip) run of the above
int query_lit_check(crt_ctx *ctx, const char *what, const crt_ray *d_rays, const crt_options *options, const float *d_rgb, const uint32_t ray_type) {
    uint64_t pass = 0;
    return query_check(ctx, shoot_needs(what, d_rays, options, d_rgb, ray_type, true, &pass));
}

int query_lit_run(crt_ctx *ctx, const char *what, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, const ProbeLight *lit,
                  float *d_rgb, hipStream_t stream) {
    crt_options o = *options;
    o.gi_sample_size = 0;   // no sample rays: the volume stands for them
    uint64_t pass = 0;
    if (int rc = query_check(ctx, shoot_needs(what, d_rays, &o, d_rgb, ray_type, true, &pass))) return rc;
    const ShootGi gi{nullptr, 0u, nullptr, lit};
    return shoot_run(ctx, d_rays, n, ray_type, &o, d_rgb, stream, pass, &gi);
}

int query_closest_run(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, crt_hit *d_hits, hipStream_t stream) {
    return query_run(ctx, closest_call(d_rays, n, ray_type, d_hits), stream, true);
}

void query_level_peaks_reset(crt_ctx *ctx) { std::fill(ctx->query->level_peak, ctx->query->level_peak + MAX_GENERATIONS, 0ull); }

// Behind a frame's sample 0: room in the level arrays for later samples, whose levels differ from sample 0's by the pixels whose jittered
// ray meets another material.  shoot_children reserves fan x a level's rays for the level below it; this reserves fan x (the widest such
// level of sample 0's passes and a quarter more), never more than the level can hold at all (fan^g x a pass's rays).  A later sample that
// still outgrows it grows the arrays as any radiance call does: only crt_query_scratch_generation tells.
int query_level_headroom(crt_ctx *ctx, const crt_options *o, const uint64_t pass_rays) {
    crt_query_state *q = ctx->query;
    const uint64_t fan = shoot_fan(o, true);
    uint64_t most = pass_rays, widest = 0;
    for (uint32_t g = 0; g < o->max_depth && q->level_peak[g]; g++) {
        most = std::min<uint64_t>(most * fan, SHOOT_LEVEL_RAYS);
        const uint64_t want = std::min(fan * (q->level_peak[g] + q->level_peak[g] / 4 + 64), most);
        if (int rc = shoot_level_reserve(ctx, g + 1, want, true, true)) return rc;
        widest = std::max(widest, want);
    }
    return query_list_reserve(ctx, widest);
}

extern "C" uint64_t crt_query_scratch_generation(const crt_ctx *ctx) { return ctx ? ctx->scratch_generation : 0; }

// ---- chain guides (crt_guides.hip, csrc/kernel_guides.h): a pixel's chain of closest-hit walks through mirrors and glass.  For level
// k = 0 .. max_bounces: one trace of the live chains (query_launches; behind level 0 the DEVN build, sized for n and reading the list's
// length from the work area's word k), then guide_step, which finalises a pixel or appends its next segment.  Like shoot_enqueue the call
// waits for nothing: a level that ran dry costs empty launches.

// what every guide call asks beyond query_entry's check (NULL arrays, ray_type); nothing is enqueued on a refusal
int guide_check(crt_ctx *ctx, const char *what, const uint64_t n, const uint32_t max_bounces) {
    const auto refuse = [&](const std::string &why) {
        ctx->error = std::string(what) + ": " + why;
        return (int)CRT_ERR_INVALID;
    };
    if (max_bounces > 63u) return refuse("max_bounces is " + std::to_string(max_bounces) + ", at most 63 (the status byte's bits 0-5)");
    if (n > SHOOT_LEVEL_RAYS) return refuse("n = " + std::to_string(n) + " > 2^30 rays; split the rays over several calls");
    const uint64_t meshes = ctx->scene.n_meshes;
    if (meshes * (meshes + 1) >= 0xFFFFFFFFull) return refuse("n_meshes * (n_meshes + 1) >= 2^32 - 1: the mesh tag does not fit 32 bits");
    return CRT_OK;
}

// One call's launches on `stream`; d_work holds crt_guide_work_bytes(n) bytes.  What waits, allocates or records an event happens before
// the first launch and never inside a capture, which is refused what it would need of that (capture_begin).
int guide_enqueue(crt_ctx *ctx, const crt_ray *d_rays, const uint64_t n, const uint32_t ray_type, const float reflection_bias, const float refraction_bias,
                  const uint32_t max_bounces, crt_hit *d_out_hits, uint8_t *d_out_status, crt_ray *d_out_last_rays, void *d_work, hipStream_t stream,
                  const char *what, const bool first) {
    Capture capture{ctx, what};
    int rc;
    if ((rc = capture_begin(ctx, stream, CALL_QUERY, capture, ctx->query && ctx->query->pin,
                            "the query scratch would have to be made (the context has none yet): make the same call once before the capture",
                            "an open call would have to be harvested, which waits (crt_get_query_stats before the capture)")))
        return rc;
    const bool capturing = capture.on;
    if (capturing && uses_filter(ctx) && ctx->query->list.cap < std::min(n, ctx->query_launch_rays))
        return capture.refuse("the query scratch would have to grow for these rays: make the same call once before the capture");
    if (!capturing && (rc = query_list_reserve(ctx, n))) return rc;
    crt_query_state *q = ctx->query;
    const GuideWork W = guides_work(d_work, n);
    // every word starts at zero: the queries' cursors and totals, and the levels' counts in the work area (`first` false, a later round
    // trip of the host variant: the totals stay and the call's statistics add up, as query_run's do)
    if ((rc = first ? clear_words(ctx, q->words.p, QW_WORDS, W.count, GUIDE_COUNT_WORDS, true, stream)
                    : clear_words(ctx, W.count, GUIDE_COUNT_WORDS, nullptr, 0, true, stream)))
        return rc;
    if (!capturing && (rc = call_open(ctx, CALL_QUERY, n, stream, first))) return rc;
    for (uint32_t g = 0; g <= max_bounces; g++) {
        // children are REFLECTION or REFRACTION rays, which walk alike: only the caller's own ray can be PRIMARY (Ray.cpp:13)
        QueryCall trace = closest_call(g == 0 ? d_rays : W.rays[g & 1u], n, g == 0 ? ray_type : (uint32_t)CRT_RAY_REFLECTION, W.hits);
        trace.d_count = g == 0 ? nullptr : W.count + g;
        trace.kernels_only = true;
        if ((rc = query_launches(ctx, trace, stream, g == 0 && first)) ||
            (rc = guides_launch_step(ctx, W, d_rays, (uint32_t)n, g, max_bounces, reflection_bias, refraction_bias, d_out_hits, d_out_status,
                                     d_out_last_rays, stream)))
            return rc;
    }
    if (capturing) return CRT_OK;   // (a captured call opens and closes nothing)
    CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->pin->words, q->words.p, QW_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    return call_close(ctx, CALL_QUERY, stream);
}

extern "C" int crt_guide_rays_device(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options, uint32_t max_bounces,
                                     crt_hit *d_out_hits, uint8_t *d_out_status, crt_ray *d_out_last_rays, void *d_work, void *stream) {
    const char *what = "crt_guide_rays_device";
    // (options are not handed to the check: use_gi may be left set, nothing of the GI build is involved)
    return query_entry(ctx, n, {what, {d_rays, options, d_out_hits}, ray_type}, [&] {
        if (int rc = guide_check(ctx, what, n, max_bounces)) return rc;
        if (!d_work || (reinterpret_cast<uintptr_t>(d_work) & 15u)) {
            ctx->error = std::string(what) + ": d_work is NULL or not aligned to 16 bytes";
            return (int)CRT_ERR_INVALID;
        }
        return guide_enqueue(ctx, d_rays, n, ray_type, options->reflection_bias, options->refraction_bias, max_bounces, d_out_hits, d_out_status,
                             d_out_last_rays, d_work, (hipStream_t)stream, what);
    });
}

// the host variant: copy in, run, copy out, query_host_rays at a time, through device copies that are kept for the next call
extern "C" int crt_guide_rays(crt_ctx *ctx, const crt_ray *rays, uint64_t n, uint32_t ray_type, const crt_options *options, uint32_t max_bounces,
                              crt_hit *out_hits, uint8_t *out_status, crt_ray *out_last_rays) {
    const char *what = "crt_guide_rays";
    return query_entry(ctx, n, {what, {rays, options, out_hits}, ray_type}, [&]() -> int {
        int rc;
        if ((rc = guide_check(ctx, what, n, max_bounces)) || (rc = query_begin(ctx, ctx->stream, CALL_QUERY))) return rc;
        crt_query_state *q = ctx->query;
        const uint64_t cap = std::min(n, ctx->query_host_rays);
        if ((rc = reserve_all(ctx, q->s_rays, cap, q->s_hits, cap, q->g_status, cap, q->g_last, cap, q->g_work,
                              float4s(crt_guide_work_bytes(cap)))))
            return rc;
        for (uint64_t done = 0; done < n; done += ctx->query_host_rays) {
            const uint64_t m = std::min(n - done, ctx->query_host_rays);
            CRT_HIP_CHECK(ctx, hipMemcpyAsync(q->s_rays.p, rays + done, m * sizeof(crt_ray), hipMemcpyHostToDevice, ctx->stream));
            if ((rc = guide_enqueue(ctx, q->s_rays.p, m, ray_type, options->reflection_bias, options->refraction_bias, max_bounces, q->s_hits.p,
                                    q->g_status.p, q->g_last.p, q->g_work.p, ctx->stream, what, done == 0)))
                return rc;
            CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_hits + done, q->s_hits.p, m * sizeof(crt_hit), hipMemcpyDeviceToHost, ctx->stream));
            if (out_status) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_status + done, q->g_status.p, m, hipMemcpyDeviceToHost, ctx->stream));
            if (out_last_rays) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_last_rays + done, q->g_last.p, m * sizeof(crt_ray), hipMemcpyDeviceToHost, ctx->stream));
            CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            if ((rc = query_harvest(ctx))) return rc;
        }
        return (int)CRT_OK;
    });
}
