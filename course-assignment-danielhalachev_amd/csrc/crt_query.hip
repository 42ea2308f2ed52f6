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
// scratch below is the queries' own.  The shape of the file:
//   an entry point    query_entry: the preamble and the one argument check (query_check, told what the call needs by a CallCheck)
//   a call            query_begin (the waiting rule: call_wait.h), then its launches between call_open and call_close
//   its launches      query_launches: the filter / reroute pair of the call's kind from one table (PAIRS); clear_words clears every word
//   a radiance pass   shoot_pass: shoot_down (level behind level), shoot_up, shoot_numbers.  The synchronous and the enqueue form part in
//                     shoot_children (a level's room and size), clear_words and shoot_numbers -- and in shoot_up's choice of build --,
//                     and nowhere in the level loop
//   a progressive frame  crt_render_progressive, at the end of this file: a GI frame sample pass by sample pass -- the rays and keys of one
//                     sample (crt_camera_sample_rays_device), shoot_run, one step of the pixel's fold (crt_accumulate_samples_device);
//                     kernels: csrc/kernel_progressive.h
//   an adaptive frame  crt_render_adaptive, behind it: the same loop over a pixel list that shrinks -- the step, the rule and the
//                     compaction of crt_adaptive_step_device; kernels: csrc/kernel_adaptive.h, the rule: csrc/adaptive_rule.h
//   a denoised frame  crt_render_denoised, last: the adaptive frame's state through the denoiser's primitives (crt_denoise.hip), guided by
//                     the first hits of the camera's rays; it changes nothing of the frame
//   an accumulated frame  crt_render_accumulated: that state merged with the last frame's history through the temporal primitive
//                     (crt_temporal.hip), then through the denoiser's launches; the context's two history slots
//   a split frame     crt_render_adaptive_split, crt_render_denoised_split, crt_render_accumulated_split: the three calls above with every
//                     sample cut into its direct light and the rest (crt_split.hip, csrc/split_rule.h) -- the rest is what is filtered and
//                     reprojected, the direct part is added back untouched; one body each for the split and the unsplit call
#include "crt_internal.h"
#include "glibc_powf.h"
#include "gi_random.h"
#include "shoot_caps.h"
#include "call_wait.h"

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
#include "kernel_progressive.h"
#include "kernel_adaptive.h"
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
// reserve_all(ctx, a, n, b, m, ...): room for n elements in a, m in b, ...; the first failure ends it
int reserve_all(crt_ctx *) { return CRT_OK; }
template <typename T, typename... More>
int reserve_all(crt_ctx *ctx, DeviceArray<T> &a, const uint64_t n, More &&...more) {
    if (int rc = a.reserve(ctx, n)) return rc;
    return reserve_all(ctx, more...);
}

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
    uint32_t adaptive_n;        // crt_render_adaptive: the next pass's list length, copied behind a pass's scatter
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
    uint64_t generation = 0;                  // crt_query_scratch_generation
    // crt_render_progressive: the frame's H*W*3 sums, one sample's rays, keys and colours for every pixel, the samples folded in so far
    DeviceArray<float> prog_sum, prog_rgb;
    DeviceArray<crt_ray> prog_rays;
    DeviceArray<uint32_t> prog_keys;
    uint32_t prog_samples = 0;
    // crt_render_adaptive: the frame above with one float and one count more per pixel, two pixel lists (this pass's and the next one's),
    // the next list's length, the compaction's work area; which kind of frame is under way, its latched settings and its list
    DeviceArray<float> prog_sq;
    DeviceArray<uint32_t> prog_counts, prog_list[2], prog_next_n;
    DeviceArray<unsigned long long> prog_work;
    bool prog_is_adaptive = false;
    // crt_render_adaptive_split: the adaptive frame is a SPLIT one (latched at pass 0) -- beside the fold's state the sums of the samples'
    // direct parts and the first and second moment of the rest (csrc/split_rule.h), and one pass's direct parts beside prog_rgb
    bool prog_is_split = false;
    DeviceArray<float> split_direct, split_dsum, split_rsum, split_rsq;
    crt_adaptive prog_adaptive{};
    uint64_t prog_active = 0;   // entries of prog_list[prog_cur]; pass 0 has no list (every pixel)
    int prog_cur = 0;
    // crt_render_denoised: the guides (the first hits of the camera's centre rays, traced at a frame's first denoise call and kept until the
    // frame is reset), the mean and variance of the fold's state, the denoised frame, the primitive's work area, the quantised frame
    DeviceArray<crt_hit> den_hits;
    DeviceArray<float> den_mean, den_var, den_out;
    DeviceArray<float4> den_work;
    DeviceArray<uint8_t> den_q8;
    bool den_guides = false;
    // crt_set_guide_bounces > 0: beside them the chain guides of the same rays (crt_guide_rays_device's records), which the spatial filter
    // then runs under, and that call's work area; traced and dropped with den_hits.  The biases are those of the frame's pass 0
    DeviceArray<crt_hit> den_chain;
    DeviceArray<float4> guide_work;
    float prog_reflection_bias = 0, prog_refraction_bias = 0;
    // crt_guide_rays: the host variant's device copies of the status bytes and terminal rays, and its work area
    DeviceArray<uint8_t> g_status;
    DeviceArray<crt_ray> g_last;
    DeviceArray<float4> g_work;
    // crt_render_accumulated*: the frame's serial number (it advances wherever den_guides is dropped); a History -- two slots with the pose
    // of the frame that wrote each: slot[cur] is `current`, slot[cur ^ 1] `previous`; the serial `current` was written at; the frames
    // merged since crt_history_reset --; and the merged colour, variance and valid-tap counts.  There are two histories: hist[0] holds the
    // moments of whole colours (crt_render_accumulated), hist[1] those of the rest (crt_render_accumulated_split), which must never meet
    uint64_t frame_serial = 0;
    struct History {
        uint64_t serial = 0;
        DeviceArray<crt_history_pixel> slot[2];
        crt_camera_pose pose[2] = {};
        int cur = 0;
        bool has_cur = false, has_prev = false;
        uint32_t frames = 0;
        void reset() { has_cur = has_prev = false; frames = 0; }   // (the slots stay allocated: nothing reads them until a call has written one again)
    } hist[2];
    DeviceArray<float> acc_rgb, acc_var;
    DeviceArray<uint8_t> acc_valid;
    void new_frame() { den_guides = false; frame_serial++; }   // the guides and `current` are the ended frame's
    uint64_t level_peak[MAX_GENERATIONS] = {};   // the widest level g of a pass since a progressive frame's sample 0 began (shoot_numbers)
    // the radiance queries' own device words: made by the first radiance call of a context (shoot_words_reserve)
    bool shoot_words_made() const { return swords.p && d_report.p && d_hits0.p; }
    ~crt_query_state() {
        if (pin) (void)hipHostFree(pin);
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

// crt_set_camera and crt_render*: the progressive frame under way, if any, is no longer the context's frame
void query_progressive_reset(crt_ctx *ctx) {
    if (!ctx->query) return;
    ctx->query->prog_samples = 0;
    ctx->query->prog_active = 0;
    ctx->query->new_frame();
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
static int query_begin(crt_ctx *ctx, hipStream_t stream, const CallKind kind) {
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
        if (!ctx->query || !ctx->query->shoot_words_made())
            return refuse("the query scratch would have to grow (the context has none yet): size it with a radiance call before the capture");
        if (ctx->query->call.open)
            return refuse("an open call would have to be harvested, which waits (crt_get_shoot_stats or crt_get_query_stats before the capture)");
    } else if ((rc = query_begin(ctx, stream, CALL_ENQUEUE)) || (rc = shoot_words_reserve(ctx))) return rc;
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

extern "C" uint64_t crt_query_scratch_generation(const crt_ctx *ctx) { return ctx && ctx->query ? ctx->query->generation : 0; }

// ---- chain guides (crt_guides.hip, csrc/kernel_guides.h): a pixel's chain of closest-hit walks through mirrors and glass.  For level
// k = 0 .. max_bounces: one trace of the live chains (query_launches; behind level 0 the DEVN build, sized for n and reading the list's
// length from the work area's word k), then guide_step, which finalises a pixel or appends its next segment.  Like shoot_enqueue the call
// waits for nothing: a level that ran dry costs empty launches.

// what every guide call asks beyond query_entry's check (NULL arrays, ray_type); nothing is enqueued on a refusal
static int guide_check(crt_ctx *ctx, const char *what, const uint64_t n, const uint32_t max_bounces) {
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
// the first launch and never inside a capture, which is refused what it would need of that (shoot_enqueue's rule).
static int guide_enqueue(crt_ctx *ctx, const crt_ray *d_rays, const uint64_t n, const uint32_t ray_type, const float reflection_bias,
                         const float refraction_bias, const uint32_t max_bounces, crt_hit *d_out_hits, uint8_t *d_out_status, crt_ray *d_out_last_rays,
                         void *d_work, hipStream_t stream, const char *what, const bool first = true) {
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
        if (!ctx->query || !ctx->query->pin) return refuse("the query scratch would have to be made (the context has none yet): make the same call once before the capture");
        if (ctx->query->call.open) return refuse("an open call would have to be harvested, which waits (crt_get_query_stats before the capture)");
        if (uses_filter(ctx) && ctx->query->list.cap < std::min(n, ctx->query_launch_rays))
            return refuse("the query scratch would have to grow for these rays: make the same call once before the capture");
    } else if ((rc = query_begin(ctx, stream, CALL_QUERY)) || (rc = query_list_reserve(ctx, n))) return rc;
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
                              (crt_guide_work_bytes(cap) + sizeof(float4) - 1) / sizeof(float4))))
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

// ---- progressive GI frames (csrc/kernel_progressive.h): the frame's left fold over a pixel's samples, cut into sample passes.

static QueryCamera camera_of(const crt_ctx *ctx) {
    QueryCamera cam;
    memcpy(cam.pos, ctx->frame.cam_pos, sizeof(cam.pos));   // crt_set_camera's last word, as crt_camera_rays_device takes it
    memcpy(cam.m, ctx->frame.cam, sizeof(cam.m));
    cam.width = ctx->width; cam.height = ctx->height;
    return cam;
}

// what the two primitives ask of (d_pixels, n): without a list the call is for the whole frame; one thread per entry must fit a grid
int progressive_check(crt_ctx *ctx, const char *what, const uint32_t *d_pixels, const uint64_t n) {
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    if (!d_pixels && n != pixels) {
        ctx->error = std::string(what) + ": d_pixels is NULL, so n must be width * height = " + std::to_string(pixels) + ", not " + std::to_string(n);
        return CRT_ERR_INVALID;
    }
    if (pixels > 0xFFFFFFFFull || (n + BLOCK - 1) / BLOCK > 0x7FFFFFFFull) {
        ctx->error = std::string(what) + ": more pixels or entries than 32-bit pixel indices and one launch hold";
        return CRT_ERR_INVALID;
    }
    return CRT_OK;
}

static int launch_sample_rays(crt_ctx *ctx, uint32_t gi_seed, uint32_t sample, const uint32_t *d_pixels, uint64_t n, crt_ray *d_rays, uint32_t *d_keys,
                              hipStream_t stream) {
    SampleRaysArgs P{};
    P.cam = camera_of(ctx);
    P.seed = gi_seed; P.sample = sample; P.pixels = d_pixels; P.n = n; P.rays = d_rays; P.keys = d_keys;
    hipLaunchKernelGGL(progressive_sample_rays, dim3((uint32_t)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, P);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

static int launch_accumulate(crt_ctx *ctx, const float *d_rgb, const uint32_t *d_pixels, uint64_t n, uint32_t sample, float *d_sum, float *d_mean,
                             hipStream_t stream) {
    AccumulateArgs P{};
    P.rgb = d_rgb; P.pixels = d_pixels; P.n = n; P.frame_pixels = (uint64_t)ctx->width * ctx->height; P.sample = sample; P.sum = d_sum; P.mean = d_mean;
    hipLaunchKernelGGL(progressive_accumulate, dim3((uint32_t)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, P);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

extern "C" int crt_camera_sample_rays_device(crt_ctx *ctx, uint32_t gi_seed, uint32_t sample, const uint32_t *d_pixels, uint64_t n, crt_ray *d_rays,
                                             uint32_t *d_keys, void *stream) {
    const char *what = "crt_camera_sample_rays_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = progressive_check(ctx, what, d_pixels, n)) return rc;
    if (n == 0) return CRT_OK;
    if (!d_rays) { ctx->error = std::string(what) + ": d_rays is NULL"; return CRT_ERR_INVALID; }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return launch_sample_rays(ctx, gi_seed, sample, d_pixels, n, d_rays, d_keys, (hipStream_t)stream);
}

extern "C" int crt_accumulate_samples_device(crt_ctx *ctx, const float *d_rgb, const uint32_t *d_pixels, uint64_t n, uint32_t sample, float *d_sum,
                                             float *d_mean, void *stream) {
    const char *what = "crt_accumulate_samples_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = progressive_check(ctx, what, d_pixels, n)) return rc;
    if (n == 0) return CRT_OK;
    if (!d_rgb || !d_sum) { ctx->error = std::string(what) + ": d_rgb or d_sum is NULL"; return CRT_ERR_INVALID; }
    if (sample == 0xFFFFFFFFu) { ctx->error = std::string(what) + ": sample + 1 does not fit 32 bits"; return CRT_ERR_INVALID; }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return launch_accumulate(ctx, d_rgb, d_pixels, n, sample, d_sum, d_mean, (hipStream_t)stream);
}

extern "C" uint32_t crt_progressive_samples(const crt_ctx *ctx) { return ctx && ctx->query ? ctx->query->prog_samples : 0u; }

// Behind a frame's sample 0: room in the level arrays for later samples, whose levels differ from sample 0's by the pixels whose jittered
// ray meets another material.  shoot_children reserves fan x a level's rays for the level below it; this reserves fan x (the widest such
// level of sample 0's passes and a quarter more), never more than the level can hold at all (fan^g x a pass's rays).  A later sample that
// still outgrows it grows the arrays as any radiance call does: only crt_query_scratch_generation tells.
static int progressive_headroom(crt_ctx *ctx, const crt_options *o, const uint64_t pass_rays) {
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

extern "C" int crt_render_progressive(crt_ctx *ctx, const crt_options *options, uint32_t first_sample, uint32_t n_samples, float *out_rgb) {
    const char *what = "crt_render_progressive";
    if (!ctx) return CRT_ERR_INVALID;
    if (n_samples == 0) return CRT_OK;
    // the GI radiance calls' own check: the camera's rays are PRIMARY rays, the arrays are the context's
    uint64_t pass = 0;
    if (int rc = query_check(ctx, shoot_needs(what, ctx, options, ctx, CRT_RAY_PRIMARY, true, &pass))) return rc;
    if (first_sample != 0 && first_sample != crt_progressive_samples(ctx)) {   // (0 starts a new frame, whatever the context holds)
        ctx->error = std::string(what) + ": first_sample is " + std::to_string(first_sample) + ", but the context's frame holds " +
                     std::to_string(crt_progressive_samples(ctx)) + " samples (crt_progressive_samples; 0 starts a new frame)";
        return CRT_ERR_INVALID;
    }
    if (first_sample != 0 && ctx->query->prog_is_adaptive) {   // (first_sample == the count > 0: the context has a query state)
        ctx->error = std::string(what) + ": the frame under way is an ADAPTIVE frame (crt_render_adaptive continues it; first_sample 0 starts a new frame)";
        return CRT_ERR_INVALID;
    }
    if ((uint64_t)first_sample + n_samples > 0xFFFFFFFFull) { ctx->error = std::string(what) + ": more than 2^32 - 1 samples"; return CRT_ERR_INVALID; }
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    if (pixels == 0) return CRT_OK;
    int rc;
    if ((rc = progressive_check(ctx, what, nullptr, pixels)) || (rc = query_begin(ctx, ctx->stream, CALL_RADIANCE))) return rc;
    crt_query_state *q = ctx->query;
    if ((rc = reserve_all(ctx, q->prog_sum, 3 * pixels, q->prog_rgb, 3 * pixels, q->prog_rays, pixels, q->prog_keys, pixels))) return rc;
    const ShootGi gi{q->prog_keys.p, 0u};
    for (uint32_t s = first_sample; s - first_sample < n_samples; s++) {   // one at a time and in order: the fold's order is the frame's
        if (s == 0) {
            std::fill(q->level_peak, q->level_peak + MAX_GENERATIONS, 0ull);
            q->prog_is_adaptive = q->prog_is_split = false;
            q->new_frame();
            q->prog_active = pixels;   // (a uniform frame shoots every pixel in every pass)
        }
        if ((rc = launch_sample_rays(ctx, options->gi_seed, s, nullptr, pixels, q->prog_rays.p, q->prog_keys.p, ctx->stream)) ||
            (rc = shoot_run(ctx, q->prog_rays.p, pixels, CRT_RAY_PRIMARY, options, q->prog_rgb.p, ctx->stream, pass, &gi)) ||
            (rc = launch_accumulate(ctx, q->prog_rgb.p, nullptr, pixels, s, q->prog_sum.p, ctx->d_frame, ctx->stream)))
            return rc;
        q->prog_samples = s + 1;
        if (s == 0 && (rc = progressive_headroom(ctx, options, std::min(pixels, pass)))) return rc;
    }
    if (out_rgb) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb, ctx->d_frame, 3 * pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return CRT_OK;
}

// ---- adaptive sampling (csrc/kernel_adaptive.h, csrc/adaptive_rule.h): the progressive frame's loop over a pixel list that shrinks.

extern "C" void crt_adaptive_defaults(crt_adaptive *a) {
    if (!a) return;
    a->size = (uint32_t)sizeof(crt_adaptive);
    a->min_samples = 4;
    a->max_samples = 64;
    a->threshold = 0.05f;
    a->floor = 1e-4f;
}

static uint64_t adaptive_blocks(const uint64_t n) { return (n + BLOCK - 1) / BLOCK; }

extern "C" size_t crt_adaptive_work_bytes(uint64_t n) {
    const uint64_t blocks = adaptive_blocks(n);
    return (size_t)(blocks * ADAPTIVE_WAVES * sizeof(unsigned long long) + 2 * blocks * sizeof(uint32_t));
}

static int adaptive_check(crt_ctx *ctx, const char *what, const crt_adaptive *a) {
    const char *why = nullptr;
    if (!a) why = "adaptive is NULL";
    else if (a->size != sizeof(crt_adaptive)) why = "adaptive->size is not sizeof(crt_adaptive)";
    else if (a->min_samples == 0) why = "min_samples is 0";
    else if (a->max_samples < a->min_samples) why = "max_samples < min_samples";
    else if (!(a->threshold >= 0.0f) || !std::isfinite(a->threshold)) why = "threshold is negative or not finite";
    else if (!(a->floor >= 0.0f) || !std::isfinite(a->floor)) why = "floor is negative or not finite";
    if (!why) return CRT_OK;
    ctx->error = std::string(what) + ": " + why;
    return CRT_ERR_INVALID;
}

// the step, the scan and the scatter of n > 0 entries, one behind the other on `stream`
static int launch_adaptive(crt_ctx *ctx, const float *d_rgb, const uint32_t *d_pixels, uint64_t n, uint32_t sample, const crt_adaptive *a, float *d_sum,
                           float *d_sq, float *d_mean, uint32_t *d_counts, uint32_t *d_next, uint32_t *d_next_n, void *d_work, hipStream_t stream) {
    const uint32_t blocks = (uint32_t)adaptive_blocks(n);
    AdaptiveWork work{};
    work.masks = (unsigned long long *)d_work;
    work.counts = (uint32_t *)(work.masks + (uint64_t)blocks * ADAPTIVE_WAVES);
    work.offsets = work.counts + blocks;
    AdaptiveStepArgs S{};
    S.rgb = d_rgb; S.pixels = d_pixels; S.n = n; S.frame_pixels = (uint64_t)ctx->width * ctx->height; S.sample = sample;
    S.rule = crt_adaptive_rule{a->min_samples, a->max_samples, a->threshold, a->floor};
    S.sum = d_sum; S.sq = d_sq; S.mean = d_mean; S.count = d_counts; S.work = work;
    hipLaunchKernelGGL(adaptive_step, dim3(blocks), dim3(BLOCK), 0, stream, S);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    const AdaptiveScanArgs C{work.counts, work.offsets, d_next_n, blocks};
    hipLaunchKernelGGL(adaptive_scan, dim3(1), dim3(BLOCK), 0, stream, C);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    const AdaptiveScatterArgs T{d_pixels, n, work, d_next};
    hipLaunchKernelGGL(adaptive_scatter, dim3(blocks), dim3(BLOCK), 0, stream, T);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

extern "C" int crt_adaptive_step_device(crt_ctx *ctx, const float *d_rgb, const uint32_t *d_pixels, uint64_t n, uint32_t sample, const crt_adaptive *adaptive,
                                        float *d_sum, float *d_sq, float *d_mean, uint32_t *d_counts, uint32_t *d_next_pixels, uint32_t *d_next_n,
                                        void *d_work, void *stream) {
    const char *what = "crt_adaptive_step_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = adaptive_check(ctx, what, adaptive)) return rc;
    if (int rc = progressive_check(ctx, what, d_pixels, n)) return rc;
    if (n > 0xFFFFFFFFull) { ctx->error = std::string(what) + ": the next list's length is one 32-bit word: n = " + std::to_string(n) + " > 2^32 - 1"; return CRT_ERR_INVALID; }
    if (!d_next_n) { ctx->error = std::string(what) + ": d_next_n is NULL"; return CRT_ERR_INVALID; }
    if (n != 0) {
        if (!d_rgb || !d_sum || !d_sq || !d_counts || !d_next_pixels || !d_work) {
            ctx->error = std::string(what) + ": d_rgb, d_sum, d_sq, d_counts, d_next_pixels or d_work is NULL";
            return CRT_ERR_INVALID;
        }
        if (d_next_pixels == d_pixels) { ctx->error = std::string(what) + ": d_next_pixels must not alias d_pixels"; return CRT_ERR_INVALID; }
        if ((uintptr_t)d_work % alignof(unsigned long long)) { ctx->error = std::string(what) + ": d_work must be aligned to 8 bytes"; return CRT_ERR_INVALID; }
        if (sample == 0xFFFFFFFFu) { ctx->error = std::string(what) + ": sample + 1 does not fit 32 bits"; return CRT_ERR_INVALID; }
    }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (n == 0) {   // no entry: the next list is empty, and nothing else is written
        CRT_HIP_CHECK(ctx, hipMemsetAsync(d_next_n, 0, sizeof(uint32_t), (hipStream_t)stream));
        return CRT_OK;
    }
    return launch_adaptive(ctx, d_rgb, d_pixels, n, sample, adaptive, d_sum, d_sq, d_mean, d_counts, d_next_pixels, d_next_n, d_work, (hipStream_t)stream);
}

extern "C" uint64_t crt_progressive_active(const crt_ctx *ctx) {
    return ctx && ctx->query && ctx->query->prog_samples ? ctx->query->prog_active : 0ull;
}

static bool same_adaptive(const crt_adaptive &a, const crt_adaptive &b) {
    return a.min_samples == b.min_samples && a.max_samples == b.max_samples && a.threshold == b.threshold && a.floor == b.floor;
}

// crt_render_adaptive and, `split`, crt_render_adaptive_split: the same loop with the split shoot and, behind a pass's step, split_fold on
// the same list and sample.  What the unsplit call produces is untouched by it.
static int render_adaptive(crt_ctx *ctx, const char *what, const bool split, const crt_options *options, const crt_adaptive *adaptive, uint32_t first_pass,
                           uint32_t n_passes, float *out_rgb, uint32_t *out_counts) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n_passes == 0) return CRT_OK;
    uint64_t pass = 0;
    if (int rc = query_check(ctx, shoot_needs(what, ctx, options, ctx, CRT_RAY_PRIMARY, true, &pass))) return rc;
    if (int rc = adaptive_check(ctx, what, adaptive)) return rc;
    if (first_pass != 0 && first_pass != crt_progressive_samples(ctx)) {   // (0 starts a new frame, whatever the context holds)
        ctx->error = std::string(what) + ": first_pass is " + std::to_string(first_pass) + ", but the context's frame holds " +
                     std::to_string(crt_progressive_samples(ctx)) + " passes (crt_progressive_samples; 0 starts a new frame)";
        return CRT_ERR_INVALID;
    }
    if (first_pass != 0 && !ctx->query->prog_is_adaptive) {
        ctx->error = std::string(what) + ": the frame under way is a UNIFORM progressive frame (crt_render_progressive continues it; first_pass 0 starts a new frame)";
        return CRT_ERR_INVALID;
    }
    if (first_pass != 0 && ctx->query->prog_is_split != split) {
        ctx->error = std::string(what) + (split ? ": the frame under way is an UNSPLIT adaptive frame (crt_render_adaptive continues it; first_pass 0 starts a new frame)"
                                                : ": the frame under way is a SPLIT adaptive frame (crt_render_adaptive_split continues it; first_pass 0 starts a new frame)");
        return CRT_ERR_INVALID;
    }
    if (first_pass != 0 && !same_adaptive(*adaptive, ctx->query->prog_adaptive)) {
        ctx->error = std::string(what) + ": adaptive differs from the settings latched by the frame's pass 0";
        return CRT_ERR_INVALID;
    }
    if ((uint64_t)first_pass + n_passes > 0xFFFFFFFFull) { ctx->error = std::string(what) + ": more than 2^32 - 1 passes"; return CRT_ERR_INVALID; }
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    if (pixels == 0) return CRT_OK;
    int rc;
    if ((rc = progressive_check(ctx, what, nullptr, pixels)) || (rc = query_begin(ctx, ctx->stream, CALL_RADIANCE))) return rc;
    crt_query_state *q = ctx->query;
    if ((rc = reserve_all(ctx, q->prog_sum, 3 * pixels, q->prog_rgb, 3 * pixels, q->prog_rays, pixels, q->prog_keys, pixels, q->prog_sq, pixels,
                          q->prog_counts, pixels, q->prog_list[0], pixels, q->prog_list[1], pixels, q->prog_next_n, 1, q->prog_work,
                          (crt_adaptive_work_bytes(pixels) + 7) / 8)) ||
        (split && (rc = reserve_all(ctx, q->split_direct, 3 * pixels, q->split_dsum, 3 * pixels, q->split_rsum, 3 * pixels, q->split_rsq, pixels))))
        return rc;
    const ShootGi gi{q->prog_keys.p, 0u, split ? q->split_direct.p : nullptr};
    for (uint32_t s = first_pass; s - first_pass < n_passes; s++) {   // one at a time and in order: the fold's order is the frame's
        if (s == 0) {
            std::fill(q->level_peak, q->level_peak + MAX_GENERATIONS, 0ull);
            q->prog_is_adaptive = true;
            q->prog_is_split = split;
            q->new_frame();            // (a new frame: crt_render_denoised traces its guides again)
            q->prog_adaptive = *adaptive;
            q->prog_reflection_bias = options->reflection_bias;
            q->prog_refraction_bias = options->refraction_bias;
            q->prog_active = pixels;
        }
        const uint64_t n = q->prog_active;
        if (n != 0) {   // (an empty list launches nothing: every pixel has stopped, or reached max_samples)
            const uint32_t *list = s == 0 ? nullptr : q->prog_list[q->prog_cur].p;   // pass 0: every pixel
            uint32_t *next = q->prog_list[s == 0 ? 0 : q->prog_cur ^ 1].p;
            if ((rc = launch_sample_rays(ctx, options->gi_seed, s, list, n, q->prog_rays.p, q->prog_keys.p, ctx->stream)) ||
                (rc = shoot_run(ctx, q->prog_rays.p, n, CRT_RAY_PRIMARY, options, q->prog_rgb.p, ctx->stream, pass, &gi)) ||
                (rc = launch_adaptive(ctx, q->prog_rgb.p, list, n, s, adaptive, q->prog_sum.p, q->prog_sq.p, ctx->d_frame, q->prog_counts.p, next,
                                      q->prog_next_n.p, q->prog_work.p, ctx->stream)) ||
                (split && (rc = split_launch_fold(ctx, q->prog_rgb.p, q->split_direct.p, list, n, s, q->split_dsum.p, q->split_rsum.p, q->split_rsq.p,
                                                  ctx->stream))))
                return rc;
            // the next list's length: 4 bytes through pinned memory, once a pass
            CRT_HIP_CHECK(ctx, hipMemcpyAsync(&q->pin->adaptive_n, q->prog_next_n.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            q->prog_active = q->pin->adaptive_n;
            if (s != 0) q->prog_cur ^= 1;
            else q->prog_cur = 0;
        }
        q->prog_samples = s + 1;
        if (s == 0 && (rc = progressive_headroom(ctx, options, std::min(pixels, pass)))) return rc;
    }
    if (out_rgb) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb, ctx->d_frame, 3 * pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (out_counts) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_counts, q->prog_counts.p, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return CRT_OK;
}

extern "C" int crt_render_adaptive(crt_ctx *ctx, const crt_options *options, const crt_adaptive *adaptive, uint32_t first_pass, uint32_t n_passes,
                                   float *out_rgb, uint32_t *out_counts) {
    return render_adaptive(ctx, "crt_render_adaptive", false, options, adaptive, first_pass, n_passes, out_rgb, out_counts);
}

extern "C" int crt_render_adaptive_split(crt_ctx *ctx, const crt_options *options, const crt_adaptive *adaptive, uint32_t first_pass, uint32_t n_passes,
                                         float *out_rgb, uint32_t *out_counts) {
    return render_adaptive(ctx, "crt_render_adaptive_split", true, options, adaptive, first_pass, n_passes, out_rgb, out_counts);
}

extern "C" int crt_read_split_state(crt_ctx *ctx, float *out_dsum, float *out_rsum, float *out_rsq) {
    const char *what = "crt_read_split_state";
    if (!ctx) return CRT_ERR_INVALID;
    if (crt_progressive_samples(ctx) == 0 || !ctx->query->prog_is_adaptive || !ctx->query->prog_is_split) {
        ctx->error = std::string(what) + ": no split adaptive frame is under way (crt_render_adaptive_split starts one; crt_set_camera and crt_render* end it)";
        return CRT_ERR_INVALID;
    }
    const crt_query_state *q = ctx->query;
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (out_dsum) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_dsum, q->split_dsum.p, 3 * pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (out_rsum) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rsum, q->split_rsum.p, 3 * pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (out_rsq) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rsq, q->split_rsq.p, pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return CRT_OK;
}

// ---- denoising (crt_denoise.hip, csrc/kernel_denoise.h, csrc/denoise_rule.h): the adaptive frame under way or finished, filtered into a
// buffer of its own.  Nothing of the frame changes: the persistent colour buffer, sum, sq, counts, the lists and crt_progressive_samples
// are only read, so the frame can be denoised after any pass and continued.

// what crt_render_denoised and crt_render_accumulated ask of the context's frame
static int adaptive_frame_check(crt_ctx *ctx, const char *what, const bool split) {
    if (crt_progressive_samples(ctx) == 0) {
        ctx->error = std::string(what) + ": no adaptive frame is under way (crt_render_adaptive starts one; crt_set_camera and crt_render* end it)";
        return CRT_ERR_INVALID;
    }
    if (!ctx->query->prog_is_adaptive) {
        ctx->error = std::string(what) + ": the frame under way is a UNIFORM progressive frame, which keeps no second moment (sq): use crt_render_adaptive "
                                         "with min_samples = max_samples";
        return CRT_ERR_INVALID;
    }
    if (split && !ctx->query->prog_is_split) {
        ctx->error = std::string(what) + ": the frame under way is an UNSPLIT adaptive frame, which keeps no direct part: crt_render_adaptive_split makes a split one";
        return CRT_ERR_INVALID;
    }
    if ((uint64_t)ctx->width * ctx->height >= (1ull << 31)) { ctx->error = std::string(what) + ": width * height >= 2^31"; return CRT_ERR_INVALID; }
    return CRT_OK;
}

// the fold's state the two frame calls below filter: the whole colour's, or -- `split` -- the rest's (csrc/split_rule.h)
struct FoldState { const float *sum, *sq; };
static FoldState fold_state(const crt_query_state *q, const bool split) {
    return split ? FoldState{q->split_rsum.p, q->split_rsq.p} : FoldState{q->prog_sum.p, q->prog_sq.p};
}

// the frame's guides, traced at the frame's first call of either kind: the first hits of the camera's centre rays, as CRT_RAY_PRIMARY (the
// rays of a pass are scratch between passes); den_hits is reserved
// crt_set_guide_bounces > 0: and, behind them, the chain guides of the same rays, for the spatial filter alone (the temporal stage keeps the
// first hits: with a still camera "as if painted" is exact)
static int frame_guides(crt_ctx *ctx, const uint64_t pixels) {
    crt_query_state *q = ctx->query;
    if (q->den_guides) return CRT_OK;
    int rc;
    if ((rc = crt_camera_rays_device(ctx, q->prog_rays.p, ctx->stream)) ||
        (rc = query_run(ctx, closest_call(q->prog_rays.p, pixels, CRT_RAY_PRIMARY, q->den_hits.p), ctx->stream, true)))
        return rc;
    if (ctx->guide_bounces) {
        const char *what = "crt_set_guide_bounces";
        if ((rc = guide_check(ctx, what, pixels, ctx->guide_bounces)) ||
            (rc = reserve_all(ctx, q->den_chain, pixels, q->guide_work, (crt_guide_work_bytes(pixels) + sizeof(float4) - 1) / sizeof(float4))) ||
            (rc = guide_enqueue(ctx, q->prog_rays.p, pixels, CRT_RAY_PRIMARY, q->prog_reflection_bias, q->prog_refraction_bias, ctx->guide_bounces,
                                q->den_chain.p, nullptr, nullptr, q->guide_work.p, ctx->stream, what)))
            return rc;
    }
    q->den_guides = true;
    return CRT_OK;
}
// the guides of the spatial filter stage
static const crt_hit *filter_guides(const crt_ctx *ctx) { return ctx->guide_bounces ? ctx->query->den_chain.p : ctx->query->den_hits.p; }

extern "C" int crt_set_guide_bounces(crt_ctx *ctx, uint32_t max_bounces) {
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = guide_check(ctx, "crt_set_guide_bounces", 0, max_bounces)) return rc;
    if (max_bounces == ctx->guide_bounces) return CRT_OK;
    ctx->guide_bounces = max_bounces;
    if (ctx->query) ctx->query->den_guides = false;   // the kept guides alone: the history and the frame's serial stay
    return CRT_OK;
}
extern "C" uint32_t crt_guide_bounces(const crt_ctx *ctx) { return ctx ? ctx->guide_bounces : 0u; }

// crt_render_denoised and, `split`, crt_render_denoised_split: the rest is filtered and the direct part's mean added back untouched
static int render_denoised(crt_ctx *ctx, const char *what, const bool split, const crt_denoise *denoise, float *out_rgb, uint8_t *out_rgb8) {
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = denoise_check(ctx, what, denoise)) return rc;
    if (int rc = adaptive_frame_check(ctx, what, split)) return rc;
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    int rc;
    if ((rc = query_begin(ctx, ctx->stream, CALL_QUERY))) return rc;
    crt_query_state *q = ctx->query;
    if ((rc = reserve_all(ctx, q->den_hits, pixels, q->den_mean, 3 * pixels, q->den_var, pixels, q->den_out, 3 * pixels, q->den_work,
                          (crt_denoise_work_bytes(ctx->width, ctx->height) + sizeof(float4) - 1) / sizeof(float4), q->den_q8, 3 * pixels)) ||
        (rc = frame_guides(ctx, pixels)))
        return rc;
    const FoldState state = fold_state(q, split);
    if ((rc = denoise_launch_variance(ctx, state.sum, state.sq, q->prog_counts.p, pixels, q->den_mean.p, q->den_var.p, ctx->stream)) ||
        (rc = denoise_launch(ctx, denoise, ctx->width, ctx->height, q->den_mean.p, q->den_var.p, filter_guides(ctx), q->den_out.p, nullptr, q->den_work.p,
                             ctx->stream)) ||
        (split && (rc = split_launch_recombine(ctx, q->den_out.p, q->split_dsum.p, q->prog_counts.p, pixels, q->den_out.p, ctx->stream))))
        return rc;
    if (out_rgb) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb, q->den_out.p, 3 * pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (out_rgb8) {
        if ((rc = crt_quantize_device(ctx, q->den_out.p, 3 * pixels, q->den_q8.p, ctx->stream))) return rc;
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb8, q->den_q8.p, 3 * pixels, hipMemcpyDeviceToHost, ctx->stream));
    }
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return CRT_OK;
}

extern "C" int crt_render_denoised(crt_ctx *ctx, const crt_denoise *denoise, float *out_rgb, uint8_t *out_rgb8) {
    return render_denoised(ctx, "crt_render_denoised", false, denoise, out_rgb, out_rgb8);
}

extern "C" int crt_render_denoised_split(crt_ctx *ctx, const crt_denoise *denoise, float *out_rgb, uint8_t *out_rgb8) {
    return render_denoised(ctx, "crt_render_denoised_split", true, denoise, out_rgb, out_rgb8);
}

// ---- temporal accumulation (crt_temporal.hip, csrc/kernel_temporal.h, csrc/temporal_rule.h): the adaptive frame's state merged with the
// last frame's history, into buffers of its own.  The frame is only read, as crt_render_denoised reads it.  `previous` changes only when a
// call finds a new frame's serial, so every call on one frame merges the same history.

// crt_render_accumulated and, `split`, crt_render_accumulated_split: the history pair hist[split] holds the moments of what the call
// merges -- whole colours, or the rest --, and the direct part's mean is this frame's own, added back behind the optional filter
static int render_accumulated(crt_ctx *ctx, const char *what, const bool split, const crt_temporal *temporal, const crt_denoise *denoise, float *out_rgb,
                              uint8_t *out_rgb8, uint8_t *out_valid) {
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = temporal_check(ctx, what, temporal)) return rc;
    if (denoise)
        if (int rc = denoise_check(ctx, what, denoise)) return rc;
    if (int rc = adaptive_frame_check(ctx, what, split)) return rc;
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    int rc;
    if ((rc = query_begin(ctx, ctx->stream, CALL_QUERY))) return rc;
    crt_query_state *q = ctx->query;
    crt_query_state::History &hist = q->hist[split ? 1 : 0];
    if ((rc = reserve_all(ctx, q->den_hits, pixels, hist.slot[0], pixels, hist.slot[1], pixels, q->acc_rgb, 3 * pixels, q->acc_var, pixels, q->acc_valid,
                          pixels, q->den_q8, 3 * pixels)) ||
        (denoise && (rc = reserve_all(ctx, q->den_out, 3 * pixels, q->den_work,
                                      (crt_denoise_work_bytes(ctx->width, ctx->height) + sizeof(float4) - 1) / sizeof(float4)))) ||
        (rc = frame_guides(ctx, pixels)))
        return rc;
    if (hist.has_cur && hist.serial != q->frame_serial) {   // `current` is an ended frame's: it is the previous history from here on
        hist.cur ^= 1;
        hist.has_prev = true;
        hist.has_cur = false;
    }
    const int cur = hist.cur;
    const FoldState state = fold_state(q, split);
    if ((rc = temporal_launch(ctx, temporal, ctx->width, ctx->height, &hist.pose[cur ^ 1], hist.has_prev ? hist.slot[cur ^ 1].p : nullptr, state.sum,
                              state.sq, q->prog_counts.p, q->den_hits.p, hist.slot[cur].p, q->acc_rgb.p, q->acc_var.p, q->acc_valid.p, ctx->stream)))
        return rc;
    if (!hist.has_cur) hist.frames++;   // once a frame
    hist.has_cur = true;
    hist.serial = q->frame_serial;
    memcpy(hist.pose[cur].position, ctx->frame.cam_pos, sizeof(hist.pose[cur].position));
    memcpy(hist.pose[cur].matrix, ctx->frame.cam, sizeof(hist.pose[cur].matrix));
    float *result = q->acc_rgb.p;
    if (denoise) {
        if ((rc = denoise_launch(ctx, denoise, ctx->width, ctx->height, q->acc_rgb.p, q->acc_var.p, filter_guides(ctx), q->den_out.p, nullptr, q->den_work.p,
                                 ctx->stream)))
            return rc;
        result = q->den_out.p;
    }
    if (split && (rc = split_launch_recombine(ctx, result, q->split_dsum.p, q->prog_counts.p, pixels, result, ctx->stream))) return rc;
    if (out_rgb) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb, result, 3 * pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (out_rgb8) {
        if ((rc = crt_quantize_device(ctx, result, 3 * pixels, q->den_q8.p, ctx->stream))) return rc;
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb8, q->den_q8.p, 3 * pixels, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (out_valid) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_valid, q->acc_valid.p, pixels, hipMemcpyDeviceToHost, ctx->stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return CRT_OK;
}

extern "C" int crt_render_accumulated(crt_ctx *ctx, const crt_temporal *temporal, const crt_denoise *denoise, float *out_rgb, uint8_t *out_rgb8,
                                      uint8_t *out_valid) {
    return render_accumulated(ctx, "crt_render_accumulated", false, temporal, denoise, out_rgb, out_rgb8, out_valid);
}

extern "C" int crt_render_accumulated_split(crt_ctx *ctx, const crt_temporal *temporal, const crt_denoise *denoise, float *out_rgb, uint8_t *out_rgb8,
                                            uint8_t *out_valid) {
    return render_accumulated(ctx, "crt_render_accumulated_split", true, temporal, denoise, out_rgb, out_rgb8, out_valid);
}

extern "C" int crt_history_reset(crt_ctx *ctx) {
    if (!ctx) return CRT_ERR_INVALID;
    if (crt_query_state *q = ctx->query) {
        q->hist[0].reset();
        q->hist[1].reset();
    }
    return CRT_OK;
}

extern "C" uint32_t crt_history_frames(const crt_ctx *ctx) { return ctx && ctx->query ? ctx->query->hist[0].frames : 0u; }
extern "C" uint32_t crt_history_frames_split(const crt_ctx *ctx) { return ctx && ctx->query ? ctx->query->hist[1].frames : 0u; }
