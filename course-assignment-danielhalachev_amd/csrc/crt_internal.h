// crt_internal.h -- what the translation units behind include/crt_hip.h share: the context, the layouts the kernels and the host
// agree on (kernel_common.h), and the few functions that cross a file boundary.  Nothing here is part of the ABI.
//   crt_scene.hip     crt_create / crt_destroy: the flattened scene and everything derived from it, uploaded once
//   crt_launch.hip    the kernels and one frame's launches: the frame's plan (make_plan: the one place its kernels are chosen), the kernels'
//                     tables, queue sizing, events
//   crt_abi.hip       the render entry points, tiles, statistics
//   crt_multi.hip     one scene on several devices behind one call
//   crt_query.hip     the queries for what the caller supplies, behind one call path: ray queries (closest hit / occlusion, the camera's rays),
//                     direct lighting of hit records and points, radiance queries, chain guides; their scratch and statistics
//   crt_giframe.hip   the GI frame calls: progressive, adaptive, denoised, accumulated and split frames on the context's colour buffer; the
//                     frame's state and the histories (the rules: giframe_rule.h)
//   crt_denoise.hip   the denoiser's primitives: the variance of the fold's state, the a-trous filter on first-hit guides
//   crt_temporal.hip  the temporal accumulation's primitive: the last frame's history reprojected and merged with the fold's state
//   crt_split.hip     the split GI frames' primitives: a sample's direct light kept, the fold of the two parts, putting them back together
//   crt_guides.hip    the chain guides' kernel launch and work-area layout: filter guides that follow mirrors and glass
//   crt_variance.hip  the variance estimate's primitive: a 7x7 cross-bilateral estimate of the variance where a pixel's history is short
//   crt_bake.hip      lightmap baking: a mesh's UV texels rasterised to records and probe rays, lit by the radiance queries, dilated
//   crt_probes.hip    the irradiance probe volume: a probe's rays, their colours projected onto SH9 records, validity, the lookup at points
//   crt_testhooks.hip unit-test hooks (libcrt_hip_test.so only)
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <new>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/crt_hip.h"
#include "crt_bvh.h"
#include "call_wait.h"
#include "kernel_common.h"

#define CRT_INTERNAL __attribute__((visibility("hidden")))

// crt_query.hip's chunk sizes, as a context starts with them (crt_ctx::query_launch_rays ...: a test hook may lower them).
// rays per launch: indices, the cursor's overshoot (claimed and dropped) and the list's length stay well inside 31 bits
constexpr uint64_t QUERY_LAUNCH_RAYS = 1ull << 27;
// rays per round trip of the host variants (their device copies: 24 + 48 bytes a ray)
constexpr uint64_t QUERY_HOST_RAYS = 1ull << 22;
// radiance queries: the caller's rays per pass (every level of a pass has arrays of its own: 117 bytes a ray)
constexpr uint64_t SHOOT_PASS_RAYS = 1ull << 22;

// =================================================================================================
// host side of the C ABI
struct crt_ctx {
    int device = 0;
    std::string error;
    hipStream_t stream = nullptr;
    static constexpr int EV_RING = 64;       // event sets of the most recent render launches
    hipEvent_t ev0[EV_RING] = {}, ev1[EV_RING] = {}, ev2[EV_RING] = {}, ev3[EV_RING] = {}, ev4[EV_RING] = {};  // phase boundaries of a render
    hipEvent_t ev_fork[EV_RING] = {}, ev_s0[EV_RING] = {}, ev_s1[EV_RING] = {}, ev_s2[EV_RING] = {};        // ... of its side stream
    bool slot_ev2_is_s1[EV_RING] = {};       // the slot's frame ran its pass on the frame's stream and did not record ev2: the later of ev1 and ev_s1 marks that point (crt_launch.hip, crt_kernel_times_ms)
    bool shadow0_by_pixel = true;            // the last filter frame's plan walked its bulk shadow pass by pixel, not by slot (the GI mode, a frame without fixed slots): crt_launch.hip, finish_plan
    uint64_t launches = 0;
    uint32_t width = 0, height = 0, tiles_x = 0, tiles_y = 0;
    SceneArgs scene{};                // host copy of what crt_create uploads to d_scene
    FrameArgs frame{};                // host copy of the NEXT frame's block (camera, queues ...)
    SceneArgs *d_scene = nullptr;
    FrameArgs *d_frame_ring = nullptr, *h_frame_ring = nullptr;  // one slot per launch in flight (EV_RING): device, and the pinned source of its copy
    const FrameArgs *h_frame_ring_dev = nullptr;                 // ... as the device addresses it (stream_frame_reset does the copy)
    std::vector<void *> allocs;
    float *d_frame = nullptr;
    uint8_t *d_quant = nullptr;
    WorkItem *d_items = nullptr;
    size_t items_cap = 0;
    std::vector<crt_rect> cached_rects;   // coverage the work items were built for: crt_render's rectangles ...
    bool cached_is_partition = false;     // ... or crt_render_tiles_device's {first, stride} (held in cached_rects[0].row / .col)
    uint32_t cached_n_items = 0;
    uint64_t cached_pixels = 0;
    uint32_t *d_sync = nullptr;      // [0] render_lanes' pixel counter (zeroed by the frame's reset launch)
    uint64_t level_counters[C_N] = {}, shadow0_counters[C_N] = {};  // of the last counted render: recursion levels, bulk shadow pass
    enum Mode { MODE_STREAM, MODE_LANES } mode = MODE_STREAM;  // crt_tuning::mode (both produce identical pixels)
    float4 *d_rayq[2] = {nullptr, nullptr};
    float4 *d_shadowq = nullptr;
    uint8_t *d_occluded = nullptr;
    float *d_kfac = nullptr;          // the slots' light factors (same capacity)
    float4 *d_nodes = nullptr;
    uint32_t *d_scounts = nullptr;
    unsigned long long *d_exec = nullptr;           // executed-test tallies of a collect_counters == 2 render
    unsigned long long exec_counters[6] = {0, 0, 0, 0, 0, 0};  // {box, tri} x {all but shadow pass 0, shadow pass 0}, plan tests x the same
    uint32_t *d_fallback_total = nullptr;  // frames redone by the queue-less kernel since crt_create: d_scounts + SC_FALLBACK_TOTAL
    uint32_t *d_heavy = nullptr;      // evicted ray ids
    uint32_t *d_sheavy = nullptr;     // evicted shadow ray ids
    float4 *d_hits = nullptr;         // their closest hits
    float4 *d_hits_all = nullptr;     // a level's closest hits by ray index (kernel_plan.h: the walk-only builds)
    unsigned long long *d_lq = nullptr;   // kernel_bvh.h: the level queue (one entry per ray-tree node at most), 8 granules per ray
    uint32_t *d_lq_words = nullptr;       // ... and its counters (kernel_stream.h: LQ_*)
    uint32_t *d_bvh_spill = nullptr;  // kernel_bvh.h: the walks' stacks beyond their LDS part: BVH_SPILL_REGIONS regions of bvh_spill_words() words (crt_launch.hip: who uses which)
    uint32_t bvh_stack_built = 0;     // SceneArgs::bvh_stack as crt_create sized it (a test hook may lower the scene's value, never this one)
    // words of one spill region: a column of (built stack - LDS part) entries for every thread of the largest grid
    size_t bvh_spill_words() const { return bvh_stack_built > BVH_LDS_STACK ? (size_t)grid_blocks * BLOCK * (bvh_stack_built - BVH_LDS_STACK) : 0u; }
    hipStream_t side = nullptr;       // shadow pass 0 overlaps the deeper recursion levels on this stream (where a frame's levels are launches of their own)
    hipStream_t early = nullptr;      // the level queue's launch starts WITH level 0 on this one (crt_launch.hip)
    hipEvent_t ev_reset[EV_RING] = {}, ev_queue[EV_RING] = {};   // the frame's counters are zeroed / the level queue's launch has ended
    // What a finished frame tells the next ones (queue sizing, launch sizes, fallback count): every frame copies its counter
    // block, whose last word is the fallback total, to ITS slot of this pinned ring in one copy, and the host reads a slot only once that frame's last
    // event has completed (harvest_counts), so launch decisions are a function of a completed frame, never of a copy in flight.
    static constexpr uint32_t H_SLOT_WORDS = 512;       // SC_ALLOC_WORDS
    uint32_t *h_ring = nullptr;       // EV_RING x H_SLOT_WORDS, pinned
    uint64_t next_count_harvest = 0;  // the oldest launch whose slot has not been read
    uint32_t slot_items[EV_RING] = {};               // work items of the frame in each slot
    std::vector<uint32_t> last_counts;               // the most recent COMPLETED frame's counter block (SC_* layout) ...
    uint32_t last_counts_items = 0;                  // ... and the work items it rendered (0: none yet)
    uint32_t fallbacks_seen = 0;                     // fallback total of that frame
    // queue sizing (ensure_stream): capacities as multiples of the frame's pixels, adapted from frame to frame
    double node_mult = 4.0, ray_mult = 2.0, shadow_extra = 1.0;  // (a GB at 1920x1080 with four lights: memory is not what this device lacks)
    uint32_t sizing_seen_fallbacks = 0;
    uint64_t queue_bytes = 0;         // bytes of the per-frame buffers as allocated now
    uint64_t regrows = 0;             // attempts repeated with larger queues (launch_render)
    uint32_t last_counts_cfg = 0;     // frame_config_of the frame last_counts came from
    uint32_t slot_cfg[64] = {};       // ... of the frame in each event slot
    hipEvent_t ev_call0 = nullptr, ev_call1 = nullptr;  // around the last crt_render / crt_render_async call's device work
    bool pending = false;             // a frame enqueued by crt_render_async has not been waited for
    crt_options pending_options{};
    uint32_t heavy_cap = 0;
    uint32_t step_budget = 384;       // crt_tuning::step_budget (0 = never evict: also set when a mesh has too many leaves for the wave-per-ray walk)
    bool lean_ok = true;              // 32-bit byte offsets reach every node and leaf entry
    uint64_t stream_items = 0;        // work items the stream buffers are sized for
    uint64_t overflows = 0;           // frames redone by the fallback (diagnostic)
    uint32_t n_lights = 0;
    uint32_t lights() const { return n_lights ? n_lights : 1u; }   // what sizes are made for: a scene without lights still has queues
    crt_tuning tuning{};
    std::string bvh_note;             // why this scene has no candidate filter (empty: it has one)
    std::string bvh_stats;            // ... and what it consists of
    unsigned long long *d_counters = nullptr;
    float *d_frames = nullptr;
    size_t frames_floats = 0;
    uint32_t grid_blocks = 0;
    crt_stats stats{};
    int num_cus = 0;
    struct crt_query_state *query = nullptr;   // crt_query.hip: the ray queries' scratch and statistics, created by the first query
    struct crt_giframe_state *giframe = nullptr;   // crt_giframe.hip: the GI frame under way and the histories, created by the first frame call
    struct crt_bake_state *bake = nullptr;     // crt_bake.hip: the meshes' triangle lists and the bake call's arrays, created by the first bake call
    struct crt_probe_state *probes = nullptr;  // crt_probes.hip: the probe calls' arrays and statistics, created by the first crt_bake_probes or crt_probe_irradiance
    uint32_t probe_chunk = 0;                  // crt_debug_set_probe_chunk: probes per chunk of crt_bake_probes (0: as many as fit its scratch)
    uint64_t scratch_generation = 0;           // crt_query_scratch_generation: every growth of an array of either (device_array.h)
    uint32_t guide_bounces = 0;                // crt_set_guide_bounces: > 0, the frame calls' spatial filter runs under chain guides
    uint64_t query_host_rays = QUERY_HOST_RAYS, query_launch_rays = QUERY_LAUNCH_RAYS, shoot_pass_rays = SHOOT_PASS_RAYS;   // ... and its chunk sizes
    // the camera of the NEXT frame: crt_set_camera's last word, as crt_camera_rays_device and the frame calls' sample rays take it
    QueryCamera camera() const {
        QueryCamera cam;
        memcpy(cam.pos, frame.cam_pos, sizeof(cam.pos));
        memcpy(cam.m, frame.cam, sizeof(cam.m));
        cam.width = width; cam.height = height;
        return cam;
    }
};

// constants that round 2 carried as crt_tuning fields (DESIGN.md section 7 has the measurements)
static constexpr uint32_t HEAVY_BLOCKS = 4096;   // grid of the wave-per-ray kernels (more blocks than fit: late ones balance the load)
static constexpr uint32_t REFILL_BUNDLE = 16;    // the plan kernels refill a wave when at most this many lanes still walk

extern CRT_INTERNAL std::string g_create_error;   // crt_scene.hip

#define CRT_HIP_CHECK(ctx, expr)                                                                    \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (ctx)->error = std::string(#expr) + ": " + hipGetErrorString(e_);                       \
            return CRT_ERR_HIP;                                                                     \
        }                                                                                           \
    } while (0)

// an invalid call: the message is "<what>: <why>"
static inline int refuse(crt_ctx *ctx, const char *what, const std::string &why) {
    ctx->error = std::string(what) + ": " + why;
    return CRT_ERR_INVALID;
}

// width * height of an image the filter stages take stays below it: pixel coordinates are int32_t
constexpr uint64_t CRT_MAX_PIXELS = 1ull << 31;
static inline int pixels_check(crt_ctx *ctx, const char *what, const uint64_t n) {
    return n >= CRT_MAX_PIXELS ? refuse(ctx, what, "width * height = " + std::to_string(n) + " >= 2^31") : (int)CRT_OK;
}

template <typename T>
static int upload(crt_ctx *ctx, const T *src, size_t count, const T **dst) {
    void *p = nullptr;
    size_t bytes = (count ? count : 1) * sizeof(T);
    CRT_HIP_CHECK(ctx, hipMalloc(&p, bytes));
    ctx->allocs.push_back(p);
    if (count) CRT_HIP_CHECK(ctx, hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    *dst = (const T *)p;
    return CRT_OK;
}

// ---- crt_launch.hip
CRT_INTERNAL int check_options(crt_ctx *ctx, const crt_options *o);
CRT_INTERNAL int ensure_items(crt_ctx *ctx, size_t n);
CRT_INTERNAL int launch_render(crt_ctx *ctx, const crt_options *o, uint32_t n_items, float *d_out, uint32_t packed, hipStream_t stream);
CRT_INTERNAL void note_overflow(crt_ctx *ctx);
CRT_INTERNAL int fetch_counters(crt_ctx *ctx, const crt_options *o, uint64_t pixels);
CRT_INTERNAL std::string describe_frame_kernels(const crt_ctx *ctx);   // crt_describe_kernels: a production frame's plan, named from the kernels' tables
// ---- crt_query.hip: what the GI frame calls (crt_giframe.hip) run of the queries, on the queries' scratch
CRT_INTERNAL void query_destroy(crt_ctx *ctx);
CRT_INTERNAL int query_begin(crt_ctx *ctx, hipStream_t stream, CallKind kind);   // before a call on `stream`: the waiting rule, the scratch every query needs
// the GI radiance calls' own check for a frame's rays (PRIMARY rays, the context's arrays); *pass: the rays of one pass
CRT_INTERNAL int query_gi_check(crt_ctx *ctx, const char *what, const crt_options *options, uint64_t *pass);
CRT_INTERNAL int query_shoot_check(crt_ctx *ctx, const char *what, const crt_options *options);   // what the radiance entry point of options->use_gi would refuse of them
// crt_shoot_rays_gi_device (d_direct: crt_shoot_rays_gi_split_device) for n PRIMARY rays, `pass` at a time
CRT_INTERNAL int query_gi_run(crt_ctx *ctx, const crt_ray *d_rays, const uint32_t *d_keys, uint64_t n, const crt_options *options, float *d_rgb,
                              float *d_direct, uint64_t pass, hipStream_t stream);
CRT_INTERNAL int query_closest_run(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, crt_hit *d_hits, hipStream_t stream);   // crt_trace_rays_device, unchecked
// the widest levels of the radiance passes since this call (query_level_headroom reads them)
CRT_INTERNAL void query_level_peaks_reset(crt_ctx *ctx);
CRT_INTERNAL int query_level_headroom(crt_ctx *ctx, const crt_options *o, uint64_t pass_rays);   // behind a frame's sample 0: room in the level arrays for later samples
// the probe-lit radiance queries (crt_probes.hip: crt_shoot_rays_lit*, crt_render_probe_lit): the GI radiance call's own check of the caller's
// options, and its passes with gi_sample_size = 0 and probe_light_launch behind every level's lighting launches
CRT_INTERNAL int query_lit_check(crt_ctx *ctx, const char *what, const crt_ray *d_rays, const crt_options *options, const float *d_rgb, uint32_t ray_type);
CRT_INTERNAL int query_lit_run(crt_ctx *ctx, const char *what, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, const crt_options *options,
                               const struct ProbeLight *lit, float *d_rgb, hipStream_t stream);
CRT_INTERNAL int guide_check(crt_ctx *ctx, const char *what, uint64_t n, uint32_t max_bounces);   // what every guide call asks beyond its arrays
CRT_INTERNAL int guide_enqueue(crt_ctx *ctx, const crt_ray *d_rays, uint64_t n, uint32_t ray_type, float reflection_bias, float refraction_bias,
                               uint32_t max_bounces, crt_hit *d_out_hits, uint8_t *d_out_status, crt_ray *d_out_last_rays, void *d_work, hipStream_t stream,
                               const char *what, bool first = true);
// ---- crt_giframe.hip
CRT_INTERNAL void giframe_destroy(crt_ctx *ctx);
CRT_INTERNAL void giframe_reset(crt_ctx *ctx);   // crt_set_camera, crt_render*: the frame under way has ended, crt_progressive_samples is 0 again
CRT_INTERNAL int progressive_check(crt_ctx *ctx, const char *what, const uint32_t *d_pixels, uint64_t n);   // what the fold's primitives ask of (d_pixels, n)
// ---- crt_bake.hip
CRT_INTERNAL void bake_destroy(crt_ctx *ctx);
// ---- crt_probes.hip
CRT_INTERNAL void probes_destroy(crt_ctx *ctx);
// what a probe-lit radiance pass hands to every level (csrc/probe_lit_rule.h): the volume, checked by the entry point, and the caller's S
struct ProbeLight {
    const crt_probe_volume *volume;
    const crt_probe_visibility *visibility;   // or null: the plain lookup
    const crt_probe *d_probes;
    const crt_probe_depth *d_depth;           // with a visibility
    uint32_t samples;
    unsigned long long *d_counts;             // or null: [0] += LIT records, [1] += UNLIT records
};
// probe_light_records for a level's records, unchecked: behind the level's lighting launches, for the radiance passes (crt_query.hip)
CRT_INTERNAL int probe_light_launch(crt_ctx *ctx, const ProbeLight &L, const crt_hit *d_hits, const uint8_t *d_status, uint64_t n, float *d_rgb,
                                    hipStream_t stream);
// ---- crt_denoise.hip: the denoiser's settings check and launches, for crt_render_denoised (crt_giframe.hip)
CRT_INTERNAL int denoise_check(crt_ctx *ctx, const char *what, const crt_denoise *d);
CRT_INTERNAL int denoise_launch_variance(crt_ctx *ctx, const float *d_sum, const float *d_sq, const uint32_t *d_counts, uint64_t n, float *d_mean,
                                         float *d_var, hipStream_t stream);
CRT_INTERNAL int denoise_launch(crt_ctx *ctx, const crt_denoise *d, uint32_t width, uint32_t height, const float *d_rgb, const float *d_var,
                                const crt_hit *d_hits, float *d_out_rgb, float *d_out_var, void *d_work, hipStream_t stream);
// ---- crt_temporal.hip: the temporal accumulation's settings check and launch, for crt_render_accumulated (crt_giframe.hip)
CRT_INTERNAL int temporal_check(crt_ctx *ctx, const char *what, const crt_temporal *t);
CRT_INTERNAL int temporal_launch(crt_ctx *ctx, const crt_temporal *t, uint32_t width, uint32_t height, const crt_camera_pose *prev_pose,
                                 const crt_history_pixel *d_prev, const float *d_sum, const float *d_sq, const uint32_t *d_counts, const crt_hit *d_hits,
                                 crt_history_pixel *d_next, float *d_out_rgb, float *d_out_var, uint8_t *d_out_valid, hipStream_t stream);
// ---- crt_variance.hip: the variance estimate's settings check and launch, for the frame calls' setting (crt_giframe.hip)
CRT_INTERNAL int variance_check(crt_ctx *ctx, const char *what, const crt_variance_estimate *e);
CRT_INTERNAL int variance_launch(crt_ctx *ctx, const crt_variance_estimate *e, uint32_t width, uint32_t height, const crt_history_pixel *d_moments,
                                 const crt_hit *d_hits, const float *d_var, float *d_out_var, hipStream_t stream);
// ---- crt_split.hip: the split GI frames' launches, for the radiance passes (crt_query.hip) and the *_split frame calls (crt_giframe.hip)
CRT_INTERNAL int split_launch_keep_direct(crt_ctx *ctx, const uint8_t *d_status, const float *d_rgb, uint32_t n, uint32_t gi_sample_size, float *d_direct,
                                          hipStream_t stream);
CRT_INTERNAL int split_launch_fold(crt_ctx *ctx, const float *d_rgb, const float *d_direct, const uint32_t *d_pixels, uint64_t n, uint32_t sample,
                                   float *d_dsum, float *d_rsum, float *d_rsq, hipStream_t stream);
CRT_INTERNAL int split_launch_recombine(crt_ctx *ctx, const float *d_filtered, const float *d_dsum, const uint32_t *d_counts, uint64_t n_pixels,
                                        float *d_out, hipStream_t stream);
// ---- crt_guides.hip: the chain guides' work area and the launch behind a level's trace, for crt_guide_rays* (crt_query.hip)
constexpr uint32_t GUIDE_COUNT_WORDS = 128;   // the head of the work area: entries appended to level k at [k]
struct GuideWork {
    uint32_t *count;
    crt_hit *hits;          // the level's closest hits, by list position
    crt_ray *rays[2];       // two lists: level k reads list k & 1 and appends to the other
    uint32_t *pixel[2];
    float *tsum[2];
    uint32_t *mesh0[2];
};
CRT_INTERNAL GuideWork guides_work(void *d_work, uint64_t n);
CRT_INTERNAL int guides_launch_step(crt_ctx *ctx, const GuideWork &W, const crt_ray *d_rays, uint32_t n, uint32_t level, uint32_t max_bounces,
                                    float reflection_bias, float refraction_bias, crt_hit *d_out_hits, uint8_t *d_out_status, crt_ray *d_out_last_rays,
                                    hipStream_t stream);
// ---- crt_abi.hip
CRT_INTERNAL uint64_t coverage_items(uint32_t width, uint32_t height, const crt_rect *rects, uint32_t n_rects, std::vector<WorkItem> &items);
CRT_INTERNAL void launch_unpack_items(const float *packed, const WorkItem *items, uint32_t n_items, float *frame, uint32_t width, uint32_t height,
                                      uint32_t tiles_x, hipStream_t stream);
