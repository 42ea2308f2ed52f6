// crt_launch.hip -- the kernels of the MI355X (gfx950) implementation behind include/crt_hip.h, and one frame's launches.
//
// What runs here is the reference's per-pixel hot path, tree mode, USE_GI = false
// (reference: SourceCode/src/RayTracer.cpp:61-112, 300-451, 507-517; src/KDTree.cpp:48-87,
// 127-192; src/AccelerationStructure.cpp:56-94; include/tracer/BoundingBox.h:85-108;
// src/Ray.cpp:9-31; src/Triangle.cpp:37-73; src/Texture.cpp:14-72; src/Color.cpp:12-16).
//
// Design (DESIGN.md has the measurements behind it):
//  * default path (kernel_stream.h): the reference's recursion unrolled BY RECURSION LEVEL.  Level g is one
//    launch of a per-lane walk kernel (kernel_plan.h: binary threaded nodes, the top-level tree as a plan) whose
//    lanes are refilled from a queue; it writes ray-tree nodes, child rays for level g+1 and shadow rays.  Walks that outlast a step budget, and whole small levels, go to a wave-per-ray kernel
//    (kernel_heavy.h).  The shadow rays of level 0 -- the bulk of the frame -- run on a side stream beside the
//    deeper levels.  stream_resolve evaluates every pixel's ray tree in the reference's post-order, so that
//    every float is combined in the same order.  A fixed shadow slot (level 0's) is written by whoever walks it
//    and read by stream_resolve -- except in a filter frame outside the GI mode, whose bulk pass walks level 0's
//    records pixel by pixel and leaves each pixel's direct light in its root node (kernel_bvh.h: bvh_shadow_pixels);
//  * the reference's stack DFS has a FIXED visit order and no distance pruning, so the trees are flattened into
//    hit/miss links (crt_node) and walked without a stack; the plan and leaf-sequence forms rest on the boxes
//    being nested, which crt_create verifies;
//  * fallback, bit-exact and tested: render_lanes (kernel_lane.h: the full recursion per lane on an
//    explicit frame stack; redoes a frame whose queues overflowed, and renders the GI mode);
//  * arithmetic is IEEE binary32 with no contraction (-ffp-contract=off), correctly rounded divide and sqrt,
//    std::min/std::max semantics written out, so results are bit-identical to the x86-64 reference build.
//
// A frame's kernels are chosen in ONE place: make_plan decides everything about the frame (FramePlan), the tables behind it hold every kernel of
// every role under the name a profile prints, and a launch site is one lookup by the plan's fields.  crt_describe_kernels reads the same plan and tables.
// Kernel selection and sizing come in through crt_tuning (include/crt_hip.h); this file reads no environment
// variables and keeps no state outside the context.
#include "crt_internal.h"
#include "glibc_powf.h"

namespace {

#include "kernel_lane.h"
#include "kernel_stream.h"
#include "kernel_heavy.h"
#include "kernel_plan.h"
#include "kernel_bvh.h"

}  // namespace

int check_options(crt_ctx *ctx, const crt_options *o) {
    if (!o) { ctx->error = "options is NULL"; return CRT_ERR_INVALID; }
    if (o->use_gi && o->collect_counters == 2) { ctx->error = "collect_counters == 2 belongs to the ray-stream kernels; the GI mode renders with render_lanes"; return CRT_ERR_INVALID; }
    if (o->use_gi && (o->gi_sample_size > 64u || o->rays_per_pixel > 65536u)) { ctx->error = "gi_sample_size > 64 or rays_per_pixel > 65536"; return CRT_ERR_INVALID; }
    if (o->max_depth > 4096) { ctx->error = "max_depth too large"; return CRT_ERR_INVALID; }
    return CRT_OK;
}

int ensure_items(crt_ctx *ctx, size_t n) {
    if (n <= ctx->items_cap) return CRT_OK;
    CRT_HIP_CHECK(ctx, hipDeviceSynchronize());  // nothing may still be reading the old items
    if (ctx->d_items) (void)hipFree(ctx->d_items);
    ctx->d_items = nullptr;
    ctx->items_cap = 0;
    CRT_HIP_CHECK(ctx, hipMalloc((void **)&ctx->d_items, (n + 4) * sizeof(WorkItem)));  // (+: padding, so that a 16-byte read at the last record stays inside)
    ctx->items_cap = n;
    ctx->cached_rects.clear();
    ctx->cached_is_partition = false;
    return CRT_OK;
}

static int ensure_frames(crt_ctx *ctx, uint32_t max_depth, bool gi) {
    const size_t waves = (size_t)ctx->grid_blocks * (BLOCK / 64);
    const size_t per_wave = (size_t)(max_depth + 1) * (gi ? FRAME_DWORDS_GI : FRAME_DWORDS) * 64;
    if (waves * per_wave > ctx->frames_floats) {
        if (ctx->d_frames) (void)hipFree(ctx->d_frames);
        ctx->d_frames = nullptr;
        ctx->frames_floats = 0;
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&ctx->d_frames, waves * per_wave * sizeof(float)));
        ctx->frames_floats = waves * per_wave;
    }
    ctx->frame.frames = ctx->d_frames;
    ctx->frame.frame_wave_stride = per_wave;
    return CRT_OK;
}

// What the finished frames left behind.  Every frame copies its counter block (the fallback total is its last word) into its own slot of
// the pinned ring (launch_frame); a slot is read here only once the frame's last event has completed, so the host never
// reads a buffer a copy may still be writing, and what the next launch learns is a function of a COMPLETED frame.
static void harvest_counts(crt_ctx *ctx) {
    while (ctx->next_count_harvest < ctx->launches) {
        const uint64_t j = ctx->next_count_harvest;
        if (j + crt_ctx::EV_RING <= ctx->launches) { ctx->next_count_harvest++; continue; }  // its slot has been reused
        const int slot = (int)(j % crt_ctx::EV_RING);
        if (hipEventQuery(ctx->ev4[slot]) != hipSuccess) { (void)hipGetLastError(); break; }
        const uint32_t *h = ctx->h_ring + (size_t)slot * crt_ctx::H_SLOT_WORDS;
        if (ctx->slot_items[slot]) {  // (a frame without work items launched nothing and copied nothing)
            ctx->last_counts.assign(h, h + SC_ALLOC_WORDS);
            ctx->last_counts_items = ctx->slot_items[slot];
            ctx->last_counts_cfg = ctx->slot_cfg[slot];
            ctx->fallbacks_seen = h[SC_FALLBACK_TOTAL];
        }
        ctx->next_count_harvest++;
    }
}

// Queues of the ray-stream pass.  What a frame needs depends on the scene and the camera -- a frame of diffuse surfaces
// has no child rays at all, nested glass can reach 2^(MAX_DEPTH+1)-1 rays per pixel -- so the capacities FOLLOW the frames:
// they start at px * {4 ray-tree nodes, 2 rays per level, n_lights * 2 shadow rays} (px = 64 pixels per work item),
// grow by half when the last completed frame used more than 70 % of one of them, and are regrown inside the call when an attempt
// overflows them (launch_render).  A frame that overflows queues an earlier frame had fitted is not lost either: its queues raise
// the overflow word and render_lanes, which needs no queues, redoes it in the same call (crt_stats::fallback_frames counts
// those; the factors double for the next frame).
static void adapt_queue_sizing(crt_ctx *ctx) {
    const uint32_t *c = ctx->last_counts.data();
    if (ctx->fallbacks_seen != ctx->sizing_seen_fallbacks) {
        ctx->sizing_seen_fallbacks = ctx->fallbacks_seen;
        ctx->node_mult = std::min(4096.0, ctx->node_mult * 2.0);
        ctx->ray_mult = std::min(4096.0, ctx->ray_mult * 2.0);
        ctx->shadow_extra = std::min(4096.0, ctx->shadow_extra * 2.0);
        return;
    }
    const FrameArgs &A = ctx->frame;
    if (!A.s_node_cap || !ctx->last_counts_items) return;
    const uint64_t px = (uint64_t)ctx->last_counts_items * 64;
    uint64_t rays = 0, nodes = px;
    for (int g = 1; g < MAX_GENERATIONS; g++) { rays = std::max<uint64_t>(rays, c[SC_COUNT + g]); nodes += c[SC_COUNT + g]; }
    const uint64_t shadow = c[SC_SHADOW];
    // level 0 owns one node per pixel and n_lights fixed shadow slots per pixel: what can run out is the part beyond that
    const uint64_t base_shadow = px * ctx->lights();
    const uint64_t extra_nodes = nodes > px ? nodes - px : 0, extra_shadow = shadow > base_shadow ? shadow - base_shadow : 0;
    if (A.s_node_cap > px && extra_nodes * 10 > ((uint64_t)A.s_node_cap - px) * 7) ctx->node_mult = std::min(4096.0, ctx->node_mult * 1.5);
    if (rays * 10 > (uint64_t)A.s_ray_cap * 7) ctx->ray_mult = std::min(4096.0, ctx->ray_mult * 1.5);
    if (A.s_shadow_cap > base_shadow && extra_shadow * 10 > ((uint64_t)A.s_shadow_cap - base_shadow) * 7)
        ctx->shadow_extra = std::min(4096.0, ctx->shadow_extra * 1.5);
}

static uint64_t queue_bytes_for(const crt_ctx *ctx, uint64_t px, double node_mult, double ray_mult, double shadow_extra) {
    return (uint64_t)(px * std::max(ray_mult, 1.0)) * 16 + (uint64_t)(px * ray_mult) * (64 + 24) + (uint64_t)(px * (uint64_t)ctx->lights() * (1.0 + shadow_extra)) * 37 + (uint64_t)(px * node_mult) * 32;
}

// After an attempt that overflowed (launch_render): capacities from what the attempt learnt.  The level that was emitting when a
// queue ran out still counted every ray it wanted to queue (the counters are bumped before the capacity check), so the rays of
// levels 0 .. G are known exactly; the deeper ones are extrapolated with the last growth ratio (a GI frame grows by up to
// gi_samples + 1 per level, a mirror room by 2, most frames shrink), the shadow rays in proportion to the nodes.  25 % on top;
// false when the device has no room for that.
static bool grow_queue_sizing(crt_ctx *ctx, uint32_t vitems, uint32_t max_depth) {
    const uint32_t *c = ctx->last_counts.data();
    const double px = (double)vitems * 64.0, lights = ctx->lights();
    uint32_t G = 0;
    for (uint32_t g = 1; g <= max_depth && g < (uint32_t)MAX_GENERATIONS; g++) if (c[SC_COUNT + g]) G = g;
    double known = px, widest = 0, last = px, before = px;
    for (uint32_t g = 1; g <= G; g++) { before = last; last = c[SC_COUNT + g]; known += last; widest = std::max(widest, last); }
    const double ratio = G >= 1 ? std::max(1.0, last / std::max(before, 1.0)) : 2.0;
    double total = known, level = last;
    for (uint32_t g = G + 1; g <= max_depth; g++) { level *= ratio; total += level; widest = std::max(widest, level); }
    const double shadows = (double)c[SC_SHADOW] * (total / known);
    double node_mult = std::max(ctx->node_mult, total * 1.25 / px), ray_mult = std::max(ctx->ray_mult, widest * 1.25 / px);
    double shadow_extra = std::max(ctx->shadow_extra, shadows * 1.25 / (px * lights) - 1.0);

    if (node_mult == ctx->node_mult && ray_mult == ctx->ray_mult && shadow_extra == ctx->shadow_extra) {
        node_mult *= 2.0; ray_mult *= 2.0; shadow_extra = std::max(0.5, shadow_extra * 2.0);  // (the counters explain nothing: an eviction list, say)
    }
    if (px * node_mult > 2.0e9 || px * ray_mult > 2.0e9 || px * lights * (1.0 + shadow_extra) > 2.0e9) return false;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (queue_bytes_for(ctx, (uint64_t)px, node_mult, ray_mult, shadow_extra) > (free_b + ctx->queue_bytes) / 2) return false;
    ctx->node_mult = node_mult; ctx->ray_mult = ray_mult; ctx->shadow_extra = shadow_extra;
    return true;
}

// level 0 of the ray-stream pass holds this many rays per pixel (RayTracer.cpp:90-104: the centre sample + RAYS_PER_PIXEL - 1 jittered ones)
static uint32_t level0_samples_of(const crt_options *o) { return o->use_gi && o->rays_per_pixel > 1u ? o->rays_per_pixel : 1u; }
// a GI frame goes through the ray-stream pass when its level 0 fits 31-bit ray indices (otherwise render_lanes' GI build renders it pixel by pixel)
static bool gi_fits_stream(const crt_options *o, uint32_t n_items) {
    return (uint64_t)n_items * 64u * level0_samples_of(o) * 2u < (1ull << 31) && o->gi_sample_size <= 64u;
}
// what, beside its size, decides how many rays a frame queues: two frames are "of the same kind" for the queue sizing when this agrees
static uint32_t frame_config_of(const crt_options *o) {
    return (o->use_gi ? 0x80000000u : 0u) | ((o->use_gi ? o->gi_sample_size & 0x7Fu : 0u) << 24) | (o->max_depth & 0xFFFFFFu);
}

// Who walks a frame's rays -- the row of the level and shadow tables below: the faithful kernel, its counting build, the plan kernels, the wide
// plan's, the filter kernels (a row per build variant: W_BVH + BVH_PLAIN / BVH_TALLY / BVH_CHECKED).
enum : int { W_STREAM = 0, W_COUNT = 1, W_PLAN = 2, W_WIDE = 3, W_BVH = 4, W_ROWS = W_BVH + 3 };

// What make_plan decides once per frame; everything that enqueues, sizes or describes the frame reads it.
struct FramePlan {
    int slot;                     // event / pinned-counter / argument-block slot of this frame
    uint32_t n_items, vitems;     // work items; work items' worth of level-0 rays (the GI mode: x rays_per_pixel)
    uint32_t samples, lane_blocks;  // level 0's rays per pixel; grid of the kernels that take one ray (or pixel) per lane
    bool stream_mode;             // the ray-stream pass (otherwise render_lanes renders the whole frame)
    bool gi, count, exec_count;   // GI mode; counting build; production kernels tallying the tests they execute
    int variant;                  // the build of the production kernels: BVH_PLAIN, BVH_TALLY (exec_count), BVH_CHECKED (crt_tuning::bvh == 2)
    bool heavy, lean, wide;       // wave-per-ray kernels on; plan kernels; the wide plan
    bool bvh;                     // the filter kernels (kernel_bvh.h) walk the rays
    int walk;                     // ... all of which as the tables' row (W_*)
    bool queue, early_queue;      // every level below level 0 is one launch (bvh_trace_queue); ... which starts WITH level 0, on a stream of its own
    bool queue_room;              // the context's frames may run the level queue: the stream buffers hold one (ensure_stream)
    uint32_t widest;              // rays of the widest level below level 0 a frame ago (0: not known)
    uint32_t level_budget;        // steps after which a deeper level's per-lane walk is evicted
    const uint32_t *prev;         // counters of a completed frame of this size and kind that fitted its queues, or null: the size is not proven
    bool fixed_caps;              // explicit queue capacities (crt_tuning): never regrown, never probed
    bool last_resort, debug_sync; // render_lanes behind the stream pass; development (crt_tuning::bvh == 3): launch() announces every launch on stderr and waits for it
    // known once the queues have their capacities (finish_plan):
    bool fixed0, split_known;     // level 0 owns the first vitems * 64 * n_lights shadow slots; ... and they are all the bulk pass walks: the reset launch presets the split mark
    bool by_pixel;                // the bulk shadow pass walks level 0's records pixel by pixel (kernel_bvh.h: bvh_shadow_pixels)
    bool one_stream;              // level 0, the bulk shadow pass and the resolve follow one another on the frame's stream (launch_stream_levels)
};

// The frame's plan: everything that is chosen for a frame of n_items work items under `o` on this context, chosen HERE and nowhere else.  It
// launches nothing and changes nothing.  (n_items == 0: a frame of no particular size, which no completed frame tells anything about.)
static FramePlan make_plan(const crt_ctx *ctx, const crt_options *o, uint32_t n_items, bool last_resort) {
    const SceneArgs &SC = ctx->scene;
    const crt_tuning &T = ctx->tuning;
    FramePlan P{};
    P.slot = (int)(ctx->launches % crt_ctx::EV_RING);
    P.n_items = n_items;
    P.last_resort = last_resort;
    P.debug_sync = T.bvh == 3;
    P.gi = o->use_gi != 0;  // the GI / multi-sample mode: through the ray-stream pass like any frame, unless its level 0 is too large for it
    P.stream_mode = ctx->mode == crt_ctx::MODE_STREAM && (!P.gi || gi_fits_stream(o, n_items));
    // the GI mode's level 0 holds rays_per_pixel rays per pixel: `vitems` work items' worth of rays, which is what queues and grids are sized by
    P.samples = P.stream_mode ? level0_samples_of(o) : 1u;
    P.vitems = n_items * P.samples;
    P.lane_blocks = std::max(1u, std::min((P.vitems * 64u + BLOCK - 1) / BLOCK, ctx->grid_blocks));
    P.count = o->collect_counters == 1;       // the counting build: every ray walked the reference's way
    P.exec_count = o->collect_counters == 2;  // the production kernels, tallying the tests they execute
    P.variant = P.exec_count ? BVH_TALLY : T.bvh == 2 ? BVH_CHECKED : BVH_PLAIN;
    P.fixed_caps = T.node_cap || T.ray_cap || T.shadow_cap;
    // the wave-per-ray path needs nested boxes; the counting build walks every ray the reference's way
    P.heavy = P.stream_mode && ctx->step_budget && SC.nested_boxes && (SC.top_fast || SC.plan_seq) && !P.count;
    // the plan kernels (kernel_plan.h): a small top-level tree (its leaves as a plan), 32-bit offsets, compact leaf links
    P.lean = P.heavy && ctx->lean_ok && (SC.plan_ok || SC.plan_wide);
    P.wide = P.lean && !SC.plan_ok;  // the wide plan (kernel_plan.h): more than 64 top-level leaves or meshes
    // the filter kernels (kernel_bvh.h): whenever the scene has a filter -- they need nothing of the plan or of the wave-per-ray kernels
    // (the GI mode too -- level by level, its levels are millions of rays -- except in the tallying and bounds-checked builds, which have no GI kernels)
    P.bvh = P.stream_mode && SC.bvh_ok && T.bvh && !P.count && !(P.gi && P.variant != BVH_PLAIN);
    P.walk = P.bvh ? W_BVH + P.variant : P.count ? W_COUNT : P.wide ? W_WIDE : P.lean ? W_PLAN : W_STREAM;
    // a completed frame of this size and kind: its widest level below level 0, and -- unless it overflowed: it stopped early then, its levels'
    // counts say nothing -- its counters
    const bool known = P.vitems && ctx->last_counts_items == P.vitems && ctx->last_counts_cfg == frame_config_of(o);
    if (known)
        for (uint32_t g = 1; g <= o->max_depth && g < (uint32_t)MAX_GENERATIONS; g++) P.widest = std::max(P.widest, ctx->last_counts[SC_COUNT + g]);
    P.prev = known && !ctx->last_counts[SC_OVERFLOW] ? ctx->last_counts.data() : nullptr;
    // ... the levels below level 0 as one self-feeding launch -- once a frame of this size is known to fit its queues: an attempt that
    // PROBES them (launch_render) runs level by level, because a level-by-level run that overflows leaves the counts the next attempt is
    // sized from, where the level queue stops in the middle of all its levels at once (same pixels either way)
    // And only where it pays: the queue trades launches and their tails (latency) for hand-overs through memory (throughput).  A frame whose
    // levels hold hundreds of thousands of rays each is throughput -- a mirror room at 1080p: 11.5 ms level by level, 20 ms through the queue;
    // HW12 at 3840x2160 (229 k rays per level): the same either way; HW14 / HW11 (20 - 85 k): 4.1 -> 3.3, 5.2 -> 4.0 ms -- so the widest
    // level of the last completed frame of this size decides.
    P.queue_room = SC.bvh_ok && T.bvh && T.level_queue;
    P.queue = P.bvh && !P.gi && T.level_queue && last_resort && P.widest <= 250000u;
    // (level_queue bit 9: the launch behind level 0, as it used to be -- and under debug_sync, which waits for every launch)
    P.early_queue = P.queue && T.side_blocks && !(T.level_queue & 512u) && !P.debug_sync;
    // (under the wide plan a ray crosses dozens of small mesh trees: a walk of a thousand steps is the rule there, not the outlier the
    //  wave-per-ray kernel is for -- measured on tools/many_meshes.py 200: 32.7 ms per frame with the plain budget, 25.4 with four times it)
    // (the same holds for a GI frame's levels -- millions of incoherent rays each: tools/gi_time.py hw14 960x540 d3 n2 r2 54.7 ms -> 44.2)
    P.level_budget = (P.wide || P.gi) ? std::min<uint32_t>(ctx->step_budget * 4u, 1u << 20) : ctx->step_budget;
    return P;
}

// ... and what only the queues' capacities tell (behind ensure_stream, once).  The bulk shadow pass's choice is what the frame leaves for describe_frame_kernels.
static void finish_plan(crt_ctx *ctx, FramePlan &P) {
    // level 0 owns the first n_items * 64 * n_lights slots of the shadow queue; the deeper levels append
    P.fixed0 = (uint64_t)P.vitems * 64u * ctx->n_lights <= ctx->frame.s_shadow_cap;
    // Level 0's fixed shadow slots: the shadow queue's fill starts there.  Where the level queue runs the frame (P.queue) they are also ALL
    // the bulk shadow pass walks -- the queue's lanes walk the deeper levels' shadow rays themselves, bvh_trace_shadow<1> is not launched --
    // so the split mark is a value the host knows and the reset launch presets: no stream_mark_split launch between level 0 and the pass.
    P.split_known = P.queue && P.fixed0;
    // A filter frame with fixed slots (not the GI mode, whose roots carry children) walks them BY PIXEL (kernel_bvh.h: bvh_shadow_pixels):
    // the same stream, grid, spill region and events, a pixel's lights in one lane, its direct light stored into its root node
    P.by_pixel = P.bvh && P.fixed0 && !P.gi;
    // The production frame -- the level queue beside level 0, the pass's slots known to the host -- has nothing on `stream` between level 0 and
    // the resolve but the pass: it follows level 0 there as a plain kernel-after-kernel dependency, and the resolve follows it the same way.
    // (Everywhere else the pass runs BESIDE the levels' own launches on `stream`, and the side stream is what lets it.)
    P.one_stream = P.early_queue && P.bvh && P.split_known && !(ctx->tuning.level_queue & 4096u);
    if (P.bvh) ctx->shadow0_by_pixel = P.by_pixel;
}

static int ensure_stream(crt_ctx *ctx, const FramePlan &P) {
    FrameArgs &A = ctx->frame;
    adapt_queue_sizing(ctx);
    const uint32_t n_items = P.vitems;
    const uint64_t px = (uint64_t)n_items * 64;
    const uint64_t lights = ctx->lights();
    const uint64_t floor_cap = 1u << 16;
    uint64_t node_cap = std::max<uint64_t>(floor_cap, (uint64_t)(px * ctx->node_mult));
    uint64_t ray_cap = std::max<uint64_t>(floor_cap, (uint64_t)(px * ctx->ray_mult));
    uint64_t shadow_cap = std::max<uint64_t>(floor_cap, (uint64_t)(px * lights * (1.0 + ctx->shadow_extra)));
    // explicit capacities (crt_tuning): never below what level 0 itself needs, so that only the deeper levels can overflow
    if (ctx->tuning.node_cap) node_cap = ctx->tuning.node_cap < px ? px : ctx->tuning.node_cap;
    if (ctx->tuning.ray_cap) ray_cap = ctx->tuning.ray_cap;
    if (ctx->tuning.shadow_cap) shadow_cap = ctx->tuning.shadow_cap;
    node_cap = std::min<uint64_t>(node_cap, 0x7FFFFFF0ull);
    ray_cap = std::min<uint64_t>(ray_cap, 0x7FFFFFF0ull);
    shadow_cap = std::min<uint64_t>(shadow_cap, 0x7FFFFFF0ull);
    if (px > node_cap) { ctx->error = "frame too large for the ray-stream buffers"; return CRT_ERR_INVALID; }
    const bool grow = node_cap > A.s_node_cap || ray_cap > A.s_ray_cap || shadow_cap > A.s_shadow_cap || n_items > ctx->stream_items ||
                      (P.fixed_caps && (node_cap != A.s_node_cap || ray_cap != A.s_ray_cap || shadow_cap != A.s_shadow_cap));
    if (grow) {
        CRT_HIP_CHECK(ctx, hipDeviceSynchronize());  // nothing may still be using the old buffers
        if (!P.fixed_caps) {  // never shrink: keep what is already there
            node_cap = std::max<uint64_t>(node_cap, A.s_node_cap);
            ray_cap = std::max<uint64_t>(ray_cap, A.s_ray_cap);
            shadow_cap = std::max<uint64_t>(shadow_cap, A.s_shadow_cap);
        }
        void **bufs[] = {(void **)&ctx->d_rayq[0], (void **)&ctx->d_rayq[1], (void **)&ctx->d_shadowq, (void **)&ctx->d_occluded, (void **)&ctx->d_kfac,
                         (void **)&ctx->d_nodes, (void **)&ctx->d_heavy, (void **)&ctx->d_sheavy, (void **)&ctx->d_hits, (void **)&ctx->d_hits_all,
                         (void **)&ctx->d_lq};
        for (void **b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
        ctx->stream_items = 0;
        A.s_node_cap = A.s_ray_cap = A.s_shadow_cap = 0;
        // (+ 64 bytes of padding behind the queues)
        for (int i = 0; i < 2; i++) CRT_HIP_CHECK(ctx, hipMalloc((void **)&ctx->d_rayq[i], ray_cap * 2 * sizeof(float4) + 64));
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&ctx->d_shadowq, shadow_cap * 2 * sizeof(float4) + 64));
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&ctx->d_occluded, shadow_cap));
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&ctx->d_kfac, shadow_cap * sizeof(float)));
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&ctx->d_nodes, node_cap * 2 * sizeof(float4)));
        ctx->heavy_cap = (uint32_t)std::max<uint64_t>(floor_cap, ray_cap);  // (a full list only keeps a long walk where it is)
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&ctx->d_heavy, (size_t)ctx->heavy_cap * sizeof(uint32_t) + 64));
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&ctx->d_sheavy, (size_t)ctx->heavy_cap * sizeof(uint32_t) + 64));
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&ctx->d_hits, (size_t)ctx->heavy_cap * sizeof(float4)));
        CRT_HIP_CHECK(ctx, hipMalloc((void **)&ctx->d_hits_all, (size_t)std::max<uint64_t>(ray_cap, px) * sizeof(float4)));  // (level 0 holds px rays, a deeper level at most ray_cap)
        if (P.queue_room) {
            // the level queue: every ray below level 0 owns a node, so node_cap entries always do; its tags start as "no frame's"
            CRT_HIP_CHECK(ctx, hipMalloc((void **)&ctx->d_lq, node_cap * 8 * sizeof(unsigned long long)));
            CRT_HIP_CHECK(ctx, hipMemset(ctx->d_lq, 0, node_cap * 8 * sizeof(unsigned long long)));
        }
        A.s_ray_cap = (uint32_t)ray_cap; A.s_shadow_cap = (uint32_t)shadow_cap; A.s_node_cap = (uint32_t)node_cap;
        ctx->stream_items = n_items;
        ctx->queue_bytes = ray_cap * 64 + shadow_cap * 37 + node_cap * 32 + (size_t)ctx->heavy_cap * 24 + std::max<uint64_t>(ray_cap, px) * 16 + (ctx->d_lq ? node_cap * 64 : 0);
    }
    A.s_rayq[0] = ctx->d_rayq[0]; A.s_rayq[1] = ctx->d_rayq[1];
    A.s_shadowq = ctx->d_shadowq; A.s_occluded = ctx->d_occluded; A.s_kfac = ctx->d_kfac; A.s_nodes = ctx->d_nodes;
    A.s_heavy = ctx->d_heavy; A.s_sheavy = ctx->d_sheavy; A.s_hits = ctx->d_hits; A.s_hits_all = ctx->d_hits_all; A.s_heavy_cap = ctx->heavy_cap;
    // (an explicit ray capacity -- crt_tuning, the tests' way to an overflow -- bounds the level queue too)
    A.s_lq = ctx->d_lq; A.s_lq_cap = ctx->d_lq ? (ctx->tuning.ray_cap ? std::min(A.s_ray_cap, A.s_node_cap) : A.s_node_cap) : 0u;
    return CRT_OK;
}

// The order in which the kernel templates are first named is the order in which they are instantiated and laid out in the code object, and the
// compiler's code for three GI kernels (stream_shade_all<true>, stream_trace_shade<false, true>, stream_shade_evicted<false, true>) depends on it.
// This list pins the order the launch ladders used to give, so that the device code stays what it was, instruction for instruction; nothing reads it.
#define REF(...) (const void *)__VA_ARGS__
[[maybe_unused]] static const void *const INSTANTIATION_ORDER[] = {
    REF(bvh_trace_queue<1>), REF(bvh_trace_queue<2>), REF(bvh_trace_queue<0>), REF(bvh_trace_level0<1>), REF(bvh_trace_level0<2>), REF(bvh_trace_level0<0>), REF(stream_shade_all<true>),
    REF(stream_trace_shade<true, true>), REF(stream_trace_shade<true>), REF(stream_trace_shade<false, true>), REF(stream_trace_shade<false>), REF(stream_shade_evicted<false, true>),
    REF(stream_shade_evicted<false>), REF(bvh_trace_shadow<0, 1, true>), REF(bvh_trace_shadow<0, 2, true>), REF(bvh_trace_shadow<0, 0, true>), REF(bvh_trace_shadow<0, 1>),
    REF(bvh_trace_shadow<0, 2>), REF(bvh_trace_shadow<0, 0>), REF(stream_trace_shadow<true>), REF(stream_trace_shadow_plan_wide<0>), REF(stream_trace_shadow_plan<0>),
    REF(stream_trace_shadow<false>), REF(bvh_trace_shadow<1, 1>), REF(bvh_trace_shadow<1, 2>), REF(bvh_trace_shadow<1, 0>), REF(stream_trace_shadow_plan_wide<1>),
    REF(stream_trace_shadow_plan<1>), REF(stream_resolve<true>), REF(stream_resolve<false>), REF(render_lanes<true, true>), REF(render_lanes<false, true>), REF(render_lanes<true>), REF(render_lanes<false>)};

// One kernel of a role's table, under the name a profile prints for it -- the entry's own text, so the two cannot part (describe_frame_kernels prints
// the names).  A kernel takes the argument block alone, or a level or a pass beside it: launch() hands both to either.  NO_BUILD: the combination has no kernel.
struct Kernel { const void *fn; const char *name; };
#define K(...) {REF(__VA_ARGS__), #__VA_ARGS__}
#define NO_BUILD {nullptr, nullptr}
static_assert(BVH_PLAIN == 0 && BVH_TALLY == 1 && BVH_CHECKED == 2, "the tables' variant rows are written out as 0, 1, 2");
// the level-0 walk beside the level queue, and the level queue: [variant]
static const Kernel LEVEL0[3] = {K(bvh_trace_level0<0>), K(bvh_trace_level0<1>), K(bvh_trace_level0<2>)};
static const Kernel QUEUE[3] = {K(bvh_trace_queue<0>), K(bvh_trace_queue<1>), K(bvh_trace_queue<2>)};
// the level kernel: [walk][gi].  (The GI builds of the plan and filter rows walk only: stream_shade_all<true> shades the level behind them.)
static const Kernel LEVEL[W_ROWS][2] = {{K(stream_trace_shade<false>), K(stream_trace_shade<false, true>)}, {K(stream_trace_shade<true>), K(stream_trace_shade<true, true>)},
                                        {K(stream_trace_shade_plan), K(stream_trace_plan_gi)}, {K(stream_trace_shade_plan_wide), K(stream_trace_plan_wide_gi)},
                                        {K(bvh_trace_shade), K(bvh_trace_shade_gi)}, {K(bvh_trace_shade_tally), NO_BUILD}, {K(bvh_trace_shade_checked), NO_BUILD}};
static const Kernel SHADE_ALL = K(stream_shade_all<true>);
// the bulk shadow pass (level 0's shadow rays) and the deeper levels' shadow pass: [pass][walk][by pixel]
static const Kernel SHADOW[2][W_ROWS][2] = {
    {{K(stream_trace_shadow<false>), NO_BUILD}, {K(stream_trace_shadow<true>), NO_BUILD}, {K(stream_trace_shadow_plan<0u>), NO_BUILD}, {K(stream_trace_shadow_plan_wide<0u>), NO_BUILD},
     {K(bvh_trace_shadow<0u, 0, false>), K(bvh_trace_shadow<0u, 0, true>)}, {K(bvh_trace_shadow<0u, 1, false>), K(bvh_trace_shadow<0u, 1, true>)},
     {K(bvh_trace_shadow<0u, 2, false>), K(bvh_trace_shadow<0u, 2, true>)}},
    {{K(stream_trace_shadow<false>), NO_BUILD}, {K(stream_trace_shadow<true>), NO_BUILD}, {K(stream_trace_shadow_plan<1u>), NO_BUILD}, {K(stream_trace_shadow_plan_wide<1u>), NO_BUILD},
     {K(bvh_trace_shadow<1u, 0, false>), NO_BUILD}, {K(bvh_trace_shadow<1u, 1, false>), NO_BUILD}, {K(bvh_trace_shadow<1u, 2, false>), NO_BUILD}}};
// the wave-per-ray kernels: [variant][gi] and [variant] (the bounds-checked build is the filter kernels' alone: the plain ones), their shading kernels: [gi].
// (The tallying build has no GI kernel, where the ladder it replaces would have taken heavy_trace_closest_gi: check_options refuses use_gi with
//  collect_counters == 2, so no frame gets there.)
static const Kernel HEAVY_CLOSEST[3][2] = {{K(heavy_trace_closest), K(heavy_trace_closest_gi)}, {K(heavy_trace_closest_tally), NO_BUILD}, {K(heavy_trace_closest), K(heavy_trace_closest_gi)}};
static const Kernel HEAVY_SHADOW[3] = {K(heavy_trace_shadow), K(heavy_trace_shadow_tally), K(heavy_trace_shadow)};
static const Kernel SHADE_EVICTED[2] = {K(stream_shade_evicted<false>), K(stream_shade_evicted<false, true>)};
// the resolve: [count]; the queue-less kernel -- a whole frame (launch_lanes_pass) or the last resort behind the stream pass: [count][gi]
static const Kernel RESOLVE[2] = {K(stream_resolve<false>), K(stream_resolve<true>)};
static const Kernel LANES[2][2] = {{K(render_lanes<false>), K(render_lanes<false, true>)}, {K(render_lanes<true>), K(render_lanes<true, true>)}};

// development (FramePlan::debug_sync): every kernel of every table with its address, ahead of a frame's launches
static void print_tables() {
    const std::pair<const Kernel *, size_t> tables[] = {{LEVEL0, sizeof(LEVEL0)}, {QUEUE, sizeof(QUEUE)}, {LEVEL[0], sizeof(LEVEL)}, {&SHADE_ALL, sizeof(SHADE_ALL)}, {SHADOW[0][0], sizeof(SHADOW)},
        {HEAVY_CLOSEST[0], sizeof(HEAVY_CLOSEST)}, {HEAVY_SHADOW, sizeof(HEAVY_SHADOW)}, {SHADE_EVICTED, sizeof(SHADE_EVICTED)}, {RESOLVE, sizeof(RESOLVE)}, {LANES[0], sizeof(LANES)}};
    fprintf(stderr, "[frame]");
    for (const auto &t : tables)
        for (const Kernel *k = t.first; k < t.first + t.second / sizeof(Kernel); k++) if (k->name) fprintf(stderr, " %s %p", k->name, k->fn);
    fprintf(stderr, "\n");
}

// One launch of a table's kernel; `n`: the level or pass, which a kernel that takes none leaves alone.  A null entry is an error: the plan chose a
// build that does not exist.  Development (FramePlan::debug_sync): the launch is announced on stderr and waited for.
static hipError_t launch(const FramePlan &P, const Kernel &K, uint32_t blocks, hipStream_t stream, KernelArgs A, uint32_t n = 0u, uint32_t lds_bytes = 0u) {
    if (!K.fn) return hipErrorInvalidDeviceFunction;
    if (P.debug_sync) { fprintf(stderr, "[launch] %s blocks %u ...", K.name, blocks); fflush(stderr); }
    void *args[] = {&A, &n};
    const hipError_t rc = hipLaunchKernel(K.fn, dim3(blocks), dim3(BLOCK), args, lds_bytes, stream);
    if (P.debug_sync) { hipError_t e = hipDeviceSynchronize(); fprintf(stderr, " done (%s)\n", hipGetErrorString(e)); fflush(stderr); }
    return rc;
}

// The one launch ahead of a frame's kernels (kernel_stream.h: stream_frame_reset): this frame's argument block from its pinned slot into its
// device slot, render_lanes' pixel counter, and -- the ray-stream pass -- the frame's counters, the level queue's words, the tallies and
// the two preset words.  Every path of launch_frame starts with it, on the frame's stream, so the kernels behind it see the same order.
static void launch_frame_reset(crt_ctx *ctx, const FramePlan &P, hipStream_t stream, uint32_t shadow_preset, uint32_t split_preset) {
    hipLaunchKernelGGL(stream_frame_reset, dim3(1), dim3(256), 0, stream, P.stream_mode ? ctx->d_scounts : (uint32_t *)nullptr,
                       P.stream_mode && P.queue ? ctx->d_lq_words : (uint32_t *)nullptr, P.stream_mode && P.exec_count ? ctx->d_exec : (unsigned long long *)nullptr,
                       shadow_preset, split_preset, ctx->d_sync, (uint32_t *)(ctx->d_frame_ring + P.slot), (const uint32_t *)(ctx->h_frame_ring_dev + P.slot));
}

// Levels 0 .. MAX_DEPTH on `stream`; after level 0 the bulk shadow pass (and the walks it gives up) on the side stream -- or, where the level
// queue runs beside level 0 and `stream` has nothing else to do (FramePlan::one_stream), on `stream` itself.
static int launch_stream_levels(crt_ctx *ctx, const crt_options *o, const FramePlan &P, KernelArgs &A, hipStream_t stream) {
    const uint32_t fixed_slots = P.fixed0 ? (uint32_t)P.vitems * 64u * ctx->n_lights : 0u;
    launch_frame_reset(ctx, P, stream, fixed_slots, P.split_known ? fixed_slots : 0u);
    const uint32_t side_per_cu = ctx->tuning.side_blocks;  // workgroups per CU of the bulk shadow pass beside the levels
    A.exec_count = P.exec_count ? 1u : 0u;
    A.exec_counters = ctx->d_exec;
    A.exec_plan = ctx->d_exec + 4;
    // the plan kernels pay a wave-uniform loop per refill, whatever the number of new rays: refill in bundles
    A.bundle = REFILL_BUNDLE;
    A.wave_prio = 3u;  // the levels' waves (the frame's critical path) ahead of the bulk shadow pass's, which share their SIMDs
    A.force_whole = 0u;
    A.chunk = ctx->tuning.fetch_chunk >> 16;   // (level 0's claims; crt_tuning::fetch_chunk)
    KernelArgs S = A;  // argument block of the bulk shadow pass
    S.wave_prio = 0u;
    S.chunk = ctx->tuning.fetch_chunk & 0xFFFFu;
    S.counters = ctx->d_counters + C_N;
    S.exec_counters = ctx->d_exec + 2;  // it tallies on its own
    S.exec_plan = ctx->d_exec + 5;
    {
        // The pass is one persistent launch: it ends when its longest walk ends, so the budget after which a walk is
        // handed to heavy_trace_shadow should be about the steps one lane gets through in the whole launch --
        // rays per lane x ~130 steps per ray (measured average on the benchmark scenes) -- and no more than the cap
        // (crt_tuning::shadow_budget).  A rank that renders 1/8 of the tiles gets 1/8 of the budget.
        const uint64_t lanes = (uint64_t)ctx->num_cus * (side_per_cu ? side_per_cu : 8u) * BLOCK;
        const uint64_t est = (uint64_t)P.vitems * 64u * ctx->lights() * 130u / (lanes ? lanes : 1u);
        uint32_t budget = est > ctx->tuning.shadow_budget ? ctx->tuning.shadow_budget : (uint32_t)est;
        if (budget < ctx->step_budget) budget = std::min(ctx->step_budget, ctx->tuning.shadow_budget);
        S.step_budget = P.heavy ? budget : 0u;
    }
    // the same reasoning for level 0 (one launch over all primary rays, ~70 steps per ray)
    const uint64_t est0 = (uint64_t)P.vitems * 64u * 70u / ((uint64_t)P.lane_blocks * BLOCK);
    uint32_t budget0 = est0 >= P.level_budget ? P.level_budget : (est0 < 64u ? 64u : (uint32_t)est0);
    if (ctx->tuning.level0_budget) budget0 = ctx->tuning.level0_budget;
    // every level below level 0: one launch that feeds itself (kernel_bvh.h); one workgroup per CU holds more lanes than the widest
    // level of a frame of this size has rays
    auto launch_queue = [&](hipStream_t where) {
        KernelArgs Q = A;
        const uint32_t qblocks = std::min(P.lane_blocks, (uint32_t)ctx->num_cus * std::max(1u, ctx->tuning.level_queue & 15u));
        // A reflection child continues in the lane that shaded its parent (no hand-over through memory) where the launch is a matter of
        // latency -- few rays: HW14 3.37 -> 3.29 ms, an eighth of its tiles 2.25 -> 2.04 -- and goes through the queue like the others where
        // it is a matter of balance (HW11, 65 - 85 k rays per level: 4.0 ms through the queue, 4.5 with chains kept in their lanes)
        Q.force_whole = (P.widest > 70000u || (ctx->tuning.level_queue & 256u)) ? 1u : 0u;
        Q.bundle = ctx->tuning.level0_budget ? ctx->tuning.level0_budget - 1u : 15u;   // (development: turns between two housekeeping rounds, as a mask)
        return launch(P, QUEUE[P.variant], qblocks, where, Q);
    };
    // the plan kernels' mesh lists (kernel_plan.h) live in dynamic LDS
    const uint32_t plds = P.walk == W_PLAN || P.walk == W_WIDE ? ctx->scene.plan_list_words * BLOCK * (uint32_t)sizeof(uint32_t) : 0u;
    for (uint32_t g = 0; g <= o->max_depth; g++) {
        A.step_budget = P.heavy ? (g == 0 ? budget0 : P.level_budget) : 0u;
        // The per-lane kernel of a deeper level fetches its rays through a cursor, so any grid does the whole level; beside
        // the bulk shadow pass every workgroup of it waits for a free P.slot, and a level below heavy_level_threshold has
        // nothing for it to do (measured: 0.15 ms for an empty full-size grid).  Sized by what the level held a frame ago.
        // (the filter kernels' GI builds keep the full grid)
        uint32_t level_blocks = P.lane_blocks;
        if (g >= 1 && P.lean && P.prev && !(P.bvh && P.gi)) {
            const uint32_t was = P.prev[SC_COUNT + g];
            const uint32_t want = was < ctx->frame.heavy_level_threshold ? 64u : std::max<uint32_t>((uint32_t)ctx->num_cus, (was + was / 2u + BLOCK - 1) / BLOCK);
            level_blocks = std::min(P.lane_blocks, want);
        }
        if (P.queue && g == 0) {
            // The level queue's launch starts WITH level 0, on a stream of its own: its waves sleep until level 0's first reflective or
            // refractive hits reserve entries, and a pixel's chain of up to eight dependent walks -- the frame's critical path -- begins while
            // the other primary rays are still being walked, not after the last of them.  It may end once level 0 has (LQ_LEVEL0).
            if (P.early_queue && o->max_depth >= 1) {
                CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev_reset[P.slot], stream));
                CRT_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->early, ctx->ev_reset[P.slot], 0));
                CRT_HIP_CHECK(ctx, launch_queue(ctx->early));
                if (ctx->tuning.level_queue & 4096u) {
                    // (tests: level 0 held back until that launch has ENDED -- what a profiler that serialises launches, or two streams on one
                    //  hardware queue, do to it: the launch must sit out its patience and leave, and the one behind level 0 must walk everything)
                    CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev_queue[P.slot], ctx->early));
                    CRT_HIP_CHECK(ctx, hipStreamWaitEvent(stream, ctx->ev_queue[P.slot], 0));
                }
            }
            CRT_HIP_CHECK(ctx, launch(P, LEVEL0[P.variant], P.lane_blocks, stream, A));
        }
        else {
            CRT_HIP_CHECK(ctx, launch(P, LEVEL[P.walk][P.gi], level_blocks, stream, A, g, plds));
            // the GI mode of the plan and filter kernels: the walk alone, then the level's shading -- sample directions, gi_samples child rays -- with every lane busy
            // (kernel_plan.h, SPLIT; tools/gi_time.py hw14 960x540 d3 n2 r2: 42.3 ms on the device against 44.0 with the shading inside the walk)
            if (P.gi && P.walk >= W_PLAN) CRT_HIP_CHECK(ctx, launch(P, SHADE_ALL, level_blocks, stream, A, g));
        }
        if (P.heavy && !P.bvh) {   // (the filter kernels walk what they cannot decide themselves, in the reference's order: nothing is handed over)
            CRT_HIP_CHECK(ctx, launch(P, HEAVY_CLOSEST[P.variant][P.gi], HEAVY_BLOCKS, stream, A, g));
            CRT_HIP_CHECK(ctx, launch(P, SHADE_EVICTED[P.gi], 256u, stream, A, g));
        }
        if (g == 0) {
            // where level 0's shadow rays end (unless the reset launch has said so already); they start now, on the side stream, beside the deeper levels
            if (!P.split_known) hipLaunchKernelGGL(stream_mark_split, dim3(1), dim3(64), 0, stream, A, (uint32_t)SC_SHADOW_SPLIT, (uint32_t)SC_SHADOW);
            hipStream_t where = side_per_cu && !P.one_stream ? ctx->side : stream;
            // (one stream: ev_s0 below marks level 0's end too -- the queue's second launch waits for that one; each record between two
            //  launches of a stream holds the second back by ~5 us, timed or not)
            if (side_per_cu && !P.one_stream) {
                CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev_fork[P.slot], stream));
                CRT_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_fork[P.slot], 0));
            }
            if (P.one_stream && o->max_depth == 0) CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev1[P.slot], stream));   // (no queue launch: the levels end here)
            CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev_s0[P.slot], where));
            // (beside the levels its persistent waves must leave wave slots on every CU for the level kernels)
            const uint32_t blocks0 = side_per_cu ? std::min(ctx->grid_blocks, (uint32_t)ctx->num_cus * side_per_cu) : ctx->grid_blocks;   // (a spill region holds grid_blocks workgroups' columns)
            // (by pixel, a claimed pixel is n_lights walks: the chunk that suits the slot pass, in pixels, is n_lights times as much work for a
            //  wave to sit on beside the queue's waves -- DESIGN.md section 7, the cursor word; whole tiles, never below a wave's refill of 64)
            if (P.by_pixel) S.chunk = std::max(64u, (S.chunk / std::max(1u, ctx->n_lights)) & ~63u);
            CRT_HIP_CHECK(ctx, launch(P, SHADOW[0][P.walk][P.by_pixel], blocks0, where, S, 0u));
            // ... and behind it the walks it gave up, still beside the levels; the mark comes before the event the
            // caller's stream waits for, so nothing the later pass appends is below it
            if (P.heavy && !P.bvh) hipLaunchKernelGGL(stream_mark_split, dim3(1), dim3(64), 0, where, S, (uint32_t)SC_SHEAVY_SPLIT, (uint32_t)SC_SHEAVY);
            CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev_s1[P.slot], where));
            if (P.heavy && !P.bvh) CRT_HIP_CHECK(ctx, launch(P, HEAVY_SHADOW[P.variant], HEAVY_BLOCKS, where, S, 0u));
            if (!P.one_stream) CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev_s2[P.slot], where));   // (one stream: nothing waits for it, nobody reads it)
        }
        if (P.queue) {
            if (P.early_queue && o->max_depth >= 1) {
                // ... and once more behind level 0 AND the first launch: nothing promises that two streams' kernels run side by side, so the
                // first launch's patience with an empty queue is bounded, and what it left is walked here (normally nothing: ~15 us)
                CRT_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->early, P.one_stream ? ctx->ev_s0[P.slot] : ctx->ev_fork[P.slot], 0));
                CRT_HIP_CHECK(ctx, launch_queue(ctx->early));
                // (the pass holds `stream` until it ends: "recursion levels" still ends where this launch does)
                if (P.one_stream) CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev1[P.slot], ctx->early));
                CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev_queue[P.slot], ctx->early));
                CRT_HIP_CHECK(ctx, hipStreamWaitEvent(stream, ctx->ev_queue[P.slot], 0));
            }
            else if (o->max_depth >= 1) CRT_HIP_CHECK(ctx, launch_queue(stream));
            break;
        }
    }
    return CRT_OK;
}

// The deeper levels' shadow rays, the wave-per-ray walks of both passes, the per-pixel combination, the last resort.
static int launch_stream_tail(crt_ctx *ctx, const FramePlan &P, KernelArgs &A, hipStream_t stream) {
    const uint32_t side_per_cu = ctx->tuning.side_blocks;
    CRT_HIP_CHECK(ctx, hipGetLastError());
    if (!P.one_stream) CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev1[P.slot], stream));   // (one stream: recorded where the levels ended, launch_stream_levels)
    // the shadow rays of the deeper levels (queued behind level 0's), then the wave-per-ray walks of both passes
    if (side_per_cu && !P.one_stream) CRT_HIP_CHECK(ctx, hipStreamWaitEvent(stream, ctx->ev_s1[P.slot], 0));
    KernelArgs S1 = A;
    S1.wave_prio = 0u;
    S1.counters = ctx->d_counters + 2 * C_N;
    {
        // few rays, all tail: the short budget of the levels, or less when this launch is small (the deeper levels
        // queue about a quarter of a shadow ray per pixel on the benchmark scenes)
        const uint64_t rays1 = P.prev && P.prev[SC_SHADOW] >= P.prev[SC_SHADOW_SPLIT] ? P.prev[SC_SHADOW] - P.prev[SC_SHADOW_SPLIT] : (uint64_t)P.vitems * 16u;
        const uint64_t est1 = rays1 * 130u / ((uint64_t)P.lane_blocks * BLOCK);
        // (a GI frame queues most of its shadow rays here -- tens of millions: then this pass is a bulk pass like pass 0 and gets its cap)
        const uint32_t cap1 = std::max(P.level_budget, ctx->tuning.shadow_budget);
        S1.step_budget = P.heavy ? (est1 >= cap1 ? cap1 : (est1 < 64u ? 64u : (uint32_t)est1)) : 0u;
    }
    // (the level queue's lanes have walked the deeper levels' shadow rays themselves: kernel_bvh.h, BVH_SHADOWS)
    if (!P.queue) CRT_HIP_CHECK(ctx, launch(P, SHADOW[1][P.walk][0], P.lane_blocks, stream, S1, 1u));
    if (side_per_cu && !P.one_stream) CRT_HIP_CHECK(ctx, hipStreamWaitEvent(stream, ctx->ev_s2[P.slot], 0));
    if (P.heavy && !P.bvh) CRT_HIP_CHECK(ctx, launch(P, HEAVY_SHADOW[P.variant], HEAVY_BLOCKS, stream, S1, 1u));
    CRT_HIP_CHECK(ctx, hipGetLastError());
    // (one stream: the later of ev_s1, recorded behind the pass on this stream, and ev1 marks this point: crt_kernel_times_ms reads them, slot_ev2_is_s1)
    if (!P.one_stream) CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev2[P.slot], stream));
    A.counters = ctx->d_counters + 2 * C_N;
    // post-order combination per pixel, then the queue-less fallback, which only runs after an overflow
    CRT_HIP_CHECK(ctx, launch(P, RESOLVE[P.count], P.lane_blocks, stream, A));
    A.only_if_overflow = 1;
    const uint32_t fallback_blocks = std::max(1u, std::min(ctx->grid_blocks, (P.n_items * 64u + BLOCK - 1) / BLOCK));
    // (not behind a probing attempt, launch_render: the host looks at the overflow word itself)
    if (P.last_resort) CRT_HIP_CHECK(ctx, launch(P, LANES[P.count][P.gi], fallback_blocks, stream, A));
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

// The whole frame by render_lanes: crt_tuning::mode = lanes, and GI frames too large for the ray-stream pass.
static int launch_lanes_pass(crt_ctx *ctx, const FramePlan &P, KernelArgs &A, hipStream_t stream) {
    launch_frame_reset(ctx, P, stream, 0u, 0u);   // (the argument block and the pixel counter: this pass has no counters of the stream's)
    CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev1[P.slot], stream));
    A.counters = ctx->d_counters + C_N;
    CRT_HIP_CHECK(ctx, launch(P, LANES[P.count][P.gi], P.lane_blocks, stream, A));
    CRT_HIP_CHECK(ctx, hipGetLastError());
    for (hipEvent_t e : {ctx->ev_s0[P.slot], ctx->ev_s1[P.slot], ctx->ev_s2[P.slot], ctx->ev2[P.slot]}) CRT_HIP_CHECK(ctx, hipEventRecord(e, stream));
    return CRT_OK;
}

// The plan of the context's next frame, of everything the COMPLETED frames have left: nothing is harvested between it and the frame's launches.
static int next_plan(crt_ctx *ctx, const crt_options *o, uint32_t n_items, bool last_resort, FramePlan &P) {
    harvest_counts(ctx);
    if (ctx->launches >= (uint64_t)crt_ctx::EV_RING) {
        // the slot's previous frame (64 launches ago) must be complete before its events, its pinned words and its argument block are reused
        CRT_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev4[ctx->launches % crt_ctx::EV_RING]));
        harvest_counts(ctx);
    }
    P = make_plan(ctx, o, n_items, last_resort);
    return CRT_OK;
}

// One frame's launches.  Ray-stream path (kernel_stream.h), per recursion level g = 0 .. MAX_DEPTH on `stream`:
//   the per-lane kernel (plan kernels; the faithful kernel for the counting build and for scenes without a plan),
//   heavy_trace_closest for the walks it handed over (or the whole level), stream_shade_evicted for their hits;
// the bulk shadow pass (level 0's shadow rays) on the side stream (or `stream`: launch_stream_levels) as soon as level 0 is done, then the deeper levels'
// shadow rays, the wave-per-ray shadow walks, stream_resolve, and render_lanes, which only runs after a queue overflow.
static int launch_frame(crt_ctx *ctx, const crt_options *o, FramePlan &P, float *d_out, uint32_t packed, hipStream_t stream) {
    const uint32_t n_items = P.n_items;
    const int slot = P.slot;
    if (P.stream_mode && o->max_depth + 1 > (uint32_t)MAX_GENERATIONS) {
        ctx->error = "max_depth too large for the ray-stream pass";
        return CRT_ERR_INVALID;
    }
    int rc = ensure_frames(ctx, o->max_depth, P.gi);
    if (rc) return rc;
    FrameArgs &F = ctx->frame;
    F.use_gi = P.gi ? 1u : 0u;
    F.gi_samples = o->gi_sample_size;
    F.rays_per_pixel = o->rays_per_pixel;
    F.monte_carlo_bias = o->monte_carlo_bias;
    F.gi_seed = o->gi_seed;
    F.level0_samples = P.samples;
    F.max_depth = o->max_depth;
    F.shadow_bias = o->shadow_bias;
    F.reflection_bias = o->reflection_bias;
    F.refraction_bias = o->refraction_bias;
    F.items = ctx->d_items;
    F.n_items = n_items;
    F.pixel_counter = ctx->d_sync + 0;
    F.out = d_out;
    F.packed = packed;
    F.s_counts = ctx->d_scounts;
    F.fallback_total = ctx->d_fallback_total;
    F.s_lq_words = ctx->d_lq_words;
    F.lq_epoch = (uint32_t)(ctx->launches & 0x7FFFFFFFull) + 1u;   // the level queue's tag of this frame (this context's buffer has never seen it: tags only grow)
    // The walks' spill regions (kernel_bvh.h: bvh_stack_of), one per stream of a frame, because these launches may run side by side:
    //   bvh_spill        `stream`: bvh_trace_level0 / bvh_trace_shade* (lane_blocks or level_blocks <= grid_blocks workgroups), and behind
    //                    them bvh_trace_shadow<1> (lane_blocks), which uses the side region: pass 0 has ended by then (ev_s1)
    //   bvh_spill_side   ctx->side (`stream` behind level 0 on the one-stream path): bvh_trace_shadow<0> (num_cus x side_blocks, at most
    //                    grid_blocks) beside the levels and the queue
    //   bvh_spill_queue  ctx->early (or `stream` behind level 0): bvh_trace_queue (at most lane_blocks), beside level 0 and pass 0; its
    //                    second launch runs behind the first on the same stream
    // Frames of one context follow one another on `stream`; a query has scratch of its own (crt_query.hip).
    F.bvh_spill = ctx->d_bvh_spill;
    F.bvh_spill_side = ctx->d_bvh_spill ? ctx->d_bvh_spill + ctx->bvh_spill_words() : nullptr;
    F.bvh_spill_queue = ctx->d_bvh_spill ? ctx->d_bvh_spill + 2u * ctx->bvh_spill_words() : nullptr;
    F.bvh_spill_words = ctx->d_bvh_spill ? ctx->bvh_spill_words() : 0u;
    if (P.count) CRT_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_counters, 0, 3 * C_N * sizeof(unsigned long long), stream));
    ctx->slot_items[slot] = 0;
    CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev0[slot], stream));
    if (n_items == 0) {
        // nothing to render: the events still bracket an (empty) frame, so that every reader of a slot finds recorded events
        for (hipEvent_t e : {ctx->ev1[slot], ctx->ev_s0[slot], ctx->ev_s1[slot], ctx->ev_s2[slot], ctx->ev2[slot], ctx->ev3[slot], ctx->ev4[slot]})
            CRT_HIP_CHECK(ctx, hipEventRecord(e, stream));
        ctx->slot_ev2_is_s1[slot] = false;
        ctx->launches++;
        return CRT_OK;
    }
    if (P.debug_sync) print_tables();
    if (P.stream_mode) {
        rc = ensure_stream(ctx, P);
        if (rc) return rc;
        finish_plan(ctx, P);
        F.heavy_level_threshold = (P.lean && !P.bvh) ? ctx->tuning.heavy_level : 0u;  // (filter frames: the wave-per-ray kernel takes the evicted rays only)
        F.fixed0 = P.fixed0 ? 1u : 0u;
    }
    // this frame's argument block, into its own pinned slot: the frame's reset launch -- the first on `stream` in either pass below --
    // copies it to the device slot the kernels read
    ctx->h_frame_ring[slot] = F;
    KernelArgs A{};
    A.s = (scene_args_p)ctx->d_scene;
    A.f = (frame_args_p)(ctx->d_frame_ring + slot);
    A.counters = ctx->d_counters;
    rc = P.stream_mode ? launch_stream_levels(ctx, o, P, A, stream) : launch_lanes_pass(ctx, P, A, stream);
    if (rc == CRT_OK && P.stream_mode) rc = launch_stream_tail(ctx, P, A, stream);
    if (rc) return rc;
    // what this frame leaves for the next ones: its counter block, the fallback total in its last word, into this frame's own pinned slot
    // in ONE copy (render_lanes alone leaves no counters: the total only)
    uint32_t *h = ctx->h_ring + (size_t)slot * crt_ctx::H_SLOT_WORDS;
    if (P.stream_mode) CRT_HIP_CHECK(ctx, hipMemcpyAsync(h, ctx->d_scounts, SC_ALLOC_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    else CRT_HIP_CHECK(ctx, hipMemcpyAsync(h + SC_FALLBACK_TOTAL, ctx->d_fallback_total, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    ctx->slot_items[slot] = P.stream_mode ? P.vitems : 0u;
    ctx->slot_cfg[slot] = frame_config_of(o);
    ctx->slot_ev2_is_s1[slot] = P.one_stream;
    CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev3[slot], stream));
    CRT_HIP_CHECK(ctx, hipEventRecord(ctx->ev4[slot], stream));
    ctx->launches++;
    return CRT_OK;
}

// A frame whose queues are not yet known to fit -- the first of its size on this context, or the one after a frame that
// overflowed -- is PROBED: the stream pass is enqueued without the queue-less fallback behind it, the call waits for it and
// reads its overflow word, and an attempt that did not fit is repeated with queues sized by what it learnt (grow_queue_sizing) until it
// does; every attempt ends early at the first overflow, so a failed one costs less than a frame.  Once a frame of this size has
// completed without overflow the call is asynchronous again, with render_lanes behind the stream pass as the last resort for a
// frame that outgrows its queues all the same (and for explicit capacities, crt_tuning, which are never regrown).
int launch_render(crt_ctx *ctx, const crt_options *o, uint32_t n_items, float *d_out, uint32_t packed, hipStream_t stream) {
    FramePlan P;
    int rc = next_plan(ctx, o, n_items, true, P);
    const bool probe = P.stream_mode && !P.fixed_caps && !P.prev && n_items != 0;   // (otherwise this plan is the frame's: one plan per frame)
    for (int attempt = 0; rc == CRT_OK; attempt++) {
        const bool last = !probe || attempt == 5;
        if (probe) rc = next_plan(ctx, o, n_items, last, P);   // (an attempt's own plan: without the last resort, of what the attempt before it left)
        if (rc == CRT_OK) rc = launch_frame(ctx, o, P, d_out, packed, stream);
        if (rc || last) return rc;
        CRT_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev4[P.slot]));
        harvest_counts(ctx);
        if (ctx->last_counts_items != P.vitems) { ctx->error = "internal: a probing frame left no counters"; return CRT_ERR_HIP; }
        if (!ctx->last_counts[SC_OVERFLOW]) return CRT_OK;
        ctx->regrows++;
        const bool can_grow = !ctx->last_counts[SC_GUARD] && grow_queue_sizing(ctx, P.vitems, o->max_depth);
        if (!can_grow) {  // (a walk beyond its bound, or no memory to grow into)
            rc = next_plan(ctx, o, n_items, true, P);
            return rc ? rc : launch_frame(ctx, o, P, d_out, packed, stream);
        }
    }
    return rc;
}

// Which kernels a production frame of this context runs (bench.py names the roofline's kernel with it): the plan of a frame under default
// options with the last resort behind it, named from the tables -- the plain builds' names, whatever build the tuning or the last frame asked
// for.  "shadow0" follows the LAST frame's plan: by pixel before the first frame and after a frame that had fixed slots outside the GI mode,
// by slot after a GI frame or a frame without fixed slots -- it describes what ran, not what the next frame's options will choose.
std::string describe_frame_kernels(const crt_ctx *ctx) {
    crt_options o{};
    o.max_depth = 5;
    const FramePlan P = make_plan(ctx, &o, 0u, true);
    if (!P.stream_mode) return std::string("all=") + LANES[0][0].name;
    const int walk = P.bvh ? W_BVH + BVH_PLAIN : P.walk;
    const Kernel &level = LEVEL[walk][0];
    return std::string("level0=") + (P.queue ? LEVEL0[BVH_PLAIN] : level).name + ";shadow0=" + SHADOW[0][walk][P.bvh && ctx->shadow0_by_pixel].name +
           ";levels=" + (P.queue ? QUEUE[BVH_PLAIN] : P.heavy && !P.bvh ? HEAVY_CLOSEST[BVH_PLAIN][0] : level).name;
}

// Called after a synchronisation: the last frame's slot tells whether the frame was redone by the queue-less kernel.
void note_overflow(crt_ctx *ctx) {
    harvest_counts(ctx);
    ctx->overflows = ctx->fallbacks_seen;
    ctx->stats.fallback_frames = (uint32_t)ctx->overflows;
    ctx->stats.queue_bytes = ctx->queue_bytes;
    ctx->stats.queue_regrows = ctx->regrows;
}

int fetch_counters(crt_ctx *ctx, const crt_options *o, uint64_t pixels) {
    ctx->stats.pixels = pixels;
    ctx->stats.counters_valid = o->collect_counters == 1 ? 1 : 0;
    if (o->collect_counters == 2)
        CRT_HIP_CHECK(ctx, hipMemcpy(ctx->exec_counters, ctx->d_exec, sizeof(ctx->exec_counters), hipMemcpyDeviceToHost));
    if (o->collect_counters == 1) {
        unsigned long long c2[3 * C_N], c[C_N];
        CRT_HIP_CHECK(ctx, hipMemcpy(c2, ctx->d_counters, sizeof(c2), hipMemcpyDeviceToHost));
        for (int k = 0; k < C_N; k++) {
            c[k] = c2[k] + c2[C_N + k] + c2[2 * C_N + k];
            ctx->level_counters[k] = c2[k];
            ctx->shadow0_counters[k] = c2[C_N + k];
        }
        ctx->stats.box_tests = c[C_BOX]; ctx->stats.tri_tests = c[C_TRI]; ctx->stats.leaf_index_reads = c[C_LEAFIDX];
        ctx->stats.shaded_hits = c[C_HIT]; ctx->stats.light_evals = c[C_LIGHT]; ctx->stats.texel_fetches = c[C_TEXEL];
        ctx->stats.primary_rays = c[C_PRIMARY]; ctx->stats.secondary_rays = c[C_SECONDARY]; ctx->stats.shadow_rays = c[C_SHADOW];
    }
    return CRT_OK;
}
