// crt_giframe.hip -- the GI frame calls (include/crt_hip.h): a GI frame of the context's camera on the context's colour buffer, rendered
// sample pass by sample pass, and what is made of its state.  The radiance passes, the guides' traces and the level arrays are the
// queries' (crt_query.hip, through the few functions of crt_internal.h); the frame's state, the guides and the histories are this file's:
//   a progressive frame  crt_render_progressive: the rays and keys of one sample (crt_camera_sample_rays_device), the GI radiance query, one
//                     step of the pixel's fold (crt_accumulate_samples_device); kernels: csrc/kernel_progressive.h
//   an adaptive frame  crt_render_adaptive: the same loop over a pixel list that shrinks -- the step, the rule and the compaction of
//                     crt_adaptive_step_device; kernels: csrc/kernel_adaptive.h, the rule: csrc/adaptive_rule.h
//   a denoised frame  crt_render_denoised: the adaptive frame's state through the denoiser's primitives (crt_denoise.hip), guided by the
//                     first hits of the camera's rays; it changes nothing of the frame
//   an accumulated frame  crt_render_accumulated: that state merged with the last frame's history through the temporal primitive
//                     (crt_temporal.hip), then through the denoiser's launches; the context's two history pairs
//   a split frame     crt_render_adaptive_split, crt_render_denoised_split, crt_render_accumulated_split: the three calls above with every
//                     sample cut into its direct light and the rest (crt_split.hip, csrc/split_rule.h) -- the rest is what is filtered and
//                     reprojected, the direct part is added back untouched
//   the variance estimate  crt_set_variance_estimate: one launch more (crt_variance.hip) between the stage that produces colour and variance
//                     and the a-trous filter of the denoised and accumulated calls, under the filter's guides
// One body per stage: render_samples for the three sample-pass calls, post_begin and post_output around the two kinds of post-processing.
// Which call may continue which frame, and when a history's `current` becomes `previous`: csrc/giframe_rule.h.
#include "device_array.h"
#include "gi_random.h"
#include "giframe_rule.h"

namespace {
#include "kernel_progressive.h"
#include "kernel_adaptive.h"
}  // namespace

// a history pair: the ledger (giframe_rule.h), its two slots and the pose of the frame that wrote each
struct History : HistoryLedger {
    DeviceArray<crt_history_pixel> slot[2];
    crt_camera_pose pose[2] = {};
};

struct crt_giframe_state {
    // the frame under way: its kind, the samples (passes) folded in so far, its serial number (it advances wherever the guides are dropped
    // with the frame), and whether its guides have been traced
    FrameKind kind = FRAME_NONE;
    uint32_t samples = 0;
    uint64_t serial = 0;
    bool guides = false;
    // crt_render_progressive: the frame's H*W*3 sums, one sample's rays, keys and colours for every pixel
    DeviceArray<float> prog_sum, prog_rgb;
    DeviceArray<crt_ray> prog_rays;
    DeviceArray<uint32_t> prog_keys;
    // crt_render_adaptive: one float and one count more per pixel, two pixel lists (this pass's and the next one's), the next list's length
    // -- and where it comes back through pinned memory --, the compaction's work area; the settings and biases latched at pass 0
    DeviceArray<float> prog_sq;
    DeviceArray<uint32_t> prog_counts, prog_list[2], prog_next_n;
    uint32_t *pin_next_n = nullptr;
    DeviceArray<unsigned long long> prog_work;
    crt_adaptive adaptive{};
    float reflection_bias = 0, refraction_bias = 0;
    uint64_t active = 0;   // entries of prog_list[cur]; pass 0 has no list (every pixel), nor has a uniform frame
    int cur = 0;
    // crt_render_adaptive_split: beside the fold's state the sums of the samples' direct parts and the first and second moment of the rest
    // (csrc/split_rule.h), and one pass's direct parts beside prog_rgb
    DeviceArray<float> split_direct, split_dsum, split_rsum, split_rsq;
    // crt_render_denoised: the guides (the first hits of the camera's centre rays, traced at a frame's first post-processing call and kept
    // until the frame ends), the mean and variance of the fold's state, the denoised frame, the primitive's work area, the quantised frame
    DeviceArray<crt_hit> den_hits;
    DeviceArray<float> den_mean, den_var, den_out;
    DeviceArray<float4> den_work;
    DeviceArray<uint8_t> den_q8;
    // crt_set_guide_bounces > 0: beside them the chain guides of the same rays (crt_guide_rays_device's records), which the spatial filter
    // then runs under, and that call's work area; traced and dropped with den_hits
    DeviceArray<crt_hit> den_chain;
    DeviceArray<float4> guide_work;
    // crt_render_accumulated*: hist[0] holds the moments of whole colours (crt_render_accumulated), hist[1] those of the rest
    // (crt_render_accumulated_split), which must never meet; the merged colour, variance and valid-tap counts
    History hist[2];
    DeviceArray<float> acc_rgb, acc_var;
    DeviceArray<uint8_t> acc_valid;
    // crt_set_variance_estimate: the setting (off by default), and for the denoised calls, which have no records, the moment records of
    // the frame's state: written by the temporal launch with no history, read by the estimate, never a history slot
    bool estimate_on = false;
    crt_variance_estimate estimate{};
    DeviceArray<crt_history_pixel> est_records;
    void new_frame() { guides = false; serial++; }   // the guides and `current` are the ended frame's
    ~crt_giframe_state() {
        if (pin_next_n) (void)hipHostFree(pin_next_n);
    }
};

void giframe_destroy(crt_ctx *ctx) {
    delete ctx->giframe;
    ctx->giframe = nullptr;
}

void giframe_reset(crt_ctx *ctx) {
    crt_giframe_state *f = ctx->giframe;
    if (!f) return;
    f->kind = FRAME_NONE;
    f->samples = 0;
    f->active = 0;
    f->new_frame();
}

// this file's state, made by the first call that needs it
static int giframe_state(crt_ctx *ctx) {
    if (!ctx->giframe) ctx->giframe = new (std::nothrow) crt_giframe_state;
    if (!ctx->giframe) { ctx->error = "out of memory"; return CRT_ERR_NOMEM; }
    return CRT_OK;
}

// a frame call's bracket
static int giframe_begin(crt_ctx *ctx, const CallKind kind) {
    if (int rc = query_begin(ctx, ctx->stream, kind)) return rc;
    return giframe_state(ctx);
}

// the adaptive calls' pinned word, made by the first of them (a uniform frame reads nothing back)
static int pin_reserve(crt_ctx *ctx, uint32_t *&pin) {
    if (!pin) CRT_HIP_CHECK(ctx, hipHostMalloc((void **)&pin, sizeof(uint32_t)));
    return CRT_OK;
}

// ---- progressive GI frames (csrc/kernel_progressive.h): the frame's left fold over a pixel's samples, cut into sample passes.

// what the two primitives ask of (d_pixels, n): without a list the call is for the whole frame; one thread per entry must fit a grid
int progressive_check(crt_ctx *ctx, const char *what, const uint32_t *d_pixels, const uint64_t n) {
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    if (!d_pixels && n != pixels)
        return refuse(ctx, what, "d_pixels is NULL, so n must be width * height = " + std::to_string(pixels) + ", not " + std::to_string(n));
    if (pixels > 0xFFFFFFFFull || (n + BLOCK - 1) / BLOCK > 0x7FFFFFFFull)
        return refuse(ctx, what, "more pixels or entries than 32-bit pixel indices and one launch hold");
    return CRT_OK;
}

static int launch_sample_rays(crt_ctx *ctx, uint32_t gi_seed, uint32_t sample, const uint32_t *d_pixels, uint64_t n, crt_ray *d_rays, uint32_t *d_keys,
                              hipStream_t stream) {
    SampleRaysArgs P{};
    P.cam = ctx->camera();
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
    if (!d_rays) return refuse(ctx, what, "d_rays is NULL");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return launch_sample_rays(ctx, gi_seed, sample, d_pixels, n, d_rays, d_keys, (hipStream_t)stream);
}

extern "C" int crt_accumulate_samples_device(crt_ctx *ctx, const float *d_rgb, const uint32_t *d_pixels, uint64_t n, uint32_t sample, float *d_sum,
                                             float *d_mean, void *stream) {
    const char *what = "crt_accumulate_samples_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = progressive_check(ctx, what, d_pixels, n)) return rc;
    if (n == 0) return CRT_OK;
    if (!d_rgb || !d_sum) return refuse(ctx, what, "d_rgb or d_sum is NULL");
    if (sample == 0xFFFFFFFFu) return refuse(ctx, what, "sample + 1 does not fit 32 bits");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return launch_accumulate(ctx, d_rgb, d_pixels, n, sample, d_sum, d_mean, (hipStream_t)stream);
}

extern "C" uint32_t crt_progressive_samples(const crt_ctx *ctx) { return ctx && ctx->giframe ? ctx->giframe->samples : 0u; }
extern "C" uint64_t crt_progressive_active(const crt_ctx *ctx) { return ctx && ctx->giframe && ctx->giframe->samples ? ctx->giframe->active : 0ull; }

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
    return why ? refuse(ctx, what, why) : (int)CRT_OK;
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
    if (n > 0xFFFFFFFFull) return refuse(ctx, what, "the next list's length is one 32-bit word: n = " + std::to_string(n) + " > 2^32 - 1");
    if (!d_next_n) return refuse(ctx, what, "d_next_n is NULL");
    if (n != 0) {
        if (!d_rgb || !d_sum || !d_sq || !d_counts || !d_next_pixels || !d_work)
            return refuse(ctx, what, "d_rgb, d_sum, d_sq, d_counts, d_next_pixels or d_work is NULL");
        if (d_next_pixels == d_pixels) return refuse(ctx, what, "d_next_pixels must not alias d_pixels");
        if ((uintptr_t)d_work % alignof(unsigned long long)) return refuse(ctx, what, "d_work must be aligned to 8 bytes");
        if (sample == 0xFFFFFFFFu) return refuse(ctx, what, "sample + 1 does not fit 32 bits");
    }
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (n == 0) {   // no entry: the next list is empty, and nothing else is written
        CRT_HIP_CHECK(ctx, hipMemsetAsync(d_next_n, 0, sizeof(uint32_t), (hipStream_t)stream));
        return CRT_OK;
    }
    return launch_adaptive(ctx, d_rgb, d_pixels, n, sample, adaptive, d_sum, d_sq, d_mean, d_counts, d_next_pixels, d_next_n, d_work, (hipStream_t)stream);
}

static bool same_adaptive(const crt_adaptive &a, const crt_adaptive &b) {
    return a.min_samples == b.min_samples && a.max_samples == b.max_samples && a.threshold == b.threshold && a.floor == b.floor;
}

// The sample passes of a frame of `kind`: crt_render_progressive (FRAME_UNIFORM: `adaptive` is null, every pass shoots every pixel and
// folds it with progressive_accumulate, nothing is read back), crt_render_adaptive and crt_render_adaptive_split (the pixel list, the
// adaptive step and its four-byte read-back; split: the split shoot and, behind a pass's step, split_fold on the same list and sample).
static int render_samples(crt_ctx *ctx, const char *what, const FrameKind kind, const crt_options *options, const crt_adaptive *adaptive, uint32_t first,
                          uint32_t n_passes, float *out_rgb, uint32_t *out_counts) {
    if (!ctx) return CRT_ERR_INVALID;
    if (n_passes == 0) return CRT_OK;
    const bool uniform = kind == FRAME_UNIFORM, split = kind == FRAME_ADAPTIVE_SPLIT;
    const std::string arg = uniform ? "first_sample" : "first_pass", unit = uniform ? "samples" : "passes";
    // the GI radiance calls' own check: the camera's rays are PRIMARY rays, the arrays are the context's
    uint64_t pass = 0;
    int rc;
    if ((rc = query_gi_check(ctx, what, options, &pass)) || (!uniform && (rc = adaptive_check(ctx, what, adaptive)))) return rc;
    crt_giframe_state *f = ctx->giframe;
    switch (frame_continues(f ? f->kind : FRAME_NONE, f ? f->samples : 0u, first, kind, uniform || (f && same_adaptive(*adaptive, f->adaptive)))) {
        case CONTINUE_OK: break;
        case CONTINUE_WRONG_COUNT:
            return refuse(ctx, what, arg + " is " + std::to_string(first) + ", but the context's frame holds " + std::to_string(crt_progressive_samples(ctx)) + " " +
                                         unit + " (crt_progressive_samples; 0 starts a new frame)");
        case CONTINUE_IS_ADAPTIVE:
            return refuse(ctx, what, "the frame under way is an ADAPTIVE frame (crt_render_adaptive continues it; first_sample 0 starts a new frame)");
        case CONTINUE_IS_UNIFORM:
            return refuse(ctx, what, "the frame under way is a UNIFORM progressive frame (crt_render_progressive continues it; first_pass 0 starts a new frame)");
        case CONTINUE_IS_UNSPLIT:
            return refuse(ctx, what, "the frame under way is an UNSPLIT adaptive frame (crt_render_adaptive continues it; first_pass 0 starts a new frame)");
        case CONTINUE_IS_SPLIT:
            return refuse(ctx, what, "the frame under way is a SPLIT adaptive frame (crt_render_adaptive_split continues it; first_pass 0 starts a new frame)");
        case CONTINUE_SETTINGS_DIFFER: return refuse(ctx, what, "adaptive differs from the settings latched by the frame's pass 0");
    }
    if ((uint64_t)first + n_passes > 0xFFFFFFFFull) return refuse(ctx, what, "more than 2^32 - 1 " + unit);
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    if (pixels == 0) return CRT_OK;
    if ((rc = progressive_check(ctx, what, nullptr, pixels)) || (rc = giframe_begin(ctx, CALL_RADIANCE))) return rc;
    f = ctx->giframe;
    if ((rc = reserve_all(ctx, f->prog_sum, 3 * pixels, f->prog_rgb, 3 * pixels, f->prog_rays, pixels, f->prog_keys, pixels)) ||
        (!uniform && (rc = reserve_all(ctx, f->prog_sq, pixels, f->prog_counts, pixels, f->prog_list[0], pixels, f->prog_list[1], pixels, f->prog_next_n, 1,
                                       f->prog_work, (crt_adaptive_work_bytes(pixels) + 7) / 8))) ||
        (!uniform && (rc = pin_reserve(ctx, f->pin_next_n))) ||
        (split && (rc = reserve_all(ctx, f->split_direct, 3 * pixels, f->split_dsum, 3 * pixels, f->split_rsum, 3 * pixels, f->split_rsq, pixels))))
        return rc;
    for (uint32_t s = first; s - first < n_passes; s++) {   // one at a time and in order: the fold's order is the frame's
        if (s == 0) {   // a new frame: the post-processing calls trace its guides again
            query_level_peaks_reset(ctx);
            f->kind = kind;
            f->new_frame();
            if (!uniform) f->adaptive = *adaptive;
            f->reflection_bias = options->reflection_bias;
            f->refraction_bias = options->refraction_bias;
            f->active = pixels;   // (a uniform frame shoots every pixel in every pass)
        }
        const uint64_t n = f->active;
        if (n != 0) {   // (an empty list launches nothing: every pixel has stopped, or reached max_samples)
            const uint32_t *list = uniform || s == 0 ? nullptr : f->prog_list[f->cur].p;   // pass 0: every pixel
            if ((rc = launch_sample_rays(ctx, options->gi_seed, s, list, n, f->prog_rays.p, f->prog_keys.p, ctx->stream)) ||
                (rc = query_gi_run(ctx, f->prog_rays.p, f->prog_keys.p, n, options, f->prog_rgb.p, split ? f->split_direct.p : nullptr, pass, ctx->stream)))
                return rc;
            if (uniform) {
                if ((rc = launch_accumulate(ctx, f->prog_rgb.p, nullptr, n, s, f->prog_sum.p, ctx->d_frame, ctx->stream))) return rc;
            } else {
                uint32_t *next = f->prog_list[s == 0 ? 0 : f->cur ^ 1].p;
                if ((rc = launch_adaptive(ctx, f->prog_rgb.p, list, n, s, adaptive, f->prog_sum.p, f->prog_sq.p, ctx->d_frame, f->prog_counts.p, next,
                                          f->prog_next_n.p, f->prog_work.p, ctx->stream)) ||
                    (split && (rc = split_launch_fold(ctx, f->prog_rgb.p, f->split_direct.p, list, n, s, f->split_dsum.p, f->split_rsum.p, f->split_rsq.p,
                                                      ctx->stream))))
                    return rc;
                // the next list's length: 4 bytes through pinned memory, once a pass
                CRT_HIP_CHECK(ctx, hipMemcpyAsync(f->pin_next_n, f->prog_next_n.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
                CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
                f->active = *f->pin_next_n;
                f->cur = s == 0 ? 0 : f->cur ^ 1;
            }
        }
        f->samples = s + 1;
        if (s == 0 && (rc = query_level_headroom(ctx, options, std::min(pixels, pass)))) return rc;
    }
    if (out_rgb) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb, ctx->d_frame, 3 * pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (out_counts) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_counts, f->prog_counts.p, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return CRT_OK;
}

extern "C" int crt_render_progressive(crt_ctx *ctx, const crt_options *options, uint32_t first_sample, uint32_t n_samples, float *out_rgb) {
    return render_samples(ctx, "crt_render_progressive", FRAME_UNIFORM, options, nullptr, first_sample, n_samples, out_rgb, nullptr);
}

extern "C" int crt_render_adaptive(crt_ctx *ctx, const crt_options *options, const crt_adaptive *adaptive, uint32_t first_pass, uint32_t n_passes,
                                   float *out_rgb, uint32_t *out_counts) {
    return render_samples(ctx, "crt_render_adaptive", FRAME_ADAPTIVE, options, adaptive, first_pass, n_passes, out_rgb, out_counts);
}

extern "C" int crt_render_adaptive_split(crt_ctx *ctx, const crt_options *options, const crt_adaptive *adaptive, uint32_t first_pass, uint32_t n_passes,
                                         float *out_rgb, uint32_t *out_counts) {
    return render_samples(ctx, "crt_render_adaptive_split", FRAME_ADAPTIVE_SPLIT, options, adaptive, first_pass, n_passes, out_rgb, out_counts);
}

extern "C" int crt_read_split_state(crt_ctx *ctx, float *out_dsum, float *out_rsum, float *out_rsq) {
    const char *what = "crt_read_split_state";
    if (!ctx) return CRT_ERR_INVALID;
    const crt_giframe_state *f = ctx->giframe;
    if (!f || f->samples == 0 || f->kind != FRAME_ADAPTIVE_SPLIT)
        return refuse(ctx, what, "no split adaptive frame is under way (crt_render_adaptive_split starts one; crt_set_camera and crt_render* end it)");
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (out_dsum) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_dsum, f->split_dsum.p, 3 * pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (out_rsum) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rsum, f->split_rsum.p, 3 * pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (out_rsq) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rsq, f->split_rsq.p, pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return CRT_OK;
}

// ---- post-processing: denoising (crt_denoise.hip, csrc/denoise_rule.h) and temporal accumulation (crt_temporal.hip,
// csrc/temporal_rule.h) of the adaptive frame under way or finished, into buffers of their own.  Nothing of the frame changes: the
// persistent colour buffer, sum, sq, counts, the lists and crt_progressive_samples are only read, so the frame can be post-processed after
// any pass and continued.

// what the post-processing calls ask of the context's frame
static int adaptive_frame_check(crt_ctx *ctx, const char *what, const bool split) {
    const FrameKind kind = ctx->giframe ? ctx->giframe->kind : FRAME_NONE;
    if (kind == FRAME_NONE || ctx->giframe->samples == 0)
        return refuse(ctx, what, "no adaptive frame is under way (crt_render_adaptive starts one; crt_set_camera and crt_render* end it)");
    if (kind == FRAME_UNIFORM)
        return refuse(ctx, what, "the frame under way is a UNIFORM progressive frame, which keeps no second moment (sq): use crt_render_adaptive "
                                 "with min_samples = max_samples");
    if (split && kind != FRAME_ADAPTIVE_SPLIT)
        return refuse(ctx, what, "the frame under way is an UNSPLIT adaptive frame, which keeps no direct part: crt_render_adaptive_split makes a split one");
    if ((uint64_t)ctx->width * ctx->height >= CRT_MAX_PIXELS) return refuse(ctx, what, "width * height >= 2^31");
    return CRT_OK;
}

// the frame's guides, traced at the frame's first post-processing call: the first hits of the camera's centre rays, as CRT_RAY_PRIMARY
// (the rays of a pass are scratch between passes); den_hits is reserved
// crt_set_guide_bounces > 0: and, behind them, the chain guides of the same rays, for the spatial filter alone (the temporal stage keeps the
// first hits: with a still camera "as if painted" is exact).  The biases are those of the frame's pass 0
static int frame_guides(crt_ctx *ctx, const uint64_t pixels) {
    crt_giframe_state *f = ctx->giframe;
    if (f->guides) return CRT_OK;
    int rc;
    if ((rc = crt_camera_rays_device(ctx, f->prog_rays.p, ctx->stream)) ||
        (rc = query_closest_run(ctx, f->prog_rays.p, pixels, CRT_RAY_PRIMARY, f->den_hits.p, ctx->stream)))
        return rc;
    if (ctx->guide_bounces) {
        const char *what = "crt_set_guide_bounces";
        if ((rc = guide_check(ctx, what, pixels, ctx->guide_bounces)) ||
            (rc = reserve_all(ctx, f->den_chain, pixels, f->guide_work, float4s(crt_guide_work_bytes(pixels)))) ||
            (rc = guide_enqueue(ctx, f->prog_rays.p, pixels, CRT_RAY_PRIMARY, f->reflection_bias, f->refraction_bias, ctx->guide_bounces, f->den_chain.p,
                                nullptr, nullptr, f->guide_work.p, ctx->stream, what)))
            return rc;
    }
    f->guides = true;
    return CRT_OK;
}
// the guides of the spatial filter stage
static const crt_hit *filter_guides(const crt_ctx *ctx) { return ctx->guide_bounces ? ctx->giframe->den_chain.p : ctx->giframe->den_hits.p; }

extern "C" int crt_set_guide_bounces(crt_ctx *ctx, uint32_t max_bounces) {
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = guide_check(ctx, "crt_set_guide_bounces", 0, max_bounces)) return rc;
    if (max_bounces == ctx->guide_bounces) return CRT_OK;
    ctx->guide_bounces = max_bounces;
    if (ctx->giframe) ctx->giframe->guides = false;   // the kept guides alone: the histories and the frame's serial stay
    return CRT_OK;
}
extern "C" uint32_t crt_guide_bounces(const crt_ctx *ctx) { return ctx ? ctx->guide_bounces : 0u; }

// the setting alone: the guides, the histories and the frame's serial stay
extern "C" int crt_set_variance_estimate(crt_ctx *ctx, const crt_variance_estimate *est) {
    if (!ctx) return CRT_ERR_INVALID;
    if (!est) {
        if (ctx->giframe) ctx->giframe->estimate_on = false;
        return CRT_OK;
    }
    int rc;
    if ((rc = variance_check(ctx, "crt_set_variance_estimate", est)) || (rc = giframe_state(ctx))) return rc;
    ctx->giframe->estimate = *est;
    ctx->giframe->estimate_on = true;
    return CRT_OK;
}
extern "C" int crt_get_variance_estimate(const crt_ctx *ctx, crt_variance_estimate *out) {
    const bool on = ctx && ctx->giframe && ctx->giframe->estimate_on;
    if (on && out) *out = ctx->giframe->estimate;
    return on ? 1 : 0;
}

// What the denoised and -- `accumulated` -- the accumulated calls do before their own launches: the settings' checks (the accumulated
// call's filter is optional), the frame's, the call bracket, room for what the call writes, the guides.
static int post_begin(crt_ctx *ctx, const char *what, const bool split, const bool accumulated, const crt_temporal *temporal, const crt_denoise *denoise) {
    if (!ctx) return CRT_ERR_INVALID;
    int rc;
    if ((accumulated && (rc = temporal_check(ctx, what, temporal))) || ((denoise || !accumulated) && (rc = denoise_check(ctx, what, denoise))) ||
        (rc = adaptive_frame_check(ctx, what, split)) || (rc = giframe_begin(ctx, CALL_QUERY)))
        return rc;
    crt_giframe_state *f = ctx->giframe;
    History &hist = f->hist[split ? 1 : 0];
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    if ((rc = reserve_all(ctx, f->den_hits, pixels, f->den_q8, 3 * pixels)) ||
        (rc = accumulated ? reserve_all(ctx, hist.slot[0], pixels, hist.slot[1], pixels, f->acc_rgb, 3 * pixels, f->acc_var, pixels, f->acc_valid, pixels)
                          : reserve_all(ctx, f->den_mean, 3 * pixels, f->den_var, pixels)) ||
        (!accumulated && f->estimate_on && (rc = reserve_all(ctx, f->est_records, pixels))) ||
        (denoise && (rc = reserve_all(ctx, f->den_out, 3 * pixels, f->den_work, float4s(crt_denoise_work_bytes(ctx->width, ctx->height))))))
        return rc;
    return frame_guides(ctx, pixels);
}

// ... and behind them: `result` is the filtered frame -- split: the filtered rest, to which the direct part's mean is added back in
// place --; copied out as floats and quantised, with the accumulated call's valid-tap counts, and waited for.
static int post_output(crt_ctx *ctx, const bool split, float *result, float *out_rgb, uint8_t *out_rgb8, uint8_t *out_valid) {
    crt_giframe_state *f = ctx->giframe;
    const uint64_t pixels = (uint64_t)ctx->width * ctx->height;
    int rc;
    if (split && (rc = split_launch_recombine(ctx, result, f->split_dsum.p, f->prog_counts.p, pixels, result, ctx->stream))) return rc;
    if (out_rgb) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb, result, 3 * pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (out_rgb8) {
        if ((rc = crt_quantize_device(ctx, result, 3 * pixels, f->den_q8.p, ctx->stream))) return rc;
        CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_rgb8, f->den_q8.p, 3 * pixels, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (out_valid) CRT_HIP_CHECK(ctx, hipMemcpyAsync(out_valid, f->acc_valid.p, pixels, hipMemcpyDeviceToHost, ctx->stream));
    CRT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return CRT_OK;
}

// the fold's state the two calls filter: the whole colour's, or -- `split` -- the rest's (csrc/split_rule.h)
struct FoldState { const float *sum, *sq; };
static FoldState fold_state(const crt_giframe_state *f, const bool split) {
    return split ? FoldState{f->split_rsum.p, f->split_rsq.p} : FoldState{f->prog_sum.p, f->prog_sq.p};
}

// crt_set_variance_estimate: one launch between the stage that produces colour and variance and the a-trous filter, under the filter's
// guides; the variance is replaced in place, the colour is not touched
static int estimate_stage(crt_ctx *ctx, const crt_history_pixel *d_moments, float *d_var) {
    return variance_launch(ctx, &ctx->giframe->estimate, ctx->width, ctx->height, d_moments, filter_guides(ctx), d_var, d_var, ctx->stream);
}

// crt_render_denoised and, `split`, crt_render_denoised_split: the rest is filtered and the direct part's mean added back untouched
static int render_denoised(crt_ctx *ctx, const char *what, const bool split, const crt_denoise *denoise, float *out_rgb, uint8_t *out_rgb8) {
    int rc;
    if ((rc = post_begin(ctx, what, split, false, nullptr, denoise))) return rc;
    crt_giframe_state *f = ctx->giframe;
    const FoldState state = fold_state(f, split);
    if (f->estimate_on) {
        // the call has no records: the temporal launch with no history writes {G, C_c, q_c, n_c} into scratch records -- no history ledger,
        // slot or frame count is involved --, and its colour and variance are crt_sample_variance_device's, bit for bit (temporal_rule.h)
        crt_temporal none;
        crt_temporal_defaults(&none);
        if ((rc = temporal_launch(ctx, &none, ctx->width, ctx->height, nullptr, nullptr, state.sum, state.sq, f->prog_counts.p, f->den_hits.p,
                                  f->est_records.p, f->den_mean.p, f->den_var.p, nullptr, ctx->stream)) ||
            (rc = estimate_stage(ctx, f->est_records.p, f->den_var.p)))
            return rc;
    } else if ((rc = denoise_launch_variance(ctx, state.sum, state.sq, f->prog_counts.p, (uint64_t)ctx->width * ctx->height, f->den_mean.p, f->den_var.p,
                                             ctx->stream)))
        return rc;
    if ((rc = denoise_launch(ctx, denoise, ctx->width, ctx->height, f->den_mean.p, f->den_var.p, filter_guides(ctx), f->den_out.p, nullptr, f->den_work.p,
                             ctx->stream)))
        return rc;
    return post_output(ctx, split, f->den_out.p, out_rgb, out_rgb8, nullptr);
}

extern "C" int crt_render_denoised(crt_ctx *ctx, const crt_denoise *denoise, float *out_rgb, uint8_t *out_rgb8) {
    return render_denoised(ctx, "crt_render_denoised", false, denoise, out_rgb, out_rgb8);
}

extern "C" int crt_render_denoised_split(crt_ctx *ctx, const crt_denoise *denoise, float *out_rgb, uint8_t *out_rgb8) {
    return render_denoised(ctx, "crt_render_denoised_split", true, denoise, out_rgb, out_rgb8);
}

// crt_render_accumulated and, `split`, crt_render_accumulated_split: the history pair hist[split] holds the moments of what the call
// merges -- whole colours, or the rest --, and the direct part's mean is this frame's own, added back behind the optional filter
static int render_accumulated(crt_ctx *ctx, const char *what, const bool split, const crt_temporal *temporal, const crt_denoise *denoise, float *out_rgb,
                              uint8_t *out_rgb8, uint8_t *out_valid) {
    int rc;
    if ((rc = post_begin(ctx, what, split, true, temporal, denoise))) return rc;
    crt_giframe_state *f = ctx->giframe;
    History &hist = f->hist[split ? 1 : 0];
    hist.begin(f->serial);
    const int cur = hist.cur;
    const FoldState state = fold_state(f, split);
    if ((rc = temporal_launch(ctx, temporal, ctx->width, ctx->height, &hist.pose[cur ^ 1], hist.has_prev ? hist.slot[cur ^ 1].p : nullptr, state.sum,
                              state.sq, f->prog_counts.p, f->den_hits.p, hist.slot[cur].p, f->acc_rgb.p, f->acc_var.p, f->acc_valid.p, ctx->stream)))
        return rc;
    hist.wrote(f->serial);
    memcpy(hist.pose[cur].position, ctx->frame.cam_pos, sizeof(hist.pose[cur].position));
    memcpy(hist.pose[cur].matrix, ctx->frame.cam, sizeof(hist.pose[cur].matrix));
    float *result = f->acc_rgb.p;
    if (denoise) {   // (without a spatial stage there is nothing the estimate would serve)
        if (f->estimate_on && (rc = estimate_stage(ctx, hist.slot[cur].p, f->acc_var.p))) return rc;
        if ((rc = denoise_launch(ctx, denoise, ctx->width, ctx->height, f->acc_rgb.p, f->acc_var.p, filter_guides(ctx), f->den_out.p, nullptr, f->den_work.p,
                                 ctx->stream)))
            return rc;
        result = f->den_out.p;
    }
    return post_output(ctx, split, result, out_rgb, out_rgb8, out_valid);
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
    if (crt_giframe_state *f = ctx->giframe) {
        f->hist[0].reset();
        f->hist[1].reset();
    }
    return CRT_OK;
}

extern "C" uint32_t crt_history_frames(const crt_ctx *ctx) { return ctx && ctx->giframe ? ctx->giframe->hist[0].frames : 0u; }
extern "C" uint32_t crt_history_frames_split(const crt_ctx *ctx) { return ctx && ctx->giframe ? ctx->giframe->hist[1].frames : 0u; }
