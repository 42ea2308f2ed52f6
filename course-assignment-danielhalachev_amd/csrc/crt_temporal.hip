// crt_temporal.hip -- the temporal accumulation's primitive (include/crt_hip.h: "Temporal accumulation"): crt_temporal_defaults and
// crt_temporal_device, and its launch for crt_render_accumulated (crt_giframe.hip, which owns the frame's state and the history).  Kernel:
// csrc/kernel_temporal.h; the rule: csrc/temporal_rule.h.  The device call only enqueues: one launch, no wait, no allocation, no readback.
#include "crt_internal.h"

namespace {
#include "kernel_temporal.h"
}  // namespace

static_assert(sizeof(crt_temporal) == 16, "include/crt_hip.h says 16");
// crt_history_pixel and the rules' record, for this file and for crt_variance.hip, which reads the same record
static_assert(sizeof(crt_history_pixel) == 64 && sizeof(crt_history_record) == 64 && alignof(crt_history_record) == 16, "one record, two names");
static_assert(offsetof(crt_history_pixel, t) == offsetof(crt_history_record, g.t) && offsetof(crt_history_pixel, x) == offsetof(crt_history_record, g.x) &&
                  offsetof(crt_history_pixel, mesh) == offsetof(crt_history_record, g.mesh) && offsetof(crt_history_pixel, c) == offsetof(crt_history_record, c) &&
                  offsetof(crt_history_pixel, m2) == offsetof(crt_history_record, m2) && offsetof(crt_history_pixel, weight) == offsetof(crt_history_record, weight),
              "crt_history_pixel is the rule's record");
static_assert(sizeof(crt_camera_pose) == sizeof(crt_temporal_pose), "crt_camera_pose is the rule's pose");

extern "C" void crt_temporal_defaults(crt_temporal *t) {
    if (!t) return;
    t->size = (uint32_t)sizeof(crt_temporal);
    t->max_history = 64.0f;
    t->normal_min = 0.9f;
    t->sigma_plane = 0.02f;
}

int temporal_check(crt_ctx *ctx, const char *what, const crt_temporal *t) {
    const char *why = nullptr;
    if (!t) why = "temporal is NULL";
    else if (t->size != sizeof(crt_temporal)) why = "temporal->size is not sizeof(crt_temporal)";
    else if (!(t->max_history > 0.0f) || !std::isfinite(t->max_history)) why = "max_history is not finite or not above 0";
    else if (!std::isfinite(t->normal_min)) why = "normal_min is not finite";
    else if (!(t->sigma_plane >= 0.0f) || !std::isfinite(t->sigma_plane)) why = "sigma_plane is negative or not finite";
    return why ? refuse(ctx, what, why) : (int)CRT_OK;
}

// one launch; 0 < width * height < 2^31, `t` checked, no array NULL but d_prev (prev_pose is then not read), d_out_var and d_out_valid
int temporal_launch(crt_ctx *ctx, const crt_temporal *t, uint32_t width, uint32_t height, const crt_camera_pose *prev_pose, const crt_history_pixel *d_prev,
                    const float *d_sum, const float *d_sq, const uint32_t *d_counts, const crt_hit *d_hits, crt_history_pixel *d_next, float *d_out_rgb,
                    float *d_out_var, uint8_t *d_out_valid, hipStream_t stream) {
    TemporalArgs A{};
    A.rule = crt_temporal_rule{t->max_history, t->normal_min, t->sigma_plane};
    if (d_prev) {
        memcpy(A.pose.o, prev_pose->position, sizeof(A.pose.o));
        memcpy(A.pose.m, prev_pose->matrix, sizeof(A.pose.m));
    }
    A.width = (int32_t)width; A.height = (int32_t)height;
    A.tiles_x = tiles_x_of(width);
    A.prev = (const crt_history_record *)d_prev;
    A.sum = d_sum; A.sq = d_sq; A.count = d_counts; A.hits = d_hits;
    A.next = (crt_history_record *)d_next;
    A.out_rgb = d_out_rgb; A.out_var = d_out_var; A.out_valid = d_out_valid;
    const uint32_t tiles_y = tiles_y_of(height);
    hipLaunchKernelGGL(temporal_reproject, dim3(A.tiles_x * tiles_y), dim3(TILE_X, TILE_Y), 0, stream, A);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

extern "C" int crt_temporal_device(crt_ctx *ctx, const crt_temporal *temporal, uint32_t width, uint32_t height, const crt_camera_pose *prev_pose,
                                   const crt_history_pixel *d_prev, const float *d_sum, const float *d_sq, const uint32_t *d_counts, const crt_hit *d_hits,
                                   crt_history_pixel *d_next, float *d_out_rgb, float *d_out_var, uint8_t *d_out_valid, void *stream) {
    const char *what = "crt_temporal_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = temporal_check(ctx, what, temporal)) return rc;
    const uint64_t n = (uint64_t)width * height;
    if (int rc = pixels_check(ctx, what, n)) return rc;
    if (!d_sum || !d_sq || !d_counts || !d_hits || !d_next || !d_out_rgb) return refuse(ctx, what, "d_sum, d_sq, d_counts, d_hits, d_next or d_out_rgb is NULL");
    if (d_prev && !prev_pose) return refuse(ctx, what, "d_prev is given without prev_pose");
    if (d_next == d_prev) return refuse(ctx, what, "d_next must not be d_prev");
    if ((uintptr_t)d_next % 16u || (uintptr_t)d_prev % 16u) return refuse(ctx, what, "d_next and d_prev must be aligned to 16 bytes");
    if (n == 0) return CRT_OK;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return temporal_launch(ctx, temporal, width, height, prev_pose, d_prev, d_sum, d_sq, d_counts, d_hits, d_next, d_out_rgb, d_out_var, d_out_valid,
                           (hipStream_t)stream);
}
