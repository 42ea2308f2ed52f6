// crt_variance.hip -- the variance estimate's primitive (include/crt_hip.h: "Variance estimate"): crt_variance_estimate_defaults and
// crt_variance_estimate_device, and its launch for the frame calls' setting crt_set_variance_estimate (crt_giframe.hip, which owns the
// frame's state).  Kernel: csrc/kernel_variance.h; the rule: csrc/variance_rule.h.  The device call only enqueues: one launch, no wait, no
// allocation, no readback.
#include "crt_internal.h"

namespace {
#include "kernel_variance.h"
}  // namespace

static_assert(sizeof(crt_variance_estimate) == 16, "include/crt_hip.h says 16");
static_assert(sizeof(crt_variance_tap_geometry) == 16 && sizeof(crt_variance_tap_place) == 16 && sizeof(crt_variance_tap_moments) == 16,
              "a tap is three 16-byte vectors");
static_assert(3 * VARIANCE_HALO * 16 == 25536, "the LDS tile DESIGN.md 8o describes");

extern "C" void crt_variance_estimate_defaults(crt_variance_estimate *e) {
    if (!e) return;
    e->size = (uint32_t)sizeof(crt_variance_estimate);
    e->min_history = 4.0f;
    e->normal_squarings = 5;
    e->sigma_plane = 0.02f;
}

int variance_check(crt_ctx *ctx, const char *what, const crt_variance_estimate *e) {
    const char *why = nullptr;
    if (!e) why = "estimate is NULL";
    else if (e->size != sizeof(crt_variance_estimate)) why = "estimate->size is not sizeof(crt_variance_estimate)";
    else if (!(e->min_history > 0.0f) || !std::isfinite(e->min_history)) why = "min_history is not finite or not above 0";
    else if (e->normal_squarings > 16u) why = "normal_squarings > 16";
    else if (!(e->sigma_plane >= 0.0f) || !std::isfinite(e->sigma_plane)) why = "sigma_plane is negative or not finite";
    return why ? refuse(ctx, what, why) : (int)CRT_OK;
}

// one launch; 0 < width * height < 2^31, `e` checked, no array NULL, d_moments aligned to 16 bytes
int variance_launch(crt_ctx *ctx, const crt_variance_estimate *e, uint32_t width, uint32_t height, const crt_history_pixel *d_moments, const crt_hit *d_hits,
                    const float *d_var, float *d_out_var, hipStream_t stream) {
    VarianceArgs A{};
    A.rule = crt_variance_rule{e->min_history, e->normal_squarings, e->sigma_plane};
    A.width = (int32_t)width; A.height = (int32_t)height;
    A.tiles_x = tiles_x_of(width);
    A.moments = (const crt_history_record *)d_moments;
    A.hits = d_hits;
    A.var = d_var;
    A.out_var = d_out_var;
    const uint32_t tiles_y = tiles_y_of(height);
    hipLaunchKernelGGL(variance_estimate, dim3(A.tiles_x * tiles_y), dim3(TILE_X, TILE_Y), 0, stream, A);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

extern "C" int crt_variance_estimate_device(crt_ctx *ctx, const crt_variance_estimate *est, uint32_t width, uint32_t height,
                                            const crt_history_pixel *d_moments, const crt_hit *d_hits, const float *d_var, float *d_out_var, void *stream) {
    const char *what = "crt_variance_estimate_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = variance_check(ctx, what, est)) return rc;
    const uint64_t n = (uint64_t)width * height;
    if (int rc = pixels_check(ctx, what, n)) return rc;
    if (!d_moments || !d_hits || !d_var || !d_out_var) return refuse(ctx, what, "d_moments, d_hits, d_var or d_out_var is NULL");
    if ((uintptr_t)d_moments % 16u) return refuse(ctx, what, "d_moments must be aligned to 16 bytes");
    if (n == 0) return CRT_OK;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return variance_launch(ctx, est, width, height, d_moments, d_hits, d_var, d_out_var, (hipStream_t)stream);
}
