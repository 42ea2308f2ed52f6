// crt_split.hip -- the split GI frames' primitives (include/crt_hip.h: "Split GI frames"): crt_split_fold_device and
// crt_split_recombine_device, and the three launches for the radiance passes of crt_query.hip and the frame calls of crt_giframe.hip, which owns the frame's
// state.  Kernels: csrc/kernel_split.h; the rule: csrc/split_rule.h.  Everything here only enqueues: one launch, no wait, no allocation,
// no readback.
#include "crt_internal.h"

namespace {
#include "kernel_split.h"
}  // namespace

static uint32_t split_blocks(const uint64_t n) { return (uint32_t)((n + BLOCK - 1) / BLOCK); }

// level 0 of a GI radiance pass, behind its lighting launches: n > 0 rays, no array NULL
int split_launch_keep_direct(crt_ctx *ctx, const uint8_t *d_status, const float *d_rgb, uint32_t n, uint32_t gi_sample_size, float *d_direct,
                             hipStream_t stream) {
    const KeepDirectArgs P{d_status, d_rgb, d_direct, n, gi_sample_size};
    hipLaunchKernelGGL(radiance_keep_direct, dim3(split_blocks(n)), dim3(BLOCK), 0, stream, P);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

// n > 0 entries that progressive_check has seen, no array NULL but d_pixels
int split_launch_fold(crt_ctx *ctx, const float *d_rgb, const float *d_direct, const uint32_t *d_pixels, uint64_t n, uint32_t sample, float *d_dsum,
                      float *d_rsum, float *d_rsq, hipStream_t stream) {
    SplitFoldArgs P{};
    P.rgb = d_rgb; P.direct = d_direct; P.pixels = d_pixels; P.n = n; P.frame_pixels = (uint64_t)ctx->width * ctx->height; P.sample = sample;
    P.dsum = d_dsum; P.rsum = d_rsum; P.rsq = d_rsq;
    hipLaunchKernelGGL(split_fold, dim3(split_blocks(n)), dim3(BLOCK), 0, stream, P);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

// 0 < n_pixels, one launch's worth of blocks, no array NULL
int split_launch_recombine(crt_ctx *ctx, const float *d_filtered, const float *d_dsum, const uint32_t *d_counts, uint64_t n_pixels, float *d_out,
                           hipStream_t stream) {
    const SplitRecombineArgs P{d_filtered, d_dsum, d_counts, n_pixels, d_out};
    hipLaunchKernelGGL(split_recombine, dim3(split_blocks(n_pixels)), dim3(BLOCK), 0, stream, P);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

extern "C" int crt_split_fold_device(crt_ctx *ctx, const float *d_rgb, const float *d_direct, const uint32_t *d_pixels, uint64_t n, uint32_t sample,
                                     float *d_dsum, float *d_rsum, float *d_rsq, void *stream) {
    const char *what = "crt_split_fold_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = progressive_check(ctx, what, d_pixels, n)) return rc;
    if (n == 0) return CRT_OK;
    if (!d_rgb || !d_direct || !d_dsum || !d_rsum || !d_rsq) return refuse(ctx, what, "d_rgb, d_direct, d_dsum, d_rsum or d_rsq is NULL");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return split_launch_fold(ctx, d_rgb, d_direct, d_pixels, n, sample, d_dsum, d_rsum, d_rsq, (hipStream_t)stream);
}

extern "C" int crt_split_recombine_device(crt_ctx *ctx, const float *d_filtered, const float *d_dsum, const uint32_t *d_counts, uint64_t n_pixels,
                                          float *d_out, void *stream) {
    const char *what = "crt_split_recombine_device";
    if (!ctx) return CRT_ERR_INVALID;
    if ((n_pixels + BLOCK - 1) / BLOCK > 0x7FFFFFFFull) return refuse(ctx, what, "more pixels than one launch holds");
    if (n_pixels == 0) return CRT_OK;
    if (!d_filtered || !d_dsum || !d_counts || !d_out) return refuse(ctx, what, "d_filtered, d_dsum, d_counts or d_out is NULL");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return split_launch_recombine(ctx, d_filtered, d_dsum, d_counts, n_pixels, d_out, (hipStream_t)stream);
}
