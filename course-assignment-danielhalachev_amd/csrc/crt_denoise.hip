// crt_denoise.hip -- the denoiser's primitives (include/crt_hip.h: "Denoising"): crt_denoise_defaults, crt_denoise_work_bytes,
// crt_sample_variance_device and crt_denoise_device, and their launches for crt_render_denoised (crt_giframe.hip, which owns the frame's
// state).  Kernels: csrc/kernel_denoise.h; the rule: csrc/denoise_rule.h.  Both device calls only enqueue: no wait, no allocation, no
// readback.
#include "crt_internal.h"

namespace {
#include "kernel_denoise.h"
}  // namespace

static_assert(sizeof(crt_denoise) == 24, "include/crt_hip.h says 24");
static_assert(sizeof(crt_guide) == 32 && sizeof(crt_denoise_pixel) == 16 && sizeof(crt_hit) == 48, "the records of the work area");
// the work area: the guides, then the two {r, g, b, V} buffers
constexpr uint64_t DENOISE_WORK_PER_PIXEL = sizeof(crt_guide) + 2 * sizeof(crt_denoise_pixel);

extern "C" void crt_denoise_defaults(crt_denoise *d) {
    if (!d) return;
    d->size = (uint32_t)sizeof(crt_denoise);
    d->iterations = 4;
    d->normal_squarings = 5;
    d->sigma_colour = 2.0f;
    d->sigma_plane = 0.02f;
    d->floor = 1e-6f;
}

extern "C" size_t crt_denoise_work_bytes(uint32_t width, uint32_t height) { return (size_t)((uint64_t)width * height * DENOISE_WORK_PER_PIXEL); }

int denoise_check(crt_ctx *ctx, const char *what, const crt_denoise *d) {
    const char *why = nullptr;
    if (!d) why = "denoise is NULL";
    else if (d->size != sizeof(crt_denoise)) why = "denoise->size is not sizeof(crt_denoise)";
    else if (d->iterations > 8u) why = "iterations > 8";
    else if (d->normal_squarings > 16u) why = "normal_squarings > 16";
    else if (!(d->sigma_colour >= 0.0f) || !std::isfinite(d->sigma_colour)) why = "sigma_colour is negative or not finite";
    else if (!(d->sigma_plane >= 0.0f) || !std::isfinite(d->sigma_plane)) why = "sigma_plane is negative or not finite";
    else if (!(d->floor > 0.0f) || !std::isfinite(d->floor)) why = "floor is not finite or not above 0";
    return why ? refuse(ctx, what, why) : (int)CRT_OK;
}

int denoise_launch_variance(crt_ctx *ctx, const float *d_sum, const float *d_sq, const uint32_t *d_counts, uint64_t n, float *d_mean, float *d_var,
                            hipStream_t stream) {
    const DenoiseVarianceArgs P{d_sum, d_sq, d_counts, n, d_mean, d_var};
    hipLaunchKernelGGL(denoise_variance, dim3((uint32_t)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, P);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    return CRT_OK;
}

// pack, then the iterations; 0 < width * height < 2^31, `d` checked, no array NULL but d_out_var
int denoise_launch(crt_ctx *ctx, const crt_denoise *d, uint32_t width, uint32_t height, const float *d_rgb, const float *d_var, const crt_hit *d_hits,
                   float *d_out_rgb, float *d_out_var, void *d_work, hipStream_t stream) {
    const uint64_t n = (uint64_t)width * height;
    if (d->iterations == 0u) {   // a copy
        if (d_out_rgb != d_rgb) CRT_HIP_CHECK(ctx, hipMemcpyAsync(d_out_rgb, d_rgb, 3 * n * sizeof(float), hipMemcpyDeviceToDevice, stream));
        if (d_out_var && d_out_var != d_var) CRT_HIP_CHECK(ctx, hipMemcpyAsync(d_out_var, d_var, n * sizeof(float), hipMemcpyDeviceToDevice, stream));
        return CRT_OK;
    }
    crt_guide *guides = (crt_guide *)d_work;
    crt_denoise_pixel *buf[2];
    buf[0] = (crt_denoise_pixel *)(guides + n);
    buf[1] = buf[0] + n;
    const DenoisePackArgs K{d_rgb, d_var, d_hits, n, guides, buf[0]};
    hipLaunchKernelGGL(denoise_pack, dim3((uint32_t)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, K);
    CRT_HIP_CHECK(ctx, hipGetLastError());
    DenoiseAtrousArgs A{};
    A.rule = crt_denoise_rule{d->normal_squarings, d->sigma_colour, d->sigma_plane, d->floor};
    A.width = (int32_t)width; A.height = (int32_t)height;
    A.tiles_x = tiles_x_of(width);
    A.guides = guides;
    const uint32_t tiles_y = tiles_y_of(height);
    for (uint32_t k = 0; k < d->iterations; k++) {
        const bool last = k + 1 == d->iterations;
        A.step = (int32_t)(1u << k);
        A.in = buf[k & 1u];
        A.out = last ? nullptr : buf[(k & 1u) ^ 1u];
        A.out_rgb = last ? d_out_rgb : nullptr;
        A.out_var = last ? d_out_var : nullptr;
        hipLaunchKernelGGL(denoise_atrous, dim3(A.tiles_x * tiles_y), dim3(TILE_X, TILE_Y), 0, stream, A);
        CRT_HIP_CHECK(ctx, hipGetLastError());
    }
    return CRT_OK;
}

extern "C" int crt_sample_variance_device(crt_ctx *ctx, const float *d_sum, const float *d_sq, const uint32_t *d_counts, uint64_t n_pixels,
                                          float *d_mean, float *d_var, void *stream) {
    const char *what = "crt_sample_variance_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (n_pixels == 0) return CRT_OK;
    if (!d_sum || !d_sq || !d_counts || !d_mean || !d_var) return refuse(ctx, what, "d_sum, d_sq, d_counts, d_mean or d_var is NULL");
    if ((n_pixels + BLOCK - 1) / BLOCK > 0x7FFFFFFFull) return refuse(ctx, what, "more pixels than one launch holds");
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return denoise_launch_variance(ctx, d_sum, d_sq, d_counts, n_pixels, d_mean, d_var, (hipStream_t)stream);
}

extern "C" int crt_denoise_device(crt_ctx *ctx, const crt_denoise *denoise, uint32_t width, uint32_t height, const float *d_rgb, const float *d_var,
                                  const crt_hit *d_hits, float *d_out_rgb, float *d_out_var, void *d_work, void *stream) {
    const char *what = "crt_denoise_device";
    if (!ctx) return CRT_ERR_INVALID;
    if (int rc = denoise_check(ctx, what, denoise)) return rc;
    const uint64_t n = (uint64_t)width * height;
    if (int rc = pixels_check(ctx, what, n)) return rc;
    if (!d_rgb || !d_var || !d_hits || !d_out_rgb || !d_work) return refuse(ctx, what, "d_rgb, d_var, d_hits, d_out_rgb or d_work is NULL");
    if ((uintptr_t)d_work % 16u) return refuse(ctx, what, "d_work must be aligned to 16 bytes");
    if (n == 0) return CRT_OK;
    CRT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return denoise_launch(ctx, denoise, width, height, d_rgb, d_var, d_hits, d_out_rgb, d_out_var, d_work, (hipStream_t)stream);
}
