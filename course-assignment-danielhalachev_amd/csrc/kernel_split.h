// kernel_split.h -- the three kernels of the split GI frames (include/crt_hip.h: crt_shoot_rays_gi_split*, crt_split_fold_device,
// crt_split_recombine_device, crt_render_*_split); the rule, one header for host and device: csrc/split_rule.h.
//   radiance_keep_direct  one thread a ray of LEVEL 0 of a GI radiance pass, behind that level's lighting launches and before anything
//                         overwrites the level's colours: 1 + 12 bytes in, 12 out;
//   split_fold            one thread a list entry: 24 bytes in, 28 bytes of the pixel's state read (sample > 0) and written;
//   split_recombine       one thread a pixel: 28 bytes in, 12 out.
// All three are elementwise: no LDS, no atomics, plain vector stores; 64-bit indices are formed from unmasked 32-bit values (as
// kernel_progressive.h does).  A list's pixel index is compared with the frame before any address is formed from it.
#pragma once

#include "split_rule.h"

static_assert(CRT_SPLIT_BACKGROUND == (uint32_t)CRT_SHADE_BACKGROUND && CRT_SPLIT_DIFFUSE == (uint32_t)CRT_SHADE_DIFFUSE, "the rule's two statuses");

struct KeepDirectArgs {
    const uint8_t *status;    // level 0's CRT_SHADE_*
    const float *rgb;         // level 0's colours as the lighting launches left them, 3 floats a ray
    float *direct;            // 3 floats a ray
    uint32_t n, gi_samples;
};
__global__ __launch_bounds__(BLOCK) void radiance_keep_direct(const KeepDirectArgs P) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= P.n) return;
    const float *c = P.rgb + 3 * r;
    const float L[3] = {c[0], c[1], c[2]};
    float d[3];
    crt_split_direct((uint32_t)P.status[r], L, P.gi_samples, d);
    float *o = P.direct + 3 * r;
    o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
}

// The pixels of one launch must be distinct (two threads of one pixel would race), as progressive_accumulate's.
struct SplitFoldArgs {
    const float *rgb, *direct;   // 3 floats an entry each
    const uint32_t *pixels;      // or null: pixel i
    uint64_t n, frame_pixels;
    uint32_t sample;
    float *dsum, *rsum, *rsq;
};
__global__ __launch_bounds__(BLOCK) void split_fold(const SplitFoldArgs P) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t p = P.pixels ? P.pixels[i] : (uint32_t)i;
    if ((uint64_t)p >= P.frame_pixels) return;
    const float *c = P.rgb + 3 * i, *d = P.direct + 3 * i;
    const float rgb[3] = {c[0], c[1], c[2]}, direct[3] = {d[0], d[1], d[2]};
    float *ds = P.dsum + 3 * (uint64_t)p, *rs = P.rsum + 3 * (uint64_t)p;
    float dsum[3] = {0.0f, 0.0f, 0.0f}, rsum[3] = {0.0f, 0.0f, 0.0f}, rsq = 0.0f;
    if (P.sample != 0u) {   // (sample 0 reads nothing of the state)
        dsum[0] = ds[0]; dsum[1] = ds[1]; dsum[2] = ds[2];
        rsum[0] = rs[0]; rsum[1] = rs[1]; rsum[2] = rs[2];
        rsq = P.rsq[p];
    }
    crt_split_fold(P.sample, rgb, direct, dsum, rsum, &rsq);
    ds[0] = dsum[0]; ds[1] = dsum[1]; ds[2] = dsum[2];
    rs[0] = rsum[0]; rs[1] = rsum[1]; rs[2] = rsum[2];
    P.rsq[p] = rsq;
}

struct SplitRecombineArgs {
    const float *filtered, *dsum;   // 3 floats a pixel each
    const uint32_t *count;
    uint64_t n;
    float *out;                     // may be `filtered`: a thread reads its three floats before it writes them
};
__global__ __launch_bounds__(BLOCK) void split_recombine(const SplitRecombineArgs P) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const float *f = P.filtered + 3 * i, *d = P.dsum + 3 * i;
    const float filtered[3] = {f[0], f[1], f[2]}, dsum[3] = {d[0], d[1], d[2]};
    float out[3];
    crt_split_recombine(P.count[i], filtered, dsum, out);
    float *o = P.out + 3 * i;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
}
