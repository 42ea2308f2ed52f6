// kernel_progressive.h -- the two kernels of a GI frame rendered sample pass by sample pass (include/crt_hip.h: crt_camera_sample_rays_device,
// crt_accumulate_samples_device, crt_render_progressive).  A frame's rule for a pixel is a left fold (RayTracer.cpp:90-104; oracle/cpu_ref.c:
// render_pixel): sum = 0; sum = sum + c_s for s = 0 .. n - 1, c_s the colour of the ray of sample s under the key mix(mix(seed, p), s);
// pixel = sum * (1 / (float)n).  A left fold can be cut anywhere: progressive_sample_rays makes the rays and keys of ONE sample,
// crt_shoot_rays_gi* shoots them, progressive_accumulate takes the fold one step further and writes the mean it stands for.  Both kernels
// only store plain vector stores; 64-bit indices are formed from unmasked 32-bit values (as kernel_radiance.h does).
#pragma once

#include "gi_random.h"

// RayTracer::getRay (RayTracer.cpp:61-80) for sample `sample` of pixel p = pixels ? pixels[i] : i, one thread per i < n: through the pixel
// centre for sample 0 -- query_camera_rays' expressions, so its bits --, else through (px + u(key, 0), py + u(key, 1)) -- the expressions of
// kernel_lane.h: primary_ray_offset, normalised ONCE, as getRay returns it (crt_shoot_rays_gi* does shootRay's own normalisation on entry).
// A pixel index outside the frame gives a ray with zero direction and key 0, and nothing is read through it.
struct SampleRaysArgs {
    QueryCamera cam;
    uint32_t seed, sample;
    const uint32_t *pixels;   // or null: pixel i
    uint64_t n;
    crt_ray *rays;
    uint32_t *keys;           // or null
};
__global__ __launch_bounds__(BLOCK) void progressive_sample_rays(const SampleRaysArgs P) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const QueryCamera &C = P.cam;
    const uint32_t p = P.pixels ? P.pixels[i] : (uint32_t)i;
    crt_ray q;
    q.origin[0] = C.pos[0]; q.origin[1] = C.pos[1]; q.origin[2] = C.pos[2];
    if ((uint64_t)p >= (uint64_t)C.width * C.height) {
        q.direction[0] = 0.0f; q.direction[1] = 0.0f; q.direction[2] = 0.0f;
        P.rays[i] = q;
        if (P.keys) P.keys[i] = 0u;
        return;
    }
    const uint32_t px = p % C.width, py = p / C.width;
    const uint32_t key = crt_gi_mix(crt_gi_mix(P.seed, p), P.sample);
    const float offx = P.sample == 0u ? 0.5f : crt_gi_uniform(key, 0u);
    const float offy = P.sample == 0u ? 0.5f : crt_gi_uniform(key, 1u);
    float x = (float)px + offx;
    float y = (float)py + offy;
    x = x / (float)C.width;
    y = y / (float)C.height;
    x = (2.0f * x) - 1.0f;
    y = 1.0f - (2.0f * y);
    x = x * ((float)C.width / (float)C.height);
    const float z = -1.0f;
    float dx = x * C.m[0] + y * C.m[3] + z * C.m[6];   // row vector x matrix, Matrix.h:137-142
    float dy = x * C.m[1] + y * C.m[4] + z * C.m[7];
    float dz = x * C.m[2] + y * C.m[5] + z * C.m[8];
    normalize3(dx, dy, dz);
    q.direction[0] = dx; q.direction[1] = dy; q.direction[2] = dz;
    P.rays[i] = q;
    if (P.keys) P.keys[i] = key;
}

// One step of the fold, one thread per i < n, pixel p as above: sum[3p + c] = (sample == 0 ? 0 : sum[3p + c]) + rgb[3i + c], and where a
// mean is wanted mean[3p + c] = sum[3p + c] * (1 / (float)(sample + 1)) -- the frame's `0 + colour` and its one multiplication.  A pixel
// index outside the frame is skipped.  The pixels of one launch must be distinct (two threads of one pixel would race).
struct AccumulateArgs {
    const float *rgb;
    const uint32_t *pixels;   // or null: pixel i
    uint64_t n, frame_pixels;
    uint32_t sample;
    float *sum, *mean;        // mean: or null
};
__global__ __launch_bounds__(BLOCK) void progressive_accumulate(const AccumulateArgs P) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t p = P.pixels ? P.pixels[i] : (uint32_t)i;
    if ((uint64_t)p >= P.frame_pixels) return;
    const float scale = 1.0f / (float)(P.sample + 1u);
    const float *c = P.rgb + 3 * i;
    float *s = P.sum + 3 * (uint64_t)p;
    for (int k = 0; k < 3; k++) {
        const float v = (P.sample == 0u ? 0.0f : s[k]) + c[k];
        s[k] = v;
        if (P.mean) P.mean[3 * (uint64_t)p + k] = v * scale;
    }
}
