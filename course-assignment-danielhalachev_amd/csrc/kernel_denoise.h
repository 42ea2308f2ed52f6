// kernel_denoise.h -- the three kernels of the GI frames' denoiser (include/crt_hip.h: crt_sample_variance_device, crt_denoise_device,
// crt_render_denoised); the rule, one header for host and device: csrc/denoise_rule.h.
//   denoise_variance  one thread per pixel: the fold's state (sum[3], sq, count) -> the mean and the variance of the mean
//   denoise_pack      one thread per pixel: the caller's crt_hit (48 bytes) -> a 32-byte guide record {nx, ny, nz, t, px, py, pz, mesh}, and
//                     colour + variance -> one 16-byte {r, g, b, V}; both into the work area, so that a tap of the filter is three 16-byte
//                     loads from aligned records, and so that the caller's output may be its input (everything is copied first)
//   denoise_atrous    one thread per pixel, a workgroup covers a TILE_X x TILE_Y tile of the image (kernel_tile.h): one iteration of the
//                     rule, every tap from global memory or L2.  The {r, g, b, V} buffers ping-pong between the iterations, the guides are
//                     read-only; the last iteration writes the caller's layout: 3 floats a pixel, and the variance apart.
// Every tap coordinate is computed in signed 32-bit arithmetic and checked against the frame before any address is formed
// (crt_denoise_atrous compares the OFFSET with the room the centre has, so not even the sum overflows).  64-bit indices are formed from
// unmasked 32-bit values (kernel_progressive.h says why).  All stores are plain vector stores.
// A wave is two rows of 32 pixels: 512 contiguous bytes of {r, g, b, V} a row, four whole 128-byte lines, and 1024 bytes of guides.
// No LDS: at step 1 and 2 a tile's halo would fit (a 40 x 16 tile of 48-byte records is 30 KB), from step 4 on it exceeds the tile; the taps of
// neighbouring pixels meet in L2 instead.
#pragma once

#include "denoise_rule.h"
#include "kernel_tile.h"

struct DenoiseVarianceArgs {
    const float *sum, *sq;
    const uint32_t *count;
    uint64_t n;
    float *mean, *var;
};
__global__ __launch_bounds__(BLOCK) void denoise_variance(const DenoiseVarianceArgs P) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const float *s = P.sum + 3 * i;
    const float total[3] = {s[0], s[1], s[2]};
    const crt_denoise_pixel p = crt_denoise_variance(total, P.sq[i], P.count[i]);
    float *m = P.mean + 3 * i;
    m[0] = p.c[0]; m[1] = p.c[1]; m[2] = p.c[2];
    P.var[i] = p.v;
}

struct DenoisePackArgs {
    const float *rgb, *var;
    const crt_hit *hits;
    uint64_t n;
    crt_guide *guides;
    crt_denoise_pixel *pixels;
};
__global__ __launch_bounds__(BLOCK) void denoise_pack(const DenoisePackArgs P) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    P.guides[i] = guide_of_hit(P.hits[i]);
    const float *c = P.rgb + 3 * i;
    crt_denoise_pixel p;
    p.c[0] = c[0]; p.c[1] = c[1]; p.c[2] = c[2];
    p.v = P.var[i];
    P.pixels[i] = p;
}

struct DenoiseAtrousArgs {
    crt_denoise_rule rule;
    int32_t width, height, step;
    uint32_t tiles_x;         // ceil(width / TILE_X)
    const crt_denoise_pixel *in;
    const crt_guide *guides;
    crt_denoise_pixel *out;   // an iteration that is not the last: the other {r, g, b, V} buffer; the last one: null
    float *out_rgb, *out_var; // the last iteration: the caller's arrays (out_var: or null)
};
__global__ __launch_bounds__(BLOCK) void denoise_atrous(const DenoiseAtrousArgs P) {
    const TilePixel t = tile_pixel(P.tiles_x, P.width, P.height);
    if (!t.inside) return;
    const crt_denoise_pixel r = crt_denoise_atrous(P.rule, P.width, P.height, P.step, (int32_t)t.uy, (int32_t)t.ux, P.in, P.guides);
    const uint64_t i = tile_index(t, P.width);
    if (P.out) {
        P.out[i] = r;
        return;
    }
    float *o = P.out_rgb + 3 * i;
    o[0] = r.c[0]; o[1] = r.c[1]; o[2] = r.c[2];
    if (P.out_var) P.out_var[i] = r.v;
}
