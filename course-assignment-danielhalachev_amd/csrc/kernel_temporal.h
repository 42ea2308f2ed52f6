// kernel_temporal.h -- the kernel of the GI frames' temporal accumulation (include/crt_hip.h: crt_temporal_device,
// crt_render_accumulated); the rule, one header for host and device: csrc/temporal_rule.h.
//   temporal_reproject  one thread per pixel, a workgroup covers a TEMPORAL_TILE_X x TEMPORAL_TILE_Y tile of the image: the pixel's crt_hit
//                       (48 bytes) and fold state (sum[3], sq, count) are read once, the first hit is projected into the previous pose --
//                       which travels in the kernel arguments --, up to four 64-byte history records are read, and one 64-byte record,
//                       three floats of colour, the variance and the valid-tap count are written.
// Memory.  A record is 64 bytes, aligned 16: a tap is four 16-byte loads from one half of a 128-byte line.  The reads of a wave are the
// bilinear footprints of two rows of 32 neighbouring pixels: for a camera that moved little they cover about two rows of 33 records, and
// the four taps of neighbouring pixels share their corners, which meet in L2 (and in the vector L1 within a wave).  The record a pixel
// writes is a whole half line; a row of 32 pixels writes 2048 contiguous bytes.
// Divergence.  The branches are per pixel: miss pixels and pixels that project outside the previous frame skip the taps; within a tile these
// are runs along silhouettes and frame edges, so most waves take one side.  The tap loop has a fixed trip count of four and each test is a
// skip, so a wave executes the loads of a tap while any of its lanes still wants it.
// Tap coordinates are signed 32-bit and are compared with the frame before any address is formed (crt_temporal_pixel).  64-bit indices are
// formed from unmasked 32-bit values (kernel_progressive.h says why).  All stores are plain vector stores; no atomics, no LDS.
#pragma once

#include "temporal_rule.h"

constexpr uint32_t TEMPORAL_TILE_X = 32, TEMPORAL_TILE_Y = 8;
static_assert(TEMPORAL_TILE_X * TEMPORAL_TILE_Y == BLOCK, "one thread per pixel of a tile");

struct TemporalArgs {
    crt_temporal_rule rule;
    crt_temporal_pose pose;          // the previous frame's camera (not read when prev is null)
    int32_t width, height;
    uint32_t tiles_x;                // ceil(width / TEMPORAL_TILE_X)
    const crt_temporal_record *prev; // or null: no history
    const float *sum, *sq;
    const uint32_t *count;
    const crt_hit *hits;
    crt_temporal_record *next;
    float *out_rgb, *out_var;        // out_var: or null
    uint8_t *out_valid;              // or null
};
// The grid is one-dimensional, tiles row-major, as denoise_atrous's: fewer than 2^29 workgroups for width * height < 2^31.
__global__ __launch_bounds__(BLOCK) void temporal_reproject(const TemporalArgs P) {
    const uint32_t tx = blockIdx.x % P.tiles_x, ty = blockIdx.x / P.tiles_x;
    const uint32_t ux = tx * TEMPORAL_TILE_X + threadIdx.x, uy = ty * TEMPORAL_TILE_Y + threadIdx.y;
    if (ux >= (uint32_t)P.width || uy >= (uint32_t)P.height) return;
    const uint64_t i = (uint64_t)uy * (uint32_t)P.width + ux;
    const crt_hit h = P.hits[i];
    const crt_denoise_guide g = crt_denoise_guide_of(h.t, h.point, h.normal, h.mesh, h.hit);
    const float *s = P.sum + 3 * i;
    const float total[3] = {s[0], s[1], s[2]};
    const crt_temporal_out r = crt_temporal_pixel(P.rule, P.width, P.height, g, total, P.sq[i], P.count[i], P.pose, P.prev);
    P.next[i] = r.r;
    float *o = P.out_rgb + 3 * i;
    o[0] = r.r.c[0]; o[1] = r.r.c[1]; o[2] = r.r.c[2];
    if (P.out_var) P.out_var[i] = r.v;
    if (P.out_valid) P.out_valid[i] = (uint8_t)r.valid;
}
