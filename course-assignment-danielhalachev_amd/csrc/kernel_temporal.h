// kernel_temporal.h -- the kernel of the GI frames' temporal accumulation (include/crt_hip.h: crt_temporal_device,
// crt_render_accumulated); the rule, one header for host and device: csrc/temporal_rule.h.
//   temporal_reproject  one thread per pixel, a workgroup covers a TILE_X x TILE_Y tile of the image (kernel_tile.h): the pixel's crt_hit
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
#include "kernel_tile.h"

struct TemporalArgs {
    crt_temporal_rule rule;
    crt_temporal_pose pose;          // the previous frame's camera (not read when prev is null)
    int32_t width, height;
    uint32_t tiles_x;                // ceil(width / TILE_X)
    const crt_history_record *prev;  // or null: no history
    const float *sum, *sq;
    const uint32_t *count;
    const crt_hit *hits;
    crt_history_record *next;
    float *out_rgb, *out_var;        // out_var: or null
    uint8_t *out_valid;              // or null
};
__global__ __launch_bounds__(BLOCK) void temporal_reproject(const TemporalArgs P) {
    const TilePixel t = tile_pixel(P.tiles_x, P.width, P.height);
    if (!t.inside) return;
    const uint64_t i = tile_index(t, P.width);
    const crt_guide g = guide_of_hit(P.hits[i]);
    const float *s = P.sum + 3 * i;
    const float total[3] = {s[0], s[1], s[2]};
    const crt_temporal_out r = crt_temporal_pixel(P.rule, P.width, P.height, g, total, P.sq[i], P.count[i], P.pose, P.prev);
    P.next[i] = r.r;
    float *o = P.out_rgb + 3 * i;
    o[0] = r.r.c[0]; o[1] = r.r.c[1]; o[2] = r.r.c[2];
    if (P.out_var) P.out_var[i] = r.v;
    if (P.out_valid) P.out_valid[i] = (uint8_t)r.valid;
}
