// kernel_tile.h -- what the three tiled stage kernels share (kernel_denoise.h: denoise_atrous, kernel_temporal.h: temporal_reproject,
// kernel_variance.h: variance_estimate): one thread per pixel, a workgroup of TILE_X x TILE_Y threads covers a tile of the image.  A wave is
// two rows of 32 pixels.  The grid is one-dimensional, tiles row-major (a grid's second dimension holds 65535 workgroups, an image may be
// higher than that): at most (width / 32 + 1) * (height / 8 + 1) < 2^29 workgroups for width * height < 2^31.
#pragma once

#include "../../include/crt_hip.h"   // crt_hit
#include "filter_rule.h"
#include "kernel_common.h"           // BLOCK

constexpr uint32_t TILE_X = 32, TILE_Y = 8;
static_assert(TILE_X * TILE_Y == BLOCK, "one thread per pixel of a tile");

// the launch of such a kernel: tiles_x goes into its arguments, dim3(tiles_x * tiles_y) is its grid, dim3(TILE_X, TILE_Y) its block
static inline uint32_t tiles_x_of(const uint32_t width) { return (width + TILE_X - 1) / TILE_X; }
static inline uint32_t tiles_y_of(const uint32_t height) { return (height + TILE_Y - 1) / TILE_Y; }

// a thread's pixel: the tile's origin (ox, oy), which is inside the frame, the pixel (ux, uy) and whether it is inside the frame
struct TilePixel {
    uint32_t ox, oy, ux, uy;
    bool inside;
};
__device__ __forceinline__ TilePixel tile_pixel(const uint32_t tiles_x, const int32_t width, const int32_t height) {
    TilePixel p;
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    p.ox = tx * TILE_X; p.oy = ty * TILE_Y;
    p.ux = p.ox + threadIdx.x; p.uy = p.oy + threadIdx.y;
    p.inside = p.ux < (uint32_t)width && p.uy < (uint32_t)height;
    return p;
}
// its row-major index, formed from unmasked 32-bit values (kernel_progressive.h says why)
__device__ __forceinline__ uint64_t tile_index(const TilePixel p, const int32_t width) { return (uint64_t)p.uy * (uint32_t)width + p.ux; }

// the guide of a crt_hit
__device__ __forceinline__ crt_guide guide_of_hit(const crt_hit h) { return crt_guide_of(h.t, h.point, h.normal, h.mesh, h.hit); }
