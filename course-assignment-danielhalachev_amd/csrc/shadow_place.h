// shadow_place.h -- where level 0's fixed shadow slots lie (kernel_stream.h has the why), as index arithmetic for both sides: the kernels
// place a pixel's slots with the forward function and find a slot's pixel and light with the inverse; a test hook runs both on the host.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define CRT_PLACE_HD __host__ __device__
#else
#define CRT_PLACE_HD
#endif

constexpr uint32_t LEVEL0_SHADOW_BLOCK = 16;
// Level-0 ray r (pixel r & 63 of item r >> 6, `total` items in all) towards light li owns slot base + li * stride + (r & 63): the items come in
// blocks of LEVEL0_SHADOW_BLOCK, light-major inside a block; the last block is as long as the items left.
CRT_PLACE_HD static inline void level0_slot_place(const uint32_t total, const uint32_t n_lights, const uint32_t r, uint32_t &base, uint32_t &stride) {
    const uint32_t item = r >> 6;
    const uint32_t blk = item / LEVEL0_SHADOW_BLOCK, in = item - blk * LEVEL0_SHADOW_BLOCK;
    const uint32_t left = total - blk * LEVEL0_SHADOW_BLOCK, nb = left < LEVEL0_SHADOW_BLOCK ? left : LEVEL0_SHADOW_BLOCK;
    base = blk * LEVEL0_SHADOW_BLOCK * n_lights * 64u + in * 64u;
    stride = nb * 64u;
}
// The inverse, for a slot below total * 64 * n_lights: slot -> block, light, tile within the block, lane -> the ray and the light.
CRT_PLACE_HD static inline void level0_slot_owner(const uint32_t total, const uint32_t n_lights, const uint32_t slot, uint32_t &r, uint32_t &li) {
    const uint32_t per_block = LEVEL0_SHADOW_BLOCK * n_lights * 64u;
    const uint32_t blk = slot / per_block, within = slot - blk * per_block;
    const uint32_t left = total - blk * LEVEL0_SHADOW_BLOCK, nb = left < LEVEL0_SHADOW_BLOCK ? left : LEVEL0_SHADOW_BLOCK;
    li = within / (nb * 64u);
    const uint32_t rest = within - li * nb * 64u;   // tile within the block * 64 + lane
    r = blk * LEVEL0_SHADOW_BLOCK * 64u + rest;
}
// What the test hook runs (crt_testhooks.hip: crt_test_shadow_place): every slot of `total` items and n_lights lights through the inverse and
// back through the forward placement; the number of slots that do not come back, or whose owner is no ray or light of the frame.
static inline uint64_t level0_slot_mismatches(const uint32_t total, const uint32_t n_lights) {
    uint64_t bad = 0;
    const uint64_t slots = (uint64_t)total * 64u * n_lights;
    for (uint64_t slot = 0; slot < slots; slot++) {
        uint32_t r, li, base, stride;
        level0_slot_owner(total, n_lights, (uint32_t)slot, r, li);
        if (r >= total * 64u || li >= n_lights) { bad++; continue; }
        level0_slot_place(total, n_lights, r, base, stride);
        if ((uint64_t)base + (uint64_t)li * stride + (r & 63u) != slot) bad++;
    }
    return bad;
}
