// shoot_caps.h -- crt_shoot_rays*_enqueue (include/crt_hip.h): the arithmetic of a call whose levels' sizes stay on the device -- what
// each level may hold, and which rays of a level one launch of its chunk loop has.  Plain C++ without a HIP type in it: crt_query.hip
// and the kernels (kernel_query.h) use it, and a host program can compile it alone.
#pragma once

#include <algorithm>
#include <cstdint>

#ifdef __HIPCC__
#define SHOOT_HD __host__ __device__
#else
#define SHOOT_HD
#endif

constexpr int SHOOT_LEVELS = 64;                       // MAX_GENERATIONS (kernel_common.h)
constexpr uint64_t SHOOT_LEVEL_RAYS = 1ull << 30;      // what a level may hold at most: indices and counts stay inside 31 bits
constexpr uint64_t SHOOT_ENQUEUE_RAYS = 1ull << 22;    // the caller's rays of one enqueue call: one pass (SHOOT_PASS_RAYS)

// Rays [first, first + n) of a level are one launch's; the level holds `count` (a 32-bit word that radiance_scatter's atomics added to,
// so it may exceed every capacity).  The launch's rays: clamp(count - first, 0, n), in 64 bits from the unmasked words.
SHOOT_HD inline uint32_t shoot_part_count(const uint32_t count, const uint32_t first, const uint32_t n) {
    const int64_t left = (int64_t)(uint64_t)count - (int64_t)(uint64_t)first;
    return (uint32_t)(left < 0 ? 0 : (left < (int64_t)(uint64_t)n ? left : (int64_t)(uint64_t)n));
}

// cap[g], g = 0 .. 63: the rays level g of a call of n rays may hold.  cap[0] = n; for 1 <= g <= max_depth
//   min(want[g], fan * cap[g - 1], 2^30)      (fan * cap[g - 1] <= fan^g n: a level has at most fan children for each ray above it)
// with want = level_cap, or `have` (what the context's arrays hold) when level_cap is null; 0 beyond max_depth.  A level that spawns
// holds at most (2^32 - 1) / fan rays, so that the 32-bit count of its children cannot wrap (fan = 2: no bound at all below 2^30).
// Once a level has no room, none below it has.  n <= SHOOT_ENQUEUE_RAYS, 2 <= fan <= 64, max_depth < 64.
inline void shoot_level_caps(const uint64_t n, const uint64_t fan, const uint32_t max_depth, const uint32_t *level_cap, const uint64_t *have,
                             uint32_t cap[SHOOT_LEVELS]) {
    const uint64_t spawning = 0xFFFFFFFFull / fan;
    cap[0] = (uint32_t)n;
    for (uint32_t g = 1; g < (uint32_t)SHOOT_LEVELS; g++) {
        uint64_t c = 0;
        if (g <= max_depth) {
            const uint64_t want = level_cap ? (uint64_t)level_cap[g] : have[g];
            c = std::min(std::min(want, fan * (uint64_t)cap[g - 1]), SHOOT_LEVEL_RAYS);
            if (g < max_depth) c = std::min(c, spawning);
        }
        cap[g] = (uint32_t)c;
    }
}
