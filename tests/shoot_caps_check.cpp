// A stand-alone host program around csrc/shoot_caps.h, the arithmetic of crt_shoot_rays*_enqueue: the levels' capacities and the rays
// of one launch of a level's chunk loop; and around csrc/call_wait.h, the rule by which a call first waits for the one still under
// way.  tests/test_shoot_enqueue_host.py compiles it with the host sanitizers and runs it; it prints "ok <cases>" and returns 0, or
// says which property failed.
//   shoot_caps_check --layout   prints sizeof(crt_shoot_report) and its fields' offsets, from the header
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "call_wait.h"
#include "crt_hip.h"
#include "shoot_caps.h"

static unsigned long long cases = 0;
#define REQUIRE(c)                                                         \
    do {                                                                   \
        cases++;                                                           \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

// a level of `count` appended rays and capacity `cap`, launched `part` rays at a time: the launches cover [0, min(count, cap)) once
static int check_parts(const uint32_t count, const uint64_t cap, const uint64_t part) {
    std::vector<uint8_t> seen(cap > (1u << 16) ? 0 : cap, 0);   // (large levels: sums only)
    uint64_t total = 0;
    for (uint64_t done = 0; done < cap; done += part) {
        const uint32_t n = (uint32_t)std::min(cap - done, part);
        const uint32_t m = shoot_part_count(count, (uint32_t)done, n);
        REQUIRE(m <= n && done + m <= cap);
        REQUIRE(m == 0 || done + m <= count);
        REQUIRE(m == n || done + m == std::min<uint64_t>(count, cap) || m == 0);
        for (uint32_t i = 0; i < m && !seen.empty(); i++) {
            REQUIRE(seen[done + i] == 0);   // (inside the vector: AddressSanitizer watches the index)
            seen[done + i] = 1;
        }
        total += m;
    }
    REQUIRE(total == std::min<uint64_t>(count, cap));
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--layout")) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(crt_shoot_report), offsetof(crt_shoot_report, levels), offsetof(crt_shoot_report, overflow),
               offsetof(crt_shoot_report, dropped), offsetof(crt_shoot_report, level_rays), offsetof(crt_shoot_report, hits),
               offsetof(crt_shoot_report, shadow_records), offsetof(crt_shoot_report, rerouted));
        return 0;
    }
    // the rays of a launch: clamp(count - first, 0, n), with words near 2^32
    REQUIRE(shoot_part_count(0, 0, 64) == 0);
    REQUIRE(shoot_part_count(10, 0, 64) == 10);
    REQUIRE(shoot_part_count(64, 0, 64) == 64);
    REQUIRE(shoot_part_count(65, 0, 64) == 64);
    REQUIRE(shoot_part_count(65, 64, 64) == 1);
    REQUIRE(shoot_part_count(65, 128, 64) == 0);
    REQUIRE(shoot_part_count(0xFFFFFFFFu, 0, 1u << 30) == 1u << 30);
    REQUIRE(shoot_part_count(0xFFFFFFFFu, 0xFFFFFF00u, 1u << 30) == 0xFFu);
    REQUIRE(shoot_part_count(0x80000001u, 0x80000000u, 7) == 1);
    REQUIRE(shoot_part_count(5, 0xFFFFFFFFu, 7) == 0);
    const uint32_t counts[] = {0, 1, 63, 64, 65, 255, 256, 257, 1000, 4096, 70000, 0x7FFFFFFFu, 0xFFFFFFFFu};
    const uint64_t caps[] = {0, 1, 64, 65, 256, 600, 4096, 65536, 1ull << 30};
    const uint64_t parts[] = {64, 100, 256, 4096, 1ull << 27};
    for (uint32_t count : counts)
        for (uint64_t cap : caps)
            for (uint64_t part : parts)
                if (cap / part <= 4096 && check_parts(count, cap, part)) return 1;
    // the capacities
    uint32_t cap[SHOOT_LEVELS];
    uint64_t have[SHOOT_LEVELS];
    uint32_t asked[SHOOT_LEVELS];
    const uint64_t ns[] = {1, 63, 4096, SHOOT_ENQUEUE_RAYS};
    const uint64_t fans[] = {2, 3, 16, 64};
    const uint32_t depths[] = {0, 1, 2, 5, 8, 63};
    const uint64_t rooms[] = {0, 64, 5000, 1ull << 31, ~0ull};
    for (uint64_t n : ns)
        for (uint64_t fan : fans)
            for (uint32_t depth : depths)
                for (uint64_t room : rooms)
                    for (int explicit_caps = 0; explicit_caps < 2; explicit_caps++) {
                        for (int g = 0; g < SHOOT_LEVELS; g++) {
                            have[g] = g % 3 == 2 ? room / 2 : room;
                            asked[g] = (uint32_t)std::min<uint64_t>(have[g], 0xFFFFFFFFu);
                        }
                        shoot_level_caps(n, fan, depth, explicit_caps ? asked : nullptr, have, cap);
                        REQUIRE(cap[0] == n);
                        uint64_t worst = n;   // fan^g n, saturated
                        for (uint32_t g = 1; g < (uint32_t)SHOOT_LEVELS; g++) {
                            worst = std::min(worst * fan, SHOOT_LEVEL_RAYS);
                            if (g > depth) { REQUIRE(cap[g] == 0); continue; }
                            REQUIRE(cap[g] <= worst && cap[g] <= SHOOT_LEVEL_RAYS && cap[g] <= fan * (uint64_t)cap[g - 1]);
                            REQUIRE(cap[g] <= (explicit_caps ? (uint64_t)asked[g] : have[g]));
                            REQUIRE(g == depth || fan * (uint64_t)cap[g] <= 0xFFFFFFFFull);   // the children's 32-bit count cannot wrap
                            REQUIRE(cap[g - 1] != 0 || cap[g] == 0);
                            // nothing but the documented bounds makes it smaller
                            const uint64_t want = std::min(std::min(explicit_caps ? (uint64_t)asked[g] : have[g], fan * (uint64_t)cap[g - 1]), SHOOT_LEVEL_RAYS);
                            REQUIRE(cap[g] == (g < depth ? std::min<uint64_t>(want, 0xFFFFFFFFull / fan) : want));
                        }
                    }
    // the waiting rule, all 36 cases written out: [a call is open][its kind][the new call's kind][0: another stream, 1: the same].
    // No open call: no wait.  Otherwise a wait, but for a query behind a query and an enqueue call behind an enqueue call on ONE stream.
    static const bool waits[2][3][3][2] = {
        {{{false, false}, {false, false}, {false, false}}, {{false, false}, {false, false}, {false, false}}, {{false, false}, {false, false}, {false, false}}},
        {/* open: a query     */ {/* query */ {true, false}, /* radiance */ {true, true}, /* enqueue */ {true, true}},
         /* open: a radiance  */ {/* query */ {true, true}, /* radiance */ {true, true}, /* enqueue */ {true, true}},
         /* open: an enqueue  */ {/* query */ {true, true}, /* radiance */ {true, true}, /* enqueue */ {true, false}}}};
    const CallKind kinds[3] = {CALL_QUERY, CALL_RADIANCE, CALL_ENQUEUE};
    for (int open = 0; open < 2; open++)
        for (int was = 0; was < 3; was++)
            for (int next = 0; next < 3; next++)
                for (int same = 0; same < 2; same++) REQUIRE(call_waits(open != 0, kinds[was], kinds[next], same != 0) == waits[open][was][next][same]);
    printf("ok %llu\n", cases);
    return 0;
}
