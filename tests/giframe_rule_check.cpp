// A stand-alone host program around csrc/giframe_rule.h, the integer rules of the GI frame calls (csrc/crt_giframe.hip): whether a call
// may continue the frame under way, and the book-keeping of a history pair.  tests/test_giframe_rule_host.py compiles it with the host
// sanitizers and runs it; it prints "ok <cases>" and returns 0, or says which property failed.
#include <cstdio>

#include "giframe_rule.h"

static unsigned long long cases = 0;
#define REQUIRE(c)                                                         \
    do {                                                                   \
        cases++;                                                           \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

// what a call on frame `serial` sees and leaves: begin, (the launch reads `previous`), wrote
struct Seen { bool has_prev; int prev_slot; };
static Seen call(HistoryLedger &h, const uint64_t serial) {
    h.begin(serial);
    const Seen seen{h.has_prev, h.cur ^ 1};
    h.wrote(serial);
    return seen;
}

static bool same(const HistoryLedger &a, const HistoryLedger &b) {
    return a.serial == b.serial && a.cur == b.cur && a.has_cur == b.has_cur && a.has_prev == b.has_prev && a.frames == b.frames;
}

static int check_history() {
    {   // two calls on one frame: counted once, no rotation, the same `previous`
        HistoryLedger h;
        const Seen a = call(h, 7);
        REQUIRE(!a.has_prev && h.frames == 1 && h.cur == 0 && h.has_cur && h.serial == 7);
        const Seen b = call(h, 7);
        REQUIRE(!b.has_prev && b.prev_slot == a.prev_slot && h.frames == 1 && h.cur == 0);
        // a call on the next serial rotates once: what was `current` is `previous`
        const Seen c = call(h, 8);
        REQUIRE(c.has_prev && c.prev_slot == 0 && h.cur == 1 && h.frames == 2 && h.serial == 8);
        const Seen d = call(h, 8);
        REQUIRE(d.has_prev && d.prev_slot == c.prev_slot && h.cur == 1 && h.frames == 2);
        // a serial that advanced several times between calls still rotates once
        const Seen e = call(h, 13);
        REQUIRE(e.has_prev && e.prev_slot == 1 && h.cur == 0 && h.frames == 3 && h.serial == 13);
        // after reset: no `previous`, and the count starts again; the slot in use stays where it was
        h.reset();
        REQUIRE(h.frames == 0 && !h.has_cur && !h.has_prev);
        const Seen f = call(h, 13);
        REQUIRE(!f.has_prev && h.frames == 1 && h.cur == 0);
        const Seen g = call(h, 14);
        REQUIRE(g.has_prev && g.prev_slot == 0 && h.frames == 2);
    }
    {   // a frame that ended before any call wrote `current` rotates nothing
        HistoryLedger h;
        h.begin(3);
        h.begin(4);
        REQUIRE(h.cur == 0 && !h.has_prev && !h.has_cur && h.frames == 0);
    }
    {   // dropping the guides alone (crt_set_guide_bounces) touches no ledger and leaves the serial: the next call is one more on the frame
        HistoryLedger h;
        call(h, 1);
        call(h, 2);
        const HistoryLedger before = h;
        const Seen a = call(h, 2);
        REQUIRE(same(h, before) && a.has_prev && a.prev_slot == 0);
    }
    {   // two ledgers, unsplit and split, driven alternately: each is what it would be alone
        HistoryLedger whole, rest, whole_alone, rest_alone;
        const uint64_t whole_serials[] = {1, 1, 2, 5, 5, 6}, rest_serials[] = {1, 3, 3, 4, 6, 6};
        for (int i = 0; i < 6; i++) {
            const Seen a = call(whole, whole_serials[i]), b = call(rest, rest_serials[i]);
            const Seen a1 = call(whole_alone, whole_serials[i]), b1 = call(rest_alone, rest_serials[i]);
            REQUIRE(same(whole, whole_alone) && same(rest, rest_alone));
            REQUIRE(a.has_prev == a1.has_prev && a.prev_slot == a1.prev_slot && b.has_prev == b1.has_prev && b.prev_slot == b1.prev_slot);
            if (i == 2) rest.reset(), rest_alone.reset();   // (crt_history_reset resets both; here one, to see that the other stays)
        }
        REQUIRE(whole.frames == 4 && rest.frames == 2);
    }
    return 0;
}

int main() {
    // The continuation rule, every case written out: [the kind under way][the kind asked - 1][first: 0, held, held + 1][settings: the
    // same, different].  held is 3, and 0 where no frame is under way.  0 always starts a new frame; a wrong count comes before the kind,
    // the kind before the split, the split before the settings; a uniform call has no settings.
    const FrameContinue OK = CONTINUE_OK, WC = CONTINUE_WRONG_COUNT, IA = CONTINUE_IS_ADAPTIVE, IU = CONTINUE_IS_UNIFORM, IS = CONTINUE_IS_SPLIT,
                        IN = CONTINUE_IS_UNSPLIT, SD = CONTINUE_SETTINGS_DIFFER;
    const FrameContinue expect[4][3][3][2] = {
        /* none           */ {/* uniform  */ {{OK, OK}, {OK, OK}, {WC, WC}},
                              /* adaptive */ {{OK, OK}, {OK, OK}, {WC, WC}},
                              /* split    */ {{OK, OK}, {OK, OK}, {WC, WC}}},
        /* uniform        */ {/* uniform  */ {{OK, OK}, {OK, OK}, {WC, WC}},
                              /* adaptive */ {{OK, OK}, {IU, IU}, {WC, WC}},
                              /* split    */ {{OK, OK}, {IU, IU}, {WC, WC}}},
        /* adaptive       */ {/* uniform  */ {{OK, OK}, {IA, IA}, {WC, WC}},
                              /* adaptive */ {{OK, OK}, {OK, SD}, {WC, WC}},
                              /* split    */ {{OK, OK}, {IN, IN}, {WC, WC}}},
        /* adaptive split */ {/* uniform  */ {{OK, OK}, {IA, IA}, {WC, WC}},
                              /* adaptive */ {{OK, OK}, {IS, IS}, {WC, WC}},
                              /* split    */ {{OK, OK}, {OK, SD}, {WC, WC}}}};
    const FrameKind kinds[4] = {FRAME_NONE, FRAME_UNIFORM, FRAME_ADAPTIVE, FRAME_ADAPTIVE_SPLIT};
    for (int under = 0; under < 4; under++)
        for (int asked = 1; asked < 4; asked++) {
            const uint32_t held = under == 0 ? 0u : 3u;
            const uint32_t firsts[3] = {0u, held, held + 1u};
            for (int f = 0; f < 3; f++)
                for (int differ = 0; differ < 2; differ++)
                    REQUIRE(frame_continues(kinds[under], held, firsts[f], kinds[asked], differ == 0) == expect[under][asked - 1][f][differ]);
        }
    // nothing under way continues nothing, whatever count is left over; the largest counts compare as they are
    REQUIRE(frame_continues(FRAME_NONE, 3, 3, FRAME_UNIFORM, true) == WC);
    REQUIRE(frame_continues(FRAME_UNIFORM, 0xFFFFFFFFu, 0xFFFFFFFFu, FRAME_UNIFORM, true) == OK);
    REQUIRE(frame_continues(FRAME_ADAPTIVE, 0xFFFFFFFFu, 0xFFFFFFFEu, FRAME_ADAPTIVE, true) == WC);
    if (check_history()) return 1;
    printf("ok %llu\n", cases);
    return 0;
}
