// giframe_rule.h -- the rules of crt_giframe.hip's frame calls that are plain integer logic: whether a call may continue the frame under
// way, and the book-keeping of a history pair (crt_render_accumulated*).  Plain C++ without a HIP type in it: a host program can compile
// it alone (tests/giframe_rule_check.cpp).
#pragma once

#include <cstdint>

// the frame under way: none (crt_set_camera and crt_render* end a frame), crt_render_progressive's, crt_render_adaptive's,
// crt_render_adaptive_split's
enum FrameKind { FRAME_NONE, FRAME_UNIFORM, FRAME_ADAPTIVE, FRAME_ADAPTIVE_SPLIT };

// why a call may not continue it, in the order the calls report them
enum FrameContinue { CONTINUE_OK, CONTINUE_WRONG_COUNT, CONTINUE_IS_ADAPTIVE, CONTINUE_IS_UNIFORM, CONTINUE_IS_SPLIT, CONTINUE_IS_UNSPLIT,
                     CONTINUE_SETTINGS_DIFFER };

// A call of kind `asked` (not FRAME_NONE) whose first sample or pass is `first`, while a frame of kind `under_way` holds `held` of them;
// `same_settings`: the call's adaptive settings are those the frame latched (a uniform call has none: true).  0 starts a new frame,
// whatever is held.
inline FrameContinue frame_continues(const FrameKind under_way, const uint32_t held, const uint32_t first, const FrameKind asked, const bool same_settings) {
    if (first == 0) return CONTINUE_OK;
    if (under_way == FRAME_NONE || first != held) return CONTINUE_WRONG_COUNT;
    if (asked == FRAME_UNIFORM) return under_way == FRAME_UNIFORM ? CONTINUE_OK : CONTINUE_IS_ADAPTIVE;
    if (under_way == FRAME_UNIFORM) return CONTINUE_IS_UNIFORM;
    if (under_way != asked) return under_way == FRAME_ADAPTIVE_SPLIT ? CONTINUE_IS_SPLIT : CONTINUE_IS_UNSPLIT;
    return same_settings ? CONTINUE_OK : CONTINUE_SETTINGS_DIFFER;
}

// A history pair without its device arrays: slot[cur] is `current`, slot[cur ^ 1] `previous`; the frame serial `current` was written
// at; the frames merged since reset.  `previous` changes only when a call finds a new frame's serial, so every call on one frame merges
// the same history.
struct HistoryLedger {
    uint64_t serial = 0;
    int cur = 0;
    bool has_cur = false, has_prev = false;
    uint32_t frames = 0;
    // a call begins on frame `s`: `current`, if it is an ended frame's, is the previous history from here on
    void begin(const uint64_t s) {
        if (!has_cur || serial == s) return;
        cur ^= 1;
        has_prev = true;
        has_cur = false;
    }
    // the call wrote `current`: once a frame
    void wrote(const uint64_t s) {
        if (!has_cur) frames++;
        has_cur = true;
        serial = s;
    }
    void reset() { has_cur = has_prev = false; frames = 0; }   // (nothing reads a slot until a call has written one again)
};
