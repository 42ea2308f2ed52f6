// call_wait.h -- the waiting rule of crt_query.hip's calls (the prose is above OpenCall there): whether a new call must first harvest
// the call still under way.  Plain C++ without a HIP type in it: a host program can compile it alone (tests/shoot_caps_check.cpp).
#pragma once

// the kinds of call: the ray and lighting queries; the radiance queries that read every level's size back (crt_shoot_rays*,
// crt_shoot_rays_gi*); the radiance queries that only enqueue (crt_shoot_rays*_enqueue)
enum CallKind { CALL_QUERY, CALL_RADIANCE, CALL_ENQUEUE };

// `open`: a call of `open_kind` is under way; `same_stream`: on the stream of the new call, which is of kind `next`
inline bool call_waits(const bool open, const CallKind open_kind, const CallKind next, const bool same_stream) {
    if (!open) return false;
    // an enqueue call behind an enqueue call on its stream is ordered behind it and supersedes its statistics, which come through a
    // report of their own, not through the words
    if (open_kind == CALL_ENQUEUE && next == CALL_ENQUEUE && same_stream) return false;
    // a query behind a query on its stream is ordered behind it and supersedes its statistics; a radiance call's statistics are read
    // through the words the next call clears, and a radiance call clears those of the call before it
    return !same_stream || open_kind != CALL_QUERY || next != CALL_QUERY;
}
