// kernel_adaptive.h -- the three kernels of an adaptively sampled GI frame (include/crt_hip.h: crt_adaptive_step_device,
// crt_render_adaptive), beside kernel_progressive.h: adaptive_step takes the fold of the listed pixels one step further as
// progressive_accumulate does, keeps one float and one count more per pixel and asks csrc/adaptive_rule.h whether the pixel goes on;
// adaptive_scan and adaptive_scatter turn the answers into the next pass's pixel list.  The compaction is a three-launch one on one
// stream: every wave's keep mask (a ballot) and every workgroup's count, an exclusive prefix sum over the counts by ONE workgroup, a
// scatter to block offset + waves before + lanes below.  It is stable (the kept entries in the order they had), no atomic decides a
// position, and no workgroup waits, spins or polls for another: the launches' order on the stream is the only ordering.  All stores are
// plain vector stores; 64-bit indices are formed from unmasked 32-bit values (kernel_progressive.h says why): a wave's words go through
// LDS, so that the global index is block x ADAPTIVE_WAVES + threadIdx.x and never a shifted or masked thread index.
// The rgb and sum accesses are three floats at stride 12 per lane, the public layout: a wave's 64 lanes cover 768 contiguous bytes, six
// whole 128-byte lines, so every fetched line is used in full whatever the width of the load the compiler picks.
#pragma once

#include "adaptive_rule.h"

constexpr uint32_t ADAPTIVE_WAVES = BLOCK / 64;   // waves of a workgroup: one 64-bit mask each
static_assert(BLOCK % 64 == 0 && ADAPTIVE_WAVES >= 1 && ADAPTIVE_WAVES <= 64, "a workgroup's waves are scanned by its first lanes");

// the caller's work area for a list of n entries: a mask per wave (every workgroup's ADAPTIVE_WAVES, the last one's idle waves too), then
// a count and an offset per workgroup
struct AdaptiveWork {
    unsigned long long *masks;
    uint32_t *counts, *offsets;
};

struct AdaptiveStepArgs {
    const float *rgb;
    const uint32_t *pixels;   // or null: pixel i
    uint64_t n, frame_pixels;
    uint32_t sample;
    crt_adaptive_rule rule;
    float *sum, *sq, *mean;   // mean: or null
    uint32_t *count;
    AdaptiveWork work;
};
// One thread per list entry i < n (the grid is ceil(n / BLOCK) workgroups; no thread leaves before the ballot and the barrier).  An
// index outside the frame is skipped and not kept.  The pixels of one launch must be distinct.
__global__ __launch_bounds__(BLOCK) void adaptive_step(const AdaptiveStepArgs P) {
    __shared__ unsigned long long wave_mask[ADAPTIVE_WAVES];
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    bool keep = false;
    if (i < P.n) {
        const uint32_t p = P.pixels ? P.pixels[i] : (uint32_t)i;
        if ((uint64_t)p < P.frame_pixels) {
            const float *c = P.rgb + 3 * i;
            float *s = P.sum + 3 * (uint64_t)p;
            float total[3] = {0.0f, 0.0f, 0.0f}, mean[3], sq = 0.0f;
            if (P.sample != 0u) {
                total[0] = s[0]; total[1] = s[1]; total[2] = s[2];
                sq = P.sq[p];
            }
            uint32_t count;
            keep = crt_adaptive_step(P.rule, P.sample, c[0], c[1], c[2], total, &sq, &count, mean);
            s[0] = total[0]; s[1] = total[1]; s[2] = total[2];
            P.sq[p] = sq;
            P.count[p] = count;
            if (P.mean) {
                float *m = P.mean + 3 * (uint64_t)p;
                m[0] = mean[0]; m[1] = mean[1]; m[2] = mean[2];
            }
        }
    }
    const unsigned long long mask = __ballot(keep);
    if ((threadIdx.x & 63u) == 0u) wave_mask[threadIdx.x >> 6] = mask;
    __syncthreads();
    if (threadIdx.x < ADAPTIVE_WAVES) P.work.masks[(uint64_t)blockIdx.x * ADAPTIVE_WAVES + threadIdx.x] = wave_mask[threadIdx.x];
    if (threadIdx.x == 0u) {
        uint32_t kept = 0;
        for (uint32_t w = 0; w < ADAPTIVE_WAVES; w++) kept += (uint32_t)__popcll(wave_mask[w]);
        P.work.counts[blockIdx.x] = kept;
    }
}

// offsets[b] = counts[0] + .. + counts[b - 1] for b < blocks, and *next_n = the total: ONE workgroup, BLOCK counts a turn, with the
// turns' running total carried in a register of every thread (all threads read the same LDS word).  blocks == 0 writes *next_n = 0.
struct AdaptiveScanArgs {
    const uint32_t *counts;
    uint32_t *offsets, *next_n;
    uint32_t blocks;
};
__global__ __launch_bounds__(BLOCK) void adaptive_scan(const AdaptiveScanArgs P) {
    __shared__ uint32_t wave_total[ADAPTIVE_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < P.blocks; base += BLOCK) {   // (uniform: every thread takes every turn, so the barriers are met by all)
        const uint32_t b = base + threadIdx.x;
        const uint32_t own = b < P.blocks ? P.counts[b] : 0u;
        uint32_t incl = own;   // the wave's inclusive sum up to this lane
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63u) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = 0, turn = 0;
        for (uint32_t w = 0; w < ADAPTIVE_WAVES; w++) {
            const uint32_t t = wave_total[w];
            if (w < wave) before += t;
            turn += t;
        }
        if (b < P.blocks) P.offsets[b] = carry + before + (incl - own);
        carry += turn;
        __syncthreads();   // wave_total is written again in the next turn
    }
    if (threadIdx.x == 0u) *P.next_n = carry;
}

// entry i kept -> next[offsets[block] + kept in the block's waves before this one + kept lanes below this one] = its pixel
struct AdaptiveScatterArgs {
    const uint32_t *pixels;   // or null: pixel i
    uint64_t n;
    AdaptiveWork work;
    uint32_t *next;
};
__global__ __launch_bounds__(BLOCK) void adaptive_scatter(const AdaptiveScatterArgs P) {
    __shared__ unsigned long long wave_mask[ADAPTIVE_WAVES];
    if (threadIdx.x < ADAPTIVE_WAVES) wave_mask[threadIdx.x] = P.work.masks[(uint64_t)blockIdx.x * ADAPTIVE_WAVES + threadIdx.x];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long mask = wave_mask[wave];
    if (i >= P.n || !((mask >> lane) & 1ull)) return;
    uint32_t at = P.work.offsets[blockIdx.x];
    for (uint32_t w = 0; w < ADAPTIVE_WAVES; w++)
        if (w < wave) at += (uint32_t)__popcll(wave_mask[w]);
    at += (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    P.next[at] = P.pixels ? P.pixels[i] : (uint32_t)i;
}
