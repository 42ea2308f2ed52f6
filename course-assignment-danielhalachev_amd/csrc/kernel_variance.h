// kernel_variance.h -- the kernel of the GI frames' variance estimate (include/crt_hip.h: crt_variance_estimate_device,
// crt_set_variance_estimate); the rule, one header for host and device: csrc/variance_rule.h.
//   variance_estimate  one thread per pixel, a workgroup covers a TILE_X x TILE_Y tile of the image (kernel_tile.h).
// Tile skip.  Every thread reads its own record (c, m2, weight: 20 of its 64 bytes), crt_hit and V_in and decides whether its pixel is
// flagged (crt_variance_flagged); a thread outside the image is not.  The workgroup agrees on "any flagged" at a barrier that EVERY thread
// reaches.  A tile without a flagged pixel writes V' = V_in and ends: nothing is staged -- the steady state of a still camera with a long
// history.
// Staging.  A tile with a flagged pixel stages its (32 + 6) x (8 + 6) halo into LDS once: the 12 words a tap needs, as three planes of
// 16-byte vectors -- {n, mesh}, {x, weight}, {c, m2} -- of 532 slots each, 25,536 bytes.  Neighbouring lanes read neighbouring 16-byte slots
// of one plane: a ds_read_b128 is served in groups of 16 lanes, whose 16 consecutive slots cover the 64 banks once, so a tap is three
// conflict-free reads (a 48-byte array of structs would put lanes 0, 4, 8, 12 of a group on the same banks).  A halo place outside the frame
// is staged with weight 0 and mesh 0xFFFFFFFF: not usable, so the loop's skips are the rule's skips.  The halo's offsets are compared with
// the room the tile's origin has before a coordinate is formed, as the rule's taps are.  The 49 taps are LDS reads, accumulated in the rule's
// row-major order by the rule's own functions: the bits are the rule's, not a reassociation of them.
// After the second barrier a thread that is not flagged writes V_in and ends; there is no barrier behind it.
// 64-bit indices are formed from unmasked 32-bit values (kernel_progressive.h says why).  All stores are plain vector stores; no atomics.
// out_var may be var: a pixel reads only its own V_in, before it writes.
#pragma once

#include "variance_rule.h"
#include "kernel_tile.h"

constexpr uint32_t VARIANCE_HALO_X = TILE_X + 2 * CRT_VARIANCE_RADIUS, VARIANCE_HALO_Y = TILE_Y + 2 * CRT_VARIANCE_RADIUS;
constexpr uint32_t VARIANCE_HALO = VARIANCE_HALO_X * VARIANCE_HALO_Y;   // 38 x 14 = 532 slots a plane

struct VarianceArgs {
    crt_variance_rule rule;
    int32_t width, height;
    uint32_t tiles_x;                    // ceil(width / TILE_X)
    const crt_history_record *moments;   // c, m2 and weight are read
    const crt_hit *hits;
    const float *var;
    float *out_var;                      // may be var
};
__global__ __launch_bounds__(BLOCK) void variance_estimate(const VarianceArgs P) {
    __shared__ crt_variance_tap_geometry tile_a[VARIANCE_HALO];
    __shared__ crt_variance_tap_place tile_b[VARIANCE_HALO];
    __shared__ crt_variance_tap_moments tile_c[VARIANCE_HALO];
    const TilePixel t = tile_pixel(P.tiles_x, P.width, P.height);
    const uint32_t ox = t.ox, oy = t.oy;   // the tile's origin: inside the frame
    const bool inside = t.inside;
    const uint64_t i = tile_index(t, P.width);
    crt_guide GP{};
    float weight_p = 0.0f, v_in = 0.0f;
    bool flagged = false;
    if (inside) {
        const crt_history_record *m = P.moments + i;
        crt_variance_tap_moments MP;
        MP.c[0] = m->c[0]; MP.c[1] = m->c[1]; MP.c[2] = m->c[2];
        MP.m2 = m->m2;
        weight_p = m->weight;
        GP = guide_of_hit(P.hits[i]);
        v_in = P.var[i];
        flagged = crt_variance_flagged(P.rule, MP, weight_p, GP.mesh);
    }
    if (!__syncthreads_or(flagged ? 1 : 0)) {   // every thread of the workgroup is here
        if (inside) P.out_var[i] = v_in;
        return;
    }
    const uint32_t tid = threadIdx.y * TILE_X + threadIdx.x;
    for (uint32_t k = tid; k < VARIANCE_HALO; k += BLOCK) {
        const int32_t dx = (int32_t)(k % VARIANCE_HALO_X) - CRT_VARIANCE_RADIUS, dy = (int32_t)(k / VARIANCE_HALO_X) - CRT_VARIANCE_RADIUS;
        crt_variance_tap_geometry A;
        crt_variance_tap_place B;
        crt_variance_tap_moments Q;
        A.n[0] = 0.0f; A.n[1] = 0.0f; A.n[2] = 0.0f; A.mesh = CRT_GUIDE_MISS;
        B.x[0] = 0.0f; B.x[1] = 0.0f; B.x[2] = 0.0f; B.weight = 0.0f;
        Q.c[0] = 0.0f; Q.c[1] = 0.0f; Q.c[2] = 0.0f; Q.m2 = 0.0f;
        // the offset against the room the origin has: ox < width and oy < height, so neither difference overflows
        if (!(dx < -(int32_t)ox || dx >= P.width - (int32_t)ox || dy < -(int32_t)oy || dy >= P.height - (int32_t)oy)) {
            const uint32_t qx = (uint32_t)((int32_t)ox + dx), qy = (uint32_t)((int32_t)oy + dy);
            const uint64_t q = (uint64_t)qy * (uint32_t)P.width + qx;
            const crt_history_record *m = P.moments + q;
            Q.c[0] = m->c[0]; Q.c[1] = m->c[1]; Q.c[2] = m->c[2];
            Q.m2 = m->m2;
            B.weight = m->weight;
            const crt_guide G = guide_of_hit(P.hits[q]);
            A.n[0] = G.n[0]; A.n[1] = G.n[1]; A.n[2] = G.n[2];
            A.mesh = G.mesh;
            B.x[0] = G.x[0]; B.x[1] = G.x[1]; B.x[2] = G.x[2];
        }
        tile_a[k] = A;
        tile_b[k] = B;
        tile_c[k] = Q;
    }
    __syncthreads();
    if (!inside) return;
    if (!flagged) {
        P.out_var[i] = v_in;
        return;
    }
    const float tol = P.rule.sigma_plane * GP.t;
    crt_variance_sums s = crt_variance_begin();
    const uint32_t centre = (threadIdx.y + CRT_VARIANCE_RADIUS) * VARIANCE_HALO_X + threadIdx.x + CRT_VARIANCE_RADIUS;
    for (int32_t dy = -CRT_VARIANCE_RADIUS; dy <= CRT_VARIANCE_RADIUS; dy++)
        for (int32_t dx = -CRT_VARIANCE_RADIUS; dx <= CRT_VARIANCE_RADIUS; dx++) {
            const uint32_t k = (uint32_t)((int32_t)centre + dy * (int32_t)VARIANCE_HALO_X + dx);   // 0 .. VARIANCE_HALO - 1
            crt_variance_tap(P.rule, GP, tol, tile_a[k], tile_b[k], tile_c[k], s);
        }
    P.out_var[i] = crt_variance_finish(s, weight_p, v_in);
}
