// kernel_bake.h -- the kernels of lightmap baking (include/crt_hip.h: crt_bake_texels_device, crt_bake_dilate_device, crt_bake_lightmap);
// the rule, one header for host and device: csrc/bake_rule.h.
//   bake_owner        the rasteriser: ONE WAVE per triangle of the mesh.  The wave's lanes stride the triangle's clipped box of texels, test
//                     each centre against the rule and resolve ties with a plain vector atomicMin on the uint32 owner plane: the lowest
//                     triangle index wins whatever the order.  A box of more than BAKE_WAVE_TEXELS texels (64 turns of a wave) is not walked
//                     here: its triangle is appended to the large list, so no wave's work exceeds 64 turns.
//   bake_reset        owner plane = 0xFFFFFFFF and the large list's count = 0: a kernel, not a memset, so that a captured call is a chain of
//                     kernel nodes and nothing else (with memset or copy nodes between kernel nodes a replayed graph did
//                     not keep the chain's order on this runtime).  bake_copy: the dilation's copy back after an odd number of passes, likewise.
//   bake_owner_large  the large list's boxes, one after the other, each strided by EVERY thread of a fixed grid: a floor quad that fills a
//                     2048 x 2048 map is 16 turns of a thread, not a million of a wave.  The list's order depends on arrival; the owner plane
//                     does not (atomicMin).
//   bake_texels       one thread per texel, a workgroup covers a TILE_X x TILE_Y tile of the map (kernel_tile.h): reads the owner, recomputes
//                     the owner's edge functions at the centre -- the same expressions, so the same bits --, and writes the 48-byte record as
//                     three 16-byte stores, the probe ray and the status byte.  EMPTY texels write a zero record and no ray.
//   bake_mark / bake_scan / bake_scatter   the stable compaction of the covered texels into a row-major list (kernel_adaptive.h's scheme:
//                     every wave's ballot, ONE workgroup's exclusive prefix sum, a scatter to block offset + waves before + lanes below; no
//                     atomic decides a position, so the list is the same on every run).  The scatter copies the texel's probe ray along.
//   bake_keys         the keys of one sample of the listed texels.
//   bake_fold         the fold of the listed texels' colours into the map (or, without a sum, the plain scatter).
//   bake_dilate       one dilation pass, one thread per texel, tiled as bake_texels: copies, no arithmetic.
//   bake_count_status / bake_count_self   the statistics' counts: one atomicAdd per wave on a word nobody orders by.
// Memory.  The UV corners a wave of bake_owner reads are wave-uniform addresses (three indices, then three 12-byte vertices); the owner
// plane's atomics of a wave fall on rows of the box, contiguous within a row.  bake_texels gathers per texel through the owner; neighbouring
// texels mostly share their owner, so the gathers meet in the vector L1.  No LDS but the compaction's wave words.
// 64-bit indices are formed from unmasked 32-bit values (kernel_progressive.h says why).  All stores are plain vector stores.
#pragma once

#include "bake_rule.h"
#include "kernel_tile.h"

constexpr uint32_t BAKE_WAVE_TEXELS = 4096;     // a wave walks boxes up to this many texels: 64 turns
constexpr uint32_t BAKE_LARGE_BLOCKS = 1024;    // the grid of bake_owner_large
constexpr uint32_t BAKE_WAVES = BLOCK / 64;
static_assert(BLOCK % 64 == 0 && BAKE_WAVES >= 1 && BAKE_WAVES <= 64, "a workgroup's waves are scanned by its first lanes");

struct BakeOwnerArgs {
    const uint32_t *tris;        // the mesh's triangles, global indices, ascending
    uint32_t n_tris;
    const uint32_t *tri_verts;   // 3 per triangle
    const float *vuvs;           // 3 per vertex
    uint32_t n_triangles;        // of the scene: an index read from the large list is compared with it before anything is read through it
    int32_t width, height;
    uint32_t *owner;             // width * height words, 0xFFFFFFFF before the launch
    uint32_t *large;             // [0]: entries (0 before the launch), [1 .. 1 + n_tris): the triangles whose boxes bake_owner_large walks
};

__device__ __forceinline__ crt_bake_uv bake_uv_of(const uint32_t *tri_verts, const float *vuvs, const uint32_t tri) {
    const uint32_t *v = tri_verts + 3 * (uint64_t)tri;
    const float *a = vuvs + 3 * (uint64_t)v[0], *b = vuvs + 3 * (uint64_t)v[1], *c = vuvs + 3 * (uint64_t)v[2];
    return crt_bake_uv{a[0], a[1], b[0], b[1], c[0], c[1]};
}

// texel k of a box, row-major within the box: tested, and claimed where covered.  The box lies inside the map (crt_bake_box_of clamps it), so
// k < width * height < 2^31: the division is a 32-bit one.
__device__ __forceinline__ void bake_claim(const BakeOwnerArgs &P, const crt_bake_uv uv, const float area, const crt_bake_box box, const uint32_t bw,
                                           const uint32_t k, const uint32_t tri) {
    const uint32_t in_row = k / bw;
    const int32_t row = box.row0 + (int32_t)in_row, col = box.col0 + (int32_t)(k - in_row * bw);
    float qx, qy, e1, e2;
    crt_bake_centre(P.width, P.height, row, col, &qx, &qy);
    if (crt_bake_covers(uv, area, qx, qy, &e1, &e2)) atomicMin(P.owner + ((uint64_t)(uint32_t)row * (uint32_t)P.width + (uint32_t)col), tri);
}

// owner[0 .. n) = 0xFFFFFFFF, large[0] = 0
__global__ __launch_bounds__(BLOCK) void bake_reset(uint32_t *owner, const uint64_t n, uint32_t *large) {
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK + threadIdx.x, stride = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t i = first; i < n; i += stride) owner[i] = CRT_BAKE_NO_OWNER;
    if (first == 0u) large[0] = 0u;
}

// dst[0 .. n) = src[0 .. n), bytes
__global__ __launch_bounds__(BLOCK) void bake_copy(const uint8_t *src, uint8_t *dst, const uint64_t n) {
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK + threadIdx.x, stride = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t i = first; i < n; i += stride) dst[i] = src[i];
}

__global__ __launch_bounds__(BLOCK) void bake_owner(const BakeOwnerArgs P) {
    const uint64_t i = (uint64_t)blockIdx.x * BAKE_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= P.n_tris) return;
    const uint32_t tri = P.tris[i];
    const crt_bake_uv uv = bake_uv_of(P.tri_verts, P.vuvs, tri);
    const float area = crt_bake_area(uv);
    if (!crt_bake_area_usable(area)) return;
    const crt_bake_box box = crt_bake_box_of(uv, P.width, P.height);
    if (box.col0 > box.col1 || box.row0 > box.row1) return;
    const uint32_t bw = (uint32_t)(box.col1 - box.col0) + 1u, bh = (uint32_t)(box.row1 - box.row0) + 1u;
    const uint32_t texels = bw * bh;   // (inside the map: below 2^31)
    if (texels > BAKE_WAVE_TEXELS) {
        if (lane == 0u) {
            const uint32_t at = atomicAdd(P.large, 1u);
            if (at < P.n_tris) P.large[1u + at] = tri;   // (a triangle is appended once, so there is always room)
        }
        return;
    }
    for (uint32_t k = lane; k < texels; k += 64u) bake_claim(P, uv, area, box, bw, k, tri);
}

__global__ __launch_bounds__(BLOCK) void bake_owner_large(const BakeOwnerArgs P) {
    const uint32_t listed = P.large[0];
    const uint32_t n = listed < P.n_tris ? listed : P.n_tris;
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK + threadIdx.x, stride = (uint64_t)gridDim.x * BLOCK;
    for (uint32_t e = 0; e < n; e++) {   // (uniform: every thread takes every entry)
        const uint32_t tri = P.large[1u + e];
        if (tri >= P.n_triangles) continue;   // (uniform; never true for an entry bake_owner wrote)
        const crt_bake_uv uv = bake_uv_of(P.tri_verts, P.vuvs, tri);
        const float area = crt_bake_area(uv);
        const crt_bake_box box = crt_bake_box_of(uv, P.width, P.height);
        const uint32_t bw = (uint32_t)(box.col1 - box.col0) + 1u, bh = (uint32_t)(box.row1 - box.row0) + 1u;
        const uint64_t texels = (uint64_t)bw * bh;   // (below 2^31; k + stride is formed in 64 bits)
        for (uint64_t k = first; k < texels; k += stride) bake_claim(P, uv, area, box, bw, (uint32_t)k, tri);
    }
}

struct BakeTexelsArgs {
    const uint32_t *owner;
    const uint32_t *tri_verts;
    const float *vuvs;
    const float4 *tris;          // 4 x float4 per crt_triangle
    int32_t width, height;
    uint32_t tiles_x, mesh;
    uint32_t n_triangles;        // of the scene: an owner word that is no triangle of it is EMPTY, and nothing is read through it
    float probe_offset;
    float4 *texels;              // 3 x float4 per crt_bake_texel
    crt_ray *rays;               // by texel; written for covered texels only
    uint8_t *status;             // or null
};
__global__ __launch_bounds__(BLOCK) void bake_texels(const BakeTexelsArgs P) {
    const TilePixel t = tile_pixel(P.tiles_x, P.width, P.height);
    if (!t.inside) return;
    const uint64_t i = tile_index(t, P.width);
    const uint32_t tri = P.owner[i];
    float4 *out = P.texels + 3 * i;
    if (tri >= P.n_triangles) {   // CRT_BAKE_NO_OWNER, or a word the rasteriser did not write
        out[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        reinterpret_cast<uint4 *>(out)[2] = make_uint4(CRT_BAKE_NO_OWNER, P.mesh, CRT_BAKE_STATUS_EMPTY, 0u);
        if (P.status) P.status[i] = (uint8_t)CRT_BAKE_STATUS_EMPTY;
        return;
    }
    const crt_bake_uv uv = bake_uv_of(P.tri_verts, P.vuvs, tri);
    const float area = crt_bake_area(uv);
    float qx, qy, e1, e2;
    crt_bake_centre(P.width, P.height, (int32_t)t.uy, (int32_t)t.ux, &qx, &qy);
    (void)crt_bake_covers(uv, area, qx, qy, &e1, &e2);
    const float4 *T = P.tris + 4 * (uint64_t)tri;
    const float4 a = T[0], b = T[1], c = T[2];
    const float v0[3] = {a.x, a.y, a.z}, v1[3] = {b.x, b.y, b.z}, v2[3] = {c.x, c.y, c.z}, normal[3] = {a.w, b.w, c.w};
    float u, v, point[3];
    crt_bake_record(area, e1, e2, v0, v1, v2, &u, &v, point);
    out[0] = make_float4(point[0], point[1], point[2], u);
    out[1] = make_float4(normal[0], normal[1], normal[2], v);
    reinterpret_cast<uint4 *>(out)[2] = make_uint4(tri, P.mesh, CRT_BAKE_STATUS_COVERED, 0u);
    crt_ray q;
    crt_bake_probe(point, normal, P.probe_offset, q.origin, q.direction);
    P.rays[i] = q;
    if (P.status) P.status[i] = (uint8_t)CRT_BAKE_STATUS_COVERED;
}

// ---- the compaction: the covered texels, in row-major order
struct BakeListWork {
    unsigned long long *masks;   // one per wave of bake_mark's grid
    uint32_t *counts, *offsets;  // one per workgroup
};
struct BakeMarkArgs {
    const uint8_t *status;
    uint64_t n;
    BakeListWork work;
};
// one thread per texel p < n (no thread leaves before the ballot and the barrier)
__global__ __launch_bounds__(BLOCK) void bake_mark(const BakeMarkArgs P) {
    __shared__ unsigned long long wave_mask[BAKE_WAVES];
    const uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool keep = p < P.n && P.status[p] == (uint8_t)CRT_BAKE_STATUS_COVERED;
    const unsigned long long mask = __ballot(keep);
    if ((threadIdx.x & 63u) == 0u) wave_mask[threadIdx.x >> 6] = mask;
    __syncthreads();
    if (threadIdx.x < BAKE_WAVES) P.work.masks[(uint64_t)blockIdx.x * BAKE_WAVES + threadIdx.x] = wave_mask[threadIdx.x];
    if (threadIdx.x == 0u) {
        uint32_t kept = 0;
        for (uint32_t w = 0; w < BAKE_WAVES; w++) kept += (uint32_t)__popcll(wave_mask[w]);
        P.work.counts[blockIdx.x] = kept;
    }
}

// offsets[b] = counts[0] + .. + counts[b - 1], *total = the sum: ONE workgroup, BLOCK counts a turn (kernel_adaptive.h: adaptive_scan)
struct BakeScanArgs {
    const uint32_t *counts;
    uint32_t *offsets, *total;
    uint32_t blocks;
};
__global__ __launch_bounds__(BLOCK) void bake_scan(const BakeScanArgs P) {
    __shared__ uint32_t wave_total[BAKE_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < P.blocks; base += BLOCK) {   // (uniform: every thread takes every turn, so the barriers are met by all)
        const uint32_t b = base + threadIdx.x;
        const uint32_t own = b < P.blocks ? P.counts[b] : 0u;
        uint32_t incl = own;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63u) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = 0, turn = 0;
        for (uint32_t w = 0; w < BAKE_WAVES; w++) {
            const uint32_t t = wave_total[w];
            if (w < wave) before += t;
            turn += t;
        }
        if (b < P.blocks) P.offsets[b] = carry + before + (incl - own);
        carry += turn;
        __syncthreads();   // wave_total is written again in the next turn
    }
    if (threadIdx.x == 0u) *P.total = carry;
}

struct BakeScatterArgs {
    uint64_t n;
    BakeListWork work;
    const crt_ray *rays;         // by texel
    uint32_t *list;              // the covered texels' indices ...
    crt_ray *list_rays;          // ... and their probe rays
};
__global__ __launch_bounds__(BLOCK) void bake_scatter(const BakeScatterArgs P) {
    __shared__ unsigned long long wave_mask[BAKE_WAVES];
    if (threadIdx.x < BAKE_WAVES) wave_mask[threadIdx.x] = P.work.masks[(uint64_t)blockIdx.x * BAKE_WAVES + threadIdx.x];
    __syncthreads();
    const uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long mask = wave_mask[wave];
    if (p >= P.n || !((mask >> lane) & 1ull)) return;
    uint32_t at = P.work.offsets[blockIdx.x];
    for (uint32_t w = 0; w < BAKE_WAVES; w++)
        if (w < wave) at += (uint32_t)__popcll(wave_mask[w]);
    at += (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    P.list[at] = (uint32_t)p;   // at < the covered texels <= n: the list holds n entries
    P.list_rays[at] = P.rays[p];
}

struct BakeKeysArgs {
    const uint32_t *list;
    uint64_t n;
    uint32_t seed, sample;
    uint32_t *keys;
};
__global__ __launch_bounds__(BLOCK) void bake_keys(const BakeKeysArgs P) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    P.keys[i] = crt_bake_key(P.seed, P.list[i], P.sample);
}

// entry i < n of the list, texel p = list[i] (skipped unless p < map_texels): with a sum, one step of the fold and the mean it stands for;
// without, map[p] = the colour as it is.  The texels of a list are distinct.
struct BakeFoldArgs {
    const float *rgb;            // 3 floats per list entry
    const uint32_t *list;
    uint64_t n, map_texels;
    uint32_t sample;
    float *sum;                  // or null
    float *map;
};
__global__ __launch_bounds__(BLOCK) void bake_fold(const BakeFoldArgs P) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t p = P.list[i];
    if ((uint64_t)p >= P.map_texels) return;
    const float *c = P.rgb + 3 * i;
    float *m = P.map + 3 * (uint64_t)p;
    if (!P.sum) {
        m[0] = c[0]; m[1] = c[1]; m[2] = c[2];
        return;
    }
    float *s = P.sum + 3 * (uint64_t)p;
    for (int k = 0; k < 3; k++) {
        float mean;
        s[k] = crt_bake_fold(P.sample, P.sample == 0u ? 0.0f : s[k], c[k], &mean);
        m[k] = mean;
    }
}

struct BakeDilateArgs {
    int32_t width, height;
    uint32_t tiles_x;
    const float *rgb;
    const uint8_t *status;
    float *out_rgb;
    uint8_t *out_status;
};
__global__ __launch_bounds__(BLOCK) void bake_dilate(const BakeDilateArgs P) {
    const TilePixel t = tile_pixel(P.tiles_x, P.width, P.height);
    if (!t.inside) return;
    const uint64_t i = tile_index(t, P.width);
    const int64_t from = crt_bake_dilate_source(P.width, P.height, (int32_t)t.uy, (int32_t)t.ux, P.status);
    const float *c = P.rgb + 3 * (from < 0 ? i : (uint64_t)from);
    float *o = P.out_rgb + 3 * i;
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    P.out_status[i] = from < 0 ? P.status[i] : (uint8_t)CRT_BAKE_STATUS_DILATED;
}

// *count += the texels p < n with status[p] == what
__global__ __launch_bounds__(BLOCK) void bake_count_status(const uint8_t *status, const uint64_t n, const uint8_t what, uint32_t *count) {
    const uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const unsigned long long mask = __ballot(p < n && status[p] == what);
    if ((threadIdx.x & 63u) == 0u && mask) atomicAdd(count, (uint32_t)__popcll(mask));
}

// *count += the list entries i < n whose probe's closest hit is the texel's owner
__global__ __launch_bounds__(BLOCK) void bake_count_self(const crt_hit *hits, const uint32_t *list, const float4 *texels, const uint64_t n, uint32_t *count) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    bool self = false;
    if (i < n) {
        const uint32_t owner = reinterpret_cast<const uint4 *>(texels)[3 * (uint64_t)list[i] + 2].x;
        self = hits[i].hit != 0u && hits[i].triangle == owner;
    }
    const unsigned long long mask = __ballot(self);
    if ((threadIdx.x & 63u) == 0u && mask) atomicAdd(count, (uint32_t)__popcll(mask));
}
